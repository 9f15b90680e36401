// tri.hip — slice-matrix chains and wraps with the hopping exponential of the triangular 16 x 16 lattice in factored form
// (n = 256).
//
// On the periodic 16 x 16 TriangularLattice (site i = x + 16 y) the hopping runs along three commuting shifts: X (x + 1),
// Y (y + 1) and D = XY.  So every hopping exponential is, up to rounding, A = (Fy (x) Fx) Ed, where Ed applies a 16 x 16
// matrix Fd along each diagonal x - y = u: (Ed v)(x, y) = sum_y' Fd[y, y'] v(x - y + y', y').  The factors come from the
// host and are checked against the dense matrices before the handle takes them (engine.cpp: dqmc_set_triangular_factors).
// A column v, read as the 16 x 16 matrix V[x][y] = v[x + 16 y], then goes through three 16-contractions: 12
// v_mfma_f64_16x16x4_f64 per column instead of the 64 of the dense product.
//
//   X_s = post_s (.) ( A_s * ( pre_s (.) X_{s-1} ) ),  s = 1 .. nsteps,    out = X_nsteps (.) col_d   (or its transpose)
//
// with the argument conventions and scaling placement of kron.hip (KronArgs; no pending chunk).  Used for
//   * add_slice_sequence_left/right (stack.jl:272-311): the safe_mult products B_l X / B_l' X;
//   * wrap_greens! (stack.jl:491-500) as two one-step launches with transposed stores (engine.cpp: wrap_greens_kron).
// The daggered products and the right-hand wrap products take the transposed factors: A' = Fx' Ed(Fd') Fy' or the like.
//
// Layout.  A wave holds a column as one MFMA accumulator tile (4 doubles per lane): register r of lane (g = lane >> 4,
// c = lane & 15) holds the entry at row k = g + 4 r, lane c of one of three states
//   A: (y, x) = (k, c)       B: (x, y) = (k, c)       S: (y, u) = (k, c), x = (u + y) mod 16   (sheared)
// Register q of a tile is the B operand of k-block q of a product that sums over its row index, so in state A a
// product applies Fy, in S Fd, in B Fx, with no data movement.  Between them the column goes through LDS (a 16 x 17 tile
// per column, written as [row][lane] of the product, read in the next state's order):
//   a step that starts in A:  Fy (A) -> LDS -> Fd (S) -> LDS -> Fx (B),    i.e. A_s = Fx Ed Fy
//   a step that starts in B:  Fx (B) -> LDS -> Fd (S) -> LDS -> Fy (A),    i.e. A_s = Fy Ed Fx
// Two LDS passes per step, and the state alternates: A at the start, where a load of one register is 64 consecutive
// doubles.  The two passes use separate tile regions, so a step needs two barriers.  Columns are independent: a
// workgroup (4 waves x TR_NC columns) owns 16 consecutive columns through all steps, and nothing crosses workgroups.  The
// result is staged in LDS and stored as whole 128-byte lines, as is or transposed.
#include "factored_common.h"

namespace dqmc {

constexpr int TR_N = 256;
constexpr int TR_NC = 4;                         // columns per wave
constexpr int TR_COLS = 4 * TR_NC;               // columns per workgroup
constexpr int TR_TLD = 17;                       // row stride of a column tile (doubles)
constexpr int TR_TILE = 16 * TR_TLD;
constexpr int TR_REGION = 4 * TR_NC * TR_TILE;   // the tiles of the four waves for one pass
constexpr int TR_SLD = 18;                       // row stride of the transposed staging image (doubles; even: 16-byte reads)
constexpr int TR_LDS = 2 * TR_REGION;            // 69 632 bytes: two workgroups per CU
static_assert(TR_LDS >= TR_N * TR_SLD && TR_LDS >= TR_COLS * TR_N, "the staging image of the result reuses the tiles");

__global__ __launch_bounds__(256) void tri_chain_kernel(KronArgs a)
{
    __shared__ __attribute__((aligned(16))) double lds[TR_LDS];
    const int unit = blockIdx.x / (TR_N / TR_COLS), c0 = TR_COLS * (blockIdx.x % (TR_N / TR_COLS));
    if (unit >= a.n_units) return;
    const int wk = a.nb == 2 ? unit >> 1 : unit, blk = a.nb == 2 ? unit & 1 : 0;
    const bool bn = blk != 0;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, ci = lane & 15;
    const long conf_off = (long)wk * a.conf_stride;
    double *t1 = lds + w * (TR_NC * TR_TILE), *t2 = t1 + TR_REGION;

    // X_0: column c0 + TR_NC w + t in state A: register r = entries ci + 16 (g + 4 r), 64 consecutive doubles
    d4 v[TR_NC];
    {
        const double *x0 = a.X0 + (long)a.x_su * unit + (long)TR_N * (c0 + TR_NC * w) + ci + 16 * g;
#pragma unroll
        for (int t = 0; t < TR_NC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[t][r] = x0[TR_N * t + 64 * r];
    }
    // entry index of register r of this lane in state A (par 0) or B (par 1)
    auto idx = [&](int par, int r) { return par ? (g + 4 * r) + 16 * ci : ci + 16 * (g + 4 * r); };
    // A operands of a step (lane: F[row ci][k = 4 q + g] of the column-major 16 x 16 factor; f1 first, f3 last) and the
    // HS-field bytes of its two scalings, requested one step ahead without a branch (a missing scaling reads X_0 and is not
    // applied), as in kron.hip
    struct Ops {
        double f1[4], fd[4], f3[4];
        int8_t cpre[4], cpost[4];
    };
    auto request = [&](int s, Ops &o) {
        const KronStep &st = a.st[s];
        const int par = s & 1;
        const double *fx = st.ax + TR_N * blk, *fy = st.ay + TR_N * blk, *fd = st.ay + TR_N * (a.nb + blk);
        const double *f1 = par ? fx : fy, *f3 = par ? fy : fx;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o.f1[q] = f1[ci + 16 * (4 * q + g)];
            o.fd[q] = fd[ci + 16 * (4 * q + g)];
            o.f3[q] = f3[ci + 16 * (4 * q + g)];
        }
        const int8_t *dummy = reinterpret_cast<const int8_t *>(a.X0);
        const int8_t *pre = st.pre_conf ? st.pre_conf + conf_off : dummy, *post = st.post_conf ? st.post_conf + conf_off : dummy;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o.cpre[r] = pre[st.pre_conf ? idx(par, r) : 0];
            o.cpost[r] = post[st.post_conf ? idx(par ^ 1, r) : 0];
        }
    };
    // P = F V for the A operands fv, written to the tiles as [row][lane]
    auto product_to = [&](const double (&fv)[4], double *tl) {
#pragma unroll
        for (int t = 0; t < TR_NC; ++t) {
            d4 p = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) p = FK_MFMA(fv[q], v[t][q], p);
#pragma unroll
            for (int r = 0; r < 4; ++r) tl[t * TR_TILE + (g + 4 * r) * TR_TLD + ci] = p[r];
        }
    };
    Ops cur, nxt;
    request(0, cur);
    double cs[TR_NC];  // final column scale (read from X_0 and not applied when there is none)
    {
        const double *cd = a.col_d ? a.col_d + (long)unit * a.col_stride + c0 + TR_NC * w : a.X0;
#pragma unroll
        for (int t = 0; t < TR_NC; ++t) cs[t] = cd[t];
    }

    for (int s = 0; s < a.nsteps; ++s) {
        const KronStep &st = a.st[s];
        const int par = s & 1;
        if (st.pre_conf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double f = fk_conf(cur.cpre[r], st.pre_sign, bn, a.epl, a.eml);
#pragma unroll
                for (int t = 0; t < TR_NC; ++t) v[t][r] *= f;
            }
        }
        // Fy (state A) or Fx (state B) -> t1[k][c]: (y, x) or (x, y)
        product_to(cur.f1, t1);
        request(min(s + 1, a.nsteps - 1), nxt);
        __syncthreads();
        // -> state S: register r of lane (g, ci) is (y, u) = (g + 4 r, ci) at x = (ci + g + 4 r) mod 16
#pragma unroll
        for (int t = 0; t < TR_NC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = g + 4 * r, x = (ci + y) & 15;
                v[t][r] = t1[t * TR_TILE + (par ? x * TR_TLD + y : y * TR_TLD + x)];
            }
        // Fd (state S) -> t2[y][u]
        product_to(cur.fd, t2);
        __syncthreads();
        // -> state B (from A) or A (from B): register r of lane (g, ci) is (k, ci) = (x, y) or (y, x), u = x - y
#pragma unroll
        for (int t = 0; t < TR_NC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = g + 4 * r;
                v[t][r] = t2[t * TR_TILE + (par ? k * TR_TLD + ((ci - k) & 15) : ci * TR_TLD + ((k - ci) & 15))];
            }
        // Fx (state B) or Fy (state A), in registers
#pragma unroll
        for (int t = 0; t < TR_NC; ++t) {
            d4 q4 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) q4 = FK_MFMA(cur.f3[q], v[t][q], q4);
            v[t] = q4;
        }
        if (st.post_conf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double f = fk_conf(cur.cpost[r], st.post_sign, bn, a.epl, a.eml);
#pragma unroll
                for (int t = 0; t < TR_NC; ++t) v[t][r] *= f;
            }
        }
        cur = nxt;
    }
    __syncthreads();  // every wave is done with its tiles (the staging image goes over both regions)
    // ---- staging image: transposed [entry][column] (row stride TR_SLD), else [column][entry] (the global image)
    const int par = a.nsteps & 1;
#pragma unroll
    for (int t = 0; t < TR_NC; ++t) {
        const int cl = TR_NC * w + t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = idx(par, r);
            lds[a.transpose_out ? i * TR_SLD + cl : cl * TR_N + i] = a.col_d ? v[t][r] * cs[t] : v[t][r];
        }
    }
    __syncthreads();
    fk_store_image<TR_N, TR_COLS, TR_SLD, 0>(a.out + (long)unit * a.out_su, lds, a, c0, tid);
}

hipError_t launch_tri_chain(const KronArgs &a, hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    if (a.nsteps < 1 || a.nsteps > SLAB_MAX_STEPS || a.nb < 1 || a.nb > 2 || a.pf_img) return hipErrorInvalidValue;
    return fk_launch(tri_chain_kernel, dim3(a.n_units * (TR_N / TR_COLS)), a, s, start, stop);
}

}  // namespace dqmc
