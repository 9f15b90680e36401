// ttp.hip — slice-matrix chains and wraps with the hopping exponential of the t-t' square 16 x 16 lattice in four-factor
// form (n = 256).  An extension: the reference has no next-nearest-neighbour hopping.
//
// On the periodic 16 x 16 SquareLattice (site i = x + 16 y) with nearest-neighbour hopping t and next-nearest-neighbour
// hopping t' the hopping runs along four commuting shifts: X (x + 1), Y (y + 1), D = XY and A = X Y^-1.  So every hopping
// exponential is, up to rounding, E = (Fy (x) Fx) Ed Ea, where Ed applies a 16 x 16 matrix Fd along each diagonal
// x - y = u and Ea a matrix Fa along each anti-diagonal x + y = w:
//   (Ed v)(x, y) = sum_y' Fd[y, y'] v(x - y + y', y')        (Ea v)(x, y) = sum_y' Fa[y, y'] v(x + y - y', y')
// The factors come from the host and are checked against the dense matrices before the handle takes them (engine.cpp:
// dqmc_set_square_tp_factors).  A column v, read as the 16 x 16 matrix V[x][y] = v[x + 16 y], then goes through four
// 16-contractions: 16 v_mfma_f64_16x16x4_f64 per column instead of the 64 of the dense product.
//
//   X_s = post_s (.) ( A_s * ( pre_s (.) X_{s-1} ) ),  s = 1 .. nsteps,    out = X_nsteps (.) col_d   (or its transpose)
//
// with the argument conventions and scaling placement of kron.hip (KronArgs; no pending chunk), used as tri.hip is: for
// add_slice_sequence_left/right and, as two one-step launches with transposed stores, for wrap_greens! (engine.cpp:
// wrap_greens_kron).  The daggered products and the right-hand wrap products take the transposed factors.
//
// Layout.  As in tri.hip a wave holds a column as one MFMA accumulator tile: register r of lane (g = lane >> 4,
// c = lane & 15) holds the entry at row k = g + 4 r, lane c of one of four states
//   A: (y, x) = (k, c)     S: (y, u) = (k, c), x = (u + y) mod 16     R: (y, w) = (k, c), x = (w - y) mod 16     B: (x, y) = (k, c)
// A product sums over the row index of a tile, so in state A it applies Fy, in S Fd, in R Fa, in B Fx, with no data
// movement.  Between them the column goes through LDS (a 16 x 17 tile per column, written as [row][lane] of the product,
// read in the next state's order):
//   a step that starts in A:  Fy (A) -> LDS -> Fd (S) -> LDS -> Fa (R) -> LDS -> Fx (B),    i.e. A_s = Fx Ea Ed Fy
//   a step that starts in B:  Fx (B) -> LDS -> Fd (S) -> LDS -> Fa (R) -> LDS -> Fy (A),    i.e. A_s = Fy Ea Ed Fx
// Three LDS passes per step, and the state alternates: A at the start, where a load of one register is 64 consecutive
// doubles.  The pass S -> R keeps the row and rotates the 16 lanes of row y by 2 y; it goes through a tile like the other
// two.  There are two tile regions: the third pass writes the region of the first again, whose reads lie in front of the
// second pass's barrier.  Columns are independent: a workgroup (4 waves x TP_NC columns) owns 16 consecutive columns
// through all steps, and nothing crosses workgroups.  The result is staged in LDS and stored as whole 128-byte lines, as
// is or transposed.
#include "factored_common.h"

namespace dqmc {

constexpr int TP_N = 256;
constexpr int TP_NC = 4;                         // columns per wave
constexpr int TP_COLS = 4 * TP_NC;               // columns per workgroup
constexpr int TP_TLD = 17;                       // row stride of a column tile (doubles)
constexpr int TP_TILE = 16 * TP_TLD;
constexpr int TP_REGION = 4 * TP_NC * TP_TILE;   // the tiles of the four waves for one pass
constexpr int TP_SLD = 18;                       // row stride of the transposed staging image (doubles; even: 16-byte reads)
constexpr int TP_LDS = 2 * TP_REGION;            // 69 632 bytes: two workgroups per CU
static_assert(TP_LDS >= TP_N * TP_SLD && TP_LDS >= TP_COLS * TP_N, "the staging image of the result reuses the tiles");

__global__ __launch_bounds__(256) void ttp_chain_kernel(KronArgs a)
{
    __shared__ __attribute__((aligned(16))) double lds[TP_LDS];
    const int unit = blockIdx.x / (TP_N / TP_COLS), c0 = TP_COLS * (blockIdx.x % (TP_N / TP_COLS));
    if (unit >= a.n_units) return;
    const int wk = a.nb == 2 ? unit >> 1 : unit, blk = a.nb == 2 ? unit & 1 : 0;
    const bool bn = blk != 0;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, ci = lane & 15;
    const long conf_off = (long)wk * a.conf_stride;
    double *t1 = lds + w * (TP_NC * TP_TILE), *t2 = t1 + TP_REGION;

    // X_0: column c0 + TP_NC w + t in state A: register r = entries ci + 16 (g + 4 r), 64 consecutive doubles
    d4 v[TP_NC];
    {
        const double *x0 = a.X0 + (long)a.x_su * unit + (long)TP_N * (c0 + TP_NC * w) + ci + 16 * g;
#pragma unroll
        for (int t = 0; t < TP_NC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[t][r] = x0[TP_N * t + 64 * r];
    }
    // entry index of register r of this lane in state A (par 0) or B (par 1)
    auto idx = [&](int par, int r) { return par ? (g + 4 * r) + 16 * ci : ci + 16 * (g + 4 * r); };
    // A operands of a step (lane: F[row ci][k = 4 q + g] of the column-major 16 x 16 factor; f1 first, f4 last) and the
    // HS-field bytes of its two scalings, requested one step ahead without a branch (a missing scaling reads X_0 and is not
    // applied), as in kron.hip.  Fd and Fa lie behind Fy in the buffer st.ay points to.
    struct Ops {
        double f1[4], fd[4], fa[4], f4[4];
        int8_t cpre[4], cpost[4];
    };
    auto request = [&](int s, Ops &o) {
        const KronStep &st = a.st[s];
        const int par = s & 1;
        const double *fx = st.ax + TP_N * blk, *fy = st.ay + TP_N * blk;
        const double *fd = st.ay + TP_N * (a.nb + blk), *fa = st.ay + TP_N * (2 * a.nb + blk);
        const double *f1 = par ? fx : fy, *f4 = par ? fy : fx;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o.f1[q] = f1[ci + 16 * (4 * q + g)];
            o.fd[q] = fd[ci + 16 * (4 * q + g)];
            o.fa[q] = fa[ci + 16 * (4 * q + g)];
            o.f4[q] = f4[ci + 16 * (4 * q + g)];
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
        for (int t = 0; t < TP_NC; ++t) {
            d4 p = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) p = FK_MFMA(fv[q], v[t][q], p);
#pragma unroll
            for (int r = 0; r < 4; ++r) tl[t * TP_TILE + (g + 4 * r) * TP_TLD + ci] = p[r];
        }
    };
    Ops cur, nxt;
    request(0, cur);
    double cs[TP_NC];  // final column scale (read from X_0 and not applied when there is none)
    {
        const double *cd = a.col_d ? a.col_d + (long)unit * a.col_stride + c0 + TP_NC * w : a.X0;
#pragma unroll
        for (int t = 0; t < TP_NC; ++t) cs[t] = cd[t];
    }

    for (int s = 0; s < a.nsteps; ++s) {
        const KronStep &st = a.st[s];
        const int par = s & 1;
        if (st.pre_conf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double f = fk_conf(cur.cpre[r], st.pre_sign, bn, a.epl, a.eml);
#pragma unroll
                for (int t = 0; t < TP_NC; ++t) v[t][r] *= f;
            }
        }
        // Fy (state A) or Fx (state B) -> t1[k][c]: (y, x) or (x, y)
        product_to(cur.f1, t1);
        request(min(s + 1, a.nsteps - 1), nxt);
        __syncthreads();
        // -> state S: register r of lane (g, ci) is (y, u) = (g + 4 r, ci) at x = (ci + g + 4 r) mod 16
#pragma unroll
        for (int t = 0; t < TP_NC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = g + 4 * r, x = (ci + y) & 15;
                v[t][r] = t1[t * TP_TILE + (par ? x * TP_TLD + y : y * TP_TLD + x)];
            }
        // Fd (state S) -> t2[y][u]
        product_to(cur.fd, t2);
        __syncthreads();
        // -> state R: register r of lane (g, ci) is (y, w) = (g + 4 r, ci) at u = x - y = (ci - 2 y) mod 16
#pragma unroll
        for (int t = 0; t < TP_NC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = g + 4 * r;
                v[t][r] = t2[t * TP_TILE + y * TP_TLD + ((ci - 2 * y) & 15)];
            }
        // Fa (state R) -> t1[y][w] (every read of the first pass lies in front of the barrier above)
        product_to(cur.fa, t1);
        __syncthreads();
        // -> state B (from A) or A (from B): register r of lane (g, ci) is (k, ci) = (x, y) or (y, x), w = x + y
#pragma unroll
        for (int t = 0; t < TP_NC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = g + 4 * r;
                v[t][r] = t1[t * TP_TILE + (par ? k : ci) * TP_TLD + ((k + ci) & 15)];
            }
        // Fx (state B) or Fy (state A), in registers
#pragma unroll
        for (int t = 0; t < TP_NC; ++t) {
            d4 q4 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) q4 = FK_MFMA(cur.f4[q], v[t][q], q4);
            v[t] = q4;
        }
        if (st.post_conf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double f = fk_conf(cur.cpost[r], st.post_sign, bn, a.epl, a.eml);
#pragma unroll
                for (int t = 0; t < TP_NC; ++t) v[t][r] *= f;
            }
        }
        cur = nxt;
        // (the next step's first pass writes t1 again: a wave reads and writes only its own tiles, in program order)
    }
    __syncthreads();  // every wave is done with its tiles (the staging image goes over both regions)
    // ---- staging image: transposed [entry][column] (row stride TP_SLD), else [column][entry] (the global image)
    const int par = a.nsteps & 1;
#pragma unroll
    for (int t = 0; t < TP_NC; ++t) {
        const int cl = TP_NC * w + t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = idx(par, r);
            lds[a.transpose_out ? i * TP_SLD + cl : cl * TP_N + i] = a.col_d ? v[t][r] * cs[t] : v[t][r];
        }
    }
    __syncthreads();
    fk_store_image<TP_N, TP_COLS, TP_SLD, 0>(a.out + (long)unit * a.out_su, lds, a, c0, tid);
}

hipError_t launch_ttp_chain(const KronArgs &a, hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    if (a.nsteps < 1 || a.nsteps > SLAB_MAX_STEPS || a.nb < 1 || a.nb > 2 || a.pf_img) return hipErrorInvalidValue;
    return fk_launch(ttp_chain_kernel, dim3(a.n_units * (TP_N / TP_COLS)), a, s, start, stop);
}

}  // namespace dqmc
