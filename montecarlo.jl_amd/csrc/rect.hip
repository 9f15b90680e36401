// rect.hip — slice-matrix chains and wraps with the hopping exponential of the 32 x 8 rectangular lattice applied in
// factored form (n = 256 = 32 x 8).
//
// On the periodic RectangularLattice(32, 8) (site i = x + 32 y) every hopping exponential is, up to rounding, a Kronecker
// product A = Ey (x) Ex with Ex 32 x 32 and Ey 8 x 8 (hopping_forms.h: kron_split checks it at handle creation).  A column v of
// 256 entries is a plane V[y][x] = v[x + 32 y], and A v = vec(Ey V Ex^T): one 8-contraction along y and one 32-contraction
// along x instead of the dense 256-contraction.
//
//   X_s = post_s (.) ( A_s * ( pre_s (.) X_{s-1} ) ),  s = 1 .. nsteps,    out = X_nsteps (.) col_d   (or its transpose)
//
// with the argument conventions of kron.hip (KronArgs); the factors of block b are column-major at
//   st.ax + 1024 b: Ex (32 x 32)          st.ay + 64 b: Ey (8 x 8)
//
// Layout.  A wave owns two consecutive columns (h = 0, 1) and stacks their planes to Z[(h, y)][x], 16 x 32: two MFMA
// accumulator tiles t = 0, 1 (x = 16 t ..).  The y-contraction of both columns is one product with the block-diagonal
// Dy = diag(Ey, Ey), 16 x 16, so that no half of a v_mfma_f64_16x16x4_f64 tile idles: 4 MFMAs per tile, 8 for the two
// columns.  The x-contraction is Ex Z^T, 32 x 32 times 32 x 16: two output tiles of 8 MFMAs, 16 for the two columns.
// 12 MFMAs per column and step (dense: 64; the 16 x 16 form of kron.hip: 16).
// Two layouts alternate by step parity, with one transpose through LDS per step, as in kron.hip:
//   R (even steps start here; a load of one register is 16-double runs of a column):
//     register r of lane (g = lane >> 4, c = lane & 15) of tile t is Z[(h, y) = g + 4 r][x = 16 t + c]
//   C: register r of lane (g, c) of tile t is Z^T[x = 16 t + g + 4 r][(h, y) = c]
//   from R:  P = Dy Z (B operands: the registers), P -> LDS, Q^T = Ex P^T (B operands: LDS, transposed)  -> C
//   from C:  P^T = Ex Z^T (B operands: the registers), P^T -> LDS, Q = Dy P (B operands: LDS)             -> R
// (Ey and Ex act on different indices, so either order is the same product up to rounding.)  The LDS image of a wave is
// always [(h, y)][x] with a row stride of 36 doubles: the accesses with (h, y) on the 16-lane index and x on the 4-lane
// index (R's read, C's write) then put two lanes on every bank pair, the minimum for 64 eight-byte lanes; the other two
// (R's write, C's read) put up to four.  A workgroup (4 waves, 8 columns) owns its columns through all steps; the result is
// staged in LDS and stored as whole 64-byte runs, as is or transposed.
#include "factored_common.h"

namespace dqmc {

constexpr int RC_N = 256;
constexpr int RC_LX = 32, RC_LY = 8;
constexpr int RC_WAVES = 4;
constexpr int RC_COLS = 2 * RC_WAVES;             // columns per workgroup
constexpr int RC_TLD = 36;                        // row stride of a wave's transpose image [16][32] (doubles)
constexpr int RC_LDS_T = RC_WAVES * 16 * RC_TLD;
// transposed staging image [entry][column]: entry e, column cl at e RC_SLD + (e >> 4) RC_SPAD + cl (bilayer.hip's scheme)
constexpr int RC_SLD = 10, RC_SPAD = 2;
constexpr int RC_LDS_S = RC_N * RC_SLD + (RC_N / 16) * RC_SPAD;
constexpr int RC_LDS = RC_LDS_T > RC_LDS_S ? RC_LDS_T : RC_LDS_S;  // 20 736 bytes
static_assert(RC_LDS >= RC_COLS * RC_N, "the untransposed staging image [column][entry] reuses the LDS");
static_assert(RC_LX * RC_LY == RC_N && 2 * RC_LY == 16 && RC_LX == 32, "two columns of 8 rows fill a 16-row tile; x spans two tiles");

__global__ __launch_bounds__(256) void rect_chain_kernel(KronArgs a)
{
    __shared__ __attribute__((aligned(16))) double lds[RC_LDS];
    const int unit = blockIdx.x / (RC_N / RC_COLS), c0 = RC_COLS * (blockIdx.x % (RC_N / RC_COLS));
    if (unit >= a.n_units) return;
    const int wk = a.nb == 2 ? unit >> 1 : unit, blk = a.nb == 2 ? unit & 1 : 0;
    const bool bn = blk != 0;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, ci = lane & 15;
    const int cp = c0 + 2 * w;  // this wave's columns cp, cp + 1
    const long conf_off = (long)wk * a.conf_stride;
    double *tile = lds + w * (16 * RC_TLD);
    const double *x0u = a.X0 + (long)unit * a.x_su;

    // entry x + 32 y of register r of tile t of this lane, and the column h it belongs to, at layout par (0: R, 1: C)
    auto idx = [&](int par, int t, int r) {
        return par ? (16 * t + g + 4 * r) + RC_LX * (ci & 7) : (16 * t + ci) + RC_LX * (g + 4 * (r & 1));
    };
    auto col = [&](int par, int r) { return par ? ci >> 3 : r >> 1; };

    // X_0 in layout R
    d4 v[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[t][r] = x0u[(long)RC_N * (cp + (r >> 1)) + idx(0, t, r)];

    // the operands and the HS-field bytes of a step, requested one step ahead (a missing scaling reads X_0 and is not
    // applied), as in kron.hip.  A operands, row ci, k = 4 q + g:  dy[q] = Dy[ci][4 q + g] (zero off the diagonal blocks),
    // ex[t][q] = Ex[16 t + ci][4 q + g]
    struct Ops {
        double dy[4], ex[2][8];
        int8_t cpre[2][4], cpost[2][4];
    };
    auto request = [&](int s, Ops &o) {
        const KronStep &st = a.st[s];
        const int par = s & 1;
        const double *fx = st.ax + RC_LX * RC_LX * blk, *fy = st.ay + RC_LY * RC_LY * blk;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 4 * q + g;
            const double e = fy[(ci & 7) + RC_LY * (k & 7)];
            o.dy[q] = (ci >> 3) == (k >> 3) ? e : 0.0;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 8; ++q) o.ex[t][q] = fx[(16 * t + ci) + RC_LX * (4 * q + g)];
        const int8_t *dummy = reinterpret_cast<const int8_t *>(x0u);
        const int8_t *pre = st.pre_conf ? st.pre_conf + conf_off : dummy, *post = st.post_conf ? st.post_conf + conf_off : dummy;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o.cpre[t][r] = pre[st.pre_conf ? idx(par, t, r) : 0];
                o.cpost[t][r] = post[st.post_conf ? idx(par ^ 1, t, r) : 0];
            }
    };
    Ops cur, nxt;
    request(0, cur);
    double cs[2];  // final column scale (read from X_0 and not applied when there is none)
    {
        const double *cd = a.col_d ? a.col_d + (long)unit * a.col_stride + cp : x0u;
        cs[0] = cd[0];
        cs[1] = cd[1];
    }

    for (int s = 0; s < a.nsteps; ++s) {
        const KronStep &st = a.st[s];
        const int par = s & 1;
        if (st.pre_conf) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[t][r] *= fk_conf(cur.cpre[t][r], st.pre_sign, bn, a.epl, a.eml);
        }
        if (!par) {
            // P = Dy Z  ->  tile[(h, y)][x]
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                d4 p = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < 4; ++q) p = FK_MFMA(cur.dy[q], v[t][q], p);
#pragma unroll
                for (int r = 0; r < 4; ++r) tile[(g + 4 * r) * RC_TLD + 16 * t + ci] = p[r];
            }
        } else {
            // P^T = Ex Z^T  ->  tile[(h, y)][x]: the B operand of k-block q = 4 t' + q' is register q' of tile t'
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                d4 p = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < 8; ++q) p = FK_MFMA(cur.ex[t][q], v[q >> 2][q & 3], p);
#pragma unroll
                for (int r = 0; r < 4; ++r) tile[ci * RC_TLD + 16 * t + g + 4 * r] = p[r];
            }
        }
        request(min(s + 1, a.nsteps - 1), nxt);
        __syncthreads();
        if (!par) {
            // Q^T = Ex P^T: B operand of k-block q is P[(h, y) = ci][x = 4 q + g]  ->  layout C
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                d4 q4 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < 8; ++q) q4 = FK_MFMA(cur.ex[t][q], tile[ci * RC_TLD + 4 * q + g], q4);
                v[t] = q4;
            }
        } else {
            // Q = Dy P: B operand of k-block q is P[(h, y) = 4 q + g][x = 16 t + ci]  ->  layout R
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                d4 q4 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < 4; ++q) q4 = FK_MFMA(cur.dy[q], tile[(4 * q + g) * RC_TLD + 16 * t + ci], q4);
                v[t] = q4;
            }
        }
        __syncthreads();  // (the next step's tile writes, or the staging image, reuse the LDS)
        if (st.post_conf) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[t][r] *= fk_conf(cur.cpost[t][r], st.post_sign, bn, a.epl, a.eml);
        }
        cur = nxt;
    }
    // ---- staging image: transposed [entry][column] (see RC_SLD), else [column][entry] (the global image)
    const int par = a.nsteps & 1;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = idx(par, t, r), h = col(par, r), cl = 2 * w + h;
            const double val = a.col_d ? v[t][r] * (h ? cs[1] : cs[0]) : v[t][r];
            lds[a.transpose_out ? e * RC_SLD + (e >> 4) * RC_SPAD + cl : cl * RC_N + e] = val;
        }
    __syncthreads();
    fk_store_image<RC_N, RC_COLS, RC_SLD, RC_SPAD>(a.out + (long)unit * a.out_su, lds, a, c0, tid);
}

hipError_t launch_rect_chain(const KronArgs &a, hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    if (a.nsteps < 1 || a.nsteps > SLAB_MAX_STEPS || a.nb < 1 || a.nb > 2 || a.n_units < 1) return hipErrorInvalidValue;
    if (a.x_su < (long)RC_N * RC_N || a.out_su < (long)RC_N * RC_N || a.pf_img) return hipErrorInvalidValue;
    return fk_launch(rect_chain_kernel, dim3(a.n_units * (RC_N / RC_COLS)), a, s, start, stop);
}

}  // namespace dqmc
