// kron3.hip — slice-matrix chains and wraps with the hopping exponential applied in three-factor Kronecker form (n = 512).
//
// On the periodic 8 x 8 x 8 CubicLattice (site i = x + 8 y + 64 z) every hopping exponential is, up to rounding, a
// Kronecker product A = Ez (x) Ey (x) Ex of three 8 x 8 matrices (hopping_forms.h: kron_split checks it at handle creation).
// The kernel groups it as A = Ez (x) Exy with Exy = Ey (x) Ex (64 x 64, multiplied out on the host).  A column v of 512
// entries, read as the 64 x 8 matrix V[i][z] = v[i + 64 z] (i = x + 8 y), then gives (A v) = vec(Exy V Ez^T): a
// 64-contraction and an 8-contraction, 40 v_mfma_f64_16x16x4_f64 per column instead of the 256 of the dense product
// (DESIGN 4.6 has the count and why this grouping).
//
//   X_s = post_s (.) ( A_s * ( pre_s (.) X_{s-1} ) ),  s = 1 .. nsteps,    out = X_nsteps (.) col_d   (or its transpose)
//
// with the argument conventions of kron.hip (KronArgs), except that the factor pointers are operand images:
//   st.ax + 4096 b: Exy of block b as the A operands of the 64-contraction, [mp][m][r][lane] =
//                   Exy[16 mp + (lane & 15)][16 m + 4 r + (lane >> 4)]
//   st.ay + 256 b:  I2 (x) Ez (16 x 16 block diagonal) as the A operands of the 8-contraction, [q][lane] =
//                   (I2 (x) Ez)[lane & 15][4 q + (lane >> 4)]
//
// Layout.  A wave owns two consecutive columns (h = 0, 1) as the 64 x 16 matrix W[i][8 h + z], held in four MFMA
// accumulator tiles m = 0..3 (rows 16 m .. 16 m + 15 of i).  Two states, lane (g = lane >> 4, c = lane & 15), register r:
//   state I: tile m register r = W[i = 16 m + g + 4 r][8 h + z = c]        (i in the registers, (h, z) on the lanes)
//   state Z: tile m register r = W[i = 16 m + c][8 h + z = g + 4 r]        ((h, z) in the registers, i on the lanes)
// A product that sums over the register index takes the tiles as its B operands with no data movement: Exy W in state I
// (4 output tiles x 16 k-steps = 64 MFMAs per pair, A operands read from LDS), (I2 (x) Ez) W^T in state Z (4 tiles x 4
// k-steps = 16 MFMAs per pair).  Between them the pair goes once through a 16 x 65 LDS tile of its wave, so each step is one
// transpose and the state alternates: a step starts in Z when it is even (the first load reads 128 consecutive bytes per
// 16 lanes) and in I when it is odd.  A workgroup (4 waves, 8 columns) owns its columns through all steps; the result is
// staged in LDS and stored as whole lines, as is or transposed.
#include "factored_common.h"

namespace dqmc {

constexpr int K3_N = 512;
constexpr int K3_WAVES = 4;
constexpr int K3_COLS = 2 * K3_WAVES;            // columns per workgroup
constexpr int K3_TLD = 65;                       // row stride of a transpose tile (doubles)
constexpr int K3_T = 16 * K3_TLD;                // transpose tile of one wave
constexpr int K3_XY = 4096;                      // Exy operand image
constexpr int K3_EZ = 256;                       // I2 (x) Ez operand image
constexpr int K3_LDS = K3_XY + K3_WAVES * K3_T;  // 66 KB: two workgroups per CU
static_assert(K3_LDS >= K3_COLS * K3_N, "the staging image of the result reuses the LDS");

__global__ __launch_bounds__(256) void kron3_chain_kernel(KronArgs a)
{
    __shared__ __attribute__((aligned(16))) double lds[K3_LDS];
    const int unit = blockIdx.x / (K3_N / K3_COLS), c0 = K3_COLS * (blockIdx.x % (K3_N / K3_COLS));
    if (unit >= a.n_units) return;
    const int wk = a.nb == 2 ? unit >> 1 : unit, blk = a.nb == 2 ? unit & 1 : 0;
    const bool bn = blk != 0;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, ci = lane & 15;
    const int cp = c0 + 2 * w;  // this wave's columns cp, cp + 1
    const long conf_off = (long)wk * a.conf_stride;
    double *exy = lds, *tile = lds + K3_XY + w * K3_T;

    // entry index (0 .. 511) of tile m register r in state st (0: Z, 1: I), and the column (0, 1) it belongs to
    auto eidx = [&](int st, int m, int r) { return st ? 16 * m + g + 4 * r + 64 * (ci & 7) : 16 * m + ci + 64 * (g + 4 * (r & 1)); };
    auto hcol = [&](int st, int r) { return st ? ci >> 3 : r >> 1; };

    // X_0 in state Z: for one (m, r) the 64 lanes read 4 runs of 16 consecutive doubles
    d4 v[4];
    {
        const double *x0 = a.X0 + (long)unit * a.x_su + (long)K3_N * cp;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[m][r] = x0[K3_N * hcol(0, r) + eidx(0, m, r)];
    }
    // the Ez operands and the HS-field bytes of a step, requested one step ahead (a missing scaling reads X_0 and is not
    // applied), as in kron.hip
    struct Ops {
        double ez[4];
        int8_t cpre[16], cpost[16];
    };
    auto request = [&](int s, Ops &o) {
        const KronStep &st = a.st[s];
        const int par = s & 1;
        const double *fz = st.ay + (long)K3_EZ * blk;
#pragma unroll
        for (int q = 0; q < 4; ++q) o.ez[q] = fz[64 * q + lane];
        const int8_t *dummy = reinterpret_cast<const int8_t *>(a.X0);
        const int8_t *pre = st.pre_conf ? st.pre_conf + conf_off : dummy, *post = st.post_conf ? st.post_conf + conf_off : dummy;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o.cpre[4 * m + r] = pre[st.pre_conf ? eidx(par, m, r) : 0];
                o.cpost[4 * m + r] = post[st.post_conf ? eidx(par ^ 1, m, r) : 0];
            }
    };
    auto scale = [&](const int8_t *cb, int sign) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[m][r] *= fk_conf(cb[4 * m + r], sign, bn, a.epl, a.eml);
    };
    // state Z -> Z: W <- (I2 (x) Ez) W, tile by tile
    auto contract_z = [&](const Ops &o) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            d4 q4 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) q4 = FK_MFMA(o.ez[q], v[m][q], q4);
            v[m] = q4;
        }
    };
    // state I -> I: W <- Exy W, k-step (m, r) is register r of tile m
    auto contract_i = [&]() {
        d4 p[4];
#pragma unroll
        for (int mp = 0; mp < 4; ++mp) p[mp] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int mp = 0; mp < 4; ++mp) p[mp] = FK_MFMA(exy[((mp * 4 + m) * 4 + r) * 64 + lane], v[m][r], p[mp]);
#pragma unroll
        for (int m = 0; m < 4; ++m) v[m] = p[m];
    };
    // through this wave's tile T[8 h + z][i] (row stride K3_TLD); from state st to state st ^ 1
    auto transpose = [&](int st) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                tile[st ? ci * K3_TLD + 16 * m + g + 4 * r : (g + 4 * r) * K3_TLD + 16 * m + ci] = v[m][r];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                v[m][r] = tile[st ? (g + 4 * r) * K3_TLD + 16 * m + ci : ci * K3_TLD + 16 * m + g + 4 * r];
        __syncthreads();  // (the next transpose, or the staging image, rewrites the tile)
    };

    Ops cur, nxt;
    request(0, cur);
    double cs[2];  // final column scale (read from X_0 and not applied when there is none)
    {
        const double *cd = a.col_d ? a.col_d + (long)unit * a.col_stride + cp : a.X0;
        cs[0] = cd[0];
        cs[1] = cd[1];
    }

    for (int s = 0; s < a.nsteps; ++s) {
        const KronStep &st = a.st[s];
        if (s == 0 || st.ax != a.st[s - 1].ax) {  // Exy operand image of this step into the LDS
            const double *src = st.ax + (long)K3_XY * blk;
#pragma unroll
            for (int k = 0; k < K3_XY / 512; ++k) {
                const int e = 2 * (tid + 256 * k);
                *reinterpret_cast<double2 *>(exy + e) = *reinterpret_cast<const double2 *>(src + e);
            }
            __syncthreads();
        }
        const int par = s & 1;
        if (st.pre_conf) scale(cur.cpre, st.pre_sign);
        if (par == 0) {
            contract_z(cur);
            request(min(s + 1, a.nsteps - 1), nxt);
            transpose(0);
            contract_i();
        } else {
            contract_i();
            request(min(s + 1, a.nsteps - 1), nxt);
            transpose(1);
            contract_z(cur);
        }
        if (st.post_conf) scale(cur.cpost, st.post_sign);
        cur = nxt;
        if (s + 1 < a.nsteps && a.st[s + 1].ax != st.ax) __syncthreads();  // every wave is done with this Exy image
    }
    // ---- staging image: transposed [entry][column] (row stride K3_COLS), else [column][entry] (the global image)
    const int fin = a.nsteps & 1;  // 1: the last step ended in state I
    __syncthreads();               // (the image overwrites the Exy operands)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = eidx(fin, m, r), h = hcol(fin, r), cl = 2 * w + h;
            const double val = a.col_d ? v[m][r] * (h ? cs[1] : cs[0]) : v[m][r];
            lds[a.transpose_out ? e * K3_COLS + cl : cl * K3_N + e] = val;
        }
    __syncthreads();
    fk_store_image<K3_N, K3_COLS, K3_COLS, 0>(a.out + (long)unit * a.out_su, lds, a, c0, tid);
}

hipError_t launch_kron3_chain(const KronArgs &a, hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    if (a.nsteps < 1 || a.nsteps > SLAB_MAX_STEPS || a.nb < 1 || a.nb > 2) return hipErrorInvalidValue;
    return fk_launch(kron3_chain_kernel, dim3(a.n_units * (K3_N / K3_COLS)), a, s, start, stop);
}

}  // namespace dqmc
