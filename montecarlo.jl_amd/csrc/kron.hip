// kron.hip — slice-matrix chains and wraps with the hopping exponential applied in Kronecker-factored form (n = 256).
//
// On the periodic 16 x 16 SquareLattice (site i = x + 16 y) every hopping exponential is, up to rounding, a Kronecker
// product A = Ay (x) Ax of two 16 x 16 matrices (engine.cpp: kron_factor checks it at handle creation).  A column v of
// 256 entries, read as the 16 x 16 matrix V[x][y] = v[x + 16 y], then gives (A v) = vec(Ax V Ay^T): two 16-contractions,
// 8 v_mfma_f64_16x16x4_f64 per column instead of the 64 of the dense product.
//
//   X_s = post_s (.) ( A_s * ( pre_s (.) X_{s-1} ) ),  s = 1 .. nsteps,    out = X_nsteps (.) col_d   (or its transpose)
//
// with the argument conventions and scaling placement of slab.hip.  Used for
//   * add_slice_sequence_left/right (stack.jl:272-311): the safe_mult products B_l X / B_l' X;
//   * wrap_greens! (stack.jl:491-500) as two one-step launches with transposed stores (engine.cpp: wrap_greens_kron).
//
// Layout.  A wave holds a column as one MFMA accumulator tile (4 doubles per lane): register r of lane (g = lane >> 4,
// c = lane & 15) is V[a = g + 4 r][b = c], where (a, b) = (y, x) or (x, y) by step parity.  Register q of that tile is
// also the B operand of k-block q of a product that sums over a, so P = Fa V needs no data movement; P^T goes through
// LDS once (a 16 x 17 tile per column), and Q = Fb P^T leaves the tile with its roles swapped.  So each step is one
// transpose, and the parity alternates: (y, x) at the start, where a load of one register is 64 consecutive doubles.
// Columns are independent: a workgroup (4 waves x KR_NC columns) owns 16 consecutive columns through all steps, and
// nothing crosses workgroups.  The result is staged in LDS and stored as whole 128-byte lines, as is or transposed.
#include "kernels.h"
#include <hip/hip_ext.h>

namespace dqmc {

typedef double d4k __attribute__((ext_vector_type(4)));
#define KR_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

constexpr int KR_N = 256;
constexpr int KR_NC = 4;                 // columns per wave
constexpr int KR_COLS = 4 * KR_NC;       // columns per workgroup
constexpr int KR_TLD = 17;               // row stride of a transpose tile (doubles)
constexpr int KR_SLD = 18;               // row stride of the transposed staging image (doubles; even: 16-byte reads)
constexpr int KR_LDS_T = 4 * KR_NC * 16 * KR_TLD;  // transpose tiles of the four waves
constexpr int KR_LDS_S = KR_N * KR_SLD;            // staging image of the result (>= KR_COLS * KR_N)
constexpr int KR_LDS = KR_LDS_T > KR_LDS_S ? KR_LDS_T : KR_LDS_S;

// exp(sign lambda conf[i]) of block blk (vs_conf() of engine.cpp, slab_conf_val() of slab.hip)
__device__ __forceinline__ double kr_conf(int8_t c, int sign, bool bn, double epl, double eml)
{
    return (((c > 0) == (sign > 0)) != bn) ? epl : eml;
}

__global__ __launch_bounds__(256) void kron_chain_kernel(KronArgs a)
{
    __shared__ __attribute__((aligned(16))) double lds[KR_LDS];
    const int unit = blockIdx.x / (KR_N / KR_COLS), c0 = KR_COLS * (blockIdx.x % (KR_N / KR_COLS));
    if (unit >= a.n_units) return;
    const int wk = a.nb == 2 ? unit >> 1 : unit, blk = a.nb == 2 ? unit & 1 : 0;
    const bool bn = blk != 0;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, ci = lane & 15;
    const long conf_off = (long)wk * a.conf_stride;
    double *tile = lds + w * (KR_NC * 16 * KR_TLD);

    // X_0: column c0 + KR_NC w + t, parity (y, x): register r = entries ci + 16 (g + 4 r), 64 consecutive doubles
    d4k v[KR_NC];
    {
        const double *x0 = a.X0 + (long)unit * a.x_su + (long)KR_N * (c0 + KR_NC * w) + ci + 16 * g;
#pragma unroll
        for (int t = 0; t < KR_NC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[t][r] = x0[KR_N * t + 64 * r];
    }
    // entry index of register r of this lane at parity par (0: a = y, b = x; 1: a = x, b = y)
    auto idx = [&](int par, int r) { return par ? (g + 4 * r) + 16 * ci : ci + 16 * (g + 4 * r); };
    // Everything a step needs from memory besides its column tiles - A operands (lane: F[row ci][k = 4 q + g] of the
    // column-major 16 x 16 factor; fa sums over a, fb over b) and the HS-field bytes of its two scalings - is requested one
    // step ahead, behind the step before's MFMAs, and without a branch (a missing scaling reads X_0 and is not applied):
    // requested at the top of each step, each was a full trip to the L2 in front of the first product.
    struct Ops {
        double av[4], bv[4];
        int8_t cpre[4], cpost[4];
    };
    auto request = [&](int s, Ops &o) {
        const KronStep &st = a.st[s];
        const int par = s & 1;
        const double *fx = st.ax + KR_N * blk, *fy = st.ay + KR_N * blk;
        const double *fa = par ? fx : fy, *fb = par ? fy : fx;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o.av[q] = fa[ci + 16 * (4 * q + g)];
            o.bv[q] = fb[ci + 16 * (4 * q + g)];
        }
        const int8_t *dummy = reinterpret_cast<const int8_t *>(a.X0);
        const int8_t *pre = st.pre_conf ? st.pre_conf + conf_off : dummy, *post = st.post_conf ? st.post_conf + conf_off : dummy;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o.cpre[r] = pre[st.pre_conf ? idx(par, r) : 0];
            o.cpost[r] = post[st.post_conf ? idx(par ^ 1, r) : 0];
        }
    };
    Ops cur, nxt;
    request(0, cur);
    double cs[KR_NC];  // final column scale (read from X_0 and not applied when there is none)
    {
        const double *cd = a.col_d ? a.col_d + (long)unit * a.col_stride + c0 + KR_NC * w : a.X0;
#pragma unroll
        for (int t = 0; t < KR_NC; ++t) cs[t] = cd[t];
    }

    for (int s = 0; s < a.nsteps; ++s) {
        const KronStep &st = a.st[s];
        if (st.pre_conf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double f = kr_conf(cur.cpre[r], st.pre_sign, bn, a.epl, a.eml);
#pragma unroll
                for (int t = 0; t < KR_NC; ++t) v[t][r] *= f;
            }
        }
        // P = Fa V  ->  tile[a][b]
#pragma unroll
        for (int t = 0; t < KR_NC; ++t) {
            d4k p = (d4k){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) p = KR_MFMA(cur.av[q], v[t][q], p);
#pragma unroll
            for (int r = 0; r < 4; ++r) tile[t * 16 * KR_TLD + (g + 4 * r) * KR_TLD + ci] = p[r];
        }
        request(min(s + 1, a.nsteps - 1), nxt);
        __syncthreads();
        // Q = Fb P^T: B operand of k-block q is P[a = ci][b = 4 q + g]; the result has b in the registers, a on the lanes
#pragma unroll
        for (int t = 0; t < KR_NC; ++t) {
            d4k q4 = (d4k){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) q4 = KR_MFMA(cur.bv[q], tile[t * 16 * KR_TLD + ci * KR_TLD + 4 * q + g], q4);
            v[t] = q4;
        }
        __syncthreads();  // (the next step's tile writes, or the staging image, reuse the LDS)
        if (st.post_conf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double f = kr_conf(cur.cpost[r], st.post_sign, bn, a.epl, a.eml);
#pragma unroll
                for (int t = 0; t < KR_NC; ++t) v[t][r] *= f;
            }
        }
        cur = nxt;
    }
    // ---- staging image: transposed [entry][column] (row stride KR_SLD), else [column][entry] (the global image)
    const int par = a.nsteps & 1;
#pragma unroll
    for (int t = 0; t < KR_NC; ++t) {
        const int cl = KR_NC * w + t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = idx(par, r);
            lds[a.transpose_out ? i * KR_SLD + cl : cl * KR_N + i] = a.col_d ? v[t][r] * cs[t] : v[t][r];
        }
    }
    __syncthreads();
    double *o = a.out + (long)unit * a.out_su;
    if (a.transpose_out) {  // out[c][i] = X[i][c]: row i of the image is 16 consecutive doubles at c0 + 256 i
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = 2 * (tid + 256 * k), i = e >> 4, cl = e & 15;
            *reinterpret_cast<double2 *>(o + c0 + (long)KR_N * i + cl) = *reinterpret_cast<const double2 *>(lds + i * KR_SLD + cl);
        }
    } else {  // columns c0 .. c0 + 15 are 4096 consecutive doubles
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = 2 * (tid + 256 * k);
            *reinterpret_cast<double2 *>(o + (long)KR_N * c0 + e) = *reinterpret_cast<const double2 *>(lds + e);
        }
    }
}

hipError_t launch_kron_chain(const KronArgs &a, hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    if (a.nsteps < 1 || a.nsteps > SLAB_MAX_STEPS || a.nb < 1 || a.nb > 2) return hipErrorInvalidValue;
    const dim3 grid(a.n_units * (KR_N / KR_COLS)), block(256);
    if (start) hipExtLaunchKernelGGL(kron_chain_kernel, grid, block, 0, s, start, stop, 0, a);
    else hipLaunchKernelGGL(kron_chain_kernel, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace dqmc
