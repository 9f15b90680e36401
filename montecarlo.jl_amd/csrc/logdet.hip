// logdet.hip — log|det| and sign of I + B_M ... B_1 per unit, and the device side of the DQMC global moves
// (include/dqmc_hip.h: dqmc_logdet, dqmc_global_move).
//
// calculate_greens_AVX! (stack.jl:337-393) writes G^-1 = (Ul U1) A2 (T1 Ur'), A2 being the matrix its second
// udt_AVX_pivot! factors (:368-376).  U1 and Ul are orthogonal, T1 = D1^-1 R1 P1' has a triangular diagonal of +-1
// (UDT.jl:270-277), so
//     log|det G^-1| = log|det A2| = sum_i log D2_i                      (D2 = |diag R2|, the Dr of that second UDT)
//     sign det G^-1 = sign det(Ul Dl Tl) sign det(Ur Dr Tr) sign det A2 = sign det A2,
// the first two being +1: both are products of B_l = eT2 eV(l), exp of a symmetric matrix times a positive diagonal.
// logdet_kernel takes D2 from the engine's UDT and the sign of det A2 from an LU with partial pivoting of a copy of A2,
// of which only the parity of the row exchanges and the signs of the pivots are kept.  One workgroup per unit; every sum
// and every pivot choice is taken in a fixed order, so a unit's result does not depend on the batch it is computed in.
// No MFMA: the LU is n^3 / 3 multiply-adds once per logdet, against the ~2 n^3 M of the slice chain in front of it.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dqmc {

constexpr int LD_THREADS = 256;
constexpr int LD_WAVES = LD_THREADS / 64;
constexpr int LD_LDS_N = 64;  // up to this size the copy of A2 is eliminated in LDS (32 KiB), above it in place in memory

// sign of det A (n x n, column-major, leading dimension ld; overwritten): Gaussian elimination with partial pivoting, the
// pivot of column k being the entry of largest magnitude on or below the diagonal, the lowest row among equals.  The
// multipliers are not stored: only the trailing block is updated.  Returns 0 for a zero or non-finite pivot.  Every
// thread of the workgroup returns the same value.
__device__ int lu_sign(double *A, int n, int ld, double *red_v, int *red_i)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int sgn = 1;
    for (int k = 0; k < n; ++k) {
        // pivot search down column k
        double bv = -1.0;
        int bi = n;
        for (int i = k + t; i < n; i += LD_THREADS) {
            const double v = fabs(A[i + (long)ld * k]);
            if (v > bv) { bv = v; bi = i; }  // (ascending i within a thread: the first of equals is kept)
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_down(bv, off, 64);
            const int oi = __shfl_down(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
        __syncthreads();
        bv = red_v[0]; bi = red_i[0];
#pragma unroll
        for (int w = 1; w < LD_WAVES; ++w) {
            const double ov = red_v[w];
            const int oi = red_i[w];
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (!(bv > 0.0) || !(bv < INFINITY) || bi >= n) return 0;  // singular, NaN or Inf (uniform over the workgroup)
        const double piv = A[bi + (long)ld * k];  // read before the exchange below; the barrier after it orders the two
        if (piv < 0.0) sgn = -sgn;
        if (bi != k) sgn = -sgn;
        __syncthreads();
        if (k == n - 1) break;
        // row exchange k <-> bi over the columns that are still read (j > k), then the trailing update
        if (bi != k) {
            for (int j = k + 1 + t; j < n; j += LD_THREADS) {
                const double a = A[k + (long)ld * j], b = A[bi + (long)ld * j];
                A[k + (long)ld * j] = b;
                A[bi + (long)ld * j] = a;
            }
            // column k itself: only its entries below the diagonal are read again (as multipliers); put the old row k's
            // entry where the pivot was
            if (t == 0) A[bi + (long)ld * k] = A[k + (long)ld * k];
            __syncthreads();
        }
        const double rinv = 1.0 / piv;
        for (int j = k + 1 + wave; j < n; j += LD_WAVES) {
            const double akj = A[k + (long)ld * j];
            for (int i = k + 1 + lane; i < n; i += 64)
                A[i + (long)ld * j] -= (A[i + (long)ld * k] * rinv) * akj;
        }
        __syncthreads();
    }
    return sgn;
}

// one workgroup per unit: logabsdet[u] = sum_i log D2[u][i] (fixed order: thread t takes i = t, t + 256, ..., then a
// butterfly-free tree over the lanes and the waves in index order), sign[u] = sign det A2[u] (A2 is destroyed)
__global__ __launch_bounds__(LD_THREADS) void logdet_kernel(int n, double *__restrict__ A2, long strideA,
                                                            const double *__restrict__ D2, long strideD,
                                                            double *__restrict__ logabsdet, int *__restrict__ sign)
{
    __shared__ double lds_A[LD_LDS_N * LD_LDS_N];
    __shared__ double red_v[LD_WAVES];
    __shared__ int red_i[LD_WAVES];
    const int u = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double *d = D2 + (long)u * strideD;
    double s = 0.0;
    for (int i = t; i < n; i += LD_THREADS) s += log(d[i]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) red_v[wave] = s;
    __syncthreads();
    if (t == 0) {
        double tot = red_v[0];
#pragma unroll
        for (int w = 1; w < LD_WAVES; ++w) tot += red_v[w];
        logabsdet[u] = tot;
    }
    __syncthreads();  // red_v is used again by lu_sign
    double *A = A2 + (long)u * strideA;
    int ld = n;
    if (n <= LD_LDS_N) {
        for (int e = t; e < n * n; e += LD_THREADS) lds_A[e] = A[e];
        __syncthreads();
        A = lds_A;
    }
    const int sg = lu_sign(A, n, ld, red_v, red_i);
    if (t == 0) sign[u] = sg;
}

hipError_t launch_logdet(int n, int n_units, double *A2, long strideA, const double *D2, long strideD, double *logabsdet,
                         int *sign, hipStream_t s)
{
    if (n < 1 || n_units < 1 || strideA < (long)n * n || strideD < n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(logdet_kernel, dim3(n_units), dim3(LD_THREADS), 0, s, n, A2, strideA, D2, strideD, logabsdet, sign);
    return hipGetLastError();
}

// ---- global moves ---------------------------------------------------------------------------------------------------
// u(m, t) of a walker: the host stream in dqmc_set_uniforms mode (2.0 = exhausted: never accepted), else Philox4x32-10
// with counter words (t, low32(m), 1, high32(m)) - the local stream has words 2 and 3 zero
__device__ __forceinline__ double gm_uniform(WalkerRng &r, unsigned long long m, unsigned int t)
{
    if (r.uniforms) {
        if (r.draw >= r.n_uniforms) { r.exhausted = 1; return 2.0; }
        return r.uniforms[r.draw++];
    }
    return philox4_uniform(r.seed, t, (unsigned int)m, 1u, (unsigned int)(m >> 32));
}

// the flip of one walker's field: every entry (FLIP_ALL) or the time line of `site`; an involution, so a rejected
// proposal is taken back by applying it again.  Returns this thread's part of the sum of the entries before the flip.
__device__ __forceinline__ long gm_flip(int8_t *conf, int N, int M, int kind, int site)
{
    long s = 0;
    if (kind == 0) {
        for (long e = threadIdx.x; e < (long)N * M; e += LD_THREADS) {
            const int8_t c = conf[e];
            s += c;
            conf[e] = (int8_t)-c;
        }
    } else {
        for (int l = threadIdx.x; l < M; l += LD_THREADS) {
            const int8_t c = conf[site + (long)N * l];
            s += c;
            conf[site + (long)N * l] = (int8_t)-c;
        }
    }
    return s;
}

// proposal: one workgroup per walker.  walker < 0: every walker, else that one; the others are marked inactive.
// dS = sum(conf) - sum(conf') = 2 x the sum of the flipped entries before the flip (an exact integer).
__global__ __launch_bounds__(LD_THREADS) void gm_propose_kernel(int N, int M, int kind, int walker, int8_t *conf,
                                                                WalkerRng *rng, GlobalMoveState *gm)
{
    __shared__ int sh_site;
    __shared__ long sh_sum[LD_WAVES];
    const int w = blockIdx.x, t = threadIdx.x;
    if (walker >= 0 && walker != w) {
        if (t == 0) gm[w].active = 0;
        return;
    }
    if (t == 0) {
        int site = 0;
        if (kind == 1) {
            WalkerRng r = rng[w];
            const double u = gm_uniform(r, gm[w].moves_drawn, 0u);
            rng[w] = r;
            site = (int)floor(u * (double)N);
            site = site < 0 ? 0 : (site > N - 1 ? N - 1 : site);  // (u = 2.0 of an exhausted stream lands on N - 1)
        }
        sh_site = site;
    }
    __syncthreads();
    long s = gm_flip(conf + (long)w * N * M, N, M, kind, sh_site);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
    if ((t & 63) == 0) sh_sum[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
        long tot = 0;
        for (int v = 0; v < LD_WAVES; ++v) tot += sh_sum[v];
        gm[w].active = 1;
        gm[w].site = sh_site;
        gm[w].dS = 2 * tot;
    }
}

// decision: one workgroup per walker.  lad / sg: logabsdet and sign per unit of the field before (cur) and after (prop)
// the flip.  Attractive (HubbardModelAttractive.jl:113-127): p = exp(lambda dS + 2 (lad' - lad)); repulsive
// (HubbardModelRepulsive.jl:128-156): p = prod of the four signs x exp(sum_b (lad'_b - lad_b)).  Accept iff p > 1 ||
// u < p, u drawn only when p <= 1 (DQMC.jl:573); a negative p is counted like a local one (DQMC.jl:562-563).  Accepted:
// cur <- prop; rejected: the flip is taken back.
__global__ __launch_bounds__(LD_THREADS) void gm_decide_kernel(int N, int M, int nb, int kind, double lambda,
                                                               int check_sign, int8_t *conf, WalkerRng *rng,
                                                               GlobalMoveState *gm, DevStats *stats, double *lad_cur,
                                                               int *sg_cur, const double *lad_prop, const int *sg_prop)
{
    __shared__ int sh_accept;
    const int w = blockIdx.x, t = threadIdx.x;
    if (!gm[w].active) return;
    if (t == 0) {
        double p;
        if (nb == 1) {
            p = exp(lambda * (double)gm[w].dS + 2.0 * (lad_prop[w] - lad_cur[w]));
            if (sg_prop[w] == 0 || sg_cur[w] == 0) p = __builtin_nan("");
        } else {
            const int sp = sg_prop[2 * w] * sg_prop[2 * w + 1] * sg_cur[2 * w] * sg_cur[2 * w + 1];
            p = (double)sp * exp((lad_prop[2 * w] - lad_cur[2 * w]) + (lad_prop[2 * w + 1] - lad_cur[2 * w + 1]));
            if (sp == 0) p = __builtin_nan("");
        }
        if (check_sign && p < 0.0) magstats_push(stats[w].negative_probability, p);
        int acc = p > 1.0;
        if (!acc && p == p) {  // (a NaN weight - singular A2 - draws nothing and is rejected)
            WalkerRng r = rng[w];
            const double u = gm_uniform(r, gm[w].moves_drawn, 1u);
            rng[w] = r;
            acc = u < p;
        }
        gm[w].moves_drawn += 1;
        gm[w].prop_global += 1;
        gm[w].acc_global += acc;
        gm[w].last_p = p;
        gm[w].last_accepted = acc;
        if (acc)
            for (int b = 0; b < nb; ++b) {
                lad_cur[nb * w + b] = lad_prop[nb * w + b];
                sg_cur[nb * w + b] = sg_prop[nb * w + b];
            }
        sh_accept = acc;
    }
    __syncthreads();
    if (!sh_accept) (void)gm_flip(conf + (long)w * N * M, N, M, kind, gm[w].site);
}

hipError_t launch_gm_propose(int N, int M, int n_walkers, int kind, int walker, int8_t *conf, WalkerRng *rng,
                             GlobalMoveState *gm, hipStream_t s)
{
    if (kind != 0 && kind != 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gm_propose_kernel, dim3(n_walkers), dim3(LD_THREADS), 0, s, N, M, kind, walker, conf, rng, gm);
    return hipGetLastError();
}

hipError_t launch_gm_decide(int N, int M, int nb, int n_walkers, int kind, double lambda, int check_sign, int8_t *conf,
                            WalkerRng *rng, GlobalMoveState *gm, DevStats *stats, double *lad_cur, int *sg_cur,
                            const double *lad_prop, const int *sg_prop, hipStream_t s)
{
    hipLaunchKernelGGL(gm_decide_kernel, dim3(n_walkers), dim3(LD_THREADS), 0, s, N, M, nb, kind, lambda, check_sign, conf,
                       rng, gm, stats, lad_cur, sg_cur, lad_prop, sg_prop);
    return hipGetLastError();
}

}  // namespace dqmc
