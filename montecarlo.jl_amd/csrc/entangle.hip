// entangle.hip — Renyi-2 entanglement entropy from walker pairs (include/dqmc_hip.h "entanglement"): Grover's estimator
// (T. Grover, PRL 111, 130402).  The reference, a single-chain code, has no such measurement.  For a subsystem A of N_A
// sites and two walkers w < w' the sample is
//     x(w, w') = prod_b det M_b,   M_b = I - G_A - G_A' + 2 G_A G_A'      (squared for the one block of the attractive model)
// with G_A the true equal-time G of block b restricted to A.
//
// Three kernels per measurement point:
//   ent_gather_kernel   G_A of every (subsystem, walker, block) out of the n x n true G into two compact column-major
//                       N_A x N_A images, G_A and its transpose, so that both MFMA operands of the pair kernel are read
//                       along their contiguous direction and the site-list indirection is paid W times, not W^2 times
//   ent_pair_kernel     one workgroup of 256 threads per (pair, block) of one subsystem: M in LDS from v_mfma_f64_16x16x4
//                       tiles (operands straight from the images, which the L2 holds; I - G - G' is the accumulators'
//                       initial value and the A operand carries the factor 2), then Gaussian elimination of M in LDS
//                       with the pivot rule of lu_sign (logdet.hip: largest magnitude, lowest row among equals), keeping
//                       sum log|pivot| and the sign
//   ent_combine_kernel  x = sign exp(sum), the sample [W][W] (strictly upper triangle) and the sums
// LDS: M has the leading dimension NP + 1, NP = N_A rounded up to 16 (an odd stride in doubles: the row exchange of the
// elimination walks along a row).  N_A <= 64 takes the static 32.5 KiB form, four workgroups to a CU; above it the image
// is dynamic, 129 KiB at N_A = 128 of the CU's 160 KiB.  Tile edges: operand and initial-value loads beyond N_A are
// clamped to a valid address and replaced by zero, the elimination runs over the N_A x N_A corner only.
// Every sum and every pivot choice is taken in a fixed order: x(w, w') depends on the two walkers' G alone.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dqmc {

namespace {
typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int EN_THREADS = 256;
constexpr int EN_WAVES = EN_THREADS / 64;
constexpr int EN_STATIC_N = 64;                                   // up to this N_A the LDS image is static
constexpr int EN_STATIC_DOUBLES = EN_STATIC_N * (EN_STATIC_N + 1);
constexpr int EN_TJ = 4;                                          // column tiles per work item: one A operand serves four MFMAs

__host__ __device__ inline int en_pad(int na) { return (na + 15) / 16 * 16; }

// lu_sign of logdet.hip with the log of the pivots kept as well: A (n x n, column-major, leading dimension ld) is
// overwritten; *logabs = sum_k log|pivot_k|, k ascending.  Returns the sign of det A, 0 for a zero or non-finite pivot.
// Every thread of the workgroup returns the same values.
__device__ int en_lu_logdet(double *A, int n, int ld, double *red_v, int *red_i, double *logabs)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int sgn = 1;
    double ls = 0.0;
    for (int k = 0; k < n; ++k) {
        // pivot search down column k
        double bv = -1.0;
        int bi = n;
        for (int i = k + t; i < n; i += EN_THREADS) {
            const double v = fabs(A[i + ld * k]);
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
        for (int w = 1; w < EN_WAVES; ++w) {
            const double ov = red_v[w];
            const int oi = red_i[w];
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (!(bv > 0.0) || !(bv < INFINITY) || bi >= n) { *logabs = 0.0; return 0; }  // singular, NaN or Inf (uniform)
        const double piv = A[bi + ld * k];  // read before the exchange below; the barrier after it orders the two
        if (piv < 0.0) sgn = -sgn;
        if (bi != k) sgn = -sgn;
        ls += log(bv);
        __syncthreads();
        if (k == n - 1) break;
        // row exchange k <-> bi over the columns that are still read (j > k), then the trailing update
        if (bi != k) {
            for (int j = k + 1 + t; j < n; j += EN_THREADS) {
                const double a = A[k + ld * j], b = A[bi + ld * j];
                A[k + ld * j] = b;
                A[bi + ld * j] = a;
            }
            // column k itself: only its entries below the diagonal are read again (as multipliers)
            if (t == 0) A[bi + ld * k] = A[k + ld * k];
            __syncthreads();
        }
        const double rinv = 1.0 / piv;
        for (int j = k + 1 + wave; j < n; j += EN_WAVES) {
            const double akj = A[k + ld * j];
            for (int i = k + 1 + lane; i < n; i += 64)
                A[i + ld * j] -= (A[i + ld * k] * rinv) * akj;
        }
        __syncthreads();
    }
    *logabs = ls;
    return sgn;
}

// element (r, c) of a compact na x na column-major image, 0 outside it (the address is always inside)
__device__ __forceinline__ double en_at(const double *__restrict__ p, int na, int r, int c)
{
    const double v = p[min(r, na - 1) + na * min(c, na - 1)];
    return (r < na && c < na) ? v : 0.0;
}
}  // namespace

// images of subsystem s at img + img_off[s]: [W][nb][2][na^2], the second of a pair the transpose.  One workgroup per
// (unit, subsystem); sites [sub_ptr[s] .. sub_ptr[s + 1]) of `sites`.
__global__ __launch_bounds__(EN_THREADS) void ent_gather_kernel(int n, const double *__restrict__ G, long stride_unit,
                                                                const int *__restrict__ sub_ptr,
                                                                const int *__restrict__ sites,
                                                                const long *__restrict__ img_off, double *__restrict__ img)
{
    const int u = blockIdx.x, s = blockIdx.y;
    const int s0 = sub_ptr[s], na = sub_ptr[s + 1] - s0;
    const int *a = sites + s0;
    const double *Gu = G + (long)u * stride_unit;
    double *g = img + img_off[s] + (long)u * 2 * na * na, *gt = g + (long)na * na;
    for (int e = threadIdx.x; e < na * na; e += EN_THREADS) {
        const int i = e % na, j = e / na;
        const double v = Gu[a[i] + (long)n * a[j]];
        g[e] = v;
        gt[j + na * i] = v;
    }
}

// one subsystem: blockIdx.x = pair (w < w', w-major), blockIdx.y = block.  img: the subsystem's images (ent_gather_kernel).
// lad / sg [n_pairs][nb]: sum log|pivot| and sign of det M_b.
template <bool STATIC>
__global__ __launch_bounds__(EN_THREADS) void ent_pair_kernel(int na, int nb, int n_walkers, const double *__restrict__ img,
                                                              double *__restrict__ lad, int *__restrict__ sg)
{
    __shared__ double en_static[STATIC ? EN_STATIC_DOUBLES : 1];
    extern __shared__ __attribute__((aligned(16))) double en_dynamic[];
    __shared__ double red_v[EN_WAVES];
    __shared__ int red_i[EN_WAVES];
    double *M = STATIC ? en_static : en_dynamic;

    const int p = blockIdx.x, b = blockIdx.y;
    int w0 = 0, rem = p;
    while (rem >= n_walkers - 1 - w0) { rem -= n_walkers - 1 - w0; ++w0; }
    const int w1 = w0 + 1 + rem;
    const long isz = (long)na * na;
    const double *G0 = img + ((long)w0 * nb + b) * 2 * isz;        // G_A of w
    const double *G1 = img + ((long)w1 * nb + b) * 2 * isz;        // G_A of w'
    const double *G1t = G1 + isz;                                  // its transpose

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lq = lane >> 4;
    const int np = en_pad(na), ld = np + 1, T = np / 16, groups = (T + EN_TJ - 1) / EN_TJ;

    // M = (I - G - G') + (2 G) G': work item = (row tile ti, group of four column tiles), round robin over the waves.
    // The MFMA is issued as gemm_f64.hip issues it (A-operand <- the right factor, B-operand <- the left one), so a lane
    // holds M[m = 16 ti + li][n = 16 tj + lq + 4 r]: the LDS stores run along m, the contiguous direction.
    for (int item = wave; item < T * groups; item += EN_WAVES) {
        const int ti = item % T, tj0 = (item / T) * EN_TJ;
        const int m = 16 * ti + li;
        d4 acc[EN_TJ];
#pragma unroll
        for (int j = 0; j < EN_TJ; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int nn = 16 * (tj0 + j) + lq + 4 * r;
                acc[j][r] = ((m == nn) ? 1.0 : 0.0) - en_at(G0, na, m, nn) - en_at(G1, na, m, nn);
            }
        }
        for (int k0 = 0; k0 < np; k0 += 4) {
            const int k = k0 + lq;
            const double a = 2.0 * en_at(G0, na, m, k);            // G[m, k], m contiguous
            double bb[EN_TJ];
#pragma unroll
            for (int j = 0; j < EN_TJ; ++j) bb[j] = en_at(G1t, na, 16 * (tj0 + j) + li, k);  // G'[k, n] = G't[n, k], n contiguous
#pragma unroll
            for (int j = 0; j < EN_TJ; ++j)
                if (tj0 + j < T) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bb[j], a, acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < EN_TJ; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int nn = 16 * (tj0 + j) + lq + 4 * r;
                if (m < na && nn < na) M[m + ld * nn] = acc[j][r];
            }
        }
    }
    __syncthreads();
    double ls;
    const int sgn = en_lu_logdet(M, na, ld, red_v, red_i, &ls);
    if (t == 0) {
        lad[(long)p * nb + b] = ls;
        sg[(long)p * nb + b] = sgn;
    }
}

// one thread per pair of one subsystem: x = prod_b sign_b exp(sum_b lad_b), the one block of the attractive model
// counted twice.  A pair with a zero sign (singular or non-finite pivot) or a non-finite x gives the sample 0 and bumps
// *failures.  sample / sums [W][W], element (w, w') at W w + w'.
__global__ __launch_bounds__(EN_THREADS) void ent_combine_kernel(int nb, int n_walkers, int n_pairs,
                                                                 const double *__restrict__ lad, const int *__restrict__ sg,
                                                                 double *__restrict__ sample, double *__restrict__ sums,
                                                                 unsigned long long *__restrict__ failures)
{
    const int p = blockIdx.x * EN_THREADS + threadIdx.x;
    if (p >= n_pairs) return;
    int w0 = 0, rem = p;
    while (rem >= n_walkers - 1 - w0) { rem -= n_walkers - 1 - w0; ++w0; }
    const int w1 = w0 + 1 + rem;
    double l = lad[(long)p * nb];
    int s = sg[(long)p * nb];
    if (nb == 1) {
        l = 2.0 * l;
        s = s * s;
    } else {
        l += lad[(long)p * nb + 1];
        s *= sg[(long)p * nb + 1];
    }
    double x = (double)s * exp(l);
    if (s == 0 || !(fabs(x) < INFINITY)) {
        x = 0.0;
        atomicAdd(failures, 1ULL);
    }
    const long e = (long)n_walkers * w0 + w1;
    sample[e] = x;
    sums[e] += x;
}

size_t entanglement_lds_bytes(int na)
{
    return na <= EN_STATIC_N ? 0 : (size_t)en_pad(na) * (en_pad(na) + 1) * sizeof(double);
}

hipError_t entanglement_prepare(int na_max)
{
    if (na_max <= EN_STATIC_N) return hipSuccess;
    return hipFuncSetAttribute((const void *)ent_pair_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)entanglement_lds_bytes(na_max));
}

hipError_t launch_entanglement_gather(int n, int n_units, int n_sub, const double *G, long stride_unit, const int *sub_ptr,
                                      const int *sites, const long *img_off, double *img, hipStream_t s)
{
    if (n < 1 || n_units < 1 || n_sub < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ent_gather_kernel, dim3(n_units, n_sub), dim3(EN_THREADS), 0, s, n, G, stride_unit, sub_ptr, sites,
                       img_off, img);
    return hipGetLastError();
}

hipError_t launch_entanglement_pairs(int na, int nb, int n_walkers, const double *img, double *lad, int *sg, double *sample,
                                     double *sums, unsigned long long *failures, hipStream_t s)
{
    if (na < 1 || na > DQMC_ENT_MAX_SITES_K || nb < 1 || nb > 2 || n_walkers < 2) return hipErrorInvalidValue;
    const int n_pairs = n_walkers * (n_walkers - 1) / 2;
    if (na <= EN_STATIC_N)
        hipLaunchKernelGGL(ent_pair_kernel<true>, dim3(n_pairs, nb), dim3(EN_THREADS), 0, s, na, nb, n_walkers, img, lad, sg);
    else
        hipLaunchKernelGGL(ent_pair_kernel<false>, dim3(n_pairs, nb), dim3(EN_THREADS), entanglement_lds_bytes(na), s, na,
                           nb, n_walkers, img, lad, sg);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ent_combine_kernel, dim3((n_pairs + EN_THREADS - 1) / EN_THREADS), dim3(EN_THREADS), 0, s, nb,
                       n_walkers, n_pairs, lad, sg, sample, sums, failures);
    return hipGetLastError();
}

}  // namespace dqmc
