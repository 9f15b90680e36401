// sign.hip — sign-reweighted measurement sums (include/dqmc_hip.h "sign reweighting"): the weight of a field is
// w = |w| s with s = prod_b sign det(I + B_M ... B_1)_b, and an average under w is <O s> / <s> under |w|.  The kernels
// here are the signed forms of the sums in sweep.hip: they add s_w x_w where those add x_w, walkers in the same order
// and every expression in the same shape, so that with every s_w = +1 (a product with 1.0 is exact) each sum comes out
// bit for bit as the unsigned kernel leaves it.  The unsigned kernels are not touched.
//
// sw [W + 2]: s_w of every walker as a double (+1, -1, or 0: a unit's sign was 0 - singular or non-finite A2 - and the
// walker's sample is left out), then sum_w s_w and the number of walkers kept.  A walker that is left out is never
// multiplied in (0 x NaN would poison the sum): its sample is not read into the sums at all.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dqmc {

// per-unit signs (sg [W][nb]; nullptr: every sign is +1 by construction, the attractive model) -> sw, the per-walker
// counters of left-out samples, and the sum of the signs added to the sections fed at this measurement point (sum_a,
// sum_b: one or two entries of the DQMC_RED_SIGN accumulator; sum_b may be nullptr).  One workgroup.
__global__ __launch_bounds__(256) void sign_prepare_kernel(int nb, int W, const int *__restrict__ sg,
                                                          double *__restrict__ sw, long long *__restrict__ failures,
                                                          double *__restrict__ sum_a, double *__restrict__ sum_b)
{
    for (int w = threadIdx.x; w < W; w += blockDim.x) {
        int s = 1;
        if (sg)
            for (int b = 0; b < nb; ++b) s *= sg[w * nb + b];
        sw[w] = (double)s;
        if (s == 0) failures[w] += 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double S = 0.0, kept = 0.0;
        for (int w = 0; w < W; ++w) {  // (exact: small integers)
            S += sw[w];
            kept += sw[w] != 0.0 ? 1.0 : 0.0;
        }
        sw[W] = S;
        sw[W + 1] = kept;
        *sum_a += S;
        if (sum_b) *sum_b += S;
    }
}
hipError_t launch_sign_prepare(int nb, int n_walkers, const int *sg, double *sw, long long *failures, double *sum_a,
                               double *sum_b, hipStream_t s)
{
    hipLaunchKernelGGL(sign_prepare_kernel, dim3(1), dim3(256), 0, s, nb, n_walkers, sg, sw, failures, sum_a, sum_b);
    return hipGetLastError();
}

// accumulate_kernel with the sign: sum s G, sum s G.^2, sum s (1 - G_ii), and the number of walkers kept as the count
__global__ void accumulate_signed_kernel(int n, int nb, int n_walkers, const double *__restrict__ G, long stride_unit,
                                         const double *__restrict__ sw, double *__restrict__ acc)
{
    const long per = (long)nb * n * n;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < per; e += (long)gridDim.x * blockDim.x) {
        const int b = (int)(e / ((long)n * n));
        const long idx = e - (long)b * n * n;
        double s1 = 0.0, s2 = 0.0;
        for (int w = 0; w < n_walkers; ++w) {
            const double sg = sw[w];
            if (sg == 0.0) continue;
            const double g = G[((long)w * nb + b) * stride_unit + idx], g1 = sg * g;
            s1 += g1;
            s2 += g1 * g;
        }
        acc[e] += s1;
        acc[per + e] += s2;
        const int r = (int)(idx % n), c = (int)(idx / n);
        if (r == c) acc[2 * per + (long)b * n + r] += sw[n_walkers] - s1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[2 * per + (long)nb * n] += sw[n_walkers + 1];
}
hipError_t launch_accumulate_signed(int n, int nb, int n_walkers, const double *G, long stride_unit, const double *sw,
                                    double *acc, hipStream_t s)
{
    const long per = (long)nb * n * n;
    int bx = (int)((per + 255) / 256);
    if (bx > 512) bx = 512;
    hipLaunchKernelGGL(accumulate_signed_kernel, dim3(bx), dim3(256), 0, s, n, nb, n_walkers, G, stride_unit, sw, acc);
    return hipGetLastError();
}

// corr_reduce_kernel with the sign.  The pair sums of corr_pairs_kernel come in unsigned and are rewritten in place as
// s_w x (0 for a walker left out), which is what the binner then reads; the magnetisation is read from G as there.
__global__ void corr_reduce_signed_kernel(int n, int nb, int model, int n_walkers, const double *__restrict__ G,
                                          long stride_unit, int n_dirs, double *__restrict__ per_walker,
                                          long per_stride, const double *__restrict__ sw, double *__restrict__ acc)
{
    const int total = 4 * n_dirs + 3 * n;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        double s = 0.0;
        if (e < 4 * n_dirs) {
            for (int w = 0; w < n_walkers; ++w) {
                const double sg = sw[w];
                double x = 0.0;
                if (sg != 0.0) {
                    x = sg * per_walker[(long)w * per_stride + e];
                    s += x;
                }
                per_walker[(long)w * per_stride + e] = x;
            }
        } else if (e >= 4 * n_dirs + 2 * n && model != 0) {  // mz = G_dn[i,i] - G_up[i,i]
            const int i = e - 4 * n_dirs - 2 * n;
            for (int w = 0; w < n_walkers; ++w) {
                const double sg = sw[w];
                if (sg == 0.0) continue;
                const double *G1 = G + (long)(w * nb) * stride_unit;
                s += sg * (G1[stride_unit + i + (long)n * i] - G1[i + (long)n * i]);
            }
        }
        acc[e] += s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[total] += sw[n_walkers + 1];
}
hipError_t launch_corr_reduce_signed(int n, int nb, int model, int n_walkers, const double *G, long stride_unit,
                                     int n_dirs, double *per_walker, const double *sw, double *acc, hipStream_t s)
{
    const int total = 4 * n_dirs + 3 * n;
    hipLaunchKernelGGL(corr_reduce_signed_kernel, dim3((total + 255) / 256), dim3(256), 0, s, n, nb, model, n_walkers, G,
                       stride_unit, n_dirs, per_walker, 4L * n_dirs, sw, acc);
    return hipGetLastError();
}

// pairing_reduce_kernel (factor = 1) and sus_reduce_kernel with the sign: acc[e] += factor sum_w s_w x[w][e], walkers
// in order, acc[total] += walkers kept; x[w][e] is rewritten in place as s_w x[w][e] for the binner that reads it next
__global__ void reduce_signed_kernel(int n_walkers, long total, double factor, double *__restrict__ per_walker,
                                     const double *__restrict__ sw, double *__restrict__ acc)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int w = 0; w < n_walkers; ++w) {
            const double sg = sw[w];
            double x = 0.0;
            if (sg != 0.0) {
                x = sg * per_walker[(long)w * total + e];
                s += x;
            }
            per_walker[(long)w * total + e] = x;
        }
        acc[e] += factor * s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[total] += sw[n_walkers + 1];
}
hipError_t launch_reduce_signed(int n_walkers, long total, double factor, double *per_walker, const double *sw,
                                double *acc, hipStream_t s)
{
    hipLaunchKernelGGL(reduce_signed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, n_walkers, total,
                       factor, per_walker, sw, acc);
    return hipGetLastError();
}

}  // namespace dqmc
