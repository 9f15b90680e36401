// binner.hip — logarithmic binning of the measurements on the device (BinningAnalysis.LogBinner behind
// push!(LogBinner, ...) of the reference's DQMCMeasurement, measurements/generic.jl:207-215,260-263): one binner per
// (walker, scalar element), state [level][walker][element] for each of x_sum, x2_sum and the one-value compressor, so
// every level a push touches is one contiguous stream.  Counts are the same for every element (floor(T / 2^level)) and
// live on the host.  Both kernels are pure streaming: no LDS, no atomics, no data-dependent branch.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dqmc {

// one walker's sample of element e, read from the buffers the measurement kernels have just filled
template <int MODE>
__device__ __forceinline__ double bin_sample(int w, int e, const double *__restrict__ src,
                                             const double *__restrict__ G, long stride_unit, int n, int nb, int model,
                                             int n_dirs, int E, double scale)
{
    if (MODE == BIN_SRC_GREENS) {  // [G of nb blocks][1 - G_ii of nb blocks]: the accumulator layout without G.^2
        const int nn = n * n, per = nb * nn;
        if (e < per) {
            const int b = e / nn;
            return G[((long)w * nb + b) * stride_unit + (e - b * nn)];
        }
        const int q = e - per, b = q / n, r = q - b * n;
        return 1.0 - G[((long)w * nb + b) * stride_unit + r + (long)n * r];
    }
    if (MODE == BIN_SRC_CORR) {  // [cdc][sdc_x][sdc_y][sdc_z] from per_walker, then mx, my (zero) and mz as corr_reduce_kernel
        if (e < 4 * n_dirs) return src[(long)w * 4 * n_dirs + e];
        const int i = e - 4 * n_dirs - 2 * n;
        if (i < 0 || model == 0) return 0.0;
        const double *G1 = G + (long)w * nb * stride_unit;
        return G1[stride_unit + i + (long)n * i] - G1[i + (long)n * i];
    }
    return scale * src[(long)w * E + e];  // BIN_SRC_PLAIN: [walker][element]
}

// push(x) of every (walker, element): lmax = number of trailing 1-bits of the push index (from the host, so the loop
// length is uniform).  Levels below lmax complete a pair with their compressor and carry the average upwards; level
// lmax keeps the value for the next push.  top = the last level, which has no compressor (its pair never completes
// within the capacity).
template <int MODE>
__global__ __launch_bounds__(256) void binner_push_kernel(int E, int lmax, int top, long WE,
                                                          const double *__restrict__ src,
                                                          const double *__restrict__ G, long stride_unit, int n, int nb,
                                                          int model, int n_dirs, double scale, double *__restrict__ xs,
                                                          double *__restrict__ x2, double *__restrict__ c)
{
    const int w = blockIdx.y;
    for (long el = blockIdx.x * 256L + threadIdx.x; el < E; el += gridDim.x * 256L) {  // (long: E may be near 2^31)
        const int e = (int)el;
        double x = bin_sample<MODE>(w, e, src, G, stride_unit, n, nb, model, n_dirs, E, scale);
        long at = (long)w * E + e;
        for (int l = 0; l < lmax; ++l, at += WE) {
            xs[at] += x;
            x2[at] += x * x;
            x = 0.5 * (c[at] + x);
        }
        xs[at] += x;
        x2[at] += x * x;
        if (lmax < top) c[at] = x;
    }
}

// binner_push_kernel for the sources that read G themselves, with the sign (sign.hip): pushes s_w x, 0 for a walker
// left out.  The pair sums of the CORR source arrive signed already (corr_reduce_signed_kernel).
template <int MODE>
__global__ __launch_bounds__(256) void binner_push_signed_kernel(int E, int lmax, int top, long WE,
                                                                 const double *__restrict__ src,
                                                                 const double *__restrict__ G, long stride_unit, int n,
                                                                 int nb, int model, int n_dirs,
                                                                 const double *__restrict__ sw, double *__restrict__ xs,
                                                                 double *__restrict__ x2, double *__restrict__ c)
{
    const int w = blockIdx.y;
    const double sg = sw[w];
    for (long el = blockIdx.x * 256L + threadIdx.x; el < E; el += gridDim.x * 256L) {
        const int e = (int)el;
        double x = 0.0;
        if (MODE == BIN_SRC_CORR && e < 4 * n_dirs) x = src[(long)w * 4 * n_dirs + e];
        else if (sg != 0.0) x = sg * bin_sample<MODE>(w, e, src, G, stride_unit, n, nb, model, n_dirs, E, 1.0);
        long at = (long)w * E + e;
        for (int l = 0; l < lmax; ++l, at += WE) {
            xs[at] += x;
            x2[at] += x * x;
            x = 0.5 * (c[at] + x);
        }
        xs[at] += x;
        x2[at] += x * x;
        if (lmax < top) c[at] = x;
    }
}

hipError_t launch_binner_push(const BinPush &p, int W, int E, int L, int lmax, double *xs, double *x2, double *c,
                              hipStream_t s)
{
    if (W < 1 || E < 1 || lmax < 0 || lmax >= L) return hipErrorInvalidValue;
    int bx = (E + 255) / 256;
    const int cap = (2048 + W - 1) / W;  // about 2048 workgroups in all, the rest by the grid stride
    if (bx > cap) bx = cap;
    const dim3 grid(bx, W), block(256);
    const long WE = (long)W * E;
#define BIN_LAUNCH(MODE)                                                                                               \
    hipLaunchKernelGGL(binner_push_kernel<MODE>, grid, block, 0, s, E, lmax, L - 1, WE, p.src, p.G, p.stride_unit,  \
                       p.n, p.nb, p.model, p.n_dirs, p.scale, xs, x2, c)
#define BIN_LAUNCH_SIGNED(MODE)                                                                                        \
    hipLaunchKernelGGL(binner_push_signed_kernel<MODE>, grid, block, 0, s, E, lmax, L - 1, WE, p.src, p.G,            \
                       p.stride_unit, p.n, p.nb, p.model, p.n_dirs, p.sw, xs, x2, c)
    if (p.sw && p.mode == BIN_SRC_GREENS) BIN_LAUNCH_SIGNED(BIN_SRC_GREENS);
    else if (p.sw && p.mode == BIN_SRC_CORR) BIN_LAUNCH_SIGNED(BIN_SRC_CORR);
    else if (p.mode == BIN_SRC_GREENS) BIN_LAUNCH(BIN_SRC_GREENS);
    else if (p.mode == BIN_SRC_CORR) BIN_LAUNCH(BIN_SRC_CORR);
    else BIN_LAUNCH(BIN_SRC_PLAIN);
#undef BIN_LAUNCH
#undef BIN_LAUNCH_SIGNED
    return hipGetLastError();
}

// varN = var / n of one level of one binner; NaN below two samples as in the reference
__device__ __forceinline__ double bin_varN(double a, double b, double cnt)
{
    if (cnt < 2.0) return __builtin_nan("");
    return (b / (cnt - 1.0) - a * a / (cnt * (cnt - 1.0))) / cnt;
}

// Per element, over the walkers in fixed order: out = [mean][std_error][std_error_walkers][tau][sum mean_w][sum mean_w^2]
// [sum varN_w(level)][sum varN_w(0)], E doubles each, then the walker count.  n0 / nl = counts of level 0 / `level`.
__global__ __launch_bounds__(256) void binner_finish_kernel(int W, int E, double n0, double nl, int level,
                                                            const double *__restrict__ xs,
                                                            const double *__restrict__ x2, double *__restrict__ out)
{
    const long lv = (long)level * W * E;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < E; e += gridDim.x * 256L) {
        double s1 = 0.0, s2 = 0.0, vl = 0.0, v0 = 0.0;
        for (int w = 0; w < W; ++w) {
            const long at = (long)w * E + e;
            const double a0 = xs[at], b0 = x2[at], m = a0 / n0;
            const double q0 = bin_varN(a0, b0, n0);
            s1 += m;
            s2 += m * m;
            v0 += q0;
            vl += level ? bin_varN(xs[lv + at], x2[lv + at], nl) : q0;
        }
        const double mean = s1 / (double)W;
        double d2 = 0.0;
        for (int w = 0; w < W; ++w) {
            const double d = xs[(long)w * E + e] / n0 - mean;
            d2 += d * d;
        }
        out[e] = mean;
        out[(long)E + e] = (vl < 0.0 ? 0.0 : sqrt(vl)) / (double)W;  // (a NaN passes through)
        out[2L * E + e] = W >= 2 ? sqrt(d2 / ((double)W * (double)(W - 1))) : __builtin_nan("");
        out[3L * E + e] = 0.5 * (vl / v0 - 1.0);
        out[4L * E + e] = s1;
        out[5L * E + e] = s2;
        out[6L * E + e] = vl;
        out[7L * E + e] = v0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[8L * E] = (double)W;
}

hipError_t launch_binner_finish(int W, int E, long T, int level, const double *xs, const double *x2, double *out,
                                hipStream_t s)
{
    if (W < 1 || E < 1 || level < 0) return hipErrorInvalidValue;
    int bx = (E + 255) / 256;
    if (bx > 2048) bx = 2048;
    hipLaunchKernelGGL(binner_finish_kernel, dim3(bx), dim3(256), 0, s, W, E, (double)T, (double)(T >> level), level, xs,
                       x2, out);
    return hipGetLastError();
}

}  // namespace dqmc
