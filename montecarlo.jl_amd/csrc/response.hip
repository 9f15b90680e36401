// response.hip — the two kernels in front of the lattice Fourier transform of the pairing and current-current samples
// (include/dqmc_hip.h "pair structure factors and superfluid stiffness"); the transform itself is momentum.hip's.
//
// pair_channel_kernel: Z[w][c][d] = sum_kk F[kk + KK c] X[w][d + n_dirs kk], kk = k1 + K k2 ascending, X the walker's
// pairing sample as pairing_kernel / sus_pairs_kernel leave it (d fastest), read in place.  Plain FMA, no MFMA and no
// LDS: at K^2 <= 81 and n_ch <= 8 the kernel does 2 n_ch flops per 8 bytes of X and is bound by the one pass over X,
// which a wave reads as 512-byte runs along d; F is indexed by wave-uniform values only and comes in through the
// constant cache.  A lane owns one d and carries the n_ch sums in registers, so every output element is one sum in a
// fixed order with no atomics: a walker's output depends neither on n_walkers nor on the other directions.
//
// bond_kinetic_kernel: kbond[w][k] = (1/N) sum_src [trg >= 0] sum_sigma T_sigma[trg, src] (delta_{src,trg} -
// G_sigma[src, trg]), trg = trg_of[src + n k]; one 64-lane workgroup per (k, w), lane-strided partial sums in ascending
// src, then a fixed binary tree through LDS.
#include "kernels.h"

namespace dqmc {

constexpr int RESP_MAX_CH = 8;

__global__ __launch_bounds__(256) void pair_channel_kernel(int n_dirs, int KK, int n_ch, const double *__restrict__ X,
                                                           long x_stride, long x_off, const double *__restrict__ F,
                                                           double *__restrict__ Z, long z_stride)
{
    const int d = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
    if (d >= n_dirs) return;
    const double *__restrict__ x = X + (long)w * x_stride + x_off + d;
    double acc[RESP_MAX_CH];
#pragma unroll
    for (int c = 0; c < RESP_MAX_CH; ++c) acc[c] = 0.0;
    for (int kk = 0; kk < KK; ++kk) {
        const double v = x[(long)kk * n_dirs];
#pragma unroll
        for (int c = 0; c < RESP_MAX_CH; ++c)
            if (c < n_ch) acc[c] = fma(F[kk + (long)KK * c], v, acc[c]);
    }
    double *__restrict__ z = Z + (long)w * z_stride + d;
#pragma unroll
    for (int c = 0; c < RESP_MAX_CH; ++c)
        if (c < n_ch) z[(long)c * n_dirs] = acc[c];
}

hipError_t launch_pair_channels(int n_dirs, int KK, int n_ch, int n_walkers, const double *X, long x_stride, long x_off,
                                const double *F, double *Z, long z_stride, hipStream_t s)
{
    if (n_dirs < 1 || KK < 1 || n_ch < 1 || n_ch > RESP_MAX_CH || n_walkers < 1 || n_walkers > 65535 || !X || !F || !Z)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pair_channel_kernel, dim3((n_dirs + 255) / 256, n_walkers), dim3(256), 0, s, n_dirs, KK, n_ch, X,
                       x_stride, x_off, F, Z, z_stride);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void bond_kinetic_kernel(int n, int nb, double fac, const double *__restrict__ G,
                                                          long stride_unit, const int *__restrict__ trg_of,
                                                          const double *__restrict__ tts, const double *__restrict__ sw,
                                                          double *__restrict__ out, long out_stride, long out_off)
{
    __shared__ double part[64];
    const int k = blockIdx.x, w = blockIdx.y, lane = threadIdx.x, K = gridDim.x;
    const long nK = (long)n * K;
    double s = 0.0;
    for (int src = lane; src < n; src += 64) {
        const int trg = trg_of[src + (long)n * k];
        if (trg < 0) continue;
        for (int b = 0; b < nb; ++b) {
            const double *__restrict__ Gb = G + ((long)w * nb + b) * stride_unit;
            const double g = (src == trg ? 1.0 : 0.0) - Gb[src + (long)n * trg];
            s = fma(tts[b * nK + src + (long)n * k], g, s);
        }
    }
    part[lane] = s;
    __syncthreads();
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        if (lane < h) part[lane] += part[lane + h];
        __syncthreads();
    }
    if (lane == 0) {
        double v = fac * part[0] / (double)n;
        if (sw) v = sw[w] != 0.0 ? sw[w] * v : 0.0;  // the sample is s_w x, as its sources are
        out[(long)w * out_stride + out_off + k] = v;
    }
}

hipError_t launch_bond_kinetic(int n, int nb, int K, int n_walkers, double fac, const double *G, long stride_unit,
                               const int *trg_of, const double *tts, const double *sw, double *out, long out_stride,
                               long out_off, hipStream_t s)
{
    if (n < 1 || nb < 1 || K < 1 || n_walkers < 1 || n_walkers > 65535 || !G || !trg_of || !tts || !out)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(bond_kinetic_kernel, dim3(K, n_walkers), dim3(64), 0, s, n, nb, fac, G, stride_unit, trg_of, tts,
                       sw, out, out_stride, out_off);
    return hipGetLastError();
}

}  // namespace dqmc
