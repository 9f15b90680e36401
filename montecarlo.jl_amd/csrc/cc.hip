// cc.hip — current_current_susceptibility on the device (measurements.jl:257-317; attractive override
// HubbardModelAttractive.jl:250-266) over EachLocalQuadBySyncedDistance{K} (lattice_iterators.jl:360-467).
//
// With block-diagonal G and T (both Hubbard models here) the generic 2N kernel splits into
//   (a_up + a_dn)(s1,k) * (b_up + b_dn)(s2,k) + cross_up + cross_dn
// with t_i = trg(s_i, k) and, per block,
//   a(s,k) = T[s,t] Gll[t,s] - T[t,s] Gll[s,t]          b(s,k) = the same with G00
//   cross  = - T[t1,s1] T[t2,s2] G0l[s2,t1] Gl0[s1,t2] + T[s1,t1] T[t2,s2] G0l[s2,s1] Gl0[t1,t2]
//            + T[t1,s1] T[s2,t2] G0l[t2,t1] Gl0[s1,s2] - T[s1,t1] T[s2,t2] G0l[t2,s1] Gl0[t1,s2]
// (the reference's identity terms are left out as it leaves them out, measurements.jl:295-309).  The attractive
// override is 4 a b + 2 cross on the single block: a and b are scaled by `afac` = 2 there, the cross terms by 2.
//
// a and b depend on one site and one direction (O(NK) work).  The cross terms are the O(N^2 K) part; their
// fast path (cc_lds_kernel) serves a chunk of C sources s1 from LDS: the columns G0l[:, r] and rows Gl0[r, :]
// for every r in {s1, trg(s1, k)} of the chunk are loaded once (runs of adjacent rows share cache lines), and
// every thread owns one s2, so that its targets, T entries and b values stay in registers.  For a fixed s1,
// s2 -> dir12 is one-to-one on the lattices the host lets onto this path, so the per-(dir12, k) bins in LDS
// take one writer each between barriers: no atomics, a fixed summation order.  The partial bins of each
// workgroup are summed over workgroups in order by cc_fold_kernel.  Lattices without that property take
// cc_pairs_kernel: one workgroup per (dir12, walker), a literal gather per quad and a tree reduction.
#include "kernels.h"

namespace dqmc {

// bsum[w][k][s] = afac * sum_b b_b(s, k) from G00 (constant over the pass)
__global__ void cc_b_kernel(int n, int nb, int K, double afac, const double *__restrict__ G00, long stride_unit,
                            const int *__restrict__ trg, const double *__restrict__ tst,
                            const double *__restrict__ tts, double *__restrict__ bsum)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x, w = blockIdx.y;
    if (e >= n * K) return;
    const int s = e % n, t = trg[e];
    const int tc = t < 0 ? s : t;
    double v = 0.0;
    for (int b = 0; b < nb; ++b) {
        const double *G = G00 + (long)(w * nb + b) * stride_unit;
        v += tst[(long)b * n * K + e] * G[tc + (long)n * s] - tts[(long)b * n * K + e] * G[s + (long)n * tc];
    }
    bsum[(long)w * n * K + e] = t < 0 ? 0.0 : afac * v;
}

// Fast path.  Dynamic LDS (doubles): Lc [umax][n] G0l columns, Lr [umax][n] Gl0 rows, bins [K][n],
// then dsel of the chunk [C][n] as ints.  rows[c][umax] = the sorted set U of the chunk, slot[c][C][K+1] = index
// into U of s1 (k' = 0) and of trg(s1, k) (k' = k+1), -1 where there is none; dsel[s1][s2] = dir12.
__global__ __launch_bounds__(1024) void cc_lds_kernel(int n, int nb, int K, int C, int umax, int chunks_per_wg,
                                                      int nchunks, double afac, double xfac,
                                                      const double *__restrict__ G0l, const double *__restrict__ Gl0,
                                                      const double *__restrict__ Gll, long stride_unit,
                                                      const int *__restrict__ trg, const double *__restrict__ tst,
                                                      const double *__restrict__ tts, const double *__restrict__ bsum,
                                                      const int *__restrict__ dsel, const int *__restrict__ rows,
                                                      const int *__restrict__ ucnt, const int *__restrict__ slot,
                                                      double *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) double ccsm[];
    const int g = blockIdx.x, w = blockIdx.y, tid = threadIdx.x, bd = blockDim.x;
    const long nK = (long)n * K;
    double *Lc = ccsm, *Lr = ccsm + (long)umax * n, *bins = Lr + (long)umax * n;
    int *dl = (int *)(bins + nK);
    const bool active = tid < n;
    const int s2 = active ? tid : n - 1;
    for (long e = tid; e < nK; e += bd) bins[e] = 0.0;
    // per-s2 values of every direction (clamped indices: the loads are issued together)
    int t2r[CC_KMAX];
    double B2[CC_KMAX];
#pragma unroll
    for (int k = 0; k < CC_KMAX; ++k) {
        const int kc = k < K ? k : K - 1;
        t2r[k] = trg[s2 + (long)n * kc];
        B2[k] = bsum[(long)w * nK + s2 + (long)n * kc];
    }
    const int c_end = min(nchunks, (g + 1) * chunks_per_wg);
    for (int c = g * chunks_per_wg; c < c_end; ++c) {
        const int s_begin = c * C, cnt = min(C, n - s_begin), u = ucnt[c];
        const int *U = rows + (long)c * umax;
        for (int b = 0; b < nb; ++b) {
            const long ub = (long)(w * nb + b) * stride_unit;
            const double *tstb = tst + (long)b * nK, *ttsb = tts + (long)b * nK;
            __syncthreads();  // (the previous block / chunk is done with the panels)
            if (b == 0)  // dir12 of (s1, s2) for the chunk, four loads in flight per thread
                for (int e0 = tid; e0 < cnt * n; e0 += 4 * bd) {
                    int v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = dsel[(long)s_begin * n + min(e0 + q * bd, cnt * n - 1)];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (e0 + q * bd < cnt * n) dl[e0 + q * bd] = v[q];
                }
            // panels, four loads in flight per thread (clamped, then stored where in range)
            const int tot = u * n;
            for (int e0 = tid; e0 < tot; e0 += 4 * bd) {
                double vc[4], vr[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = min(e0 + q * bd, tot - 1);
                    const int jc = e / n, x = e - jc * n;   // column U[jc] of G0l, element x
                    const int jr = e % u, y = e / u;       // row U[jr] of Gl0, element y (adjacent rows side by side)
                    vc[q] = G0l[ub + x + (long)n * U[jc]];
                    vr[q] = Gl0[ub + U[jr] + (long)n * y];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = e0 + q * bd;
                    if (e < tot) {
                        const int jc = e / n, x = e - jc * n, jr = e % u, y = e / u;
                        Lc[(long)jc * n + x] = vc[q];
                        Lr[(long)jr * n + y] = vr[q];
                    }
                }
            }
            double Tst2[CC_KMAX], Tts2[CC_KMAX];
#pragma unroll
            for (int k = 0; k < CC_KMAX; ++k) {
                const int kc = k < K ? k : K - 1;
                Tst2[k] = tstb[s2 + (long)n * kc];
                Tts2[k] = ttsb[s2 + (long)n * kc];
            }
            __syncthreads();
            for (int i = 0; i < cnt; ++i) {
                const int s1 = s_begin + i;
                const int *sl = slot + ((long)c * C + i) * (K + 1);
                const int j0 = sl[0];
                const int d = dl[i * n + s2];
#pragma unroll
                for (int k = 0; k < CC_KMAX; ++k) {
                    if (k >= K) break;
                    const int j1 = sl[k + 1], t2 = t2r[k];
                    if (j1 < 0 || t2 < 0 || !active) continue;
                    const double Tst1 = tstb[s1 + (long)n * k], Tts1 = ttsb[s1 + (long)n * k];  // (uniform)
                    const double *c0 = Lc + (long)j0 * n, *c1 = Lc + (long)j1 * n;  // G0l[:, s1], G0l[:, t1]
                    const double *r0 = Lr + (long)j0 * n, *r1 = Lr + (long)j1 * n;  // Gl0[s1, :], Gl0[t1, :]
                    const double x = -Tts1 * Tts2[k] * c1[s2] * r0[t2] + Tst1 * Tts2[k] * c0[s2] * r1[t2]
                                     + Tts1 * Tst2[k] * c1[t2] * r0[s2] - Tst1 * Tst2[k] * c0[t2] * r1[s2];
                    double v = xfac * x;
                    if (b == 0) {  // afac * sum_b a_b(s1, k): uniform, scalar loads
                        const int t1 = trg[s1 + (long)n * k];
                        double a = 0.0;
                        for (int bb = 0; bb < nb; ++bb) {
                            const double *G = Gll + (long)(w * nb + bb) * stride_unit;
                            const long q = (long)bb * nK + s1 + (long)n * k;
                            a += tst[q] * G[t1 + (long)n * s1] - tts[q] * G[s1 + (long)n * t1];
                        }
                        v += afac * a * B2[k];
                    }
                    bins[(long)k * n + d] += v;
                }
                __syncthreads();  // (the next s1 maps the threads onto other bins)
            }
        }
    }
    __syncthreads();
    for (long e = tid; e < nK; e += bd) partial[((long)w * gridDim.x + g) * nK + e] = bins[e];
}

// per_walker[w][offset + e] += sum_g partial[w][g][e] / n, g in order (batches of 8 loads in flight); e = dir12 + n_dirs*k
__global__ void cc_fold_kernel(int n, int n_wg, long nK, const double *__restrict__ partial,
                               double *__restrict__ per_walker, long per_stride, long offset)
{
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const int w = blockIdx.y;
    if (e >= nK) return;
    const double *p = partial + (long)w * n_wg * nK + e;
    double *out = per_walker + (long)w * per_stride + offset + e;
    const double old = *out;
    double s = 0.0;
    for (int g0 = 0; g0 < n_wg; g0 += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = p[(long)min(g0 + q, n_wg - 1) * nK];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (g0 + q < n_wg) s += v[q];
    }
    *out = old + s / (double)n;
}

// Any lattice: one workgroup per (dir12, walker), every quad gathered from global memory; partial [w][K][n_dirs].
__global__ __launch_bounds__(256) void cc_pairs_kernel(int n, int nb, int K, double afac, double xfac,
                                                      const double *__restrict__ G0l, const double *__restrict__ Gl0,
                                                      const double *__restrict__ Gll, long stride_unit,
                                                      const int *__restrict__ dir_ptr, const int *__restrict__ pair_src,
                                                      const int *__restrict__ pair_trg, int n_dirs,
                                                      const int *__restrict__ trg, const double *__restrict__ tst,
                                                      const double *__restrict__ tts, const double *__restrict__ bsum,
                                                      double *__restrict__ partial)
{
    __shared__ double red[256];
    const int d = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
    const long nK = (long)n * K;
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int q = dir_ptr[d] + tid; q < dir_ptr[d + 1]; q += 256) {
            const int s1 = pair_src[q], s2 = pair_trg[q];
            const long e1 = s1 + (long)n * k, e2 = s2 + (long)n * k;
            const int t1 = trg[e1], t2 = trg[e2];
            if (t1 < 0 || t2 < 0) continue;
            double a = 0.0, x = 0.0;
            for (int b = 0; b < nb; ++b) {
                const long ub = (long)(w * nb + b) * stride_unit;
                const double Tst1 = tst[b * nK + e1], Tts1 = tts[b * nK + e1];
                const double Tst2 = tst[b * nK + e2], Tts2 = tts[b * nK + e2];
                a += Tst1 * Gll[ub + t1 + (long)n * s1] - Tts1 * Gll[ub + s1 + (long)n * t1];
                x += -Tts1 * Tts2 * G0l[ub + s2 + (long)n * t1] * Gl0[ub + s1 + (long)n * t2]
                     + Tst1 * Tts2 * G0l[ub + s2 + (long)n * s1] * Gl0[ub + t1 + (long)n * t2]
                     + Tts1 * Tst2 * G0l[ub + t2 + (long)n * t1] * Gl0[ub + s1 + (long)n * s2]
                     - Tst1 * Tst2 * G0l[ub + t2 + (long)n * s1] * Gl0[ub + t1 + (long)n * s2];
            }
            s += afac * a * bsum[(long)w * nK + e2] + xfac * x;
        }
        red[tid] = s;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off) red[tid] += red[tid + off];
            __syncthreads();
        }
        if (tid == 0) partial[(long)w * n_dirs * K + d + (long)n_dirs * k] = red[0];
        __syncthreads();
    }
}

hipError_t launch_cc_b(int n, int nb, int n_walkers, int K, double afac, const double *G00, long stride_unit,
                       const int *trg, const double *tst, const double *tts, double *bsum, hipStream_t s)
{
    hipLaunchKernelGGL(cc_b_kernel, dim3((n * K + 255) / 256, n_walkers), dim3(256), 0, s, n, nb, K, afac, G00,
                       stride_unit, trg, tst, tts, bsum);
    return hipGetLastError();
}

hipError_t launch_cc_slice(const CCPlan &p, int n, int nb, int n_walkers, double afac, double xfac,
                           const double *G0l, const double *Gl0, const double *Gll, long stride_unit,
                           const int *dir_ptr, const int *pair_src, const int *pair_trg, int n_dirs,
                           double *per_walker, long per_stride, long offset, hipStream_t s)
{
    if (p.fast) {
        static bool attr = false;
        if (!attr) {
            (void)hipFuncSetAttribute((const void *)cc_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            attr = true;
        }
        hipLaunchKernelGGL(cc_lds_kernel, dim3(p.n_wg, n_walkers), dim3(p.threads), p.lds_bytes, s, n, nb, p.K, p.C,
                           p.umax, p.chunks_per_wg, p.nchunks, afac, xfac, G0l, Gl0, Gll, stride_unit, p.trg, p.tst,
                           p.tts, p.bsum, p.dsel, p.rows, p.ucnt, p.slot, p.partial);
    } else {
        hipLaunchKernelGGL(cc_pairs_kernel, dim3(n_dirs, n_walkers), dim3(256), 0, s, n, nb, p.K, afac, xfac, G0l, Gl0,
                           Gll, stride_unit, dir_ptr, pair_src, pair_trg, n_dirs, p.trg, p.tst, p.tts, p.bsum, p.partial);
    }
    const long nK = (long)n_dirs * p.K;
    hipLaunchKernelGGL(cc_fold_kernel, dim3((unsigned)((nK + 255) / 256), n_walkers), dim3(256), 0, s, n,
                       p.fast ? p.n_wg : 1, nK, p.partial, per_walker, per_stride, offset);
    return hipGetLastError();
}

}  // namespace dqmc
