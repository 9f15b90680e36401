// sweep.hip — the small helper and measurement kernels of the engine: identity / diagonal / elementwise helpers, the
// propagation-error check (stack.jl:538-549), the measurement sums over walkers, the equal-time correlations and the
// time-displaced susceptibilities, the HS-field packing.  The site sweep itself is in sweep_lu.hip.
#include "kernels.h"

namespace dqmc {

__global__ void set_identity_kernel(int n, double *A, long stride)
{
    double *a = A + (long)blockIdx.y * stride;
    const long nn = (long)n * n;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < nn; idx += (long)gridDim.x * blockDim.x) {
        const int r = (int)(idx % n), c = (int)(idx / n);
        a[idx] = r == c ? 1.0 : 0.0;
    }
}
hipError_t launch_set_identity(int n, int count, double *A, long stride, hipStream_t s)
{
    const long nn = (long)n * n;
    int bx = (int)((nn + 255) / 256);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(set_identity_kernel, dim3(bx, count), dim3(256), 0, s, n, A, stride);
    return hipGetLastError();
}
__global__ void set_diag_kernel(int n, int nb, double *A, long stride, VecSrc d)
{
    const int unit = blockIdx.y;
    double *a = A + (long)unit * stride;
    const long nn = (long)n * n;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < nn; idx += (long)gridDim.x * blockDim.x) {
        const int r = (int)(idx % n), c = (int)(idx / n);
        a[idx] = r == c ? vs_get(d, unit, nb, r) : 0.0;
    }
}
hipError_t launch_set_diag(int n, int nb, int units, double *A, long stride, VecSrc d, hipStream_t s)
{
    const long nn = (long)n * n;
    int bx = (int)((nn + 255) / 256);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(set_diag_kernel, dim3(bx, units), dim3(256), 0, s, n, nb, A, stride, d);
    return hipGetLastError();
}
__global__ void mat_add_kernel(double *__restrict__ A, const double *__restrict__ B, size_t count)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        A[i] += B[i];
}
hipError_t launch_mat_add(double *A, const double *B, size_t count, hipStream_t s)
{
    size_t b = (count + 255) / 256;
    if (b > 4096) b = 4096;
    if (b == 0) b = 1;
    hipLaunchKernelGGL(mat_add_kernel, dim3((unsigned)b), dim3(256), 0, s, A, B, count);
    return hipGetLastError();
}
__global__ void sub_identity_kernel(int n, double *__restrict__ O, const double *__restrict__ A, long stride)
{
    double *o = O + (long)blockIdx.y * stride;
    const double *a = A + (long)blockIdx.y * stride;
    const long nn = (long)n * n;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < nn; idx += (long)gridDim.x * blockDim.x) {
        const int r = (int)(idx % n), c = (int)(idx / n);
        o[idx] = a[idx] - (r == c ? 1.0 : 0.0);
    }
}
hipError_t launch_sub_identity(int n, int units, double *O, const double *A, long stride, hipStream_t s)
{
    const long nn = (long)n * n;
    int bx = (int)((nn + 255) / 256);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(sub_identity_kernel, dim3(bx, units), dim3(256), 0, s, n, O, A, stride);
    return hipGetLastError();
}
// O = Diagonal(row) * A * Diagonal(col), the two scalings applied in the reference's order
__global__ void scale_mat_kernel(int n, int nb, double *__restrict__ O, const double *__restrict__ A, long stride,
                                 VecSrc row, VecSrc col, int row_first)
{
    const int unit = blockIdx.y;
    double *o = O + (long)unit * stride;
    const double *a = A + (long)unit * stride;
    const long nn = (long)n * n;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < nn; idx += (long)gridDim.x * blockDim.x) {
        const int r = (int)(idx % n), c = (int)(idx / n);
        const double rs = row.mode ? vs_get(row, unit, nb, r) : 1.0, cs = col.mode ? vs_get(col, unit, nb, c) : 1.0;
        double v = a[idx];
        if (row_first) { v *= rs; v *= cs; } else { v *= cs; v *= rs; }
        o[idx] = v;
    }
}
hipError_t launch_scale_mat(int n, int nb, int units, double *O, const double *A, long stride, VecSrc row, VecSrc col,
                            int row_first, hipStream_t s)
{
    const long nn = (long)n * n;
    int bx = (int)((nn + 255) / 256);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(scale_mat_kernel, dim3(bx, units), dim3(256), 0, s, n, nb, O, A, stride, row, col, row_first);
    return hipGetLastError();
}
__global__ void vec_map_kernel(int n, int nb, double *dst, long stride, VecSrc src)
{
    const int unit = blockIdx.x;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double v = vs_get(src, unit, nb, i);  // src may alias dst: each element is read, then written
        dst[(long)unit * stride + i] = v;
    }
}
hipError_t launch_vec_map(int n, int nb, int units, double *dst, long stride, VecSrc src, hipStream_t s)
{
    hipLaunchKernelGGL(vec_map_kernel, dim3(units), dim3(256), 0, s, n, nb, dst, stride, src);
    return hipGetLastError();
}
__global__ void fill_kernel(double *p, size_t n, double v)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
hipError_t launch_fill(double *p, size_t n, double v, hipStream_t s)
{
    size_t b = (n + 255) / 256;
    if (b > 1024) b = 1024;
    if (b == 0) b = 1;
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)b), dim3(256), 0, s, p, n, v);
    return hipGetLastError();
}

// maximum(abs.(greens_temp - greens)) > 1e-7 -> push!(propagation_error, .) (stack.jl:538-549,602-611)
// PC_SPLIT workgroups per walker: partial maxima meet in a per-walker word (non-negative doubles order like their bit
// patterns), the last workgroup to arrive pushes the event and clears the scratch for the next launch
constexpr int PC_SPLIT = 8;
__global__ __launch_bounds__(1024) void prop_check_kernel(int n, int nb, const double *__restrict__ A,
                                                         const double *__restrict__ B, long stride_unit,
                                                         DevStats *stats, unsigned long long *scratch)
{
    __shared__ double red[16];
    const int w = blockIdx.x / PC_SPLIT, part = blockIdx.x % PC_SPLIT;
    const long tot = (long)nb * stride_unit;
    double d = 0.0;
    bool bad = false;  // a NaN anywhere makes the maximum NaN in the reference (maximum(abs.(...)))
    if (tot & 1) {     // odd element count (odd n): the walkers' matrices are not all 16-byte aligned
        const double *a = A + (long)w * tot, *b = B + (long)w * tot;
        for (long i = (long)part * blockDim.x + threadIdx.x; i < tot; i += (long)PC_SPLIT * blockDim.x) {
            const double e0 = fabs(a[i] - b[i]);
            bad |= (e0 != e0);
            d = fmax(d, e0);
        }
    } else {
        const double2 *a = reinterpret_cast<const double2 *>(A + (long)w * tot), *b = reinterpret_cast<const double2 *>(B + (long)w * tot);
        for (long i = (long)part * blockDim.x + threadIdx.x; i < tot / 2; i += (long)PC_SPLIT * blockDim.x) {
            const double2 x = a[i], y = b[i];
            const double e0 = fabs(x.x - y.x), e1 = fabs(x.y - y.y);
            bad |= (e0 != e0) | (e1 != e1);
            d = fmax(d, fmax(e0, e1));
        }
    }
    if (bad) d = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(d, off, 64);
        d = (d != d || o != o) ? __longlong_as_double(0x7ff8000000000000ll) : fmax(d, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < (int)(blockDim.x >> 6); ++i) d = (d != d || red[i] != red[i]) ? __longlong_as_double(0x7ff8000000000000ll) : fmax(d, red[i]);
        // NaN (0x7ff8...) sorts above every finite magnitude as an unsigned word: it survives the atomicMax
        atomicMax(&scratch[2 * w], (unsigned long long)__double_as_longlong(d));
        __threadfence();
        if (atomicAdd(&scratch[2 * w + 1], 1ull) == PC_SPLIT - 1) {
            __threadfence();
            const double m = __longlong_as_double((long long)atomicExch(&scratch[2 * w], 0ull));
            scratch[2 * w + 1] = 0ull;
            if (m > 1e-7) magstats_push(stats[w].propagation_error, m);
        }
    }
}
hipError_t launch_prop_check(int n, int nb, int n_walkers, const double *A, const double *B, long stride_unit,
                             DevStats *stats, unsigned long long *scratch, hipStream_t s)
{
    hipLaunchKernelGGL(prop_check_kernel, dim3(n_walkers * PC_SPLIT), dim3(1024), 0, s, n, nb, A, B, stride_unit, stats,
                       scratch);
    return hipGetLastError();
}

// Measurement sums over the walkers of this device, fixed walker order (deterministic).
__global__ void accumulate_kernel(int n, int nb, int n_walkers, const double *__restrict__ G, long stride_unit,
                                  double *__restrict__ acc)
{
    const long per = (long)nb * n * n;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < per; e += (long)gridDim.x * blockDim.x) {
        const int b = (int)(e / ((long)n * n));
        const long idx = e - (long)b * n * n;
        double s1 = 0.0, s2 = 0.0;
        for (int w = 0; w < n_walkers; ++w) {
            const double g = G[((long)w * nb + b) * stride_unit + idx];
            s1 += g;
            s2 += g * g;
        }
        acc[e] += s1;
        acc[per + e] += s2;
        const int r = (int)(idx % n), c = (int)(idx / n);
        if (r == c) acc[2 * per + (long)b * n + r] += (double)n_walkers - s1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[2 * per + (long)nb * n] += (double)n_walkers;
}
hipError_t launch_accumulate(int n, int nb, int n_walkers, const double *G, long stride_unit, double *acc,
                             hipStream_t s)
{
    const long per = (long)nb * n * n;
    int bx = (int)((per + 255) / 256);
    if (bx > 512) bx = 512;
    hipLaunchKernelGGL(accumulate_kernel, dim3(bx), dim3(256), 0, s, n, nb, n_walkers, G, stride_unit, acc);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Equal-time correlation measurements on the true Green's function:
// cdc_kernel, sdc_{x,y,z}_kernel over EachSitePairByDistance and m{x,y,z}_kernel over EachSite
// (src/flavors/DQMC/measurements/measurements.jl:51-190, generic.jl:325-330,
// attractive overrides HubbardModelAttractive.jl:219-246).  For the repulsive model G is block
// diagonal (up, down), so every cross-spin element of the reference's 2N x 2N formulas is 0.
// One workgroup sums one direction of one walker over its pairs in a fixed order (deterministic).
__global__ __launch_bounds__(256) void corr_pairs_kernel(int n, int nb, int model, const double *__restrict__ G,
                                                        long stride_unit, const int *__restrict__ dir_ptr,
                                                        const int *__restrict__ pair_src,
                                                        const int *__restrict__ pair_trg, int n_dirs,
                                                        double *__restrict__ per_walker, long per_stride)
{
    __shared__ double red[4][256];
    const int d = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
    const double *G1 = G + (long)(w * nb) * stride_unit;
    const double *G2 = nb == 2 ? G1 + stride_unit : G1;
    double cdc = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    for (int q = dir_ptr[d] + tid; q < dir_ptr[d + 1]; q += 256) {
        const int i = pair_src[q], j = pair_trg[q];
        const double dij = i == j ? 1.0 : 0.0;
        const double a_ii = G1[i + (long)n * i], a_jj = G1[j + (long)n * j];
        const double a_ij = G1[i + (long)n * j], a_ji = G1[j + (long)n * i];
        if (model == 0) {  // HubbardModelAttractive.jl:222-236
            const double t = 2.0 * (dij - a_ji) * a_ij;
            cdc += 4.0 * (1.0 - a_ii) * (1.0 - a_jj) + t;
            sx += t; sy += t; sz += t;
        } else {
            const double b_ii = G2[i + (long)n * i], b_jj = G2[j + (long)n * j];
            const double b_ij = G2[i + (long)n * j], b_ji = G2[j + (long)n * i];
            // measurements.jl:63-76
            cdc += (1.0 - a_ii) * (1.0 - a_jj) + (dij - a_ji) * a_ij + (1.0 - a_ii) * (1.0 - b_jj) +
                   (1.0 - b_ii) * (1.0 - a_jj) + (1.0 - b_ii) * (1.0 - b_jj) + (dij - b_ji) * b_ij;
            // measurements.jl:150-156 / :167-173 with the cross-spin elements zero
            const double t = (dij - a_ji) * b_ij + (dij - b_ji) * a_ij;
            sx += t; sy += t;
            // measurements.jl:184-189
            sz += (1.0 - a_ii) * (1.0 - a_jj) + (dij - a_ji) * a_ij - (1.0 - a_ii) * (1.0 - b_jj) -
                  (1.0 - b_ii) * (1.0 - a_jj) + (1.0 - b_ii) * (1.0 - b_jj) + (dij - b_ji) * b_ij;
        }
    }
    red[0][tid] = cdc; red[1][tid] = sx; red[2][tid] = sy; red[3][tid] = sz;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off)
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + off];
        __syncthreads();
    }
    if (tid < 4) per_walker[(long)w * per_stride + (long)tid * n_dirs + d] = red[tid][0] / (double)n;  // finish!: / N
}
// m{x,y,z}_kernel (measurements.jl:112-124; attractive: all zero) and the sum over walkers
__global__ void corr_reduce_kernel(int n, int nb, int model, int n_walkers, const double *__restrict__ G,
                                   long stride_unit, int n_dirs, const double *__restrict__ per_walker,
                                   long per_stride, double *__restrict__ acc)
{
    const int total = 4 * n_dirs + 3 * n;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        double s = 0.0;
        if (e < 4 * n_dirs) {
            for (int w = 0; w < n_walkers; ++w) s += per_walker[(long)w * per_stride + e];
        } else if (e >= 4 * n_dirs + 2 * n && model != 0) {  // mz = G_dn[i,i] - G_up[i,i]
            const int i = e - 4 * n_dirs - 2 * n;
            for (int w = 0; w < n_walkers; ++w) {
                const double *G1 = G + (long)(w * nb) * stride_unit;
                s += G1[stride_unit + i + (long)n * i] - G1[i + (long)n * i];
            }
        }
        acc[e] += s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[total] += (double)n_walkers;
}
hipError_t launch_correlations(int n, int nb, int model, int n_walkers, const double *G, long stride_unit,
                               const int *dir_ptr, const int *pair_src, const int *pair_trg, int n_dirs,
                               double *per_walker, double *acc, hipStream_t s)
{
    const long per_stride = 4L * n_dirs;
    hipLaunchKernelGGL(corr_pairs_kernel, dim3(n_dirs, n_walkers), dim3(256), 0, s, n, nb, model, G, stride_unit,
                       dir_ptr, pair_src, pair_trg, n_dirs, per_walker, per_stride);
    const int total = 4 * n_dirs + 3 * n;
    hipLaunchKernelGGL(corr_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, s, n, nb, model, n_walkers, G,
                       stride_unit, n_dirs, per_walker, per_stride, acc);
    return hipGetLastError();
}

// the pair sums alone: the signed reduce (sign.hip) follows
hipError_t launch_correlation_pairs(int n, int nb, int model, int n_walkers, const double *G, long stride_unit,
                                    const int *dir_ptr, const int *pair_src, const int *pair_trg, int n_dirs,
                                    double *per_walker, hipStream_t s)
{
    hipLaunchKernelGGL(corr_pairs_kernel, dim3(n_dirs, n_walkers), dim3(256), 0, s, n, nb, model, G, stride_unit,
                       dir_ptr, pair_src, pair_trg, n_dirs, per_walker, 4L * n_dirs);
    return hipGetLastError();
}

// pc_kernel over EachLocalQuadByDistance{K} (measurements.jl:208-214, generic.jl:341-349,
// lattice_iterators.jl:264-318; attractive override HubbardModelAttractive.jl:243-245):
//   out[dir12, dir1, dir2] += G[src1, src2] * G[trg1+N, trg2+N] - G[src1, trg2+N] * G[trg1+N, src2]
// summed over all (src1, src2) with direction dir12 and the targets trg_k(src) of src in the K
// shortest directions.  With block-diagonal G (both Hubbard models here) the second product is 0 and
// the first is G_up[src1,src2] * G_dn[trg1,trg2] (attractive: G_dn = G_up).  One workgroup owns one
// (direction, walker) and reduces every (dir1, dir2) in a fixed order (deterministic).
__global__ __launch_bounds__(256) void pairing_kernel(int n, int nb, const double *__restrict__ G, long stride_unit,
                                                     const int *__restrict__ dir_ptr,
                                                     const int *__restrict__ pair_src,
                                                     const int *__restrict__ pair_trg, int n_dirs, int K,
                                                     const int *__restrict__ trg_of,
                                                     double *__restrict__ per_walker, long per_stride)
{
    __shared__ double red[256];
    const int d = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
    const double *G1 = G + (long)(w * nb) * stride_unit;
    const double *G2 = nb == 2 ? G1 + stride_unit : G1;
    for (int k2 = 0; k2 < K; ++k2)
        for (int k1 = 0; k1 < K; ++k1) {
            double s = 0.0;
            for (int q = dir_ptr[d] + tid; q < dir_ptr[d + 1]; q += 256) {
                const int s1 = pair_src[q], s2 = pair_trg[q];
                const int t1 = trg_of[s1 + n * k1], t2 = trg_of[s2 + n * k2];
                if (t1 >= 0 && t2 >= 0) s += G1[s1 + (long)n * s2] * G2[t1 + (long)n * t2];
            }
            red[tid] = s;
            __syncthreads();
            for (int off = 128; off > 0; off >>= 1) {
                if (tid < off) red[tid] += red[tid + off];
                __syncthreads();
            }
            if (tid == 0)  // finish!: / N (generic.jl:287-290); Julia layout [dir12, dir1, dir2]
                per_walker[(long)w * per_stride + d + (long)n_dirs * (k1 + K * k2)] = red[0] / (double)n;
            __syncthreads();
        }
}
__global__ void pairing_reduce_kernel(int n_walkers, long total, const double *__restrict__ per_walker,
                                      double *__restrict__ acc)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int w = 0; w < n_walkers; ++w) s += per_walker[(long)w * total + e];
        acc[e] += s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[total] += (double)n_walkers;
}
hipError_t launch_pairing(int n, int nb, int n_walkers, const double *G, long stride_unit, const int *dir_ptr,
                          const int *pair_src, const int *pair_trg, int n_dirs, int K, const int *trg_of,
                          double *per_walker, double *acc, hipStream_t s)
{
    const long total = (long)n_dirs * K * K;
    hipLaunchKernelGGL(pairing_kernel, dim3(n_dirs, n_walkers), dim3(256), 0, s, n, nb, G, stride_unit, dir_ptr,
                       pair_src, pair_trg, n_dirs, K, trg_of, per_walker, total);
    hipLaunchKernelGGL(pairing_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, n_walkers, total,
                       per_walker, acc);
    return hipGetLastError();
}

hipError_t launch_pairing_pairs(int n, int nb, int n_walkers, const double *G, long stride_unit, const int *dir_ptr,
                                const int *pair_src, const int *pair_trg, int n_dirs, int K, const int *trg_of,
                                double *per_walker, hipStream_t s)
{
    hipLaunchKernelGGL(pairing_kernel, dim3(n_dirs, n_walkers), dim3(256), 0, s, n, nb, G, stride_unit, dir_ptr,
                       pair_src, pair_trg, n_dirs, K, trg_of, per_walker, (long)n_dirs * K * K);
    return hipGetLastError();
}

// Time-displaced versions (packed Green's functions (G00, G0l, Gl0, Gll), measurements.jl:76-92,
// 150-192, 215-219; attractive overrides HubbardModelAttractive.jl:226-246) for the susceptibilities
// that apply!(::CombinedGreensIterator, ...) integrates over l (generic.jl:226-243).  Block-diagonal G:
// every cross-spin element of the 2N x 2N formulas is 0.  Each launch ADDS the contribution of one
// time slice to the per-walker sums (fixed order inside a workgroup: deterministic).
__global__ __launch_bounds__(256) void sus_pairs_kernel(int n, int nb, int model, const double *__restrict__ G00,
                                                       const double *__restrict__ G0l,
                                                       const double *__restrict__ Gl0,
                                                       const double *__restrict__ Gll, long stride_unit,
                                                       const int *__restrict__ dir_ptr,
                                                       const int *__restrict__ pair_src,
                                                       const int *__restrict__ pair_trg, int n_dirs,
                                                       double *__restrict__ per_walker, long per_stride)
{
    __shared__ double red[3][256];
    const int d = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
    const long u0 = (long)(w * nb) * stride_unit, u1 = nb == 2 ? u0 + stride_unit : u0;
    double cdc = 0.0, sxy = 0.0, sz = 0.0;
    for (int q = dir_ptr[d] + tid; q < dir_ptr[d + 1]; q += 256) {
        const int i = pair_src[q], j = pair_trg[q];
        const double l_up = 1.0 - Gll[u0 + i + (long)n * i], z_up = 1.0 - G00[u0 + j + (long)n * j];
        const double x_up = G0l[u0 + j + (long)n * i] * Gl0[u0 + i + (long)n * j];
        if (model == 0) {
            cdc += 4.0 * l_up * z_up - 2.0 * x_up;
            sxy += -2.0 * x_up;
            sz += -2.0 * x_up;
        } else {
            const double l_dn = 1.0 - Gll[u1 + i + (long)n * i], z_dn = 1.0 - G00[u1 + j + (long)n * j];
            const double x_dn = G0l[u1 + j + (long)n * i] * Gl0[u1 + i + (long)n * j];
            cdc += l_up * z_up - x_up + l_up * z_dn + l_dn * z_up + l_dn * z_dn - x_dn;
            // - G0l[j, i] Gl0[i+N, j+N] - G0l[j+N, i+N] Gl0[i, j]
            sxy += -G0l[u0 + j + (long)n * i] * Gl0[u1 + i + (long)n * j] - G0l[u1 + j + (long)n * i] * Gl0[u0 + i + (long)n * j];
            sz += l_up * z_up - x_up - l_up * z_dn - l_dn * z_up + l_dn * z_dn - x_dn;
        }
    }
    red[0][tid] = cdc; red[1][tid] = sxy; red[2][tid] = sz;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off)
            for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + off];
        __syncthreads();
    }
    if (tid < 4) {  // [cds][sds_x][sds_y][sds_z]; x and y coincide for block-diagonal G
        const int src = tid == 0 ? 0 : (tid == 3 ? 2 : 1);
        per_walker[(long)w * per_stride + (long)tid * n_dirs + d] += red[src][0] / (double)n;
    }
}
// pc_kernel with packed Green's functions: Gl0[src1, src2] * Gl0[trg1+N, trg2+N] (- cross-spin term = 0)
__global__ __launch_bounds__(256) void sus_pairing_kernel(int n, int nb, const double *__restrict__ Gl0,
                                                         long stride_unit, const int *__restrict__ dir_ptr,
                                                         const int *__restrict__ pair_src,
                                                         const int *__restrict__ pair_trg, int n_dirs, int K,
                                                         const int *__restrict__ trg_of,
                                                         double *__restrict__ per_walker, long per_stride, long offset)
{
    __shared__ double red[256];
    const int d = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
    const double *G1 = Gl0 + (long)(w * nb) * stride_unit;
    const double *G2 = nb == 2 ? G1 + stride_unit : G1;
    for (int k2 = 0; k2 < K; ++k2)
        for (int k1 = 0; k1 < K; ++k1) {
            double s = 0.0;
            for (int q = dir_ptr[d] + tid; q < dir_ptr[d + 1]; q += 256) {
                const int s1 = pair_src[q], s2 = pair_trg[q];
                const int t1 = trg_of[s1 + n * k1], t2 = trg_of[s2 + n * k2];
                if (t1 >= 0 && t2 >= 0) s += G1[s1 + (long)n * s2] * G2[t1 + (long)n * t2];
            }
            red[tid] = s;
            __syncthreads();
            for (int off = 128; off > 0; off >>= 1) {
                if (tid < off) red[tid] += red[tid + off];
                __syncthreads();
            }
            if (tid == 0) per_walker[(long)w * per_stride + offset + d + (long)n_dirs * (k1 + K * k2)] += red[0] / (double)n;
            __syncthreads();
        }
}
// acc[e] += factor * sum_w per_walker[w][e]; acc[total] += n_walkers
__global__ void sus_reduce_kernel(int n_walkers, long total, double factor, const double *__restrict__ per_walker,
                                  double *__restrict__ acc)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int w = 0; w < n_walkers; ++w) s += per_walker[(long)w * total + e];
        acc[e] += factor * s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[total] += (double)n_walkers;
}
hipError_t launch_sus_slice(int n, int nb, int model, int n_walkers, const double *G00, const double *G0l,
                            const double *Gl0, const double *Gll, long stride_unit, const int *dir_ptr,
                            const int *pair_src, const int *pair_trg, int n_dirs, int K, const int *trg_of,
                            double *per_walker, long per_stride, hipStream_t s)
{
    hipLaunchKernelGGL(sus_pairs_kernel, dim3(n_dirs, n_walkers), dim3(256), 0, s, n, nb, model, G00, G0l, Gl0, Gll,
                       stride_unit, dir_ptr, pair_src, pair_trg, n_dirs, per_walker, per_stride);
    if (K > 0)
        hipLaunchKernelGGL(sus_pairing_kernel, dim3(n_dirs, n_walkers), dim3(256), 0, s, n, nb, Gl0, stride_unit,
                           dir_ptr, pair_src, pair_trg, n_dirs, K, trg_of, per_walker, per_stride, 4L * n_dirs);
    return hipGetLastError();
}
hipError_t launch_sus_reduce(int n_walkers, long total, double factor, const double *per_walker, double *acc,
                             hipStream_t s)
{
    hipLaunchKernelGGL(sus_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, n_walkers, total,
                       factor, per_walker, acc);
    return hipGetLastError();
}

// compress(mc, model, conf) = BitArray(conf .== 1) (HubbardModel.jl:56-59): Julia's BitArray keeps
// element i (1-based, column-major) in bit (i-1) % 64 of chunk (i-1) / 64.  One wave packs one chunk.
__global__ void conf_pack_kernel(const int8_t *__restrict__ conf, size_t n_elem, unsigned long long *__restrict__ chunks)
{
    const size_t chunk = blockIdx.x * (size_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
    const size_t nchunks = (n_elem + 63) >> 6;
    if (chunk >= nchunks) return;
    const size_t i = chunk * 64 + (threadIdx.x & 63);
    const unsigned long long b = __ballot(i < n_elem && conf[i] == 1);
    if ((threadIdx.x & 63) == 0) chunks[chunk] = b;
}
// decompress: CT(2c .- 1)
__global__ void conf_unpack_kernel(const unsigned long long *__restrict__ chunks, size_t n_elem, int8_t *__restrict__ conf)
{
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n_elem) conf[i] = ((chunks[i >> 6] >> (i & 63)) & 1ull) ? 1 : -1;
}
hipError_t launch_conf_pack(const int8_t *conf, size_t n_elem, unsigned long long *chunks, hipStream_t s)
{
    const size_t nchunks = (n_elem + 63) >> 6;
    hipLaunchKernelGGL(conf_pack_kernel, dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0, s, conf, n_elem, chunks);
    return hipGetLastError();
}
hipError_t launch_conf_unpack(const unsigned long long *chunks, size_t n_elem, int8_t *conf, hipStream_t s)
{
    hipLaunchKernelGGL(conf_unpack_kernel, dim3((unsigned)((n_elem + 255) / 256)), dim3(256), 0, s, chunks, n_elem, conf);
    return hipGetLastError();
}

}  // namespace dqmc
