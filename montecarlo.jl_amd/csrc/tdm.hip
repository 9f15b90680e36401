// tdm.hip — imaginary-time-resolved measurements (include/dqmc_hip.h "time-displaced recording"): the rows a
// dqmc_accumulate_susceptibilities pass keeps instead of integrating them away.  Row r of a walker's sample belongs to
// l = r * every and is computed from the packed tuple (G00, G0l, Gl0, Gll) of that slice; row 0 takes
// (G00, G00 - I, G00, G00), the -I formed here (minus_identity) and not as a fourth matrix.
//
//   Gl0[b][r][d] = (1/N) sum over the pairs (i, j) of direction d of Gl0_b[i, j]        G0l[b][r][d] likewise
//   CDC / SDCx / SDCy / SDCz[r][d] = the value sus_pairs_kernel (sweep.hip) adds for that slice, stored, not added
//
// Every value is a plain store of a sum in a fixed order: no atomics, a pass on the same state gives the same bits, and a
// walker's rows do not depend on the other walkers.
//
// Green's rows, two forms.  The pair lists of the correlation kernels walk a direction pair by pair, one double per
// cache line of a column-major matrix.  Where the direction table is a Latin square (n_dirs == n, every source and every
// target meets each direction once: the translation-invariant lattices) the host builds src_of[d + n j] = the source i
// with dir_of[i, j] = d, and tdm_greens_fast_kernel gives each lane one direction d and lets it walk the columns j in
// order: at every step a wave reads src_of[., j] contiguously and 64 elements of the one column j, 8 n contiguous bytes.
// A workgroup is 64 directions x 4 column quarters (one wave per quarter); the four partial sums are added in order.
// A table that is no Latin square but still injective (every source and every target meets a direction at most once,
// n_dirs <= 2 n: the two-sublattice lattices) takes tdm_greens_inj_kernel, the same walk over a src_of with holes.
// Every other table takes tdm_greens_pairs_kernel, one workgroup per (direction, matrix, walker) with a tree reduction.
#include "kernels.h"

namespace dqmc {

constexpr int TDM_DIRS = 64;  // directions per workgroup of the fast form = one wave
constexpr int TDM_SEGS = 4;   // column segments = waves per workgroup

// grid (ceil(n / 64), 2 nb, walkers): blockIdx.y = m * nb + b, m = 0: Gl0 -> offset 0, m = 1: G0l -> offset nb R n
__global__ __launch_bounds__(TDM_DIRS *TDM_SEGS) void tdm_greens_fast_kernel(
    int n, int nb, int R, int row, int minus_identity, const double *__restrict__ Gl0, const double *__restrict__ G0l,
    long stride_unit, const int *__restrict__ src_of, double *__restrict__ per_walker, long per_stride)
{
    __shared__ double part[TDM_SEGS][TDM_DIRS];
    const int lane = threadIdx.x & (TDM_DIRS - 1), seg = threadIdx.x / TDM_DIRS;
    const int d = blockIdx.x * TDM_DIRS + lane, m = blockIdx.y / nb, b = blockIdx.y % nb, w = blockIdx.z;
    const double *G = (m == 0 ? Gl0 : G0l) + (long)(w * nb + b) * stride_unit;
    const bool sub = m == 1 && minus_identity;
    const int len = (n + TDM_SEGS - 1) / TDM_SEGS, j0 = seg * len, j1 = min(n, j0 + len);
    double s = 0.0;
    if (d < n)
        for (int j = j0; j < j1; ++j) {
            const int i = src_of[d + (long)n * j];
            double v = G[i + (long)n * j];
            if (sub && i == j) v -= 1.0;
            s += v;
        }
    part[seg][lane] = s;
    __syncthreads();
    if (seg == 0 && d < n) {
        double t = part[0][lane];
        for (int q = 1; q < TDM_SEGS; ++q) t += part[q][lane];
        per_walker[(long)w * per_stride + ((long)(m * nb + b) * R + row) * n + d] = t / (double)n;
    }
}

// The injective form: the table of a lattice with a basis (honeycomb: n_dirs = 3 n / 2) is no Latin square, but every
// source and every target still meets a direction at most once, so src_of[d + n_dirs j] is well defined with holes (-1)
// where column j has no source in direction d.  The walk is that of the fast form, one lane per direction over the columns
// in order, a hole skipped; n_dirs <= 2 n bounds the table.  grid (ceil(n_dirs / 64), 2 nb, walkers), blockIdx.y as above;
// the rows have n_dirs entries, as the pair-list kernel writes them.
__global__ __launch_bounds__(TDM_DIRS *TDM_SEGS) void tdm_greens_inj_kernel(
    int n, int n_dirs, int nb, int R, int row, int minus_identity, const double *__restrict__ Gl0,
    const double *__restrict__ G0l, long stride_unit, const int *__restrict__ src_of, double *__restrict__ per_walker,
    long per_stride)
{
    __shared__ double part[TDM_SEGS][TDM_DIRS];
    const int lane = threadIdx.x & (TDM_DIRS - 1), seg = threadIdx.x / TDM_DIRS;
    const int d = blockIdx.x * TDM_DIRS + lane, m = blockIdx.y / nb, b = blockIdx.y % nb, w = blockIdx.z;
    const double *G = (m == 0 ? Gl0 : G0l) + (long)(w * nb + b) * stride_unit;
    const bool sub = m == 1 && minus_identity;
    const int len = (n + TDM_SEGS - 1) / TDM_SEGS, j0 = seg * len, j1 = min(n, j0 + len);
    double s = 0.0;
    if (d < n_dirs)
        for (int j = j0; j < j1; ++j) {
            const int i = src_of[d + (long)n_dirs * j];
            if (i < 0) continue;
            double v = G[i + (long)n * j];
            if (sub && i == j) v -= 1.0;
            s += v;
        }
    part[seg][lane] = s;
    __syncthreads();
    if (seg == 0 && d < n_dirs) {
        double t = part[0][lane];
        for (int q = 1; q < TDM_SEGS; ++q) t += part[q][lane];
        per_walker[(long)w * per_stride + ((long)(m * nb + b) * R + row) * n_dirs + d] = t / (double)n;
    }
}

// grid (n_dirs, 2 nb, walkers), the pair lists of corr_pairs_kernel
__global__ __launch_bounds__(256) void tdm_greens_pairs_kernel(
    int n, int nb, int R, int row, int minus_identity, const double *__restrict__ Gl0, const double *__restrict__ G0l,
    long stride_unit, const int *__restrict__ dir_ptr, const int *__restrict__ pair_src,
    const int *__restrict__ pair_trg, int n_dirs, double *__restrict__ per_walker, long per_stride)
{
    __shared__ double red[256];
    const int d = blockIdx.x, m = blockIdx.y / nb, b = blockIdx.y % nb, w = blockIdx.z, tid = threadIdx.x;
    const double *G = (m == 0 ? Gl0 : G0l) + (long)(w * nb + b) * stride_unit;
    const bool sub = m == 1 && minus_identity;
    double s = 0.0;
    for (int q = dir_ptr[d] + tid; q < dir_ptr[d + 1]; q += 256) {
        const int i = pair_src[q], j = pair_trg[q];
        double v = G[i + (long)n * j];
        if (sub && i == j) v -= 1.0;
        s += v;
    }
    red[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) per_walker[(long)w * per_stride + ((long)(m * nb + b) * R + row) * n_dirs + d] = red[0] / (double)n;
}

// The body of sus_pairs_kernel (sweep.hip; measurements.jl:76-92, 158-192, HubbardModelAttractive.jl:226-241) with the
// per-slice value stored into row `row`: per_walker[w][offset + (q R + row) n_dirs + d], q = CDC, SDCx, SDCy, SDCz.
// minus_identity: G0l[j, i] - delta_ij in the place of G0l[j, i] (row 0, where the kernels become the equal-time ones).
__global__ __launch_bounds__(256) void tdm_density_kernel(
    int n, int nb, int model, int R, int row, int minus_identity, const double *__restrict__ G00,
    const double *__restrict__ G0l, const double *__restrict__ Gl0, const double *__restrict__ Gll, long stride_unit,
    const int *__restrict__ dir_ptr, const int *__restrict__ pair_src, const int *__restrict__ pair_trg, int n_dirs,
    double *__restrict__ per_walker, long per_stride, long offset)
{
    __shared__ double red[3][256];
    const int d = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
    const long u0 = (long)(w * nb) * stride_unit, u1 = nb == 2 ? u0 + stride_unit : u0;
    double cdc = 0.0, sxy = 0.0, sz = 0.0;
    for (int q = dir_ptr[d] + tid; q < dir_ptr[d + 1]; q += 256) {
        const int i = pair_src[q], j = pair_trg[q];
        const double dij = minus_identity && i == j ? 1.0 : 0.0;
        const double l_up = 1.0 - Gll[u0 + i + (long)n * i], z_up = 1.0 - G00[u0 + j + (long)n * j];
        const double f_up = G0l[u0 + j + (long)n * i] - dij, b_up = Gl0[u0 + i + (long)n * j];
        const double x_up = f_up * b_up;
        if (model == 0) {
            cdc += 4.0 * l_up * z_up - 2.0 * x_up;
            sxy += -2.0 * x_up;
            sz += -2.0 * x_up;
        } else {
            const double l_dn = 1.0 - Gll[u1 + i + (long)n * i], z_dn = 1.0 - G00[u1 + j + (long)n * j];
            const double f_dn = G0l[u1 + j + (long)n * i] - dij, b_dn = Gl0[u1 + i + (long)n * j];
            const double x_dn = f_dn * b_dn;
            cdc += l_up * z_up - x_up + l_up * z_dn + l_dn * z_up + l_dn * z_dn - x_dn;
            sxy += -f_up * b_dn - f_dn * b_up;
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
    if (tid < 4) {  // x and y coincide for block-diagonal G
        const int src = tid == 0 ? 0 : (tid == 3 ? 2 : 1);
        per_walker[(long)w * per_stride + offset + ((long)tid * R + row) * n_dirs + d] = red[src][0] / (double)n;
    }
}

hipError_t launch_tdm_greens(bool fast, int n, int nb, int n_walkers, int R, int row, int minus_identity,
                             const double *Gl0, const double *G0l, long stride_unit, const int *src_of,
                             const int *dir_ptr, const int *pair_src, const int *pair_trg, int n_dirs,
                             double *per_walker, long per_stride, hipStream_t s)
{
    if (fast)
        hipLaunchKernelGGL(tdm_greens_fast_kernel, dim3((n + TDM_DIRS - 1) / TDM_DIRS, 2 * nb, n_walkers),
                           dim3(TDM_DIRS * TDM_SEGS), 0, s, n, nb, R, row, minus_identity, Gl0, G0l, stride_unit, src_of,
                           per_walker, per_stride);
    else
        hipLaunchKernelGGL(tdm_greens_pairs_kernel, dim3(n_dirs, 2 * nb, n_walkers), dim3(256), 0, s, n, nb, R, row,
                           minus_identity, Gl0, G0l, stride_unit, dir_ptr, pair_src, pair_trg, n_dirs, per_walker,
                           per_stride);
    return hipGetLastError();
}
hipError_t launch_tdm_greens_inj(int n, int n_dirs, int nb, int n_walkers, int R, int row, int minus_identity,
                                 const double *Gl0, const double *G0l, long stride_unit, const int *src_of,
                                 double *per_walker, long per_stride, hipStream_t s)
{
    hipLaunchKernelGGL(tdm_greens_inj_kernel, dim3((n_dirs + TDM_DIRS - 1) / TDM_DIRS, 2 * nb, n_walkers),
                       dim3(TDM_DIRS * TDM_SEGS), 0, s, n, n_dirs, nb, R, row, minus_identity, Gl0, G0l, stride_unit,
                       src_of, per_walker, per_stride);
    return hipGetLastError();
}
hipError_t launch_tdm_density(int n, int nb, int model, int n_walkers, int R, int row, int minus_identity,
                              const double *G00, const double *G0l, const double *Gl0, const double *Gll,
                              long stride_unit, const int *dir_ptr, const int *pair_src, const int *pair_trg, int n_dirs,
                              double *per_walker, long per_stride, long offset, hipStream_t s)
{
    hipLaunchKernelGGL(tdm_density_kernel, dim3(n_dirs, n_walkers), dim3(256), 0, s, n, nb, model, R, row,
                       minus_identity, G00, G0l, Gl0, Gll, stride_unit, dir_ptr, pair_src, pair_trg, n_dirs, per_walker,
                       per_stride, offset);
    return hipGetLastError();
}

}  // namespace dqmc
