// thermo.hip — scalar thermodynamics of one measurement point (include/dqmc_hip.h "thermodynamics"): filling, double
// occupancy, local moment, energies and the two fluctuation sums <N^2>/N and <Mz^2>/N, ten doubles per walker, from the
// true equal-time G of every unit.  The reference has no such measurement; the Wick contraction of the last two is the
// one of its cdc_kernel / sdc_z_kernel (measurements.jl:60-74, 180-186) summed over all pairs.
//
// One workgroup per walker.  The O(n^2) part is tr(G G) = sum_ij G_ij G_ji: G is streamed once in 64 x 64 tiles, tile
// (I, J) straight into registers and its partner (J, I), for I < J, through an LDS image that is read back transposed
// (rows padded by one double: the transposed read is free of bank conflicts), so both global reads run along columns.
// The bond sum gathers the nnz(T) entries G_ji of the neighbour list and the densities read the diagonal: both lie in
// the tiles just streamed.  No atomics: a lane adds its terms in tile order, the lanes of a wave go through one shuffle
// tree and the four waves are added in order, so a walker's sample has the same bits in every run and next to any
// number of other walkers.  No MFMA.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dqmc {

namespace {
constexpr int TH_TS = 64;           // tile edge = lanes of a wave: one wave reads one 512-byte column segment
constexpr int TH_LD = TH_TS + 1;    // padded row of the LDS image
constexpr int TH_THREADS = 256;
constexpr int TH_K = TH_TS * TH_TS / TH_THREADS;  // tile elements per lane

// sum over the workgroup, the same value in every lane: shuffle tree per wave, then the waves in order
__device__ __forceinline__ double th_block_sum(double v, double *red)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();  // (red is free again)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
}  // namespace

// row_ptr [nb n + 1], col / val: the off-diagonal non-zeros T_ij of row i of block b at row_ptr[b n + i] ..; tdiag [nb n]:
// T_ii.  out [walker][per_stride]: the ten elements of include/dqmc_hip.h, written (not added).
__global__ __launch_bounds__(TH_THREADS) void thermo_sample_kernel(int n, int nb, const double *__restrict__ G,
                                                                   long stride_unit, const int *__restrict__ row_ptr,
                                                                   const int *__restrict__ col,
                                                                   const double *__restrict__ val,
                                                                   const double *__restrict__ tdiag, double U_s,
                                                                   double *__restrict__ out, long per_stride)
{
    __shared__ double sB[TH_TS * TH_LD];
    __shared__ double red[TH_THREADS / 64];
    const int w = blockIdx.x, t = threadIdx.x, tx = t & 63, ty = t >> 6;
    const int nt = (n + TH_TS - 1) / TH_TS;
    const double *G0 = G + (long)w * nb * stride_unit;
    double ns[2] = {0.0, 0.0}, gg[2] = {0.0, 0.0}, bd[2] = {0.0, 0.0}, de[2] = {0.0, 0.0};
    for (int b = 0; b < nb; ++b) {
        const double *Gb = G0 + (long)b * stride_unit;
        double acc = 0.0;
        for (int TJ = 0; TJ < nt; ++TJ)
            for (int TI = 0; TI <= TJ; ++TI) {
                const int i0 = TI * TH_TS, j0 = TJ * TH_TS;
                const bool off = TI != TJ;
                // A(r, c) = G[i0 + r, j0 + c] with r = tx, c = ty + 4 k
                double a[TH_K];
#pragma unroll
                for (int k = 0; k < TH_K; ++k) {
                    const int c = ty + 4 * k;
                    a[k] = (i0 + tx < n && j0 + c < n) ? Gb[(i0 + tx) + (long)n * (j0 + c)] : 0.0;
                }
                // B(r, c) = G[j0 + r, i0 + c] at sB[c][r]; the diagonal tile is its own partner
#pragma unroll
                for (int k = 0; k < TH_K; ++k) {
                    const int c = ty + 4 * k;
                    double v = a[k];
                    if (off) v = (j0 + tx < n && i0 + c < n) ? Gb[(j0 + tx) + (long)n * (i0 + c)] : 0.0;
                    sB[c * TH_LD + tx] = v;
                }
                __syncthreads();
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < TH_K; ++k) s += a[k] * sB[tx * TH_LD + ty + 4 * k];  // A(r, c) B(c, r)
                acc += off ? 2.0 * s : s;
                __syncthreads();
            }
        double s_n = 0.0, s_b = 0.0, s_d = 0.0;
        for (int i = t; i < n; i += TH_THREADS) {
            const double ni = 1.0 - Gb[i + (long)n * i];
            s_n += ni;
            s_d += tdiag[b * n + i] * ni;
            double s = 0.0;
            for (int p = row_ptr[b * n + i]; p < row_ptr[b * n + i + 1]; ++p) s += val[p] * Gb[col[p] + (long)n * i];
            s_b -= s;  // T_ij (-G_ji)
        }
        gg[b] = th_block_sum(acc, red);
        ns[b] = th_block_sum(s_n, red);
        bd[b] = th_block_sum(s_b, red);
        de[b] = th_block_sum(s_d, red);
    }
    // n_up n_dn per site (one block: G_up = G_dn)
    const double *G1 = G0 + (long)(nb - 1) * stride_unit;
    double s_dd = 0.0;
    for (int i = t; i < n; i += TH_THREADS) s_dd += (1.0 - G0[i + (long)n * i]) * (1.0 - G1[i + (long)n * i]);
    const double dd = th_block_sum(s_dd, red);
    if (t != 0) return;
    const int o = nb - 1;  // the block of spin down
    const double inv = 1.0 / (double)n;
    const double Nup = ns[0], Ndn = ns[o];
    const double n_up = Nup * inv, n_dn = Ndn * inv, dens = n_up + n_dn, D = dd * inv;
    const double e_kin = (bd[0] + bd[o]) * inv;
    const double e_int = U_s * (D - 0.5 * dens + 0.25);
    // sum_sigma sum_ij (delta_ij - G_ji) G_ij = sum_sigma (tr G - tr G G), tr G = n - sum_i n_i
    const double wick = (((double)n - ns[0]) - gg[0]) + (((double)n - ns[o]) - gg[o]);
    double *y = out + (long)w * per_stride;
    y[0] = n_up;
    y[1] = n_dn;
    y[2] = dens;
    y[3] = D;
    y[4] = dens - 2.0 * D;
    y[5] = e_kin;
    y[6] = e_int;
    y[7] = e_kin + (de[0] + de[o]) * inv + e_int;
    y[8] = ((Nup + Ndn) * (Nup + Ndn) + wick) * inv;
    y[9] = ((Nup - Ndn) * (Nup - Ndn) + wick) * inv;
}

// the cross-walker sums as the reduce kernels of sweep.hip / sign.hip form them: acc[e] += sum_w x[w][e], walkers in
// order.  sw == nullptr: unsigned, acc[10] (the sum of signs) and acc[11] (the count) both grow by n_walkers.  With sw
// (sign.hip) x[w][e] is rewritten in place as s_w x[w][e] (0 for a walker left out, whose sample is never read into a sum),
// x[w][10] = s_w for the binner, acc[11] grows by the walkers kept; acc[10] has been fed by launch_sign_prepare.
__global__ __launch_bounds__(64) void thermo_reduce_kernel(int n_walkers, double *__restrict__ x, long per_stride,
                                                           const double *__restrict__ sw, double *__restrict__ acc)
{
    const int e = threadIdx.x;
    if (e < DQMC_THERMO_ELEMENTS_K) {
        double s = 0.0;
        for (int w = 0; w < n_walkers; ++w) {
            double v;
            if (sw) {
                const double sg = sw[w];
                v = 0.0;
                if (sg != 0.0) v = sg * x[(long)w * per_stride + e];
                x[(long)w * per_stride + e] = v;
            } else {
                v = x[(long)w * per_stride + e];
            }
            s += v;
        }
        acc[e] += s;
    } else if (e == DQMC_THERMO_ELEMENTS_K) {
        if (sw) {
            for (int w = 0; w < n_walkers; ++w) x[(long)w * per_stride + e] = sw[w];
        } else {
            acc[e] += (double)n_walkers;
        }
    } else if (e == DQMC_THERMO_ELEMENTS_K + 1) {
        acc[e] += sw ? sw[n_walkers + 1] : (double)n_walkers;
    }
}

hipError_t launch_thermodynamics(int n, int nb, int n_walkers, const double *G, long stride_unit, const int *row_ptr,
                                 const int *col, const double *val, const double *tdiag, double U_s, double *per_walker,
                                 long per_stride, const double *sw, double *acc, hipStream_t s)
{
    if (n < 1 || nb < 1 || nb > 2 || n_walkers < 1 || per_stride < DQMC_THERMO_ELEMENTS_K + (sw ? 1 : 0))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(thermo_sample_kernel, dim3(n_walkers), dim3(TH_THREADS), 0, s, n, nb, G, stride_unit, row_ptr, col,
                       val, tdiag, U_s, per_walker, per_stride);
    hipLaunchKernelGGL(thermo_reduce_kernel, dim3(1), dim3(64), 0, s, n_walkers, per_walker, per_stride, sw, acc);
    return hipGetLastError();
}

}  // namespace dqmc
