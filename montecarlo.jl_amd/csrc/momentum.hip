// momentum.hip — the lattice Fourier transform of every walker's sample (include/dqmc_hip.h "momentum-space
// observables"): Y[w][row][q] = scale * sum_d X[w][row][d] Tab[d][q], X the rows of n_dirs doubles (direction fastest)
// that the measurement kernels leave in a section's per-walker buffer, read in place, Tab the cosine or the sine table
// of dqmc_set_momenta [n_dirs x n_q, d fastest].  One GEMM on v_mfma_f64_16x16x4_f64 per segment of rows.
//
// Tiling: one 64 x 64 tile of Y per 256-thread workgroup, the four waves stacked along the rows (16 rows x 64 columns
// each, four accumulators), BK = 32.  The table tile is staged in LDS, zero-filled past n_dirs and n_q; X goes from
// global memory straight into the MFMA's first operand (the four lanes of a row read 32 contiguous bytes per k-step, a
// k-tile is one 256-byte run per row).  The operands are ordered as in gemm_f64.hip: the second one, here the table,
// is the one whose index comes out as the accumulator's lane index, so a wave's stores run along q, the contiguous
// direction of Y.
//
// The k-loop runs d = 0, 1, ... in tiles of 32 and steps of 4, always from 0, no atomics, no split: row `row` of Y is a
// function of row `row` of X and of the table alone.  A walker's output does not depend on the other rows of the tile,
// on the other walkers or on n_walkers, and a second pass gives the same bits.
#include "kernels.h"

namespace dqmc {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int MT = 64, MK = 32;
// LDS row stride of the table tile (doubles): rows k and k + 1, which one 32-lane half reads with ds_read_b64, lie 16
// double-banks apart (gemm_f64.hip: LS)
constexpr int MLS = 80;

__global__ __launch_bounds__(256) void momentum_kernel(MomentumArgs a)
{
    __shared__ double Ts[MK][MLS];
    const int w = blockIdx.z, r0 = blockIdx.x * MT, q0 = blockIdx.y * MT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const double *__restrict__ X = a.X + (long)w * a.x_stride + a.x_off;
    double *__restrict__ Y = a.Y + (long)w * a.y_stride + a.y_off;
    // the row of X this lane feeds (clamped: a row past the end computes a value that is never stored)
    const int row = min(r0 + wave * 16 + li, a.rows - 1);
    const double *__restrict__ xr = X + (long)row * a.n_dirs;

    d4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = (d4){0.0, 0.0, 0.0, 0.0};

    for (int k0 = 0; k0 < a.n_dirs; k0 += MK) {
        // table tile: element (k, c) = Tab[(k0 + k) + n_dirs (q0 + c)]; thread -> c = tid / 4, k = (tid % 4) * 8 .. + 7
        {
            const int c = tid >> 2, kb = (tid & 3) << 3, q = q0 + c;
            const double *t = a.tab + (long)a.n_dirs * min(q, a.n_q - 1);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = k0 + kb + i;
                const double v = t[min(k, a.n_dirs - 1)];
                Ts[kb + i][c] = (q < a.n_q && k < a.n_dirs) ? v : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < MK; kk += 4) {
            const int k = k0 + kk + lq;
            const double xv = xr[min(k, a.n_dirs - 1)];
            const double x = k < a.n_dirs ? xv : 0.0;  // (a select, not a product: the tail of the table is 0, X may hold anything)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, Ts[kk + lq][c * 16 + li], acc[c], 0, 0, 0);
        }
        __syncthreads();
    }
    // epilogue: the lane holds Y[row = .. + lq + 4 r][q = .. + li]
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int q = q0 + c * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rr = r0 + wave * 16 + lq + 4 * r;
            if (rr < a.rows && q < a.n_q) Y[(long)rr * a.n_q + q] = a.scale * acc[c][r];
        }
    }
    // with sign weighting the sample ends with s_w itself (one lane of one workgroup per walker)
    if (a.sw && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) a.Y[(long)w * a.y_stride + a.sign_at] = a.sw[w];
}

hipError_t launch_momentum(const MomentumArgs &a, int n_walkers, hipStream_t s)
{
    if (n_walkers < 1 || a.rows < 1 || a.n_dirs < 1 || a.n_q < 1 || !a.X || !a.Y || !a.tab) return hipErrorInvalidValue;
    const dim3 grid((a.rows + MT - 1) / MT, (a.n_q + MT - 1) / MT, n_walkers), block(256);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(momentum_kernel, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace dqmc
