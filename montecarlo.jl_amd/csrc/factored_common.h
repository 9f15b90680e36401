// factored_common.h — what the factored-hopping chain kernels (kron.hip, kron3.hip, tri.hip, ttp.hip, bilayer.hip, rect.hip)
// have in common around their products and compile to the instructions they had written out in each file: the HS-field
// factor, the store of the staged result, and the launch.  (The prologue, the one-step-ahead requests, the scalings and
// the staging stores stay in the kernels: shared as helpers they reorder the kernels' instruction streams.)
#pragma once
#include "kernels.h"
#include <hip/hip_ext.h>

namespace dqmc {

typedef double d4 __attribute__((ext_vector_type(4)));
#define FK_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// exp(sign lambda conf[i]) of block blk (vs_conf() of engine.cpp, slab_conf_val() of slab.hip)
__device__ __forceinline__ double fk_conf(int8_t c, int sign, bool bn, double epl, double eml)
{
    return (((c > 0) == (sign > 0)) != bn) ? epl : eml;
}

// The staged image of a workgroup's COLS result columns to memory in 16-byte pieces.  Transposed image [entry][column]:
// entry e, column cl at e SLD + (e >> 4) SPAD + cl (SPAD: see bilayer.hip), stored as out[c][e] = X[e][c], row e of the
// image being COLS consecutive doubles at c0 + N e; else the image is the global one, N COLS consecutive doubles
template <int N, int COLS, int SLD, int SPAD>
__device__ __forceinline__ void fk_store_image(double *o, const double *lds, const KronArgs &a, int c0, int tid)
{
    static_assert(COLS == 8 || COLS == 16, "a power of two");
    if (a.transpose_out) {
#pragma unroll
        for (int k = 0; k < N * COLS / 512; ++k) {
            const int e2 = 2 * (tid + 256 * k), e = e2 >> (COLS == 16 ? 4 : 3), cl = e2 & (COLS - 1);
            const double *src = SLD == COLS && SPAD == 0 ? lds + e2 : lds + e * SLD + (e >> 4) * SPAD + cl;  // (dense: as it comes)
            *reinterpret_cast<double2 *>(o + c0 + (long)N * e + cl) = *reinterpret_cast<const double2 *>(src);
        }
    } else {
#pragma unroll
        for (int k = 0; k < N * COLS / 512; ++k) {
            const int e2 = 2 * (tid + 256 * k);
            *reinterpret_cast<double2 *>(o + (long)N * c0 + e2) = *reinterpret_cast<const double2 *>(lds + e2);
        }
    }
}

// 256 threads per workgroup; with events the dispatch's own begin / end timestamps are taken (kernels.h: launch_gemm)
template <class Kernel>
inline hipError_t fk_launch(Kernel kernel, dim3 grid, const KronArgs &a, hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    if (start) hipExtLaunchKernelGGL(kernel, grid, dim3(256), 0, s, start, stop, 0, a);
    else hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace dqmc
