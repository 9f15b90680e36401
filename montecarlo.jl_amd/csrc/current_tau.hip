// current_tau.hip — the kernels of the imaginary-time-resolved current-current recording (include/dqmc_hip.h "current
// response in imaginary time"; host side in current_tau.inl).
//
// At a recorded slice launch_cc_slice leaves the slice's own sums x[w][d + n_dirs k] in a zeroed scratch instead of
// adding them to the susceptibility sample.  current_tau_row_kernel then does two things with it:
//   * the contraction with both phase tables into row r of every walker's sums,
//       C[r][k][q] += s_w sum_d cos(q . r_d) x[d + n_dirs k],   S[r][k][q] += s_w sum_d sin(q . r_d) x[d + n_dirs k],
//     d ascending.  A small fp64 product per walker (K_cc x n_dirs by n_dirs x 2 n_q, a few hundred kflop at 16 x 16):
//     no MFMA; it is bound by the one pass over the tables.  One wave per (64 momenta, k, walker): a lane owns one q
//     and carries both sums in registers, so that every stored value is one sum in a fixed order with no atomics and no
//     reduction across lanes: a walker's rows depend neither on n_walkers nor on the launch shape.  The tables come
//     interleaved and q fastest, tab[2 (q + n_q d)] = cos, + 1 = sin, so a wave reads one 1 KiB run per d (16-byte
//     loads, four d in flight); x[d] is wave-uniform.
//   * the hand-over of the scratch to the susceptibility sample, add_to[w][add_off + e] += x[e], done by the waves of
//     the first momentum tile: cc_fold_kernel's `old + s / n` with old = 0 is s / n exactly, so old + (0 + s / n) has
//     the bits of the unrecorded pass.  Row 0 (add_to == nullptr) is not part of that sample.
// current_tau_finish_kernel closes a pass: kbond (launch_bond_kinetic's values, s_w x already) and the three counters.
#include "kernels.h"

namespace dqmc {

__global__ __launch_bounds__(64) void current_tau_row_kernel(int n_dirs, int n_q, int K, const double *__restrict__ x,
                                                             const double2 *__restrict__ tab,
                                                             const double *__restrict__ sw, double *__restrict__ sums,
                                                             long sums_stride, long off_c, long off_s,
                                                             double *__restrict__ add_to, long add_stride, long add_off)
{
    const int lane = threadIdx.x, k = blockIdx.y, w = blockIdx.z;
    const int q = blockIdx.x * 64 + lane;
    const double *__restrict__ xr = x + ((long)w * K + k) * n_dirs;
    if (add_to && blockIdx.x == 0) {
        double *__restrict__ a = add_to + (long)w * add_stride + add_off + (long)k * n_dirs;
        for (int d = lane; d < n_dirs; d += 64) a[d] = a[d] + xr[d];
    }
    const double s = sw ? sw[w] : 1.0;
    if (q >= n_q || s == 0.0) return;  // (a walker whose sign came out 0 is left out)
    const double2 *__restrict__ t = tab + q;
    double c = 0.0, sn = 0.0;
    int d = 0;
    for (; d + 4 <= n_dirs; d += 4) {
        double2 v[4];
        double xv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = t[(long)(d + j) * n_q];
            xv[j] = xr[d + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c = fma(v[j].x, xv[j], c);
            sn = fma(v[j].y, xv[j], sn);
        }
    }
    for (; d < n_dirs; ++d) {
        const double2 v = t[(long)d * n_q];
        const double xv = xr[d];
        c = fma(v.x, xv, c);
        sn = fma(v.y, xv, sn);
    }
    double *__restrict__ o = sums + (long)w * sums_stride + (long)k * n_q + q;
    o[off_c] += s * c;
    o[off_s] += s * sn;
}

// sums[w]: ... [kbond: K][sum of s_w][samples kept][samples left out] at `tail`
__global__ __launch_bounds__(64) void current_tau_finish_kernel(int K, const double *__restrict__ kb,
                                                                const double *__restrict__ sw,
                                                                double *__restrict__ sums, long sums_stride, long tail)
{
    const int w = blockIdx.x, lane = threadIdx.x;
    double *__restrict__ o = sums + (long)w * sums_stride + tail;
    const double s = sw ? sw[w] : 1.0;
    if (s != 0.0)
        for (int k = lane; k < K; k += 64) o[k] += kb[(long)w * K + k];
    if (lane == 0) {
        o[K] += s;
        o[K + 1] += s != 0.0 ? 1.0 : 0.0;
        o[K + 2] += s != 0.0 ? 0.0 : 1.0;
    }
}

hipError_t launch_current_tau_row(int n_dirs, int n_q, int K, int n_walkers, const double *x, const double *tab,
                                  const double *sw, double *sums, long sums_stride, long off_c, long off_s,
                                  double *add_to, long add_stride, long add_off, hipStream_t s)
{
    if (n_dirs < 1 || n_q < 1 || K < 1 || K > 65535 || n_walkers < 1 || n_walkers > 65535 || !x || !tab || !sums)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(current_tau_row_kernel, dim3((n_q + 63) / 64, K, n_walkers), dim3(64), 0, s, n_dirs, n_q, K, x,
                       (const double2 *)tab, sw, sums, sums_stride, off_c, off_s, add_to, add_stride, add_off);
    return hipGetLastError();
}

hipError_t launch_current_tau_finish(int K, int n_walkers, const double *kb, const double *sw, double *sums,
                                     long sums_stride, long tail, hipStream_t s)
{
    if (K < 1 || n_walkers < 1 || !kb || !sums) return hipErrorInvalidValue;
    hipLaunchKernelGGL(current_tau_finish_kernel, dim3(n_walkers), dim3(64), 0, s, K, kb, sw, sums, sums_stride, tail);
    return hipGetLastError();
}

}  // namespace dqmc
