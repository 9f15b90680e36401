// taucov.hip — the kernel of the tau-tau' covariance accumulators (include/dqmc_hip.h "tau-tau' covariance"; host side in
// taucov.inl).
//
// A series is R values along tau of one walker's sample.  Per (walker, series) the state is the open bin's sum a[R], the
// shift c[R], S1[R] and S2[R][R] (row-major, full).  One push does a += x; a push that closes the bin (the host counts:
// all walkers close together, so `close` and `first` are launch arguments) goes on with
//     b = a / bin_size,  c = b on the walker's first bin,  d = b - c,  S1 += d,  S2[r][r'] += d[r] d[r'],  a = 0.
// Every stored value is one accumulator updated once per closed bin, bins in ascending order, no atomics and no reduction
// across lanes: the state depends on the walker's samples only, and S2[r][r'] and S2[r'][r] receive fma(d[r], d[r'], .)
// and fma(d[r'], d[r], .), the same bits.
//
// One workgroup of 256 lanes per (walker, series); for R <= TC_SMALL_R four series share it, one wave each, so that a
// short series does not leave three waves idle.  Three phases:
//   gather  the R values of the workgroup's series go from the sample into LDS.  Their stride in the sample is r_stride
//           (n_q in a momentum sample), so where series share the workgroup the lanes run over the series first:
//           neighbouring lanes read neighbouring q.  Their LDS rows are padded to an odd length, which keeps those
//           writes off a common bank.
//   state   lane r of a series' team updates a, and on a closing push c, S1 and leaves d[r] in LDS in place of x[r].
//   S2      the R^2 elements of the series are streamed once as a flat run, 16 bytes (two neighbours along r') per
//           lane and step; (r, r') of an element come from one 32-bit division.  A series' run starts on an odd double
//           when R and its index are odd, so a misaligned head element and a left-over tail element are done on their
//           own by the team's first lane, and R need not be a multiple of anything.  d[r] is uniform over most of a wave
//           (an LDS broadcast), d[r'] a run of neighbours.
// A push that closes no bin ends behind the state phase: R doubles read and written per series.  A closing push moves
// 2 R^2 doubles per series and does one FMA per element: memory-bound by construction.
#include "kernels.h"

namespace dqmc {

__global__ __launch_bounds__(TAUCOV_THREADS) void taucov_push_kernel(TauCovPush p, int spb)
{
    __shared__ double lds[TAUCOV_MAX_R];
    const int R = p.R, tps = TAUCOV_THREADS / spb;
    const int team = threadIdx.x / tps, t = threadIdx.x % tps, w = blockIdx.y;
    const int RP = spb == 1 ? R : (R | 1);
    const long first_series = (long)blockIdx.x * spb;  // (within this launch's n_series)
    const double *__restrict__ X = p.X + (long)w * p.x_walker + p.x_off;
    for (int e = threadIdx.x; e < spb * R; e += TAUCOV_THREADS) {
        const int sq = e % spb, r = e / spb;
        const long sl = first_series + sq;
        if (sl < p.n_series) {
            const long j = sl / p.n_q, q = sl % p.n_q;
            lds[sq * RP + r] = X[j * p.j_stride + (long)r * p.r_stride + q];
        }
    }
    __syncthreads();
    const long sl = first_series + team;
    const bool live = sl < p.n_series;
    const long so = (((long)w * p.S + p.series0 + sl) * R);  // this series' a / c / S1; its S2 starts at so * R
    double *__restrict__ d = lds + team * RP;
    if (live) {
        for (int r = t; r < R; r += tps) {
            const double a = p.a[so + r] + d[r];
            if (!p.close) {
                p.a[so + r] = a;
                continue;
            }
            const double b = a / p.bin_size;
            double c = b;
            if (p.first) p.c[so + r] = b;
            else c = p.c[so + r];
            const double dv = b - c;
            p.s1[so + r] += dv;
            p.a[so + r] = 0.0;
            d[r] = dv;
        }
    }
    if (!p.close) return;
    __syncthreads();
    if (!live) return;
    double *__restrict__ s2 = p.s2 + so * R;
    const unsigned n2 = (unsigned)R * (unsigned)R;
    const unsigned head = (unsigned)(((unsigned long long)s2 >> 3) & 1ull);  // (n2 >= 1)
    if (t == 0 && head) s2[0] = fma(d[0], d[0], s2[0]);
    const unsigned n_pairs = (n2 - head) >> 1;
    for (unsigned k = t; k < n_pairs; k += tps) {
        const unsigned e = head + 2u * k;
        const unsigned r0 = e / (unsigned)R, c0 = e - r0 * (unsigned)R;
        unsigned r1 = r0, c1 = c0 + 1u;
        if (c1 == (unsigned)R) {
            c1 = 0u;
            r1 = r0 + 1u;
        }
        double2 *__restrict__ at = reinterpret_cast<double2 *>(s2 + e);
        double2 v = *at;
        v.x = fma(d[r0], d[c0], v.x);
        v.y = fma(d[r1], d[c1], v.y);
        *at = v;
    }
    if (t == 0 && ((n2 - head) & 1u)) s2[n2 - 1] = fma(d[R - 1], d[R - 1], s2[n2 - 1]);
}

hipError_t launch_taucov_push(const TauCovPush &p, int n_walkers, hipStream_t s)
{
    if (p.R < 1 || p.R > TAUCOV_MAX_R || p.n_q < 1 || p.n_series < 1 || p.series0 < 0 || p.series0 + p.n_series > p.S
        || n_walkers < 1 || n_walkers > 65535 || !(p.bin_size >= 1.0) || !p.X || !p.a || !p.c || !p.s1 || !p.s2)
        return hipErrorInvalidValue;
    const int spb = p.R <= TAUCOV_SMALL_R ? TAUCOV_SMALL_SPB : 1;
    const long blocks = (p.n_series + spb - 1) / spb;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(taucov_push_kernel, dim3((unsigned)blocks, n_walkers), dim3(TAUCOV_THREADS), 0, s, p, spb);
    return hipGetLastError();
}

}  // namespace dqmc
