// ising_fss.inl - the finite-size-scaling measurement of ising.hip (include/dqmc_hip.h, "finite-size-scaling observables"):
// one stand-alone kernel that dqmc_mc_sweep launches behind every measured sweep when FSS is on, on the state the
// sweep's last kernel (sweep, cluster move or exchange round) left in device memory.  The sweep kernels, the cluster move
// and the exchange kernel are not touched: with FSS off the launches are those of a handle that never had it.
//
// Per measurement and walker: M4 = m2 m2 with m2 = (double)(M M) (one rounding; contraction is off in the kernel, so it
// is never fused into the running sum), and for each wave vector k Fc = sum_i s_i cos_q30[k][i], Fs likewise, in 64-bit
// integers (exact,
// order-free), S_k = ((double)Fc (double)Fc + (double)Fs (double)Fs) inv, inv = 1 / (N 2^60) from the host.
//
// One lane per walker, one wave per workgroup, and blockIdx.y = the pair the workgroup serves: pair 0 is (M2, M4),
// pair y >= 1 is (M2, S_{y-1}).  The pairs of a walker share nothing they write: each has its own sum, its own
// elements of the binner and its own copy of M2's compressor (mc_bin_push_shared, mc_bin_device.h).  All lanes of a
// wave visit the same site of the same table row, so the row is read with scalar loads; the walker's spin words come
// from conf[word][W], coalesced.  Results leave through ordinary vector stores.

// kernel argument of the FSS measurement; the tables are arguments of their own (read-only, not aliased)
struct FssArg {
    int n_k;
    double inv;                     // 1 / (N 2^60)
    double *sM4, *sS;               // [W], [8][W]
    long long *n_meas;              // [W]
    mc_bin_arg bin;                 // the FSS section of the binner: [L][2 + n_k][W], the same, [L][1 + n_k][W],
                                    // [L - 1][1 + n_k][2][W]
};

// The tables arrive padded: [n_k][32 nw] with zeros behind site N - 1 (dqmc_mc_set_fss), so that every spin word has its
// 32 entries, 128-byte aligned, and a row is read in whole int4s.  With m = 0 for an up spin and -1 for a down spin,
// s c = (c ^ m) - m: the loop adds c ^ m and the number of down bits is added once at the end (a padded entry is 0 under
// a 0 bit: -1 + 1).
__global__ __launch_bounds__(WAVE) void ising_fss_kernel(DevState s, FssArg f, const int4 *__restrict__ cos_q30,
                                                         const int4 *__restrict__ sin_q30, int y0)
{
#pragma clang fp contract(off)  // M4 and S_k are rounded before they are summed: the sums add the values the binner gets
    const int w = blockIdx.x * WAVE + threadIdx.x;
    if (w >= s.W) return;
    const int y = y0 + (int)blockIdx.y;  // (the host keeps y <= n_k)
    const int W = s.W, nw = s.nw;
    const long long M = s.M[w];
    const double m2 = (double)(M * M);
    double v;
    if (y == 0) {
        v = m2 * m2;
        const double sum = f.sM4[w];
        const long long n = f.n_meas[w];
        f.sM4[w] = sum + v;
        f.n_meas[w] = n + 1;
    } else {
        const int4 *__restrict__ ct = cos_q30 + (size_t)(y - 1) * nw * 8;  // uniform: scalar loads
        const int4 *__restrict__ st = sin_q30 + (size_t)(y - 1) * nw * 8;
        long long fc = 0, fs = 0;
        int down = 0;
        for (int j = 0; j < nw; ++j) {
            const unsigned int dn = ~s.conf[at(j, W, w)];  // bit = 1: spin down
            down += __popc(dn);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int4 c4 = ct[8 * j + q], s4 = st[8 * j + q];
                const int c[4] = {c4.x, c4.y, c4.z, c4.w}, sn[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int m = -(int)((dn >> (4 * q + b)) & 1u);
                    fc += (long long)(c[b] ^ m);
                    fs += (long long)(sn[b] ^ m);
                }
            }
        }
        fc += down;
        fs += down;
        const double dc = (double)fc, ds = (double)fs;
        v = (dc * dc + ds * ds) * f.inv;
        const double sum = f.sS[at(y - 1, W, w)];
        f.sS[at(y - 1, W, w)] = sum + v;
    }
    if (f.bin.xs) mc_bin_push_shared(f.bin, (size_t)(2 + f.n_k), (size_t)(1 + f.n_k), W, w, y, m2, v);
}
