// qs_scaling.inl - the finite-size-scaling measurement of qstate.hip (include/dqmc_hip.h, "Scaling" of the q-state
// section): one stand-alone kernel that dqmc_qs_sweep launches behind every measured sweep when the feature is on, on
// the configuration the sweep's last kernel (sweep or exchange round) left in device memory.  The sweep kernel, the
// exchange kernel and the cluster move are not touched: with the feature off the launches are those of a handle that
// never had it.
//
// One workgroup per walker, all wave vectors in one pass over the walker's Nw configuration words.  The per-state sums
// Ac[t], As[t] are integers, so any distribution over lanes gives the same bits: a lane takes whole words (four sites,
// one int4 of each table row) and adds every entry to the bin of its site's state with a 64-bit LDS atomic add.  What
// would serialise is many lanes of one instruction hitting one address, worst at q = 2 and 3 where all 256 lanes share
// two or three states.  So each bin is kept in R copies, R the largest power of two with q R <= 256, and a lane adds to
// copy tid mod R: for q <= 4 no two lanes of a wave share an address (R >= 64), at q = 8 two do and only when their sites
// agree, and at q = 64 (R = 4) the states themselves spread the lanes.  One table of one wave vector is 256 slots of 8
// bytes whatever q is, 4 KiB per wave vector in all, 32 KiB at n_k = 8.  Behind a barrier 2 q n_k lanes add their bin's
// copies up (in place, each its own slots), and behind another lane k < n_k does wave vector k: the four fp64
// contractions over t in the header's order, S_k, its running sum and its pair of the binner section.  Results leave
// through ordinary vector stores.
//
// The tables arrive padded: [n_k][4 Nw] with zeros behind site N - 1 (dqmc_qs_set_scaling), so that every configuration
// word has its int4, 16-byte aligned and in bounds.  The zero bytes that pad a walker's last word read as state 0 and
// add those zeros to bin 0: they are not counted.

constexpr int SC_MAX_K = 8;
constexpr int SC_SLOTS = 256;  // slots of one table of one wave vector: q states in R copies, q R <= 256

// kernel argument of the scaling measurement; the tables are arguments of their own (read-only, not aliased)
struct ScalingArgs {
    int n_k, shift;                 // R = 1 << shift
    double inv;                     // 1 / (N 2^120)
    double *sS;                     // [8][W]
    long long *n_meas;              // [W]
    mc_bin_arg bin;                 // the scaling section of the binner: [L][1 + n_k][W], the same, [L][n_k][W],
                                    // [L - 1][n_k][2][W]
};

static inline size_t scaling_lds_bytes(int n_k) { return (size_t)n_k * 2 * SC_SLOTS * sizeof(unsigned long long); }
static inline int scaling_shift(int q)  // the largest s with q 2^s <= SC_SLOTS (q <= 64: 2 at least)
{
    int s = 0;
    while ((q << (s + 1)) <= SC_SLOTS) ++s;
    return s;
}

// blockDim.x == THREADS, dynamic LDS scaling_lds_bytes(n_k); 1 <= n_k <= 8 and every state below q (the host's to keep)
__global__ __launch_bounds__(THREADS) void qs_scaling_kernel(DevState s, ScalingArgs f, const int4 *__restrict__ cos_q30,
                                                             const int4 *__restrict__ sin_q30,
                                                             const int2 *__restrict__ cs_q30)
{
#pragma clang fp contract(off)  // every product is rounded before it is added: the header's order of operations
    extern __shared__ __align__(16) unsigned char lds[];
    unsigned long long *bins = (unsigned long long *)lds;  // [n_k][2][SC_SLOTS]: cos then sin, slot (t << shift) + copy
    const int tid = threadIdx.x, w = blockIdx.x;
    if (w >= s.W) return;  // (uniform; the host's grid never gets here)
    const int Nw = s.Nw, q = s.q, n_k = f.n_k, sh = f.shift;
    for (int j = tid; j < n_k * 2 * SC_SLOTS; j += THREADS) bins[j] = 0ull;
    __syncthreads();
    {
        const unsigned int *conf = s.conf + (size_t)w * Nw;
        const int copy = tid & ((1 << sh) - 1);
        for (int j = tid; j < Nw; j += THREADS) {
            const unsigned int word = conf[j];
            int slot[4];
#pragma unroll
            for (int b = 0; b < 4; ++b)  // (a state is below q; the min keeps a slot inside the table come what may)
                slot[b] = (min((int)((word >> (8 * b)) & 0xFFu), q - 1) << sh) + copy;
            for (int k = 0; k < n_k; ++k) {
                const int4 c4 = cos_q30[(size_t)k * Nw + j], s4 = sin_q30[(size_t)k * Nw + j];
                const int c[4] = {c4.x, c4.y, c4.z, c4.w}, sn[4] = {s4.x, s4.y, s4.z, s4.w};
                unsigned long long *bc = bins + (size_t)k * 2 * SC_SLOTS, *bs = bc + SC_SLOTS;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    atomicAdd(&bc[slot[b]], (unsigned long long)(long long)c[b]);
                    atomicAdd(&bs[slot[b]], (unsigned long long)(long long)sn[b]);
                }
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < n_k * 2 * q; j += THREADS) {  // Ac[t], As[t]: the copies of one bin, into its first slot
        const int kt = j / q, t = j - kt * q;           // kt = 2 k + (0: cos, 1: sin)
        unsigned long long *b = bins + (size_t)kt * SC_SLOTS + ((size_t)t << sh);
        unsigned long long a = 0ull;
        for (int c = 0; c < (1 << sh); ++c) a += b[c];
        b[0] = a;
    }
    __syncthreads();
    if (tid < n_k) {
        const int k = tid, W = s.W;
        const unsigned long long *Ac = bins + (size_t)k * 2 * SC_SLOTS, *As = Ac + SC_SLOTS;
        double F1 = 0.0, F2 = 0.0, F3 = 0.0, F4 = 0.0;
        for (int t = 0; t < q; ++t) {
            const int2 u = cs_q30[t];
            const double c = (double)u.x, sn = (double)u.y;
            const double ac = (double)(long long)Ac[(size_t)t << sh], as = (double)(long long)As[(size_t)t << sh];
            F1 = F1 + c * ac;
            F2 = F2 + c * as;
            F3 = F3 + sn * ac;
            F4 = F4 + sn * as;
        }
        const double v = (((F1 * F1 + F2 * F2) + F3 * F3) + F4 * F4) * f.inv;
        const size_t at = (size_t)k * W + w;
        const double sum = f.sS[at];
        f.sS[at] = sum + v;
        if (k == 0) {
            const long long n = f.n_meas[w];
            f.n_meas[w] = n + 1;
        }
        if (f.bin.xs) {  // elements [M2, S_0 ..], pair k = (M2, S_k); m2 as qs_measure_slot and the sweep kernel form it
            const double x = (double)s.Mx[w] * Q30_INV, y = (double)s.My[w] * Q30_INV;
            mc_bin_push_shared(f.bin, (size_t)(1 + f.n_k), (size_t)f.n_k, W, w, k, x * x + y * y, v);
        }
    }
}
