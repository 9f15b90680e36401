// qs_stiffness.inl - the helicity-modulus measurement of qstate.hip (include/dqmc_hip.h, "Stiffness" of the q-state
// section): one stand-alone kernel that dqmc_qs_sweep launches behind every measured sweep when the feature is on, behind
// the scaling kernel where that is on as well, on the configuration the sweep's last kernel (sweep or exchange round)
// left in device memory.  No other kernel is touched: with the feature off the launches are those of a handle that
// never had it.
//
// One workgroup per walker.  The walker's Nw configuration words are staged into LDS (16 KiB at most), the two q-entry
// twist tables beside them; the neighbour reads are byte gathers from there.  A lane takes the sites tid, tid + THREADS,
// ..: one 32-byte neighbour row and one 8-byte row of slot classes per site, and for every slot with a class >= 0 the
// table entries of the difference go into the class's pair of int64 accumulators.  The accumulators are registers: the
// class index selects by comparison (8 predicated adds per slot), never by address.  Integers make any order exact, so
// the reduction is free in its shape: xor-shuffles inside a wave, one LDS slot per wave and value, and behind a barrier
// lane c < n_c adds the four waves' values of class c, keeps them in LDS and stores the sample.  Behind another barrier
// lane mu < n_dir does direction mu: the two fp64 contractions over the classes in the header's order, the three running
// sums and its pair of the binner section.  Results leave through ordinary vector stores.
//
// The padding bytes of a walker's last word are never visited (the site loop ends at N), and a neighbour index is below N
// by dqmc_qs_create's validation.

constexpr int ST_MAX_DIR = 4;
constexpr int ST_MAX_CLASSES = 8;

// kernel argument of the stiffness measurement; the tables are arguments of their own (read-only, not aliased)
struct StiffnessArgs {
    int n_dir, n_c;
    double x[ST_MAX_DIR][ST_MAX_CLASSES];  // x[mu][c], the projection of class c on direction mu
    double *sT, *sJ, *sJ2;                 // [4][W]
    long long *n_meas;                     // [W]
    long long *sI, *sK;                    // [8][W]: the class sums of the last sample
    mc_bin_arg bin;                        // the stiffness section of the binner: [L][2 n_dir][W], the same,
                                           // [L][n_dir][W], [L - 1][2 n_dir][W]
};

// d1 and d2 (q int64 each), 4 x 16 wave partials, 16 totals, the configuration words: 18 KiB at q = 64 and N = 16384
static inline size_t stiffness_lds_bytes(int q, int Nw)
{
    return (size_t)16 * q + (size_t)(THREADS / WAVE + 1) * 2 * ST_MAX_CLASSES * 8 + (size_t)4 * Nw;
}

// The push of pair p with the values (a, b) = (T_p, J2_p): elements [T_0, J2_0, T_1, J2_1 ..], pair p = (2 p, 2 p + 1),
// state [level][element][walker].  The pairs of a walker share nothing: each lane has its two elements, its cross sum
// and its two compressor values.  The level scheme is mc_bin_push_shared's (mc_bin_device.h).
__device__ __forceinline__ void qs_stiffness_bin_push(const mc_bin_arg &f, int n_dir, int W, int w, int p, double a, double b)
{
    const size_t sW = (size_t)W, ne = (size_t)(2 * n_dir), np = (size_t)n_dir;
    size_t ie = (size_t)(2 * p) * sW + w, ip = (size_t)p * sW + w;
    for (int l = 0;; ++l, ie += ne * sW, ip += np * sW) {
        const bool last = l == f.lmax;
        const double a1 = f.xs[ie], b1 = f.xs[ie + sW], a2 = f.x2[ie], b2 = f.x2[ie + sW], pr = f.xy[ip];
        double ca = 0.0, cb = 0.0;
        if (!last) {
            ca = f.c[ie];
            cb = f.c[ie + sW];
        }
        f.xs[ie] = a1 + a;
        f.xs[ie + sW] = b1 + b;
        f.x2[ie] = a2 + a * a;
        f.x2[ie + sW] = b2 + b * b;
        f.xy[ip] = pr + a * b;
        if (last) break;
        a = 0.5 * (ca + a);
        b = 0.5 * (cb + b);
    }
    if (f.lmax < f.top) {  // (the top level has no compressor; the compressor's [level][element][walker] is the sums')
        f.c[ie] = a;
        f.c[ie + sW] = b;
    }
}

// blockDim.x == THREADS, dynamic LDS stiffness_lds_bytes(q, Nw).  nbr: [N][8] 0-based neighbour rows, cls: [N][8] slot
// classes (-1: not counted; the entries at and behind z are -1), d1 / d2: [q]
__global__ __launch_bounds__(THREADS) void qs_stiffness_kernel(DevState s, StiffnessArgs f, const int4 *__restrict__ nbr,
                                                               const int2 *__restrict__ cls,
                                                               const long long *__restrict__ d1_q30,
                                                               const long long *__restrict__ d2_q30)
{
#pragma clang fp contract(off)  // every product is rounded before it is added: the header's order of operations
    extern __shared__ __align__(16) unsigned char lds[];
    const int tid = threadIdx.x, w = blockIdx.x;
    if (w >= s.W) return;  // (uniform; the host's grid never gets here)
    const int N = s.N, Nw = s.Nw, q = s.q, z = s.z, n_c = f.n_c;
    constexpr int NV = 2 * ST_MAX_CLASSES, NWAVES = THREADS / WAVE;
    long long *t1 = (long long *)lds;          // [q]
    long long *t2 = t1 + q;                    // [q]
    long long *part = t2 + q;                  // [NWAVES][NV]
    long long *tot = part + NWAVES * NV;       // [NV]: I_c at c, K_c at 8 + c
    unsigned int *stw = (unsigned int *)(tot + NV);
    const unsigned char *st = (const unsigned char *)stw;
    {
        const unsigned int *src = s.conf + (size_t)w * Nw;
        for (int j = tid; j < Nw; j += THREADS) stw[j] = src[j];
        for (int j = tid; j < q; j += THREADS) {
            t1[j] = d1_q30[j];
            t2[j] = d2_q30[j];
        }
    }
    __syncthreads();
    long long acc[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[c] = 0;
    for (int i = tid; i < N; i += THREADS) {
        const int4 n0 = nbr[2 * i], n1 = nbr[2 * i + 1];
        const int2 cw = cls[i];
        const int nb[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
        const int si = st[i];
#pragma unroll
        for (int k = 0; k < MAX_Z; ++k) {
            const int cl = (int)(signed char)(((k < 4 ? (unsigned int)cw.x : (unsigned int)cw.y) >> (8 * (k & 3))) & 0xFFu);
            if (k < z && cl >= 0) {
                // (in 0 .. N - 1 by the host's validation; the unsigned min keeps the read in the image come what may)
                const int j = (int)min((unsigned int)nb[k], (unsigned int)(N - 1));
                const int d = max(0, min(mod_q(si - (int)st[j], q), q - 1));  // (a state is below q: in 0 .. q - 1 as it is)
                const long long a = t1[d], b = t2[d];
#pragma unroll
                for (int c = 0; c < ST_MAX_CLASSES; ++c) {
                    acc[c] += cl == c ? a : 0ll;
                    acc[ST_MAX_CLASSES + c] += cl == c ? b : 0ll;
                }
            }
        }
    }
    const int wave = tid / WAVE;
#pragma unroll
    for (int c = 0; c < ST_MAX_CLASSES; ++c) {
        if (c < n_c) {  // (uniform)
            const long long a = wave_sum(acc[c]), b = wave_sum(acc[ST_MAX_CLASSES + c]);
            if ((tid & (WAVE - 1)) == 0) {
                part[wave * NV + c] = a;
                part[wave * NV + ST_MAX_CLASSES + c] = b;
            }
        }
    }
    __syncthreads();
    const int W = s.W;
    if (tid < n_c) {
        long long a = 0, b = 0;
#pragma unroll
        for (int v = 0; v < NWAVES; ++v) {
            a += part[v * NV + tid];
            b += part[v * NV + ST_MAX_CLASSES + tid];
        }
        tot[tid] = a;
        tot[ST_MAX_CLASSES + tid] = b;
        f.sI[(size_t)tid * W + w] = a;
        f.sK[(size_t)tid * W + w] = b;
    }
    __syncthreads();
    if (tid < f.n_dir) {
        const int mu = tid;
        double G = 0.0, F = 0.0;
        for (int c = 0; c < n_c; ++c) {
            const double x = f.x[mu][c];
            const double x2 = x * x;
            G = G + x * (double)tot[c];
            F = F + x2 * (double)tot[ST_MAX_CLASSES + c];
        }
        const double Jv = G * Q30_INV, Tv = F * Q30_INV;
        const double J2 = Jv * Jv;
        const size_t at = (size_t)mu * W + w;
        const double sT = f.sT[at], sJ = f.sJ[at], sJ2 = f.sJ2[at];  // requested together
        f.sT[at] = sT + Tv;
        f.sJ[at] = sJ + Jv;
        f.sJ2[at] = sJ2 + J2;
        if (mu == 0) {
            const long long n = f.n_meas[w];
            f.n_meas[w] = n + 1;
        }
        if (f.bin.xs) qs_stiffness_bin_push(f.bin, f.n_dir, W, w, mu, Tv, J2);
    }
}
