// ising_cb.inl - the checkerboard sweep of ising.hip (include/dqmc_hip.h, "checkerboard sweeps"): a defined extension like
// the cluster move and replica exchange, on a Philox domain of its own (counter word 2 = 3).  The sequential kernels
// (ising_sweep.inl) are one lane per chain; here one workgroup sweeps one walker, colour class by colour class: the sites
// of a class share no bond, so they are decided side by side from the configuration as it stood when the class began,
// and the outcome is one configuration whatever order the lanes take them in.
//
// The walker's spins are bit-packed in LDS as in device memory (bit i & 31 of word i >> 5, at most 2 KiB).  The host
// passes the sites sorted by colour (site[e], class c = entries off[c] .. off[c + 1]) and their padded neighbour rows in
// that same order (rows[e] = the row of site[e]), so that a wave reads consecutive rows.  Lane t takes the entries
// off[c] + t, + blockDim, ..; the lanes of a class may meet in one spin word, so a flip is an LDS atomic XOR of the site's
// bit (its own bit and its neighbours' bits are not touched by any other lane of the class: a plain read of the word
// beside those XORs sees them as they were when the class began).  One workgroup barrier ends a class.
//
// dE, dM and the accepted flips add up in registers (dE is additive within a class: no two of its sites share a bond)
// and are reduced over the workgroup only where E or M is needed: at a measurement and at the end of the launch.  A
// measurement is taken by lane 0 through ising_measure_slot, and pushed through ising_bin_push when the binner is on.
// The block is as many whole waves as the largest class needs, 256 lanes at most: nothing observable depends on it.

constexpr int CB_THREADS = 256;
constexpr int CB_MAX_COLOURS = 16;

// kernel argument of the checkerboard sweep; the tables are arguments of their own (read-only, not aliased)
struct CbArg {
    int C, z;                      // colour classes, neighbours per site
    unsigned long long *cursor;    // [W], checkerboard sweeps of the slot since dqmc_mc_seed
    double *bxs, *bx2, *bxy, *bc;  // the binner (bxs == nullptr: off), as ising_sweep_binned_kernel gets it
    int top;
    long long T;                   // pushes before this launch
};

__device__ __forceinline__ int ising_cb_wave_sum(int v)
{
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(CB_THREADS) void ising_cb_kernel(DevState s, CbArg a, const int *__restrict__ site,
                                                              const int4 *__restrict__ rows,
                                                              const int *__restrict__ off, int n_sweeps,
                                                              long long first_sweep, long long thermalization,
                                                              int measure_rate, long long deferred_sweep)
{
    __shared__ unsigned int sp[MAX_SITES / 32];
    __shared__ double thr[MAX_Z];
    __shared__ int red[4];  // [0] E, [1] M as of the last reduction, [2] accepted flips of the launch
    const int tid = threadIdx.x, nt = blockDim.x, w = blockIdx.x;
    const int N = s.N, nw = s.nw, W = s.W, z = a.z, C = a.C;
    for (int j = tid; j < nw; j += nt) sp[j] = s.conf[at(j, W, w)];
    if (tid < MAX_Z) thr[tid] = s.thr[at(tid, W, w)];
    if (tid == 0) {
        const int E = s.E[w], M = s.M[w];
        red[0] = E;
        red[1] = M;
        red[2] = 0;
    }
    const unsigned long long key = s.key[w];
    unsigned long long sc = a.cursor[w];
    long long T = a.T;
    // the next measured sweep at or behind first_sweep (MC.jl:262-283): one division per launch, none per sweep
    const long long g0 = first_sweep > thermalization + 1 ? first_sweep : thermalization + 1;
    long long next = (g0 + measure_rate - 1) / measure_rate * measure_rate;
    int dE = 0, dM = 0, acc = 0;
    __syncthreads();

    for (int sw = 0; sw < n_sweeps; ++sw, ++sc) {
        const unsigned int c1 = (unsigned int)sc, c3 = (unsigned int)(sc >> 32);
        for (int c = 0; c < C; ++c) {
            const int e1 = off[c + 1];
            for (int e = off[c] + tid; e < e1; e += nt) {
                const int i = site[e];
                const int4 r0 = rows[2 * e], r1 = rows[2 * e + 1];
                const int row[MAX_Z] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
                int up = 0;
#pragma unroll
                for (int k = 0; k < MAX_Z; ++k)
                    if (k < z) up += (sp[row[k] >> 5] >> (row[k] & 31)) & 1u;
                const unsigned int bit = 1u << (i & 31);
                const bool si = (sp[i >> 5] & bit) != 0u;
                const int sum = 2 * up - z;     // sum of the neighbours' spins
                const int k = si ? sum : -sum;  // dE / 2
                bool accept = k <= 0;
                if (k > 0) accept = dqmc::philox4_uniform(key, (unsigned int)i, c1, 3u, c3) < thr[k - 1];
                if (accept) {
                    atomicXor(&sp[i >> 5], bit);
                    dE += 2 * k;
                    dM += si ? -2 : 2;
                    ++acc;
                }
            }
            __syncthreads();
        }
        const long long g = first_sweep + sw;  // global 1-based sweep index
        if (g != next) continue;               // (uniform)
        next += measure_rate;
        // the measurement of deferred_sweep (-1: none) follows that sweep's cluster move or exchange round
        if (g == deferred_sweep) continue;
        const int e = ising_cb_wave_sum(dE), m = ising_cb_wave_sum(dM);
        dE = dM = 0;
        if ((tid & (WAVE - 1)) == 0) {
            atomicAdd(&red[0], e);
            atomicAdd(&red[1], m);
        }
        __syncthreads();  // (the next write of red[0..1] lies behind the next sweep's barriers)
        if (tid == 0) {
            const int E = red[0], M = red[1];
            ising_measure_slot(s, w, E, M);
            if (a.bxs)
                ising_bin_push(a.bxs, a.bx2, a.bxy, a.bc, W, w, min(a.top, __builtin_ctzll(~(unsigned long long)T)), a.top,
                               (double)E, (double)(M < 0 ? -M : M));
        }
        ++T;
    }

    __syncthreads();
    {
        const int e = ising_cb_wave_sum(dE), m = ising_cb_wave_sum(dM), n = ising_cb_wave_sum(acc);
        if ((tid & (WAVE - 1)) == 0) {
            atomicAdd(&red[0], e);
            atomicAdd(&red[1], m);
            atomicAdd(&red[2], n);
        }
    }
    __syncthreads();
    for (int j = tid; j < nw; j += nt) s.conf[at(j, W, w)] = sp[j];
    if (tid == 0) {
        const long long prop = s.prop[w], accd = s.acc[w];  // requested together
        s.E[w] = red[0];
        s.M[w] = red[1];
        s.prop[w] = prop + (long long)n_sweeps * N;
        s.acc[w] = accd + red[2];
        a.cursor[w] = sc;
    }
}
