// ising_sweep.inl - the two sweep kernels of ising.hip, included twice: ISING_EXCHANGE 0 defines ising_sweep_kernel<Z> and
// ising_sweep_binned_kernel<Z>; ISING_EXCHANGE 1 defines ising_sweep_exchange_kernel<Z> and
// ising_sweep_binned_exchange_kernel<Z>, the same kernels with an exchange round (ising_exchange_round) after every
// sweep g with g % x.rate == 0 && g != deferred_sweep (that one's round follows the cluster move, ising_exchange_kernel)
// and a trailing argument Exchange x.  The round is a compile-time option by the preprocessor, so that the forms
// without it have the argument list and, instruction for instruction, the code they had before the option existed
// (tools/diff_kernel_isa.py); sharing the body through a __device__ function gives them other registers and another
// instruction order, as it did for the site loop.
#if ISING_EXCHANGE
#define ISING_SWEEP_KERNEL ising_sweep_exchange_kernel
#define ISING_SWEEP_BINNED_KERNEL ising_sweep_binned_exchange_kernel
#define ISING_EXCHANGE_ARG , Exchange x
#else
#define ISING_SWEEP_KERNEL ising_sweep_kernel
#define ISING_SWEEP_BINNED_KERNEL ising_sweep_binned_kernel
#define ISING_EXCHANGE_ARG
#endif

// the neighbour table is a kernel argument of its own, read-only and not aliased: that is what lets the compiler read
// a row with one scalar load (a member of DevState would be an ordinary pointer the kernel's stores might alias)
template <int Z>
__global__ __launch_bounds__(WAVE) void ISING_SWEEP_KERNEL(DevState s, const int4 *__restrict__ nbr, int n_sweeps,
                                                           long long first_sweep, long long thermalization,
                                                           int measure_rate, long long deferred_sweep ISING_EXCHANGE_ARG)
{
    extern __shared__ unsigned int sp[];
    const int lane = threadIdx.x;
    const int w = blockIdx.x * WAVE + lane;
    if (w >= s.W) return;
    const int N = s.N, nw = s.nw, W = s.W;
    for (int j = 0; j < nw; ++j) sp[j * WAVE + lane] = s.conf[at(j, W, w)];
    const unsigned long long key = s.key[w];
    unsigned long long draw = s.draw[w];
    int E = s.E[w], M = s.M[w];
    double thr[Z];
#pragma unroll
    for (int k = 0; k < Z; ++k) thr[k] = s.thr[at(k, W, w)];
    double sE = s.sE[w], sE2 = s.sE2[w], sM = s.sM[w], sM2 = s.sM2[w];
    long long n_meas = s.n_meas[w], n_series = s.n_series[w], acc = 0;
#if ISING_EXCHANGE
    const int il = w % x.R, sgn = x.sgn[w];
    int rep = x.replica[w];
    long long xprop = 0, xacc = 0;
    unsigned long long xc = x.x;
#endif

    for (int sw = 0; sw < n_sweeps; ++sw) {
        int cw = 0;
        unsigned int cur = sp[lane];
        int4 r0 = nbr[0], r1 = nbr[1];  // row of site 0; the row of site i + 1 is requested while site i runs
        for (int i = 0; i < N; ++i) {
            const int iw = i >> 5, ib = i & 31;
            if (iw != cw) {  // uniform: the previous word is complete
                sp[cw * WAVE + lane] = cur;
                cw = iw;
                cur = sp[cw * WAVE + lane];
            }
            const int row[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
            r0 = nbr[2 * i + 2];  // (the table holds N + 1 rows)
            r1 = nbr[2 * i + 3];
            int up = 0;
#pragma unroll
            for (int k = 0; k < Z; ++k) {
                const int j = row[k], jw = j >> 5;
                const unsigned int v = jw == iw ? cur : sp[jw * WAVE + lane];
                up += (v >> (j & 31)) & 1u;
            }
            const int si = (cur >> ib) & 1u;
            const int sum = 2 * up - Z;         // sum of the neighbours' spins
            const int k = si ? sum : -sum;      // dE / 2
            bool accept = k <= 0;
            if (k > 0) {
                const double u = dqmc::philox_uniform(key, draw);
                ++draw;
                double t = thr[0];
#pragma unroll
                for (int q = 1; q < Z; ++q) t = k == q + 1 ? thr[q] : t;
                accept = u < t;
            }
            if (accept) {
                cur ^= 1u << ib;
                E += 2 * k;
                M += si ? -2 : 2;
                ++acc;
            }
        }
        sp[cw * WAVE + lane] = cur;
        const long long g = first_sweep + sw;  // global 1-based sweep index (MC.jl:262-283)
#if ISING_EXCHANGE
        if (g % x.rate == 0 && g != deferred_sweep) {
            ising_exchange_round(sp, x, xc, lane, w, W, nw, il, key, sgn, E, M, rep, xprop, xacc);
            ++xc;
        }
#endif
        // the measurement of deferred_sweep (-1: none) follows that sweep's cluster move (ising_wolff_kernel)
        if (g > thermalization && g % measure_rate == 0 && g != deferred_sweep) {
            const double e = (double)E, m = (double)(M < 0 ? -M : M);
            sE += e;
            sE2 += e * e;
            sM += m;
            sM2 += m * m;
            if (n_series < s.cap) {
                s.serE[at((int)n_series, W, w)] = E;
                s.serM[at((int)n_series, W, w)] = M < 0 ? -M : M;
                ++n_series;
            }
            ++n_meas;
        }
    }
    for (int j = 0; j < nw; ++j) s.conf[at(j, W, w)] = sp[j * WAVE + lane];
    s.draw[w] = draw;
    s.E[w] = E;
    s.M[w] = M;
    s.sE[w] = sE;
    s.sE2[w] = sE2;
    s.sM[w] = sM;
    s.sM2[w] = sM2;
    s.n_meas[w] = n_meas;
    s.n_series[w] = n_series;
    s.prop[w] += (long long)n_sweeps * N;
    s.acc[w] += acc;
#if ISING_EXCHANGE
    x.replica[w] = rep;
    x.prop[w] += xprop;
    x.acc[w] += xacc;
#endif
}

// ising_sweep_kernel with the binner on: the same chain, and every measurement is pushed where it is taken.  T = pushes
// before this launch (all walkers of a handle measure at the same sweeps, so one count serves them all and the cascade
// length of a push is the same in every lane).  The site loop is a copy, not a shared helper: routed through one, the
// eight forms above come out with other registers and another instruction order.
template <int Z>
__global__ __launch_bounds__(WAVE) void ISING_SWEEP_BINNED_KERNEL(DevState s, const int4 *__restrict__ nbr,
                                                                  int n_sweeps, long long first_sweep,
                                                                  long long thermalization, int measure_rate,
                                                                  long long deferred_sweep, double *__restrict__ bxs,
                                                                  double *__restrict__ bx2, double *__restrict__ bxy,
                                                                  double *__restrict__ bc, int top,
                                                                  long long T ISING_EXCHANGE_ARG)
{
    extern __shared__ unsigned int sp[];
    const int lane = threadIdx.x;
    const int w = blockIdx.x * WAVE + lane;
    if (w >= s.W) return;
    const int N = s.N, nw = s.nw, W = s.W;
    for (int j = 0; j < nw; ++j) sp[j * WAVE + lane] = s.conf[at(j, W, w)];
    const unsigned long long key = s.key[w];
    unsigned long long draw = s.draw[w];
    int E = s.E[w], M = s.M[w];
    double thr[Z];
#pragma unroll
    for (int k = 0; k < Z; ++k) thr[k] = s.thr[at(k, W, w)];
    double sE = s.sE[w], sE2 = s.sE2[w], sM = s.sM[w], sM2 = s.sM2[w];
    long long n_meas = s.n_meas[w], n_series = s.n_series[w], acc = 0;
#if ISING_EXCHANGE
    const int il = w % x.R, sgn = x.sgn[w];
    int rep = x.replica[w];
    long long xprop = 0, xacc = 0;
    unsigned long long xc = x.x;
#endif

    for (int sw = 0; sw < n_sweeps; ++sw) {
        int cw = 0;
        unsigned int cur = sp[lane];
        int4 r0 = nbr[0], r1 = nbr[1];  // row of site 0; the row of site i + 1 is requested while site i runs
        for (int i = 0; i < N; ++i) {
            const int iw = i >> 5, ib = i & 31;
            if (iw != cw) {  // uniform: the previous word is complete
                sp[cw * WAVE + lane] = cur;
                cw = iw;
                cur = sp[cw * WAVE + lane];
            }
            const int row[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
            r0 = nbr[2 * i + 2];  // (the table holds N + 1 rows)
            r1 = nbr[2 * i + 3];
            int up = 0;
#pragma unroll
            for (int k = 0; k < Z; ++k) {
                const int j = row[k], jw = j >> 5;
                const unsigned int v = jw == iw ? cur : sp[jw * WAVE + lane];
                up += (v >> (j & 31)) & 1u;
            }
            const int si = (cur >> ib) & 1u;
            const int sum = 2 * up - Z;         // sum of the neighbours' spins
            const int k = si ? sum : -sum;      // dE / 2
            bool accept = k <= 0;
            if (k > 0) {
                const double u = dqmc::philox_uniform(key, draw);
                ++draw;
                double t = thr[0];
#pragma unroll
                for (int q = 1; q < Z; ++q) t = k == q + 1 ? thr[q] : t;
                accept = u < t;
            }
            if (accept) {
                cur ^= 1u << ib;
                E += 2 * k;
                M += si ? -2 : 2;
                ++acc;
            }
        }
        sp[cw * WAVE + lane] = cur;
        const long long g = first_sweep + sw;  // global 1-based sweep index (MC.jl:262-283)
#if ISING_EXCHANGE
        if (g % x.rate == 0 && g != deferred_sweep) {
            ising_exchange_round(sp, x, xc, lane, w, W, nw, il, key, sgn, E, M, rep, xprop, xacc);
            ++xc;
        }
#endif
        // the measurement of deferred_sweep (-1: none) follows that sweep's cluster move (ising_wolff_kernel)
        if (g > thermalization && g % measure_rate == 0 && g != deferred_sweep) {
            const double e = (double)E, m = (double)(M < 0 ? -M : M);
            sE += e;
            sE2 += e * e;
            sM += m;
            sM2 += m * m;
            if (n_series < s.cap) {
                s.serE[at((int)n_series, W, w)] = E;
                s.serM[at((int)n_series, W, w)] = M < 0 ? -M : M;
                ++n_series;
            }
            ++n_meas;
            ising_bin_push(bxs, bx2, bxy, bc, W, w, min(top, __builtin_ctzll(~(unsigned long long)T)), top, e, m);
            ++T;
        }
    }
    for (int j = 0; j < nw; ++j) s.conf[at(j, W, w)] = sp[j * WAVE + lane];
    s.draw[w] = draw;
    s.E[w] = E;
    s.M[w] = M;
    s.sE[w] = sE;
    s.sE2[w] = sE2;
    s.sM[w] = sM;
    s.sM2[w] = sM2;
    s.n_meas[w] = n_meas;
    s.n_series[w] = n_series;
    s.prop[w] += (long long)n_sweeps * N;
    s.acc[w] += acc;
#if ISING_EXCHANGE
    x.replica[w] = rep;
    x.prop[w] += xprop;
    x.acc[w] += xacc;
#endif
}

#undef ISING_SWEEP_KERNEL
#undef ISING_SWEEP_BINNED_KERNEL
#undef ISING_EXCHANGE_ARG
