// ising.hip — the classical MC flavor (src/flavors/MC/MC.jl) with the IsingModel (src/models/Ising/IsingModel.jl),
// batched over independent Markov chains: kernels and the dqmc_mc_* C ABI (include/dqmc_hip.h).
//
// A chain is strictly sequential (sites 1..N in order, MC.jl:316-333), so the only parallelism is across walkers:
// one lane per walker, one wave per workgroup.  All lanes visit the same site at the same time, so the site index and
// its row of the neighbour table are wave-uniform (scalar loads).  A walker's spins stay in LDS for the whole launch,
// bit-packed as [word][lane] (bit i & 31 of word i >> 5, 1 = spin +1): a per-lane read of a uniform word index touches
// 64 consecutive dwords, one per bank.  The word that holds the current site lives in a register, so the dependency
// through the previous site's spin (the "down" neighbour i - 1 is almost always in the same word) is a register
// forward, not an LDS round trip.
//
// Metropolis: dE = 2 s_i sum_j s_j = 2k with k in -z..z.  k <= 0 accepts without a draw; k > 0 draws the walker's next
// Philox4x32-10 uniform (key = seed, counter = draw index, as orc_ising_run) and accepts iff u < thr[k], where
// thr[k] = exp(-beta 2k) comes from the host's libm: no exp on the device, so every decision is bit-identical to the
// oracle's.  E and M are tracked incrementally; a measurement adds E, E^2, |M|, M^2 to fp64 sums (exact integers).
//
// Wolff cluster move: global_move(mc, m::IsingModel, conf) (IsingModel.jl:104-140) with its evident intent
// (m.energy[] = energy(mc, m, conf) where the reference writes the undefined `model`), defined on a stream of its own so
// that it does not depend on the traversal order or on how the device parallelises the growth:
//   u(m, t) = Philox4x32-10, key = the walker's seed, counter words (t, low32(m), 1, high32(m)), made into a uniform as
//             philox_uniform does; m = the walker's move cursor (Wolff moves since dqmc_mc_seed).  Local draws have
//             c2 = c3 = 0, so the two domains never overlap.
//   seed site       min(N - 1, floor(u(m, 0) N))
//   slot (i, k)     0-based site i, k < z: active iff s_i == s_{neighs[k, i]} and u(m, 1 + 8 i + k) < p_w
//   cluster C       the sites reachable from the seed through active slots; every site of C is flipped (a one-site
//                   cluster too), accepted = |C| > 1, then E is recomputed over the bonds table and M by popcount
//   p_w             1 - exp(-2 beta) from the host's libm (dqmc_mc_set_beta), compared in fp64
// Only the slots leaving C decide its boundary, (1 - p)^(aligned boundary bonds); the internal factor is the same before
// and after the flip, so detailed balance holds.  Where neighs repeats a site (SquareLattice(2), short chains) the double
// bond counts twice in the Metropolis dE, and two independent slot tests, 1 - (1 - p)^2, are its Fortuin-Kasteleyn
// probability.  In run! order (MC.jl:230-242) the move of sweep i follows that sweep's local sweep and precedes its
// measurement.
//
// Replica exchange (parallel tempering; the reference has no such move, this is a defined extension like the cluster
// move): the handle's walkers form n_walkers / R ladders of R consecutive slots.  A slot keeps what belongs to its
// temperature (beta and tables, key and cursors, sums, series, binner, counters); an accepted exchange swaps the
// configurations of two neighbouring slots: the spin words, E, M and the replica label.  Round x (the handle's exchange
// cursor, 0 after dqmc_mc_set_exchange, + 1 per round) tries the pairs (i, i + 1), i = x mod 2, i + 1 < R, ladder-local.
// For slots (a, b = a + 1): d = (E_a - E_b) / 2 (an integer: E = n_bonds mod 2), db = beta_a - beta_b (host, fp64).  The
// pair swaps if db == 0, d == 0 or db and d have the same sign; otherwise iff u < p with p = the product, in ascending
// j, of q[j] = exp(-2 |db| 2^j) (host libm, a table per pair) over the set bits j of |d|, and
// u = philox4_uniform(key_a, low32(x), high32(x), 2, 0): a third domain, c2 = 2.  No exp on the device, and products
// of doubles are exactly rounded, so a host restatement reproduces every decision bit for bit.  In a sweep the order
// is local sweep, cluster move, exchange round, measurement.
//
// Finite-size-scaling observables (the reference measures E and M only; a defined extension, include/dqmc_hip.h): with
// FSS on every measurement also takes M4 = m2 m2, m2 = (double)(M M), and for each of the n_k <= 8 wave vectors the host
// passed as fixed-point tables cos_q30[k][i] = llround(cos(k . r_i) 2^30), sin_q30 likewise (int32 [n_k][N]):
//   Fc_k = sum_i s_i cos_q30[k][i], Fs_k = sum_i s_i sin_q30[k][i]   in 64-bit integers, |F| <= 2^44: exact, order-free
//   S_k  = ((double)Fc (double)Fc + (double)Fs (double)Fs) * (1 / (N 2^60))
// on the configuration E and |M| of that measurement are taken on (after the sweep's cluster move and exchange round; the
// values belong to the slot).  Per walker sum_M4, sum_S[8] and an n_meas of their own; with the binner on a second section
// over [M2, M4, S_0 ..] with the cross sums (M2, M4) and (M2, S_k).  A stand-alone kernel (ising_fss.inl) that
// dqmc_mc_sweep launches behind every measured sweep: the kernels above it in this file are the same with FSS on or off.
//
// Checkerboard sweep (dqmc_mc_set_update; the reference's sweep(mc) is sequential, so this is another defined extension,
// opt-in): a colouring c_i in [0, C), C <= 16, no site sharing its colour with a neighbour; a sweep visits the colours in
// order, and within a colour every site is decided from the configuration as it stood when the colour began, with the
// Metropolis rule and threshold table above and u_cb(s, i) = philox4_uniform(key, i, low32(s), 3, high32(s)), s = the
// slot's checkerboard sweeps since dqmc_mc_seed: a fourth domain, c2 = 3.  One workgroup per walker (ising_cb.inl);
// the sequential kernels, their launches and their results are untouched while the mode is off.
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dqmc_hip.h"
#include "kernels.h"
#include "mc_bin_device.h"
#include "mc_host.h"

namespace dqmc_mc {

constexpr int MAX_SITES = 16384;  // 512 words x 64 lanes x 4 B = 128 KiB of LDS per workgroup
constexpr int MAX_Z = 8;
constexpr int WAVE = 64;
constexpr int MAX_XJ = 17;  // entries of an exchange pair's table: 2^J > n_bonds, n_bonds <= MAX_Z MAX_SITES / 2 = 2^16
// one launch runs at most this many site visits summed over its walkers (sites x sweeps x walkers), a handle with
// fewer than BUDGET_WALKERS walkers counted as that many (their waves run side by side, so a launch takes as long as
// one walker's chain); dqmc_mc_sweep splits its sweeps into launches of at least one sweep each, so that no single
// kernel holds the GPU for long
constexpr double LAUNCH_BUDGET = 268435456.0;
constexpr double BUDGET_WALKERS = 16384.0;

struct DevState {
    int N, W, nw, cap;
    const int *nbr;                 // [N + 1][8] 0-based, rows padded to 8 (row N: read ahead, unused)
    const int *__restrict__ bonds;  // [n_bonds][2] 0-based
    int n_bonds;
    unsigned int *conf;             // [nw][W]
    unsigned long long *key, *draw;
    int *E, *M;
    double *thr;                    // [8][W], thr[k - 1] = exp(-beta 2k)
    double *pw;                     // [W], 1 - exp(-2 beta): the cluster move's bond probability
    unsigned long long *moves;      // [W], the cluster move cursor
    long long *gprop, *gacc, *gsum; // [W], moves, moves with |C| > 1, sum of |C|
    double *sE, *sE2, *sM, *sM2;
    long long *n_meas, *prop, *acc, *n_series;
    int *serE, *serM;               // [cap][W]
};

// flat index of lane `w` in the [row][W] arrays
__device__ __forceinline__ size_t at(int row, int W, int w) { return (size_t)row * W + w; }

// replica exchange: a kernel argument of its own, so that DevState keeps its layout
struct Exchange {
    int R, rate, J;               // ladder length, a round after every rate-th sweep (0: by hand only), entries of q per pair
    unsigned long long x;         // the exchange cursor at the start of the launch
    const double *__restrict__ q; // [J][W], column a: q[j] = exp(-2 |beta_a - beta_{a+1}| 2^j) of the pair (a, a + 1)
    const int *__restrict__ sgn;  // [W], sign of beta_a - beta_{a+1}
    int *replica;                 // [W], the label of the configuration in the slot
    long long *prop, *acc;        // [W], tries and swaps of the pair (a, a + 1)
};

// does the pair (a, a + 1) swap in round xc?  (the rule at the top of this file; a draw only when it decides)
__device__ __forceinline__ bool ising_exchange_decide(const Exchange &x, unsigned long long xc, int W, int a,
                                                      unsigned long long key_a, int sgn, int Ea, int Eb)
{
    const int d = (Ea - Eb) / 2;
    if (sgn == 0 || d == 0 || (d > 0) == (sgn > 0)) return true;
    const unsigned int ad = (unsigned int)(d < 0 ? -d : d);
    double q[MAX_XJ];  // the pair's whole table as one batch of requests, not a round trip per set bit
#pragma unroll
    for (int j = 0; j < MAX_XJ; ++j) q[j] = j < x.J ? x.q[at(j, W, a)] : 1.0;
    double p = 1.0;
#pragma unroll
    for (int j = 0; j < MAX_XJ; ++j)
        if ((ad >> j) & 1u) p = p * q[j];  // (|d| < 2^J: no bit at or above J is set)
    return dqmc::philox4_uniform(key_a, (unsigned int)xc, (unsigned int)(xc >> 32), 2u, 0u) < p;
}

// one exchange round inside the sweep kernels (64 % R == 0: a ladder never straddles a wave).  il = the slot's index in
// its ladder.  The lower lane of a pair decides; the upper one reads the decision, and both take the partner's E, M and
// label, by cross-lane reads.  Then the nw spin words change columns: every lane reads sp[j * 64 + src] and writes
// sp[j * 64 + lane], src = the partner where the pair swaps.  The write of a word waits for the data of its read, the
// workgroup is one wave, and a wave's LDS instructions execute in order for all its lanes at once: every lane has read
// word j before any lane overwrites it, so no barrier is needed (words j and j' never share an address).  Lanes past
// W have left the kernel; n_walkers % R == 0 keeps every partner below W.
__device__ __forceinline__ void ising_exchange_round(unsigned int *sp, const Exchange &x, unsigned long long xc, int lane,
                                                     int w, int W, int nw, int il, unsigned long long key, int sgn, int &E,
                                                     int &M, int &rep, long long &xprop, long long &xacc)
{
    const bool lo = ((il ^ (int)xc) & 1) == 0;
    const bool active = lo ? il + 1 < x.R : il > 0;
    const int partner = active ? (lo ? lane + 1 : lane - 1) : lane;
    const int Ep = __shfl(E, partner), Mp = __shfl(M, partner), rp = __shfl(rep, partner);
    int swap = 0;
    if (active && lo) {
        swap = ising_exchange_decide(x, xc, W, w, key, sgn, E, Ep) ? 1 : 0;
        ++xprop;
        xacc += swap;
    }
    swap = __shfl(swap, lo ? lane : partner);
    if (!__any(swap)) return;  // uniform: no pair of this wave swaps
    if (swap) {
        E = Ep;
        M = Mp;
        rep = rp;
    }
    const int src = swap ? partner : lane;
    __builtin_amdgcn_wave_barrier();
    for (int j = 0; j < nw; ++j) {
        const unsigned int v = sp[j * WAVE + src];
        __builtin_amdgcn_wave_barrier();  // (no instruction: keeps the compiler from moving LDS accesses across)
        sp[j * WAVE + lane] = v;
        __builtin_amdgcn_wave_barrier();
    }
}

// push!(observable, value) of IsingEnergyMeasurement / IsingMagnetizationMeasurement (measurements.jl:30-35,72-78) into
// the walker's logarithmic binner (include/dqmc_hip.h, "error bars of the MC flavor"): elements [E, E2, M, M2] with
// M = |M|, state [level][element][walker] for x_sum, x2_sum and the compressor, [level][pair][walker] for the cross
// sums of (E, E2) and (M, M2).  lmax = trailing 1-bits of the push count, the same in every lane: levels below it
// complete a pair with their compressor and carry the average upwards, level lmax keeps the value (top = the last
// level, which has no compressor).  A level's values are requested together; levels above lmax are not touched.
__device__ __forceinline__ void ising_bin_push(double *__restrict__ xs, double *__restrict__ x2,
                                               double *__restrict__ xy, double *__restrict__ c, int W, int w, int lmax,
                                               int top, double e, double m)
{
    double x[4] = {e, e * e, m, m * m};
    const size_t sW = (size_t)W;
    size_t a4 = (size_t)w, a2 = (size_t)w;
    for (int l = 0; l < lmax; ++l, a4 += 4 * sW, a2 += 2 * sW) {
        double s1[4], s2[4], cc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s1[k] = xs[a4 + k * sW];
            s2[k] = x2[a4 + k * sW];
            cc[k] = c[a4 + k * sW];
        }
        const double p0 = xy[a2], p1 = xy[a2 + sW];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            xs[a4 + k * sW] = s1[k] + x[k];
            x2[a4 + k * sW] = s2[k] + x[k] * x[k];
        }
        xy[a2] = p0 + x[0] * x[1];
        xy[a2 + sW] = p1 + x[2] * x[3];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = 0.5 * (cc[k] + x[k]);
    }
    double s1[4], s2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s1[k] = xs[a4 + k * sW];
        s2[k] = x2[a4 + k * sW];
    }
    const double p0 = xy[a2], p1 = xy[a2 + sW];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xs[a4 + k * sW] = s1[k] + x[k];
        x2[a4 + k * sW] = s2[k] + x[k] * x[k];
        if (lmax < top) c[a4 + k * sW] = x[k];
    }
    xy[a2] = p0 + x[0] * x[1];
    xy[a2 + sW] = p1 + x[2] * x[3];
}

// the sweep kernels, without and with the exchange round (ising_sweep.inl)
#define ISING_EXCHANGE 0
#include "ising_sweep.inl"
#undef ISING_EXCHANGE
#define ISING_EXCHANGE 1
#include "ising_sweep.inl"
#undef ISING_EXCHANGE

// the push of a measurement that ising_wolff_kernel took (the deferred measurement of the sweep its move follows): E
// and M as that kernel left them, one lane per walker
__global__ __launch_bounds__(WAVE) void ising_bin_push_kernel(const int *__restrict__ E, const int *__restrict__ M, int W,
                                                              int lmax, int top, double *__restrict__ bxs,
                                                              double *__restrict__ bx2, double *__restrict__ bxy,
                                                              double *__restrict__ bc)
{
    const int w = blockIdx.x * WAVE + threadIdx.x;
    if (w >= W) return;
    const int m = M[w];
    ising_bin_push(bxs, bx2, bxy, bc, W, w, lmax, top, (double)E[w], (double)(m < 0 ? -m : m));
}

// rand(MC, m) (IsingModel.jl:83): site i (column-major) takes the walker's next uniform, u < 0.5 -> -1.
// walker < 0: every walker.
__global__ __launch_bounds__(WAVE) void ising_rand_conf_kernel(DevState s, int walker)
{
    const int w = walker >= 0 ? walker : blockIdx.x * WAVE + threadIdx.x;
    if (w >= s.W || (walker >= 0 && threadIdx.x != 0)) return;
    const unsigned long long key = s.key[w];
    unsigned long long draw = s.draw[w];
    for (int j = 0; j < s.nw; ++j) {
        unsigned int word = 0;
        const int n = min(32, s.N - 32 * j);
        for (int b = 0; b < n; ++b) word |= (dqmc::philox_uniform(key, draw++) < 0.5 ? 0u : 1u) << b;
        s.conf[at(j, s.W, w)] = word;
    }
    s.draw[w] = draw;
}

// energy(mc, m, conf) over the bonds table (IsingModel.jl:149-186) and M = sum(conf); walker < 0: every walker
__global__ __launch_bounds__(WAVE) void ising_observables_kernel(DevState s, int walker)
{
    extern __shared__ unsigned int sp[];
    const int lane = threadIdx.x;
    const int w = walker >= 0 ? walker : blockIdx.x * WAVE + lane;
    if (w >= s.W || (walker >= 0 && lane != 0)) return;
    int M = 0;
    for (int j = 0; j < s.nw; ++j) {
        const unsigned int v = s.conf[at(j, s.W, w)];
        sp[j * WAVE + lane] = v;
        M += 2 * __popc(v);
    }
    M -= s.N;
    int E = 0;
    for (int b = 0; b < s.n_bonds; ++b) {
        const int a = s.bonds[2 * b], c = s.bonds[2 * b + 1];
        const int sa = (sp[(a >> 5) * WAVE + lane] >> (a & 31)) & 1u, sc = (sp[(c >> 5) * WAVE + lane] >> (c & 31)) & 1u;
        E -= sa == sc ? 1 : -1;
    }
    s.E[w] = E;
    s.M[w] = M;
}

// LDS of the cluster move: spin words [nw], cluster bitset [nw], 8 counters, two frontier queues of N 16-bit site
// indices (at N = 16384: 4 KiB + 64 KiB)
constexpr int WOLFF_THREADS = 256;
static inline size_t wolff_lds_bytes(int N, int nw) { return (size_t)(2 * nw + 8) * 4 + (size_t)4 * N; }

// global_move (IsingModel.jl:104-140), as defined at the top of this file, one workgroup per walker (walker < 0:
// workgroup b is walker b).  The cluster grows level by level: the frontier's slots are spread over the workgroup, a
// slot draws only when its neighbour is aligned and not yet in the cluster, and the old value of an LDS atomicOr enqueues
// every site exactly once, so the cluster is the same set whatever order the slots run in.  One barrier per level; the
// level counters rotate over three words (level l reads ctr[l % 3], appends to ctr[(l + 1) % 3] and clears
// ctr[(l + 2) % 3], which level l - 1 read before the barrier).  Then the cluster is flipped (XOR of the words), E is
// recomputed over the bonds table as ising_observables_kernel does and M by popcount.  measure != 0: the measurement
// of run! (MC.jl:262-283) for the sweep this move follows, as the sweep kernel takes it.
__global__ __launch_bounds__(WOLFF_THREADS) void ising_wolff_kernel(DevState s, const int *__restrict__ nbr, int z,
                                                                    int walker, int measure)
{
    extern __shared__ unsigned int sm[];
    const int tid = threadIdx.x;
    const int w = walker >= 0 ? walker : blockIdx.x;
    const int N = s.N, nw = s.nw, W = s.W;
    unsigned int *sp = sm, *cl = sm + nw, *ctr = sm + 2 * nw;  // ctr[0..2] level sizes, [3] |C|, [4] E, [5] up spins
    unsigned short *q = (unsigned short *)(sm + 2 * nw + 8);   // q[0..N) and q[N..2N): frontiers of even / odd levels
    const unsigned long long key = s.key[w], m = s.moves[w];
    const unsigned int c1 = (unsigned int)m, c3 = (unsigned int)(m >> 32);
    const double p = s.pw[w];
    const int seed = min(N - 1, (int)(dqmc::philox4_uniform(key, 0u, c1, 1u, c3) * N));
    for (int j = tid; j < nw; j += WOLFF_THREADS) {
        sp[j] = s.conf[at(j, W, w)];
        cl[j] = j == seed >> 5 ? 1u << (seed & 31) : 0u;
    }
    if (tid < 8) ctr[tid] = tid == 0 ? 1u : 0u;
    if (tid == 0) q[0] = (unsigned short)seed;
    __syncthreads();
    const unsigned int s0 = (sp[seed >> 5] >> (seed & 31)) & 1u;  // every site of the cluster has the seed's spin

    for (int lev = 0;; ++lev) {
        const int n = (int)ctr[lev % 3];
        if (n == 0) break;
        const unsigned short *qc = q + (lev & 1) * N;
        unsigned short *qn = q + ((lev & 1) ^ 1) * N;
        if (tid == 0) ctr[(lev + 2) % 3] = 0u;
        for (int t = tid; t < n * z; t += WOLFF_THREADS) {
            const int e = t / z, k = t - e * z;
            const int i = qc[e];
            const int j = nbr[i * MAX_Z + k];
            const unsigned int bit = 1u << (j & 31);
            if (((sp[j >> 5] >> (j & 31)) & 1u) != s0 || (cl[j >> 5] & bit)) continue;
            if (!(dqmc::philox4_uniform(key, 1u + 8u * (unsigned int)i + (unsigned int)k, c1, 1u, c3) < p)) continue;
            if (atomicOr(&cl[j >> 5], bit) & bit) continue;  // another slot reached j first
            qn[atomicAdd(&ctr[(lev + 1) % 3], 1u)] = (unsigned short)j;
        }
        __syncthreads();
    }

    unsigned int size = 0, up = 0;
    for (int j = tid; j < nw; j += WOLFF_THREADS) {
        const unsigned int c = cl[j], v = sp[j] ^ c;
        sp[j] = v;
        s.conf[at(j, W, w)] = v;
        size += __popc(c);
        up += __popc(v);
    }
    if (size) atomicAdd(&ctr[3], size);
    if (up) atomicAdd(&ctr[5], up);
    __syncthreads();
    int e = 0;
    for (int b = tid; b < s.n_bonds; b += WOLFF_THREADS) {
        const int a = s.bonds[2 * b], c = s.bonds[2 * b + 1];
        e -= ((sp[a >> 5] >> (a & 31)) & 1u) == ((sp[c >> 5] >> (c & 31)) & 1u) ? 1 : -1;
    }
    if (e) atomicAdd(&ctr[4], (unsigned int)e);
    __syncthreads();
    if (tid != 0) return;
    const int E = (int)ctr[4], M = 2 * (int)ctr[5] - N, C = (int)ctr[3];
    s.E[w] = E;
    s.M[w] = M;
    s.moves[w] = m + 1;
    s.gprop[w] += 1;
    s.gacc[w] += C > 1 ? 1 : 0;
    s.gsum[w] += C;
    if (measure) {
        const double ed = (double)E, md = (double)(M < 0 ? -M : M);
        s.sE[w] += ed;
        s.sE2[w] += ed * ed;
        s.sM[w] += md;
        s.sM2[w] += md * md;
        const long long ns = s.n_series[w];
        if (ns < s.cap) {
            s.serE[at((int)ns, W, w)] = E;
            s.serM[at((int)ns, W, w)] = M < 0 ? -M : M;
            s.n_series[w] = ns + 1;
        }
        s.n_meas[w] += 1;
    }
}

// the measurement of run! (MC.jl:262-283) of slot w, as ising_wolff_kernel takes it
__device__ __forceinline__ void ising_measure_slot(const DevState &s, int w, int E, int M)
{
    const double ed = (double)E, md = (double)(M < 0 ? -M : M);
    const double sE = s.sE[w], sE2 = s.sE2[w], sM = s.sM[w], sM2 = s.sM2[w];  // requested together
    const long long ns = s.n_series[w], nm = s.n_meas[w];
    s.sE[w] = sE + ed;
    s.sE2[w] = sE2 + ed * ed;
    s.sM[w] = sM + md;
    s.sM2[w] = sM2 + md * md;
    if (ns < s.cap) {
        s.serE[at((int)ns, s.W, w)] = E;
        s.serM[at((int)ns, s.W, w)] = M < 0 ? -M : M;
        s.n_series[w] = ns + 1;
    }
    s.n_meas[w] = nm + 1;
}

// one exchange round (x.x) on the state in global memory: any R, ladders that cross waves, a round that follows a
// cluster move, dqmc_mc_exchange.  One lane per slot; the lower lane of a pair decides and swaps E, M, the label and the
// nw words of the two columns, which no other lane touches in this round; upper lanes have nothing to do.  measure != 0:
// the measurement of the sweep this round ends, taken for both slots of a pair by its lower lane and for a slot
// without a pair by its own.
__global__ __launch_bounds__(WAVE) void ising_exchange_kernel(DevState s, Exchange x, int measure)
{
    const int w = blockIdx.x * WAVE + threadIdx.x;
    if (w >= s.W) return;
    const int il = w % x.R;
    const bool lo = ((il ^ (int)x.x) & 1) == 0;
    const bool active = lo ? il + 1 < x.R : il > 0;
    if (active && !lo) return;
    int E = s.E[w], M = s.M[w];
    if (active) {  // (il + 1 < R and W % R == 0: w + 1 < W)
        const int b = w + 1;
        int Eb = s.E[b], Mb = s.M[b];
        const int ra = x.replica[w], rb = x.replica[b], sgn = x.sgn[w];  // everything the round reads, requested together
        const unsigned long long key = s.key[w];
        const long long prop = x.prop[w], acc = x.acc[w];
        const bool swap = ising_exchange_decide(x, x.x, s.W, w, key, sgn, E, Eb);
        x.prop[w] = prop + 1;
        if (swap) {
            x.acc[w] = acc + 1;
            const int t = E, u = M;
            E = Eb;
            M = Mb;
            Eb = t;
            Mb = u;
            s.E[w] = E;
            s.M[w] = M;
            s.E[b] = Eb;
            s.M[b] = Mb;
            x.replica[w] = rb;
            x.replica[b] = ra;
            for (int j = 0; j < s.nw; ++j) {
                const unsigned int va = s.conf[at(j, s.W, w)], vb = s.conf[at(j, s.W, b)];
                s.conf[at(j, s.W, w)] = vb;
                s.conf[at(j, s.W, b)] = va;
            }
        }
        if (measure) ising_measure_slot(s, b, Eb, Mb);
    }
    if (measure) ising_measure_slot(s, w, E, M);
}

// the finite-size-scaling measurement: FssArg, ising_fss_kernel
#include "ising_fss.inl"

// the checkerboard sweep, one workgroup per walker: CbArg, ising_cb_kernel
#include "ising_cb.inl"

// The work bound of the checkerboard sweep, from its measured cost on the MI355X: with the walkers' workgroups
// all resident a sweep takes about 0.6 us + 2.45 ns per site (L = 8 .. 128: 1.3, 3.0, 10.6, 40 us), i.e. N + 512 "site
// visits" of 2.5 ns with the barriers counted as CB_SWEEP_OVERHEAD sites; about 680 workgroups of 256 lanes run side by side
// (4096 walkers take 6 times as long as 16 .. 256), counted as CB_RESIDENT_WALKERS = 512.  A launch runs at most
// CB_LAUNCH_BUDGET / ((N + 512) max(1, W / 512)) sweeps, one at least: 2^20 visits are 2.6 ms, near the 3 ms the
// sequential path aims at.
constexpr double CB_LAUNCH_BUDGET = 1048576.0;
constexpr double CB_SWEEP_OVERHEAD = 512.0;
constexpr double CB_RESIDENT_WALKERS = 512.0;

}  // namespace dqmc_mc

using namespace dqmc_mc;
static_assert(MAX_Z == mc_tables::ROW && CB_MAX_COLOURS == mc_tables::MAX_COLOURS && WAVE == mc_tables::WAVE,
              "the kernels read the tables mc_tables.h lays out");

struct dqmc_mc_handle : mc_handle_base {
    int N = 0, z = 0, nw = 0, cap = 0, n_bonds = 0;
    int global_rate = 0;       // mc.p.global_rate when global moves are on, 0 = off
    struct Tempering {         // replica exchange (dqmc_mc_set_exchange); R = 0: no ladders
        int R = 0, rate = 0, J = 0;
        uint64_t cursor = 0;   // rounds since dqmc_mc_set_exchange
        double *q = nullptr;   // [MAX_XJ][W]
        int *sgn = nullptr, *replica = nullptr;
        long long *prop = nullptr, *acc = nullptr;
        bool fused() const { return R >= 2 && rate > 0 && WAVE % R == 0; }
    } xch;
    std::vector<double> beta_h;  // [W], as dqmc_mc_set_beta got them
    std::vector<int> nbr_h;    // [N][z] 0-based
    std::vector<int> bonds_h;  // [n_bonds][2] 0-based
    DevState d{};
    struct Binner : mc_bin_section {  // ising_bin_push: elements [E, E2, |M|, M2], pairs (E, E2) and (|M|, M2)
        bool on = false;
        int64_t cap = 0;
    } bin;
    struct Fss {  // dqmc_mc_set_fss; n_k = -1: off
        int n_k = -1;
        int *cq = nullptr, *sq = nullptr;         // [n_k][32 nw]: rows padded with zeros to whole spin words
        double *sM4 = nullptr, *sS = nullptr;     // [W], [8][W] (allocated when FSS is first switched on)
        long long *n_meas = nullptr;              // [W]
        // the FSS section of the binner (there iff bin.on && n_k >= 0; its levels and capacity are bin's): elements
        // [M2, M4, S_0 ..], pairs (M2, M4), (M2, S_k), a compressor value per member of a pair
        mc_bin_section bin;
        uint64_t hash = 0;  // of the two phase tables as dqmc_mc_set_fss got them (the checkpoint blob's header)
    } fss;
    struct Update {  // dqmc_mc_set_update
        int kind = DQMC_MC_UPDATE_SEQUENTIAL, C = 0, threads = CB_THREADS;
        int *site = nullptr, *rows = nullptr, *off = nullptr;  // [N], [N][8], [C + 1]: the colour-sorted tables
        unsigned long long *cursor = nullptr;                  // [W], allocated with the handle (dqmc_mc_seed zeroes it)
        uint64_t hash = 0;  // of the colouring as dqmc_mc_set_update got it (the checkpoint blob's header)
    } upd;
    // every binner section, at its index in the checkpoint blob (mc_blob.h: SEC_MAIN, SEC_SCALING)
    std::array<mc_bin_section *, 2> sections() { return {&bin, &fss.bin}; }
};

static int mc_launch_observables(dqmc_mc_handle *h, int walker)
{
    const int grid = walker >= 0 ? 1 : (h->W + WAVE - 1) / WAVE;
    hipLaunchKernelGGL(ising_observables_kernel, dim3(grid), dim3(WAVE), (size_t)h->nw * WAVE * 4, h->stream, h->d,
                       walker);
    MCHK(hipGetLastError());
    return 0;
}

static int mc_launch_wolff(dqmc_mc_handle *h, int walker, int measure)
{
    const int grid = walker >= 0 ? 1 : h->W;
    hipLaunchKernelGGL(ising_wolff_kernel, dim3(grid), dim3(WOLFF_THREADS), wolff_lds_bytes(h->N, h->nw), h->stream,
                       h->d, (const int *)h->d.nbr, h->z, walker, measure);
    MCHK(hipGetLastError());
    return 0;
}

static Exchange mc_exchange_arg(const dqmc_mc_handle *h)
{
    const dqmc_mc_handle::Tempering &t = h->xch;
    return Exchange{t.R, t.rate, t.J, (unsigned long long)t.cursor, t.q, t.sgn, t.replica, t.prop, t.acc};
}

// one round at the handle's cursor, which it advances
static int mc_launch_exchange(dqmc_mc_handle *h, int measure)
{
    hipLaunchKernelGGL(ising_exchange_kernel, dim3((h->W + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, h->d,
                       mc_exchange_arg(h), measure);
    MCHK(hipGetLastError());
    h->xch.cursor += 1;
    return 0;
}

// the table of the pair (a, a + 1) into column a: q[j] = exp(-2 |beta_a - beta_{a+1}| 2^j) and the sign of the difference
static void mc_pair_table(const dqmc_mc_handle *h, int a, double q[MAX_XJ], int *sgn)
{
    const double db = h->beta_h[a] - h->beta_h[a + 1];
    *sgn = db > 0.0 ? 1 : (db < 0.0 ? -1 : 0);
    for (int j = 0; j < MAX_XJ; ++j) q[j] = exp(-2.0 * fabs(db) * (double)(1 << j));
}

static int mc_put_pair_table(dqmc_mc_handle *h, int a)
{
    double q[MAX_XJ];
    int sgn = 0;
    mc_pair_table(h, a, q, &sgn);
    MCHK(hipMemcpy2DAsync(h->xch.q + a, (size_t)h->W * sizeof(double), q, sizeof(double), sizeof(double), MAX_XJ,
                          hipMemcpyHostToDevice, h->stream));
    return mc_put<int>(h, h->xch.sgn, 0, a, sgn);
}

// the push of the measurement ising_wolff_kernel has just taken
static int mc_launch_bin_push(dqmc_mc_handle *h)
{
    dqmc_mc_handle::Binner &b = h->bin;
    int lmax = 0;
    if (int rc = b.next_lmax(h, "dqmc_mc_sweep", &lmax)) return rc;
    hipLaunchKernelGGL(ising_bin_push_kernel, dim3((h->W + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream,
                       (const int *)h->d.E, (const int *)h->d.M, h->W, lmax, b.L - 1, b.xs, b.x2, b.xy, b.c);
    MCHK(hipGetLastError());
    b.T += 1;
    return 0;
}

// ---- finite-size-scaling observables
constexpr int MAX_K = 8;

// every section the handle's features call for, at L levels each: the one place that knows their shapes
static int mc_bin_alloc(dqmc_mc_handle *h, int L)
{
    const int n_k = h->fss.n_k;
    if (int rc = h->bin.alloc(h, 4, 2, 4, L)) return rc;
    return n_k < 0 ? 0 : h->fss.bin.alloc(h, 2 + n_k, 1 + n_k, 2 * (1 + n_k), L);
}

static int mc_fss_clear(dqmc_mc_handle *h)  // the sums (the section: mc_bin_clear)
{
    dqmc_mc_handle::Fss &f = h->fss;
    const size_t W = h->W;
    if (f.sM4) {
        MCHK(hipMemsetAsync(f.sM4, 0, W * 8, h->stream));
        MCHK(hipMemsetAsync(f.sS, 0, (size_t)MAX_K * W * 8, h->stream));
        MCHK(hipMemsetAsync(f.n_meas, 0, W * 8, h->stream));
    }
    return 0;
}

// the FSS measurement of the sweep whose last kernel has just been launched (and its push).  The 1 + n_k pairs run side
// by side, N table visits each; where they would pass the launch budget together the pairs are spread over launches.
static int mc_launch_fss(dqmc_mc_handle *h)
{
    dqmc_mc_handle::Fss &f = h->fss;
    FssArg a{};
    a.n_k = f.n_k;
    a.inv = 1.0 / ((double)h->N * 1152921504606846976.0);  // N 2^60 is exact, one rounding
    a.sM4 = f.sM4;
    a.sS = f.sS;
    a.n_meas = f.n_meas;
    if (int rc = f.bin.push_arg(h, "dqmc_mc_sweep", &a.bin)) return rc;
    const int pairs = 1 + f.n_k;
    const double per_pair = (double)h->N * std::max((double)h->W, BUDGET_WALKERS);
    const int chunk = (int)std::max(1.0, std::min((double)pairs, std::floor(LAUNCH_BUDGET / per_pair)));
    for (int y0 = 0; y0 < pairs; y0 += chunk) {
        hipLaunchKernelGGL(ising_fss_kernel, dim3((h->W + WAVE - 1) / WAVE, std::min(chunk, pairs - y0)), dim3(WAVE), 0,
                           h->stream, h->d, a, (const int4 *)f.cq, (const int4 *)f.sq, y0);
        MCHK(hipGetLastError());
    }
    f.bin.pushed();
    return 0;
}

static const char *const MC_FSS_OFF = ": FSS is off (dqmc_mc_set_fss first)";

extern "C" {

const char *dqmc_mc_last_error(const dqmc_mc_handle *h) { return mc_last_error(h); }

int dqmc_mc_create(const dqmc_mc_params *p, dqmc_mc_handle **out)
{
    if (!p || !out) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_create: null argument");
    *out = nullptr;
    if (p->n_sites < 1 || p->n_walkers < 1)
        return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_create: n_sites and n_walkers must be >= 1");
    if (p->n_sites > MAX_SITES)
        return mc_fail(nullptr, DQMC_ERR_INVALID,
                       "dqmc_mc_create: n_sites exceeds 16384 (the walker's spins must fit in LDS)");
    if (p->z < 1 || p->z > MAX_Z)
        return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_create: z must be in 1..8 (neighbours per site)");
    const int N = p->n_sites, z = p->z, nb = p->n_bonds;
    std::vector<int> nbr_h, bonds_h;
    std::string msg;
    if (!mc_tables::lattice_tables("dqmc_mc_create", N, z, nb, p->series_capacity, p->neighs, p->bonds, nbr_h, bonds_h, &msg))
        return mc_fail(nullptr, DQMC_ERR_INVALID, msg);
    if (int rc = mc_check_device("dqmc_mc_create", p->device_id)) return rc;

    dqmc_mc_handle *h = new dqmc_mc_handle();
    h->N = N;
    h->z = z;
    h->W = p->n_walkers;
    h->nw = (N + 31) / 32;
    h->cap = p->series_capacity;
    h->n_bonds = nb;
    h->device = p->device_id;
    h->beta_h.assign((size_t)p->n_walkers, 0.0);
    h->nbr_h = nbr_h;
    h->bonds_h = bonds_h;
    auto bail = [&](int rc) { return mc_bail(h, rc); };
    if (int rc = mc_open(h, "dqmc_mc_create")) return bail(rc);
    const std::vector<int> nbr_pad = mc_tables::padded_rows(h->nbr_h, N, z, N + 1);  // (row N: read ahead, unused)
    DevState &d = h->d;
    d.N = N;
    d.W = h->W;
    d.nw = h->nw;
    d.cap = h->cap;
    d.n_bonds = nb;
    const size_t W = h->W;
    int *nbr = nullptr, *bonds = nullptr;
    int rc = 0;
    if ((rc = mc_alloc(h, &nbr, nbr_pad.size())) || (rc = mc_alloc(h, &bonds, h->bonds_h.size())) ||
        (rc = mc_alloc(h, &d.conf, (size_t)h->nw * W)) || (rc = mc_alloc(h, &d.key, W)) ||
        (rc = mc_alloc(h, &d.draw, W)) || (rc = mc_alloc(h, &d.E, W)) || (rc = mc_alloc(h, &d.M, W)) ||
        (rc = mc_alloc(h, &d.thr, (size_t)MAX_Z * W)) || (rc = mc_alloc(h, &d.sE, W)) ||
        (rc = mc_alloc(h, &d.sE2, W)) || (rc = mc_alloc(h, &d.sM, W)) || (rc = mc_alloc(h, &d.sM2, W)) ||
        (rc = mc_alloc(h, &d.n_meas, W)) || (rc = mc_alloc(h, &d.prop, W)) || (rc = mc_alloc(h, &d.acc, W)) ||
        (rc = mc_alloc(h, &d.n_series, W)) || (rc = mc_alloc(h, &d.serE, (size_t)h->cap * W)) ||
        (rc = mc_alloc(h, &d.serM, (size_t)h->cap * W)) || (rc = mc_alloc(h, &d.pw, W)) ||
        (rc = mc_alloc(h, &d.moves, W)) || (rc = mc_alloc(h, &d.gprop, W)) || (rc = mc_alloc(h, &d.gacc, W)) ||
        (rc = mc_alloc(h, &d.gsum, W)) || (rc = mc_alloc(h, &h->upd.cursor, W)))
        return bail(rc);
    d.nbr = nbr;
    d.bonds = bonds;
    if (hipMemcpyAsync(nbr, nbr_pad.data(), nbr_pad.size() * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        (nb && hipMemcpyAsync(bonds, h->bonds_h.data(), h->bonds_h.size() * 4, hipMemcpyHostToDevice, h->stream) !=
                   hipSuccess))
        return bail(mc_fail(h, DQMC_ERR_HIP, "dqmc_mc_create: table upload failed"));
    // the whole spin array of a workgroup in LDS above the 64 KiB default
    const size_t lds = (size_t)h->nw * WAVE * 4;
    const void *kernels[] = {(const void *)ising_sweep_kernel<1>, (const void *)ising_sweep_kernel<2>,
                             (const void *)ising_sweep_kernel<3>, (const void *)ising_sweep_kernel<4>,
                             (const void *)ising_sweep_kernel<5>, (const void *)ising_sweep_kernel<6>,
                             (const void *)ising_sweep_kernel<7>, (const void *)ising_sweep_kernel<8>,
                             (const void *)ising_observables_kernel};
    for (const void *k : kernels)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return bail(mc_fail(h, DQMC_ERR_HIP, "dqmc_mc_create: cannot reserve LDS for the spins"));
    if (hipFuncSetAttribute((const void *)ising_wolff_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)wolff_lds_bytes(N, h->nw)) != hipSuccess)
        return bail(mc_fail(h, DQMC_ERR_HIP, "dqmc_mc_create: cannot reserve LDS for the cluster move"));
    if (hipStreamSynchronize(h->stream) != hipSuccess)
        return bail(mc_fail(h, DQMC_ERR_HIP, "dqmc_mc_create: device initialisation failed"));
    *out = h;
    return DQMC_OK;
}

int dqmc_mc_destroy(dqmc_mc_handle *h) { return mc_destroy(h); }

int dqmc_mc_set_beta(dqmc_mc_handle *h, int32_t walker, double beta)
{
    if (int rc = mc_walker(h, walker, "dqmc_mc_set_beta")) return rc;
    if (!std::isfinite(beta) || beta < 0.0)
        return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_set_beta: beta must be finite and >= 0");
    MCHK(hipSetDevice(h->device));
    double thr[MAX_Z];
    for (int k = 1; k <= MAX_Z; ++k) thr[k - 1] = exp(-beta * (2.0 * k));  // exp(-beta dE), MC.jl:327
    MCHK(hipMemcpy2DAsync(h->d.thr + walker, (size_t)h->W * sizeof(double), thr, sizeof(double), sizeof(double), MAX_Z,
                          hipMemcpyHostToDevice, h->stream));
    if (int rc = mc_put<double>(h, h->d.pw, 0, walker, 1.0 - exp(-2.0 * beta))) return rc;  // 1 - exp(-2 beta), IsingModel.jl:126
    h->beta_h[walker] = beta;
    const int R = h->xch.R;  // the exchange tables of the two pairs this slot belongs to
    if (R >= 2 && walker % R > 0)
        if (int rc = mc_put_pair_table(h, walker - 1)) return rc;
    if (R >= 2 && walker % R + 1 < R)
        if (int rc = mc_put_pair_table(h, walker)) return rc;
    return DQMC_OK;
}

int dqmc_mc_seed(dqmc_mc_handle *h, int32_t walker, uint64_t seed)
{
    if (int rc = mc_walker(h, walker, "dqmc_mc_seed")) return rc;
    MCHK(hipSetDevice(h->device));
    if (int rc = mc_put<unsigned long long>(h, h->d.key, 0, walker, seed)) return rc;
    if (int rc = mc_put<unsigned long long>(h, h->d.moves, 0, walker, 0ull)) return rc;
    if (int rc = mc_put<unsigned long long>(h, h->upd.cursor, 0, walker, 0ull)) return rc;
    return mc_put<unsigned long long>(h, h->d.draw, 0, walker, 0ull);
}

int dqmc_mc_rand_conf(dqmc_mc_handle *h, int32_t walker)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_rand_conf: null handle");
    if (walker >= h->W) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_rand_conf: walker out of range");
    MCHK(hipSetDevice(h->device));
    const int grid = walker >= 0 ? 1 : (h->W + WAVE - 1) / WAVE;
    hipLaunchKernelGGL(ising_rand_conf_kernel, dim3(grid), dim3(WAVE), 0, h->stream, h->d, walker);
    MCHK(hipGetLastError());
    if (int rc = mc_launch_observables(h, walker)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_mc_set_conf(dqmc_mc_handle *h, int32_t walker, const int8_t *conf)
{
    if (int rc = mc_walker(h, walker, "dqmc_mc_set_conf")) return rc;
    if (!conf) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_set_conf: null conf");
    std::vector<unsigned int> words(h->nw, 0u);
    for (int i = 0; i < h->N; ++i) {
        if (conf[i] != 1 && conf[i] != -1) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_set_conf: spins must be +-1");
        if (conf[i] == 1) words[i >> 5] |= 1u << (i & 31);
    }
    MCHK(hipSetDevice(h->device));
    MCHK(hipMemcpy2DAsync(h->d.conf + walker, (size_t)h->W * 4, words.data(), 4, 4, h->nw, hipMemcpyHostToDevice,
                          h->stream));
    if (int rc = mc_launch_observables(h, walker)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

static int mc_words(dqmc_mc_handle *h, int32_t walker, std::vector<unsigned int> &words)
{
    words.assign(h->nw, 0u);
    MCHK(hipSetDevice(h->device));
    MCHK(hipMemcpy2DAsync(words.data(), 4, h->d.conf + walker, (size_t)h->W * 4, 4, h->nw, hipMemcpyDeviceToHost,
                          h->stream));
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_mc_get_conf(dqmc_mc_handle *h, int32_t walker, int8_t *conf)
{
    if (int rc = mc_walker(h, walker, "dqmc_mc_get_conf")) return rc;
    if (!conf) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_get_conf: null conf");
    std::vector<unsigned int> words;
    if (int rc = mc_words(h, walker, words)) return rc;
    for (int i = 0; i < h->N; ++i) conf[i] = (words[i >> 5] >> (i & 31)) & 1u ? 1 : -1;
    return DQMC_OK;
}

int dqmc_mc_get_conf_bits(dqmc_mc_handle *h, int32_t walker, uint64_t *chunks)
{
    if (int rc = mc_walker(h, walker, "dqmc_mc_get_conf_bits")) return rc;
    if (!chunks) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_get_conf_bits: null chunks");
    std::vector<unsigned int> words;
    if (int rc = mc_words(h, walker, words)) return rc;
    const int nc = (h->N + 63) / 64;
    for (int c = 0; c < nc; ++c)
        chunks[c] = (uint64_t)words[2 * c] | (2 * c + 1 < h->nw ? (uint64_t)words[2 * c + 1] << 32 : 0ull);
    return DQMC_OK;
}

int dqmc_mc_sweep(dqmc_mc_handle *h, int32_t n_sweeps, int64_t first_sweep_index, int64_t thermalization,
                  int32_t measure_rate)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_sweep: null handle");
    if (n_sweeps < 0 || measure_rate < 1 || first_sweep_index < 1)
        return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_sweep: n_sweeps >= 0, first_sweep_index >= 1, measure_rate >= 1");
    dqmc_mc_handle::Binner &b = h->bin;
    const int64_t n_meas = mc_tables::measurements_in(first_sweep_index, first_sweep_index + n_sweeps - 1, thermalization,
                                                      measure_rate);
    if (b.on && b.T + n_meas > b.cap)  // the reference: OverflowError of push!
        return mc_fail(h, DQMC_ERR_STATE, "dqmc_mc_sweep: the measurements of this call would pass the binner's capacity");
    dqmc_mc_handle::Fss &fs = h->fss;
    if (fs.bin.xs && fs.bin.T + n_meas > b.cap)
        return mc_fail(h, DQMC_ERR_STATE,
                       "dqmc_mc_sweep: the measurements of this call would pass the capacity of the binner's FSS section");
    MCHK(hipSetDevice(h->device));
    const size_t lds = (size_t)h->nw * WAVE * 4;
    const int grid = (h->W + WAVE - 1) / WAVE;
    const double per_sweep = (double)h->N * std::max((double)h->W, BUDGET_WALKERS);
    const dqmc_mc_handle::Update &u = h->upd;
    const bool cb = u.kind == DQMC_MC_UPDATE_CHECKERBOARD;
    const double cb_per_sweep = ((double)h->N + CB_SWEEP_OVERHEAD) * std::max(1.0, (double)h->W / CB_RESIDENT_WALKERS);
    const int chunk = (int)std::max(
        1.0, std::min((double)n_sweeps, std::floor(cb ? CB_LAUNCH_BUDGET / cb_per_sweep : LAUNCH_BUDGET / per_sweep)));
    const int r = h->global_rate;
    dqmc_mc_handle::Tempering &t = h->xch;
    const int k = t.R >= 2 ? t.rate : 0;  // an exchange round after every k-th sweep
    const bool fused = t.fused() && !cb;  // the checkerboard kernel runs no rounds: each is a launch of its own
    for (int done = 0; done < n_sweeps;) {
        int n = std::min(chunk, n_sweeps - done);
        const long long first = first_sweep_index + done;
        if (r > 0) n = (int)std::min<long long>(n, r - (first - 1) % r);  // a launch ends at the next multiple of r
        // and at the next multiple of k where the round is a launch of its own (fused: only behind a cluster move)
        if (k > 0 && !fused) n = (int)std::min<long long>(n, k - (first - 1) % k);
        if (fs.n_k >= 0) {  // and at the next measured sweep: its FSS measurement is a launch of its own
            const long long g0 = std::max<long long>(first, (long long)thermalization + 1);
            const long long gm = (g0 + measure_rate - 1) / measure_rate * measure_rate;
            n = (int)std::min<long long>(n, gm - first + 1);
        }
        const long long last = first + n - 1;
        const bool move = r > 0 && last % r == 0;  // global_move after sweep `last` (MC.jl:233-236)
        const bool round = k > 0 && last % k == 0 && (!fused || move);  // ising_exchange_kernel after sweep `last`
        const bool deferred = (move || round) && last > thermalization && last % measure_rate == 0;
        const long long defer = move || round ? last : -1LL;
        const Exchange xa = mc_exchange_arg(h);
        if (cb) {
            const CbArg ca{u.C, h->z, u.cursor, b.on ? b.xs : nullptr, b.x2, b.xy, b.c, b.L - 1, (long long)b.T};
            hipLaunchKernelGGL(ising_cb_kernel, dim3(h->W), dim3(u.threads), 0, h->stream, h->d, ca, (const int *)u.site,
                               (const int4 *)u.rows, (const int *)u.off, n, first, (long long)thermalization,
                               (int)measure_rate, defer);
        } else
        switch (h->z) {  // binner on: the forms that push every measurement they take; fused: with the exchange round
#define MC_CASE(Z)                                                                                                  \
    case Z:                                                                                                         \
        if (b.on && fused)                                                                                          \
            hipLaunchKernelGGL(ising_sweep_binned_exchange_kernel<Z>, dim3(grid), dim3(WAVE), lds, h->stream, h->d, \
                               (const int4 *)h->d.nbr, n, first, (long long)thermalization, (int)measure_rate,     \
                               defer, b.xs, b.x2, b.xy, b.c, b.L - 1, (long long)b.T, xa);                          \
        else if (b.on)                                                                                              \
            hipLaunchKernelGGL(ising_sweep_binned_kernel<Z>, dim3(grid), dim3(WAVE), lds, h->stream, h->d,         \
                               (const int4 *)h->d.nbr, n, first, (long long)thermalization, (int)measure_rate,     \
                               defer, b.xs, b.x2, b.xy, b.c, b.L - 1, (long long)b.T);                              \
        else if (fused)                                                                                             \
            hipLaunchKernelGGL(ising_sweep_exchange_kernel<Z>, dim3(grid), dim3(WAVE), lds, h->stream, h->d,       \
                               (const int4 *)h->d.nbr, n, first, (long long)thermalization, (int)measure_rate,     \
                               defer, xa);                                                                          \
        else                                                                                                        \
            hipLaunchKernelGGL(ising_sweep_kernel<Z>, dim3(grid), dim3(WAVE), lds, h->stream, h->d,                \
                               (const int4 *)h->d.nbr, n, first, (long long)thermalization, (int)measure_rate,     \
                               defer);                                                                              \
        break;
            MC_CASE(1) MC_CASE(2) MC_CASE(3) MC_CASE(4) MC_CASE(5) MC_CASE(6) MC_CASE(7) MC_CASE(8)
#undef MC_CASE
        }
        if (b.on) b.T += mc_tables::measurements_in(first, last, thermalization, measure_rate) - (deferred ? 1 : 0);
        MCHK(hipGetLastError());
        if (fused) t.cursor += (uint64_t)(last / k - (first - 1) / k - (round ? 1 : 0));  // the rounds the launch ran
        if (move)
            if (int rc = mc_launch_wolff(h, -1, deferred && !round)) return rc;  // the last kernel of a sweep measures
        if (round)
            if (int rc = mc_launch_exchange(h, deferred)) return rc;
        if (deferred && b.on)
            if (int rc = mc_launch_bin_push(h)) return rc;
        if (fs.n_k >= 0 && last > thermalization && last % measure_rate == 0)
            if (int rc = mc_launch_fss(h)) return rc;
        done += n;
    }
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_mc_get_stats(dqmc_mc_handle *h, int32_t walker, dqmc_mc_stats *out)
{
    if (int rc = mc_walker(h, walker, "dqmc_mc_get_stats")) return rc;
    if (!out) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_get_stats: null out");
    MCHK(hipSetDevice(h->device));
    const DevState &d = h->d;
    int E = 0, M = 0;
    unsigned long long draw = 0;
    long long n_meas = 0, prop = 0, acc = 0, n_series = 0;
    int rc = 0;
    if ((rc = mc_get(h, d.E, 0, walker, &E)) || (rc = mc_get(h, d.M, 0, walker, &M)) ||
        (rc = mc_get(h, d.draw, 0, walker, &draw)) || (rc = mc_get(h, d.sE, 0, walker, &out->sum_E)) ||
        (rc = mc_get(h, d.sE2, 0, walker, &out->sum_E2)) || (rc = mc_get(h, d.sM, 0, walker, &out->sum_absM)) ||
        (rc = mc_get(h, d.sM2, 0, walker, &out->sum_M2)) || (rc = mc_get(h, d.n_meas, 0, walker, &n_meas)) ||
        (rc = mc_get(h, d.prop, 0, walker, &prop)) || (rc = mc_get(h, d.acc, 0, walker, &acc)) ||
        (rc = mc_get(h, d.n_series, 0, walker, &n_series)))
        return rc;
    out->energy = E;
    out->magnetization = M;
    out->n_meas = n_meas;
    out->prop_local = prop;
    out->acc_local = acc;
    out->uniforms_used = draw;
    out->n_series = n_series;
    return DQMC_OK;
}

int dqmc_mc_set_global_rate(dqmc_mc_handle *h, int32_t rate)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_set_global_rate: null handle");
    if (rate < 0) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_set_global_rate: rate must be >= 0 (0 = off)");
    h->global_rate = rate;
    return DQMC_OK;
}

int dqmc_mc_global_move(dqmc_mc_handle *h, int32_t walker)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_global_move: null handle");
    if (walker >= h->W) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_global_move: walker out of range");
    MCHK(hipSetDevice(h->device));
    if (int rc = mc_launch_wolff(h, walker < 0 ? -1 : walker, 0)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_mc_get_global_stats(dqmc_mc_handle *h, int32_t walker, dqmc_mc_global_stats *out)
{
    if (int rc = mc_walker(h, walker, "dqmc_mc_get_global_stats")) return rc;
    if (!out) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_get_global_stats: null out");
    MCHK(hipSetDevice(h->device));
    const DevState &d = h->d;
    long long prop = 0, acc = 0, sum = 0;
    unsigned long long moves = 0;
    int rc = 0;
    if ((rc = mc_get(h, d.gprop, 0, walker, &prop)) || (rc = mc_get(h, d.gacc, 0, walker, &acc)) ||
        (rc = mc_get(h, d.gsum, 0, walker, &sum)) || (rc = mc_get(h, d.moves, 0, walker, &moves)))
        return rc;
    out->prop_global = prop;
    out->acc_global = acc;
    out->sum_cluster_size = sum;
    out->moves_drawn = moves;
    return DQMC_OK;
}

int dqmc_mc_set_exchange(dqmc_mc_handle *h, int32_t n_replicas, int32_t rate)
{
    int R = 0;
    if (int rc = mc_exchange_ladders(h, "dqmc_mc_set_exchange", n_replicas, rate, &R)) return rc;
    MCHK(hipSetDevice(h->device));
    dqmc_mc_handle::Tempering &t = h->xch;
    const size_t W = h->W;
    if (R && !t.q) {
        int rc = 0;
        if ((rc = mc_alloc(h, &t.q, (size_t)MAX_XJ * W)) || (rc = mc_alloc(h, &t.sgn, W)) ||
            (rc = mc_alloc(h, &t.replica, W)) || (rc = mc_alloc(h, &t.prop, W)) || (rc = mc_alloc(h, &t.acc, W)))
            return rc;
    }
    if (R && WAVE % R == 0) {  // the whole spin array of a workgroup in LDS above the 64 KiB default, as dqmc_mc_create
        const void *kernels[] = {
            (const void *)ising_sweep_exchange_kernel<1>,        (const void *)ising_sweep_exchange_kernel<2>,
            (const void *)ising_sweep_exchange_kernel<3>,        (const void *)ising_sweep_exchange_kernel<4>,
            (const void *)ising_sweep_exchange_kernel<5>,        (const void *)ising_sweep_exchange_kernel<6>,
            (const void *)ising_sweep_exchange_kernel<7>,        (const void *)ising_sweep_exchange_kernel<8>,
            (const void *)ising_sweep_binned_exchange_kernel<1>, (const void *)ising_sweep_binned_exchange_kernel<2>,
            (const void *)ising_sweep_binned_exchange_kernel<3>, (const void *)ising_sweep_binned_exchange_kernel<4>,
            (const void *)ising_sweep_binned_exchange_kernel<5>, (const void *)ising_sweep_binned_exchange_kernel<6>,
            (const void *)ising_sweep_binned_exchange_kernel<7>, (const void *)ising_sweep_binned_exchange_kernel<8>};
        for (const void *k : kernels)
            if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)h->nw * WAVE * 4)) !=
                hipSuccess)
                return mc_fail(h, DQMC_ERR_HIP, "dqmc_mc_set_exchange: cannot reserve LDS for the spins");
    }
    t.R = R;
    t.rate = rate;
    t.cursor = 0;
    t.J = 0;
    while ((1L << t.J) <= (long)h->n_bonds) ++t.J;  // 2^J > n_bonds >= |d|
    if (t.q) {
        MCHK(hipMemsetAsync(t.prop, 0, W * 8, h->stream));
        MCHK(hipMemsetAsync(t.acc, 0, W * 8, h->stream));
        std::vector<int> label(W, 0), sgn(W, 0);
        std::vector<double> q((size_t)MAX_XJ * W, 0.0);
        for (size_t w = 0; R && w < W; ++w) {
            label[w] = (int)(w % R);
            if (w % R + 1 == (size_t)R) continue;  // the last slot of a ladder has no pair of its own
            double col[MAX_XJ];
            mc_pair_table(h, (int)w, col, &sgn[w]);
            for (int j = 0; j < MAX_XJ; ++j) q[(size_t)j * W + w] = col[j];
        }
        MCHK(hipMemcpyAsync(t.replica, label.data(), W * 4, hipMemcpyHostToDevice, h->stream));
        MCHK(hipMemcpyAsync(t.sgn, sgn.data(), W * 4, hipMemcpyHostToDevice, h->stream));
        MCHK(hipMemcpyAsync(t.q, q.data(), q.size() * 8, hipMemcpyHostToDevice, h->stream));
    }
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_mc_exchange(dqmc_mc_handle *h)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_exchange: null handle");
    if (h->xch.R < 2)
        return mc_fail(h, DQMC_ERR_STATE, "dqmc_mc_exchange: no ladders (dqmc_mc_set_exchange with n_replicas >= 2 first)");
    MCHK(hipSetDevice(h->device));
    if (int rc = mc_launch_exchange(h, 0)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_mc_get_exchange_stats(dqmc_mc_handle *h, int32_t walker, dqmc_mc_exchange_stats *out)
{
    return mc_get_exchange_stats(h, "dqmc_mc_get_exchange_stats", walker, out);
}

int dqmc_mc_exchange_fused(dqmc_mc_handle *h, int32_t *fused)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_exchange_fused: null handle");
    if (!fused) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_exchange_fused: null fused");
    *fused = h->xch.fused() && h->upd.kind == DQMC_MC_UPDATE_SEQUENTIAL ? 1 : 0;
    return DQMC_OK;
}

int dqmc_mc_get_series(dqmc_mc_handle *h, int32_t walker, int32_t *energy, int32_t *abs_magnetization,
                       int64_t *n_recorded)
{
    if (int rc = mc_walker(h, walker, "dqmc_mc_get_series")) return rc;
    if (!n_recorded) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_get_series: null n_recorded");
    MCHK(hipSetDevice(h->device));
    long long n = 0;
    if (int rc = mc_get(h, h->d.n_series, 0, walker, &n)) return rc;
    *n_recorded = n;
    if (n > 0 && energy)
        MCHK(hipMemcpy2DAsync(energy, 4, h->d.serE + walker, (size_t)h->W * 4, 4, n, hipMemcpyDeviceToHost, h->stream));
    if (n > 0 && abs_magnetization)
        MCHK(hipMemcpy2DAsync(abs_magnetization, 4, h->d.serM + walker, (size_t)h->W * 4, 4, n, hipMemcpyDeviceToHost,
                              h->stream));
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_mc_reset_accumulators(dqmc_mc_handle *h)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_reset_accumulators: null handle");
    MCHK(hipSetDevice(h->device));
    const size_t W = h->W;
    MCHK(hipMemsetAsync(h->d.sE, 0, W * 8, h->stream));
    MCHK(hipMemsetAsync(h->d.sE2, 0, W * 8, h->stream));
    MCHK(hipMemsetAsync(h->d.sM, 0, W * 8, h->stream));
    MCHK(hipMemsetAsync(h->d.sM2, 0, W * 8, h->stream));
    MCHK(hipMemsetAsync(h->d.n_meas, 0, W * 8, h->stream));
    MCHK(hipMemsetAsync(h->d.n_series, 0, W * 8, h->stream));
    if (int rc = mc_fss_clear(h)) return rc;
    if (int rc = mc_bin_clear(h)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_mc_binner_enable(dqmc_mc_handle *h, int64_t capacity)
{
    if (int rc = mc_binner_capacity(h, "dqmc_mc_binner_enable", &capacity)) return rc;
    MCHK(hipSetDevice(h->device));
    MCHK(hipStreamSynchronize(h->stream));
    mc_bin_free(h);
    if (int rc = mc_bin_alloc(h, mc_tables::bin_levels(capacity))) {  // the FSS section too, when FSS is on
        mc_bin_free(h);
        return rc;
    }
    const void *kernels[] = {(const void *)ising_sweep_binned_kernel<1>, (const void *)ising_sweep_binned_kernel<2>,
                             (const void *)ising_sweep_binned_kernel<3>, (const void *)ising_sweep_binned_kernel<4>,
                             (const void *)ising_sweep_binned_kernel<5>, (const void *)ising_sweep_binned_kernel<6>,
                             (const void *)ising_sweep_binned_kernel<7>, (const void *)ising_sweep_binned_kernel<8>};
    for (const void *k : kernels)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)h->nw * WAVE * 4)) !=
            hipSuccess) {
            mc_bin_free(h);
            return mc_fail(h, DQMC_ERR_HIP, "dqmc_mc_binner_enable: cannot reserve LDS for the spins");
        }
    MCHK(hipStreamSynchronize(h->stream));
    h->bin.on = true;
    h->bin.cap = capacity;
    return DQMC_OK;
}

int dqmc_mc_binner_size(dqmc_mc_handle *h, int32_t *n_levels, int64_t *n_pushed)
{
    return mc_binner_size(h, "dqmc_mc_binner_size", n_levels, n_pushed);
}

int dqmc_mc_binner_reliable_level(dqmc_mc_handle *h, int32_t *level)
{
    return mc_binner_reliable_level(h, "dqmc_mc_binner_reliable_level", level);
}

int dqmc_mc_binner_get_level(dqmc_mc_handle *h, int32_t walker, int32_t level, double x_sum[4], double x2_sum[4],
                             double xy_sum[2], int64_t *count)
{
    return mc_binner_get_level(h, "dqmc_mc_binner_get_level", mc_blob::SEC_MAIN, nullptr, walker, level, x_sum, x2_sum, xy_sum,
                               count);
}

int dqmc_mc_binner_finish(dqmc_mc_handle *h, int32_t walker, int32_t level, dqmc_mc_binned *out)
{
    return mc_binner_finish(h, "dqmc_mc_binner_finish", mc_blob::SEC_MAIN, nullptr, false, walker, level, out);
}

int dqmc_mc_set_fss(dqmc_mc_handle *h, int32_t n_k, const int32_t *cos_q30, const int32_t *sin_q30)
{
    if (n_k < -1 || n_k > MAX_K)
        return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_set_fss: n_k must be in 0..8 (-1 = off)");
    if (n_k > 0 && (!cos_q30 || !sin_q30)) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_set_fss: null phase table");
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_set_fss: null handle");
    for (long i = 0; i < (long)std::max(n_k, 0) * h->N; ++i)
        if (std::abs((long)cos_q30[i]) > (1L << 30) || std::abs((long)sin_q30[i]) > (1L << 30))
            return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_set_fss: table entry above 2^30 in magnitude");
    MCHK(hipSetDevice(h->device));
    MCHK(hipStreamSynchronize(h->stream));
    dqmc_mc_handle::Fss &f = h->fss;
    f.bin.free(h);
    mc_release(h, f.cq);
    mc_release(h, f.sq);
    f.n_k = -1;
    if (n_k >= 0) {
        const size_t W = h->W, pitch = (size_t)32 * h->nw, n = (size_t)n_k * pitch;
        int rc = 0;
        if (!f.sM4 && ((rc = mc_alloc(h, &f.sM4, W)) || (rc = mc_alloc(h, &f.sS, (size_t)MAX_K * W)) ||
                       (rc = mc_alloc(h, &f.n_meas, W))))
            return rc;
        if ((rc = mc_alloc(h, &f.cq, n)) || (rc = mc_alloc(h, &f.sq, n))) return rc;
        if (n) {  // (mc_alloc zeroed the padding)
            MCHK(hipMemcpy2DAsync(f.cq, pitch * 4, cos_q30, (size_t)h->N * 4, (size_t)h->N * 4, n_k, hipMemcpyHostToDevice,
                                  h->stream));
            MCHK(hipMemcpy2DAsync(f.sq, pitch * 4, sin_q30, (size_t)h->N * 4, (size_t)h->N * 4, n_k, hipMemcpyHostToDevice,
                                  h->stream));
        }
        MCHK(hipStreamSynchronize(h->stream));  // (the tables are the caller's: copied before this returns)
        f.n_k = n_k;
        f.hash = mc_blob::hash_pair(mc_hash(cos_q30, n_k ? (size_t)n_k * h->N : 0), mc_hash(sin_q30, n_k ? (size_t)n_k * h->N : 0));
    }
    if (int rc = mc_fss_clear(h)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    if (h->bin.on) return dqmc_mc_binner_enable(h, h->bin.cap);  // every section empty, the capacity kept
    return DQMC_OK;
}

int dqmc_mc_get_fss(dqmc_mc_handle *h, int32_t walker, dqmc_mc_fss *out)
{
    if (int rc = mc_walker(h, walker, "dqmc_mc_get_fss")) return rc;
    if (!out) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_get_fss: null out");
    const dqmc_mc_handle::Fss &f = h->fss;
    *out = dqmc_mc_fss{};
    out->n_k = f.n_k;
    if (f.n_k < 0) return DQMC_OK;
    MCHK(hipSetDevice(h->device));
    long long n = 0;
    int rc = 0;
    if ((rc = mc_get(h, f.n_meas, 0, walker, &n)) || (rc = mc_get(h, f.sM4, 0, walker, &out->sum_M4))) return rc;
    for (int k = 0; k < f.n_k; ++k)
        if ((rc = mc_get(h, f.sS, k, walker, &out->sum_S[k]))) return rc;
    out->n_meas = n;
    return DQMC_OK;
}

int dqmc_mc_fss_binner_get_level(dqmc_mc_handle *h, int32_t walker, int32_t level, double *x_sum, double *x2_sum,
                                 double *xy_sum, int64_t *count)
{
    return mc_binner_get_level(h, "dqmc_mc_fss_binner_get_level", mc_blob::SEC_SCALING, MC_FSS_OFF, walker, level, x_sum,
                               x2_sum, xy_sum, count);
}

int dqmc_mc_fss_binner_finish(dqmc_mc_handle *h, int32_t walker, int32_t level, dqmc_mc_fss_binned *out)
{
    if (int rc = mc_binner_finish(h, "dqmc_mc_fss_binner_finish", mc_blob::SEC_SCALING, MC_FSS_OFF, true, walker, level, out))
        return rc;
    out->n_k = h->fss.n_k;
    return DQMC_OK;
}

int dqmc_mc_set_update(dqmc_mc_handle *h, int32_t kind, const int32_t *colour, int32_t n_colours)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_set_update: null handle");
    if (kind == DQMC_MC_UPDATE_SEQUENTIAL) {
        h->upd.kind = kind;
        return DQMC_OK;
    }
    if (kind != DQMC_MC_UPDATE_CHECKERBOARD)
        return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_set_update: kind must be 0 (sequential) or 1 (checkerboard)");
    mc_tables::Colouring t;  // the class offsets end at n_colours: [n_colours + 1]
    std::string msg;
    if (!mc_tables::colour_tables("dqmc_mc_set_update", h->nbr_h, h->N, h->z, colour, n_colours, n_colours + 1, CB_THREADS,
                                  t, &msg))
        return mc_fail(h, DQMC_ERR_INVALID, msg);
    MCHK(hipSetDevice(h->device));
    MCHK(hipStreamSynchronize(h->stream));
    dqmc_mc_handle::Update &u = h->upd;
    for (int **p : {&u.site, &u.rows, &u.off}) mc_release(h, *p);
    u.kind = DQMC_MC_UPDATE_SEQUENTIAL;  // (until the new tables are in place)
    int rc = 0;
    if ((rc = mc_alloc(h, &u.site, t.site.size())) || (rc = mc_alloc(h, &u.rows, t.rows.size())) ||
        (rc = mc_alloc(h, &u.off, t.off.size())))
        return rc;
    MCHK(hipMemcpyAsync(u.site, t.site.data(), t.site.size() * 4, hipMemcpyHostToDevice, h->stream));
    MCHK(hipMemcpyAsync(u.rows, t.rows.data(), t.rows.size() * 4, hipMemcpyHostToDevice, h->stream));
    MCHK(hipMemcpyAsync(u.off, t.off.data(), t.off.size() * 4, hipMemcpyHostToDevice, h->stream));
    MCHK(hipStreamSynchronize(h->stream));  // (the vectors are this call's: copied before it returns)
    u.C = n_colours;
    u.threads = t.threads;
    u.hash = mc_hash(colour, (size_t)h->N);
    u.kind = DQMC_MC_UPDATE_CHECKERBOARD;
    return DQMC_OK;
}

int dqmc_mc_get_update(dqmc_mc_handle *h, int32_t walker, dqmc_mc_update_stats *out)
{
    if (int rc = mc_walker(h, walker, "dqmc_mc_get_update")) return rc;
    if (!out) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_mc_get_update: null out");
    MCHK(hipSetDevice(h->device));
    unsigned long long s = 0;
    if (int rc = mc_get(h, h->upd.cursor, 0, walker, &s)) return rc;
    out->kind = h->upd.kind;
    out->n_colours = h->upd.kind == DQMC_MC_UPDATE_CHECKERBOARD ? h->upd.C : 0;
    out->sweeps_drawn = s;
    return DQMC_OK;
}

int dqmc_mc_synchronize(dqmc_mc_handle *h)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_mc_synchronize: null handle");
    MCHK(hipSetDevice(h->device));
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

}  // extern "C"

// checkpoint and resume: dqmc_mc_state_size, _export, _import
#include "ising_state.inl"
