// qstate.hip - the classical MC flavor with q-state models (Potts, clock) behind dqmc_qs_* (include/dqmc_hip.h, "the
// classical MC flavor with q-state models": that comment is the definition, this file follows it).  A handle family of its
// own with its own kernels and DevState; the host layer under it is the one under ising.hip: mc_host.h (the handle base,
// errors, device memory, single-value moves, create and destroy) and mc_tables.h (the lattice and colouring tables).
//
// One workgroup sweeps one walker, colour class by colour class, as the Ising checkerboard path does (ising_cb.inl).  The
// walker's sites are bytes in LDS, its weight table w[q][q] (fp64), e_q30 and the (cos, sin) pairs lie beside them:
// 8 q^2 + 16 q + 32 + N bytes, 50 KiB at q = 64 and N = 16384, about 1 KiB for a 32 x 32 three-state Potts model.  The host
// passes the sites sorted by colour and their padded neighbour rows in that order, read-only and shared by all walkers.
// The sites of a class share no bond: a lane's byte store touches no byte another lane of the class reads.  One barrier
// ends a class.
//
// dE_int, dMx, dMy (int64) and the accepted sites add up in registers and are reduced over the workgroup only where they
// are needed: at a measurement and at the end of the launch.  Lane 0 keeps the walker's fp64 sums in registers for the
// whole launch and adds every measurement in the header's order of operations (compiled with -ffp-contract=off).
//
// The cluster move (the header's "Cluster move") runs inside the sweep kernel's CLUSTER instantiation, on the bytes already
// in LDS, behind the colour passes of a sweep whose index is a multiple of the rate and before its measurement.  Beside the
// sites it keeps a cluster bitset (ceil(N / 32) words), one append-only queue of N 16-bit site indices and a few counters:
// 4 ceil(N / 32) + 2 N + 32 bytes more, 83 KiB in all at q = 64 and N = 16384, reserved for that instantiation alone.  A
// site enters the queue exactly once, by the old value of an LDS atomicOr on its bit, so the N entries hold all levels of
// the breadth-first growth as consecutive ranges.  The slots of a level are spread over the workgroup, one barrier ends a
// level, and the next level's range is read from LDS behind it.  One pass over the queue then adds the boundary terms to
// the lane's dE, dMx, dMy (the sweep's own registers) and writes the reflected bytes.  The host launches the instantiation
// without moves whenever the rate is 0.
//
// The scaling measurement (the header's "Scaling": the structure factor of the order parameter at up to 8 wave vectors) is
// a kernel of its own behind every measured sweep, qs_scaling.inl; the kernels above are what they are without it.  So is
// the stiffness measurement (the header's "Stiffness": the helicity modulus from per-class bond sums), qs_stiffness.inl.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dqmc_hip.h"
#include "kernels.h"
#include "mc_bin_device.h"
#include "mc_host.h"

namespace dqmc_qs {

constexpr int MAX_SITES = 16384;
constexpr int MAX_Z = 8;
constexpr int MAX_Q = 64;
constexpr int MAX_COLOURS = 16;
constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr unsigned int DOMAIN_SWEEP = 4u, DOMAIN_CONF = 5u, DOMAIN_CLUSTER = 6u, DOMAIN_EXCHANGE = 7u;
constexpr int MAX_XJ = 62;  // entries of an exchange pair's table at most: |E_a - E_b| < 2^J as an int64
constexpr double Q30_INV = 1.0 / 1073741824.0;
// The work bound of a launch, in the terms of the Ising checkerboard path (ising.hip, CB_LAUNCH_BUDGET): a sweep counts as
// N + 512 site visits, 512 walkers' workgroups run side by side, and a launch runs at most
// QS_LAUNCH_BUDGET / ((N + 512) max(1, W / 512)) sweeps, one at least.  A q-state site draws two uniforms and reads z table
// entries, so the budget is half the Ising one.
constexpr double QS_LAUNCH_BUDGET = 524288.0;
constexpr double QS_SWEEP_OVERHEAD = 512.0;
constexpr double QS_RESIDENT_WALKERS = 512.0;

struct DevState {
    int N, Nw, W, q, z, cap, n_bonds;  // Nw: 4-byte words of a walker's configuration (N bytes, padded with zeros)
    unsigned int *conf;                // [W][Nw]
    double *wt;                        // [W][q q]
    unsigned long long *key, *cursor;  // [W]
    long long *E, *Mx, *My;            // [W]
    double *sE, *sE2, *sM, *sM2, *sM4;
    long long *n_meas, *prop, *acc, *n_series;
    long long *ser;                    // [W][cap][3]
};

// what the cluster move adds to a handle: the site-ordered neighbour rows and the per-walker global counters
struct ClusterArgs {
    const int *nbr;                     // [N][8]: neighs[k, i] at 8 i + k, 0-based (shared by all walkers)
    long long *prop, *acc, *sum_size;   // [W]
    unsigned long long *cursor;         // [W]: the move cursor m
    int rate;
};

// Philox4x32-10 as kernels.h philox4_uniform, with both uniforms of the output: (o0, o1) -> u1, (o2, o3) -> u2
__device__ __forceinline__ void philox4_two(unsigned long long seed, unsigned int c0, unsigned int c1, unsigned int c2,
                                            unsigned int c3, double &u1, double &u2)
{
    unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0;
        const unsigned int n1 = (unsigned int)p1;
        const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
        const unsigned int n3 = (unsigned int)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    u1 = (double)(((unsigned long long)(c0 >> 5) << 26) | (c1 >> 6)) * (1.0 / 9007199254740992.0);
    u2 = (double)(((unsigned long long)(c2 >> 5) << 26) | (c3 >> 6)) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int mod_q(int d, int q) { return d < 0 ? d + q : d; }  // d in (-q, q)

static inline size_t sweep_lds_bytes(int q, int Nw) { return (size_t)8 * q * q + (size_t)16 * q + 32 + (size_t)4 * Nw; }
// counters (8 words), bitset, queue: what the cluster move keeps behind the sites
static inline size_t cluster_lds_bytes(int N) { return (size_t)32 + (size_t)4 * ((N + 31) / 32) + (size_t)2 * N; }

// One cluster move of the workgroup's walker at move cursor m, on the sites st[] in LDS (the header's "Cluster move").
// All lanes call it behind a barrier (st[] is at rest) and leave it behind one (st[] holds the reflected cluster).  The
// lane's share of dE_int, dMx, dMy is added to dE, dMx, dMy; |C| is returned to every lane.  scratch: 8 counter words, the
// bitset and the queue, in this order.  Any blockDim.x that is a multiple of the wave.
__device__ __forceinline__ int qs_cluster_move_lds(unsigned char *st, const double *wt, const long long *et, const int2 *cs,
                                                   unsigned int *scratch, const int *__restrict__ nbr, int N, int q, int z,
                                                   unsigned long long key, unsigned long long m, long long &dE,
                                                   long long &dMx, long long &dMy)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    unsigned int *cnt = scratch;                   // [3] used: sites appended by a level, in rotation
    unsigned int *bits = scratch + 8;              // [ceil(N / 32)]
    unsigned short *queue = (unsigned short *)(bits + (N + 31) / 32);  // [N]
    const unsigned int m_lo = (unsigned int)m, m_hi = (unsigned int)(m >> 32);
    int i0, r;
    {  // every lane forms the seed and the reflection itself (uniform)
        double u1, u2;
        philox4_two(key, 0u, m_lo, DOMAIN_CLUSTER, m_hi, u1, u2);
        i0 = min(N - 1, (int)(u1 * (double)N));
        r = (2 * (int)st[i0] + 1 + min(q - 2, (int)(u2 * (double)(q - 1)))) % q;
    }
    for (int j = tid; j < (N + 31) / 32; j += nt) bits[j] = j == (i0 >> 5) ? 1u << (i0 & 31) : 0u;
    if (tid == 0) {
        queue[0] = (unsigned short)i0;
        cnt[0] = 0u;
        cnt[1] = 0u;
        cnt[2] = 0u;
    }
    __syncthreads();
    // level by level: queue[lo .. hi) is the last level, its slots append the next one behind hi.  A level counts its
    // sites in cnt[lev]; the counter of the next level is cleared here, two barriers behind its last reader.
    int lo = 0, hi = 1, lev = 0;
    while (lo < hi) {  // (uniform: hi comes from LDS behind the barrier)
        const int nxt = lev == 2 ? 0 : lev + 1;
        if (tid == 0) cnt[nxt] = 0u;
        const int n_slots = (hi - lo) * z;
        for (int x = tid; x < n_slots; x += nt) {
            const int e = x / z, k = x - e * z;
            const int i = queue[lo + e];
            const int j = nbr[8 * i + k];
            const int si = st[i], sj = st[j];
            const int a = mod_q(si - sj, q);
            int b = r - si - sj;  // in (-2 q, q)
            b = b < 0 ? b + q : b;
            b = b < 0 ? b + q : b;
            const unsigned int bit = 1u << (j & 31);
            if (et[a] > et[b] && !(bits[j >> 5] & bit)) {
                double u1, u2;
                philox4_two(key, (unsigned int)(1 + 8 * i + k), m_lo, DOMAIN_CLUSTER, m_hi, u1, u2);
                if (u1 < 1.0 - wt[a * q + b]) {
                    if (!(atomicOr(&bits[j >> 5], bit) & bit)) queue[hi + (int)atomicAdd(&cnt[lev], 1u)] = (unsigned short)j;
                }
            }
        }
        __syncthreads();
        lo = hi;
        hi += (int)cnt[lev];
        lev = nxt;
    }
    // one lane per cluster site.  st[j] is read only for j outside C, and those bytes do not change: no barrier between
    // the reads and the writes.
    for (int x = tid; x < hi; x += nt) {
        const int i = queue[x];
        const int si = st[i];
        long long d = 0;
        for (int k = 0; k < z; ++k) {
            const int j = nbr[8 * i + k];
            if (bits[j >> 5] >> (j & 31) & 1u) continue;
            const int sj = st[j];
            const int a = mod_q(si - sj, q);
            int b = r - si - sj;
            b = b < 0 ? b + q : b;
            b = b < 0 ? b + q : b;
            d += et[a] - et[b];
        }
        const int sn = mod_q(r - si, q);
        const int2 co = cs[si], cn = cs[sn];
        dE += d;
        dMx += (long long)cn.x - co.x;
        dMy += (long long)cn.y - co.y;
        st[i] = (unsigned char)sn;
    }
    __syncthreads();
    return hi;
}

// the walker's binner (the header's "Binner"): a kernel argument of its own, so that DevState keeps its layout.
// xs == nullptr: no binner
struct BinArgs {
    double *xs, *x2, *xy, *c;  // [L][6][W], [L][6][W], [L][3][W], [L - 1][6][W]
    int top;                   // L - 1, the level without a compressor
    long long T;               // the pushes the binner stands at when the launch starts
};

// replica exchange (the header's "Replica exchange"): a kernel argument of its own
struct ExchangeArgs {
    int R, J;                      // ladder length, entries of a pair's table
    unsigned long long x;          // the exchange cursor of this round
    const double *__restrict__ t;  // [J][W], column a: t[j] = exp(-|beta_a - beta_{a+1}| 2^(j - 30)) of the pair (a, a + 1)
    const int *__restrict__ sgn;   // [W], the sign of beta_a - beta_{a+1}
    int *replica;                  // [W], the label of the configuration in the slot
    long long *prop, *acc;         // [W], tries and swaps of the pair (a, a + 1)
};

// One push of walker w at push count T: elements [E, E2, |M|, M2, M2, M4], pairs (2 p, 2 p + 1), state
// [level][element][walker].  lmax = the trailing 1-bits of T, the same for every walker: the levels below it complete a
// pair with their compressor and carry the average upwards, level lmax keeps the value (the top level has no
// compressor).  A level's values are requested together and then written; levels above lmax are not touched.
__device__ __forceinline__ void qs_bin_push(const BinArgs &ba, int W, int w, long long T, double e, double am, double m2,
                                            double m4)
{
    double x[6] = {e, e * e, am, m2, m2, m4};
    const int lmax = min(ba.top, (int)__builtin_ctzll(~(unsigned long long)T));  // (T < capacity < 2^(top + 1))
    const size_t sW = (size_t)W;
    size_t a6 = (size_t)w, a3 = (size_t)w;
    for (int l = 0; l <= lmax; ++l, a6 += 6 * sW, a3 += 3 * sW) {
        const bool carry = l < lmax;
        double s1[6], s2[6], cc[6], pr[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            s1[k] = ba.xs[a6 + k * sW];
            s2[k] = ba.x2[a6 + k * sW];
            cc[k] = carry ? ba.c[a6 + k * sW] : 0.0;
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) pr[p] = ba.xy[a3 + p * sW];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            ba.xs[a6 + k * sW] = s1[k] + x[k];
            ba.x2[a6 + k * sW] = s2[k] + x[k] * x[k];
            if (!carry && l < ba.top) ba.c[a6 + k * sW] = x[k];
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) ba.xy[a3 + p * sW] = pr[p] + x[2 * p] * x[2 * p + 1];
#pragma unroll
        for (int k = 0; k < 6; ++k) x[k] = 0.5 * (cc[k] + x[k]);
    }
}

// the sweep kernel: the two forms of a handle without binner and rounds, then the forms with BIN and DEFER
#define QS_SWEEP_MODES 0
#include "qs_sweep.inl"
#undef QS_SWEEP_MODES
#define QS_SWEEP_MODES 1
#include "qs_sweep.inl"
#undef QS_SWEEP_MODES

// does the pair (a, a + 1) swap in round x.x?  Every lane of the workgroup forms the same answer.
__device__ __forceinline__ bool qs_exchange_decide(const ExchangeArgs &x, int W, int a, unsigned long long key_a, int sgn,
                                                   long long Ea, long long Eb)
{
    const long long d = Ea - Eb;
    if (sgn == 0 || d == 0 || (d > 0) == (sgn > 0)) return true;
    const unsigned long long ad = d < 0 ? 0ull - (unsigned long long)d : (unsigned long long)d;
    double p = 1.0;
    for (int j = 0; j < x.J; ++j)  // (|d| < 2^J: no bit at or above J is set)
        if ((ad >> j) & 1ull) p = p * x.t[(size_t)j * W + a];
    double u1, u2;
    philox4_two(key_a, 0u, (unsigned int)x.x, DOMAIN_EXCHANGE, (unsigned int)(x.x >> 32), u1, u2);
    return u1 < p;
}

// the measurement of slot w on (E, Mx, My) outside the sweep kernel, by one lane: the sums in the header's order of
// operations, the series record, the binner push
__device__ __forceinline__ void qs_measure_slot(const DevState &s, const BinArgs &ba, int w, long long E, long long Mx,
                                                long long My)
{
    const double sE = s.sE[w], sE2 = s.sE2[w], sM = s.sM[w], sM2 = s.sM2[w], sM4 = s.sM4[w];  // requested together
    const long long n_meas = s.n_meas[w], n_series = s.n_series[w];
    const double ev = (double)E * Q30_INV, x = (double)Mx * Q30_INV, y = (double)My * Q30_INV;
    const double m2 = x * x + y * y;
    const double am = sqrt(m2);
    s.sE[w] = sE + ev;
    s.sE2[w] = sE2 + ev * ev;
    s.sM2[w] = sM2 + m2;
    s.sM4[w] = sM4 + m2 * m2;
    s.sM[w] = sM + am;
    s.n_meas[w] = n_meas + 1;
    if (n_series < s.cap) {
        long long *rec = s.ser + ((size_t)w * s.cap + (size_t)n_series) * 3;
        rec[0] = E;
        rec[1] = Mx;
        rec[2] = My;
        s.n_series[w] = n_series + 1;
    }
    if (ba.xs) qs_bin_push(ba, s.W, w, ba.T, ev, am, m2, m2 * m2);
}

// One exchange round (x.x) on the state in device memory, one workgroup per slot that has something to do: the lower
// slot a of each tried pair, which also acts for b = a + 1, and with measure != 0 every slot without a pair in this
// round.  Per ladder these are n_lo = (R - par) / 2 pairs (par = x mod 2) and R - 2 n_lo single slots: slot 0 when par
// is 1, slot R - 1 when R - par is odd; the grid is (W / R) (n_lo + (measure ? R - 2 n_lo : 0)) workgroups.  Every lane
// reads what the decision needs and forms it; behind a barrier the rows of Nw words change places, each word of both
// rows in registers before either is written, and lane 0 writes E_int, Mx, My, the labels and the counters.  measure:
// lane 0 then takes the measurement of the sweep this round ends, for both slots of a pair and for a single slot.
__global__ __launch_bounds__(THREADS) void qs_exchange_kernel(DevState s, ExchangeArgs x, BinArgs ba, int measure)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int par = (int)(x.x & 1ull), n_lo = (x.R - par) / 2, n_un = x.R - 2 * n_lo;
    const int per = n_lo + (measure ? n_un : 0);
    const int ladder = (int)blockIdx.x / per, j = (int)blockIdx.x - ladder * per;
    const bool active = j < n_lo;
    const int il = active ? par + 2 * j : (par && j == n_lo ? 0 : x.R - 1);
    const int a = ladder * x.R + il;
    if (a + (active ? 1 : 0) >= s.W) return;  // (uniform; the host's grid never gets here)
    long long E = s.E[a], Mx = s.Mx[a], My = s.My[a];
    if (active) {  // (uniform)
        const int b = a + 1;
        long long Eb = s.E[b], Mxb = s.Mx[b], Myb = s.My[b];
        const int ra = x.replica[a], rb = x.replica[b], sgn = x.sgn[a];
        const unsigned long long key = s.key[a];
        const long long prop = x.prop[a], acc = x.acc[a];
        const bool swap = qs_exchange_decide(x, s.W, a, key, sgn, E, Eb);
        __syncthreads();  // every lane has read what lane 0 is about to overwrite
        if (swap) {
            unsigned int *ca = s.conf + (size_t)a * s.Nw, *cb = s.conf + (size_t)b * s.Nw;
            for (int k = tid; k < s.Nw; k += nt) {
                const unsigned int va = ca[k], vb = cb[k];
                ca[k] = vb;
                cb[k] = va;
            }
            long long t = E;
            E = Eb, Eb = t;
            t = Mx;
            Mx = Mxb, Mxb = t;
            t = My;
            My = Myb, Myb = t;
        }
        if (tid == 0) {
            x.prop[a] = prop + 1;
            if (swap) {
                x.acc[a] = acc + 1;
                s.E[a] = E;
                s.Mx[a] = Mx;
                s.My[a] = My;
                s.E[b] = Eb;
                s.Mx[b] = Mxb;
                s.My[b] = Myb;
                x.replica[a] = rb;
                x.replica[b] = ra;
            }
            if (measure) qs_measure_slot(s, ba, b, Eb, Mxb, Myb);
        }
    }
    if (measure && tid == 0) qs_measure_slot(s, ba, a, E, Mx, My);
}

// the scaling measurement: ScalingArgs, qs_scaling_kernel
#include "qs_scaling.inl"

// the stiffness measurement: StiffnessArgs, qs_stiffness_bin_push, qs_stiffness_kernel
#include "qs_stiffness.inl"

// dqmc_qs_cluster_move: one move of one walker (walker >= 0) or of every walker, with the sweep kernel's LDS layout
__global__ __launch_bounds__(THREADS) void qs_cluster_move_kernel(DevState s, const long long *__restrict__ e_q30,
                                                                  const int2 *__restrict__ cs_q30, ClusterArgs ca,
                                                                  int walker)
{
    extern __shared__ __align__(16) unsigned char lds[];
    const int w = walker >= 0 ? walker : (int)blockIdx.x;
    if (w >= s.W) return;  // (uniform)
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = s.N, Nw = s.Nw, q = s.q, z = s.z;
    double *wt = (double *)lds;
    long long *et = (long long *)(wt + q * q);
    int2 *cs = (int2 *)(et + q);
    unsigned long long *red = (unsigned long long *)(cs + q);
    unsigned char *st = (unsigned char *)(red + 4);
    {
        unsigned int *stw = (unsigned int *)st;
        const unsigned int *src = s.conf + (size_t)w * Nw;
        for (int j = tid; j < Nw; j += nt) stw[j] = src[j];
        const double *wsrc = s.wt + (size_t)w * q * q;
        for (int j = tid; j < q * q; j += nt) wt[j] = wsrc[j];
        for (int j = tid; j < q; j += nt) {
            et[j] = e_q30[j];
            cs[j] = cs_q30[j];
        }
        if (tid < 3) red[tid] = 0ull;
    }
    const unsigned long long m = ca.cursor[w];
    __syncthreads();
    long long dE = 0, dMx = 0, dMy = 0;
    const int size = qs_cluster_move_lds(st, wt, et, cs, (unsigned int *)(st + 4 * Nw), ca.nbr, N, q, z, s.key[w], m, dE, dMx,
                                         dMy);
    {
        const long long e = wave_sum(dE), mx = wave_sum(dMx), my = wave_sum(dMy);
        if ((tid & (WAVE - 1)) == 0) {
            atomicAdd(&red[0], (unsigned long long)e);
            atomicAdd(&red[1], (unsigned long long)mx);
            atomicAdd(&red[2], (unsigned long long)my);
        }
    }
    __syncthreads();
    {
        const unsigned int *stw = (const unsigned int *)st;
        unsigned int *dst = s.conf + (size_t)w * Nw;
        for (int j = tid; j < Nw; j += nt) dst[j] = stw[j];
    }
    if (tid == 0) {
        s.E[w] += (long long)red[0];
        s.Mx[w] += (long long)red[1];
        s.My[w] += (long long)red[2];
        ca.prop[w] += 1;
        ca.acc[w] += size > 1;
        ca.sum_size[w] += size;
        ca.cursor[w] = m + 1;
    }
}

// the initial configuration of one walker (walker >= 0) or of every walker: site i takes min(q - 1, (int)fl(u1 q)) with
// u1 of P(key; i, low32(r), 5, high32(r)), r = the walker's conf cursor (held on the host)
__global__ __launch_bounds__(THREADS) void qs_rand_conf_kernel(DevState s, const unsigned long long *__restrict__ confs,
                                                               int walker)
{
    const int w = walker >= 0 ? walker : (int)blockIdx.x;
    if (w >= s.W) return;
    const unsigned long long key = s.key[w], r = confs[w];
    unsigned char *dst = (unsigned char *)(s.conf + (size_t)w * s.Nw);
    const double qd = (double)s.q;
    for (int i = threadIdx.x; i < s.N; i += blockDim.x) {
        double u1, u2;
        philox4_two(key, (unsigned int)i, (unsigned int)r, DOMAIN_CONF, (unsigned int)(r >> 32), u1, u2);
        dst[i] = (unsigned char)min(s.q - 1, (int)(u1 * qd));
    }
}

// E_int, Mx, My of one walker (walker >= 0) or of every walker from the configuration in device memory
__global__ __launch_bounds__(THREADS) void qs_observables_kernel(DevState s, const int *__restrict__ bonds,
                                                                 const long long *__restrict__ e_q30,
                                                                 const int2 *__restrict__ cs_q30, int walker)
{
    __shared__ unsigned long long red[3];
    const int w = walker >= 0 ? walker : (int)blockIdx.x;
    if (w >= s.W) return;  // (uniform)
    const int tid = threadIdx.x, q = s.q;
    if (tid < 3) red[tid] = 0ull;
    __syncthreads();
    const unsigned char *st = (const unsigned char *)(s.conf + (size_t)w * s.Nw);
    long long E = 0, Mx = 0, My = 0;
    for (int b = tid; b < s.n_bonds; b += blockDim.x) E -= e_q30[mod_q((int)st[bonds[2 * b]] - (int)st[bonds[2 * b + 1]], q)];
    for (int i = tid; i < s.N; i += blockDim.x) {
        const int2 c = cs_q30[st[i]];
        Mx += c.x;
        My += c.y;
    }
    E = wave_sum(E);
    Mx = wave_sum(Mx);
    My = wave_sum(My);
    if ((tid & (WAVE - 1)) == 0) {
        atomicAdd(&red[0], (unsigned long long)E);
        atomicAdd(&red[1], (unsigned long long)Mx);
        atomicAdd(&red[2], (unsigned long long)My);
    }
    __syncthreads();
    if (tid == 0) {
        s.E[w] = (long long)red[0];
        s.Mx[w] = (long long)red[1];
        s.My[w] = (long long)red[2];
    }
}

}  // namespace dqmc_qs

using namespace dqmc_qs;

static_assert(MAX_Z == mc_tables::ROW && MAX_COLOURS == mc_tables::MAX_COLOURS && WAVE == mc_tables::WAVE,
              "the kernels read the tables mc_tables.h lays out");

struct dqmc_qs_handle : mc_handle_base {
    int N = 0, z = 0, q = 0, Nw = 0, cap = 0, n_bonds = 0;
    int C = 0, threads = THREADS;
    std::vector<int> nbr_h;             // [N][z] 0-based
    std::vector<long long> e_h;         // [q]
    std::vector<unsigned long long> confs_h;  // [W]: the conf cursor r of every walker
    DevState d{};
    int *site = nullptr, *rows = nullptr, *off = nullptr, *bonds = nullptr;  // [N], [N][8], [17], [n_bonds][2]
    long long *e_q30 = nullptr;         // [q]
    int2 *cs_q30 = nullptr;             // [q]
    unsigned long long *confs = nullptr;  // [W], the device image of confs_h for qs_rand_conf_kernel
    ClusterArgs ca{};                   // rate 0: no moves inside dqmc_qs_sweep
    int *nbr_site = nullptr;            // [N][8], what ca.nbr points to
    bool cluster_lds_reserved = false;  // the kernels with a move may ask for more than 64 KiB of dynamic LDS
    struct Tempering {                  // replica exchange (dqmc_qs_set_exchange); R = 0: no ladders
        int R = 0, rate = 0, J = 0;
        uint64_t cursor = 0;            // rounds since dqmc_qs_set_exchange
        double *t = nullptr;            // [J][W]
        int *sgn = nullptr, *replica = nullptr;
        long long *prop = nullptr, *acc = nullptr;
    } xch;
    std::vector<double> beta_h;         // [W], as dqmc_qs_set_beta got them (0 at first)
    // FNV-1a 64 of the tables as the handle got them (the checkpoint blob's header): bonds, (c_q30, s_q30), the colouring
    uint64_t hash_bonds = 0, hash_order = 0, hash_colour = 0;
    struct Binner : mc_bin_section {    // qs_bin_push: elements [E, E2, |M|, M2, M2, M4], pairs (2 p, 2 p + 1)
        bool on = false;
        int64_t cap = 0;
    } bin;
    struct Scaling {                    // dqmc_qs_set_scaling; n_k = 0: off
        int n_k = 0;
        int *cq = nullptr, *sq = nullptr;      // [n_k][4 Nw]: rows padded with zeros to whole configuration words
        double *sS = nullptr;                  // [8][W] (allocated when the feature is first switched on)
        long long *n_meas = nullptr;           // [W]
        // the scaling section of the binner (there iff bin.on && n_k > 0; its levels and capacity are bin's): elements
        // [M2, S_0 ..], pairs (M2, S_k), a compressor value per member of a pair
        mc_bin_section bin;
        uint64_t hash = 0;                     // of the two phase tables as dqmc_qs_set_scaling got them
    } sc;
    struct Stiffness {                  // dqmc_qs_set_stiffness; n_dir = 0: off
        int n_dir = 0, n_c = 0;
        double x[ST_MAX_DIR][ST_MAX_CLASSES] = {};
        signed char *cls = nullptr;            // [N][8]: the slot classes in the order of nbr_site, -1 behind z
        long long *d1 = nullptr, *d2 = nullptr;  // [q]
        double *sT = nullptr, *sJ = nullptr, *sJ2 = nullptr;  // [4][W] (allocated when the feature is first switched on)
        long long *n_meas = nullptr;           // [W]
        long long *sI = nullptr, *sK = nullptr;  // [8][W]: the last sample
        // the stiffness section of the binner (there iff bin.on && n_dir > 0; its levels and capacity are bin's):
        // elements [T_0, J2_0, T_1, J2_1 ..], pairs (2 p, 2 p + 1)
        mc_bin_section bin;
        uint64_t hash_twist = 0, hash = 0;     // of (d1_q30, d2_q30) and of (slot_class, x) as dqmc_qs_set_stiffness got them
    } st;
    // every binner section, at its index in the checkpoint blob (mc_blob.h: SEC_MAIN, SEC_SCALING, SEC_STIFFNESS)
    std::array<mc_bin_section *, 3> sections() { return {&bin, &sc.bin, &st.bin}; }
};

// the binner as the kernels see it at push count T (xs == nullptr: off)
static BinArgs qs_bin_arg(const dqmc_qs_handle *h, int64_t T)
{
    const dqmc_qs_handle::Binner &b = h->bin;
    if (!b.on) return BinArgs{nullptr, nullptr, nullptr, nullptr, 0, 0};
    return BinArgs{b.xs, b.x2, b.xy, b.c, b.L - 1, (long long)T};
}

// One round at the handle's cursor, which it advances.  measure: the round ends a measured sweep, and T is the binner's
// push count at that measurement.
static int qs_launch_exchange(dqmc_qs_handle *h, int measure, int64_t T)
{
    dqmc_qs_handle::Tempering &t = h->xch;
    const int par = (int)(t.cursor & 1), n_lo = (t.R - par) / 2, per = n_lo + (measure ? t.R - 2 * n_lo : 0);
    if (per > 0) {  // (R = 2 at an odd cursor, no measurement: nothing to do)
        const ExchangeArgs xa{t.R, t.J, (unsigned long long)t.cursor, t.t, t.sgn, t.replica, t.prop, t.acc};
        hipLaunchKernelGGL(qs_exchange_kernel, dim3((h->W / t.R) * per), dim3(THREADS), 0, h->stream, h->d, xa,
                           qs_bin_arg(h, T), measure);
        MCHK(hipGetLastError());
    }
    t.cursor += 1;
    return 0;
}

// the table of the pair (a, a + 1) and the sign of beta_a - beta_{a+1}
static void qs_pair_table(const dqmc_qs_handle *h, int a, double *t, int *sgn)
{
    const double db = h->beta_h[a] - h->beta_h[a + 1];
    *sgn = db > 0.0 ? 1 : (db < 0.0 ? -1 : 0);
    mc_tables::qs_exchange_table(db, h->xch.J, t);
}

static int qs_put_pair_table(dqmc_qs_handle *h, int a)
{
    double t[MAX_XJ];
    int sgn = 0;
    qs_pair_table(h, a, t, &sgn);
    if (h->xch.J > 0)
        MCHK(hipMemcpy2DAsync(h->xch.t + a, (size_t)h->W * sizeof(double), t, sizeof(double), sizeof(double), h->xch.J,
                              hipMemcpyHostToDevice, h->stream));
    return mc_put<int>(h, h->xch.sgn, 0, a, sgn);
}

// a validated colouring's tables into the handle's fixed-size arrays (off: all 17 entries, the empty classes at N)
static int qs_put_colouring(dqmc_qs_handle *h, const mc_tables::Colouring &t, int nc)
{
    MCHK(hipSetDevice(h->device));
    MCHK(hipStreamSynchronize(h->stream));
    MCHK(hipMemcpyAsync(h->site, t.site.data(), t.site.size() * 4, hipMemcpyHostToDevice, h->stream));
    MCHK(hipMemcpyAsync(h->rows, t.rows.data(), t.rows.size() * 4, hipMemcpyHostToDevice, h->stream));
    MCHK(hipMemcpyAsync(h->off, t.off.data(), t.off.size() * 4, hipMemcpyHostToDevice, h->stream));
    MCHK(hipStreamSynchronize(h->stream));  // (the vectors are the caller's: copied before it returns)
    h->C = nc;
    h->threads = t.threads;
    return 0;
}

// the dynamic LDS of the kernels with a cluster move, 83 KiB at q = 64 and N = 16384: above the 64 KiB a kernel gets
// without asking, below the 160 KiB of a CU.  Reserved once per handle, for those kernels only, and always at the
// engine's limits: the attribute belongs to the kernel, not to the handle, and a smaller handle must not lower it.
static int qs_reserve_cluster_lds(dqmc_qs_handle *h, const char *fn)
{
    if (h->cluster_lds_reserved) return 0;
    const size_t lds = sweep_lds_bytes(MAX_Q, MAX_SITES / 4) + cluster_lds_bytes(MAX_SITES);
    const void *kernels[] = {(const void *)qs_sweep_kernel<true>, (const void *)qs_cluster_move_kernel,
                             (const void *)qs_sweep_kernel<true, true, false>,
                             (const void *)qs_sweep_kernel<true, false, true>,
                             (const void *)qs_sweep_kernel<true, true, true>};
    for (const void *k : kernels)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return mc_fail(h, DQMC_ERR_HIP, std::string(fn) + ": cannot reserve " + std::to_string(lds) +
                                                " bytes of LDS for the cluster-move kernels");
        }
    h->cluster_lds_reserved = true;
    return 0;
}

static int qs_launch_observables(dqmc_qs_handle *h, int walker)
{
    hipLaunchKernelGGL(qs_observables_kernel, dim3(walker >= 0 ? 1 : h->W), dim3(THREADS), 0, h->stream, h->d,
                       (const int *)h->bonds, (const long long *)h->e_q30, (const int2 *)h->cs_q30, walker);
    MCHK(hipGetLastError());
    return 0;
}

// every section the handle's features call for, at L levels each: the one place that knows their shapes
static int qs_bin_alloc(dqmc_qs_handle *h, int L)
{
    const int n_k = h->sc.n_k, n_dir = h->st.n_dir;
    if (int rc = h->bin.alloc(h, 6, 3, 6, L)) return rc;
    if (n_k > 0)
        if (int rc = h->sc.bin.alloc(h, 1 + n_k, n_k, 2 * n_k, L)) return rc;
    return n_dir > 0 ? h->st.bin.alloc(h, 2 * n_dir, n_dir, 2 * n_dir, L) : 0;
}

static int qs_scaling_clear(dqmc_qs_handle *h)  // the sums (the section: mc_bin_clear)
{
    dqmc_qs_handle::Scaling &f = h->sc;
    const size_t W = h->W;
    if (f.sS) {
        MCHK(hipMemsetAsync(f.sS, 0, (size_t)SC_MAX_K * W * 8, h->stream));
        MCHK(hipMemsetAsync(f.n_meas, 0, W * 8, h->stream));
    }
    return 0;
}

// the scaling measurement of the sweep whose last kernel has just been launched, and its push
static int qs_launch_scaling(dqmc_qs_handle *h)
{
    dqmc_qs_handle::Scaling &f = h->sc;
    ScalingArgs a{};
    a.n_k = f.n_k;
    a.shift = scaling_shift(h->q);
    a.inv = 1.0 / std::ldexp((double)h->N, 120);  // N 2^120 is exact, one rounding
    a.sS = f.sS;
    a.n_meas = f.n_meas;
    if (int rc = f.bin.push_arg(h, "dqmc_qs_sweep", &a.bin)) return rc;
    hipLaunchKernelGGL(qs_scaling_kernel, dim3(h->W), dim3(THREADS), scaling_lds_bytes(f.n_k), h->stream, h->d, a,
                       (const int4 *)f.cq, (const int4 *)f.sq, (const int2 *)h->cs_q30);
    MCHK(hipGetLastError());
    f.bin.pushed();
    return 0;
}

static int qs_stiffness_clear(dqmc_qs_handle *h)  // the sums and the last sample (the section: mc_bin_clear)
{
    dqmc_qs_handle::Stiffness &f = h->st;
    const size_t W = h->W;
    if (f.sT) {
        for (double *p : {f.sT, f.sJ, f.sJ2}) MCHK(hipMemsetAsync(p, 0, (size_t)ST_MAX_DIR * W * 8, h->stream));
        for (long long *p : {f.sI, f.sK}) MCHK(hipMemsetAsync(p, 0, (size_t)ST_MAX_CLASSES * W * 8, h->stream));
        MCHK(hipMemsetAsync(f.n_meas, 0, W * 8, h->stream));
    }
    return 0;
}

// the stiffness measurement of the sweep whose last kernel has just been launched, and its push
static int qs_launch_stiffness(dqmc_qs_handle *h)
{
    dqmc_qs_handle::Stiffness &f = h->st;
    StiffnessArgs a{};
    a.n_dir = f.n_dir;
    a.n_c = f.n_c;
    std::memcpy(a.x, f.x, sizeof(a.x));
    a.sT = f.sT;
    a.sJ = f.sJ;
    a.sJ2 = f.sJ2;
    a.n_meas = f.n_meas;
    a.sI = f.sI;
    a.sK = f.sK;
    if (int rc = f.bin.push_arg(h, "dqmc_qs_sweep", &a.bin)) return rc;
    hipLaunchKernelGGL(qs_stiffness_kernel, dim3(h->W), dim3(THREADS), stiffness_lds_bytes(h->q, h->Nw), h->stream, h->d, a,
                       (const int4 *)h->nbr_site, (const int2 *)f.cls, (const long long *)f.d1, (const long long *)f.d2);
    MCHK(hipGetLastError());
    f.bin.pushed();
    return 0;
}

extern "C" {

const char *dqmc_qs_last_error(const dqmc_qs_handle *h) { return mc_last_error(h); }

int dqmc_qs_create(const dqmc_qs_params *p, dqmc_qs_handle **out)
{
    const std::string f = "dqmc_qs_create";
    if (!p || !out) return mc_fail(nullptr, DQMC_ERR_INVALID, f + ": null argument");
    *out = nullptr;
    if (p->q < 2 || p->q > MAX_Q)
        return mc_fail(nullptr, DQMC_ERR_INVALID, f + ": q = " + std::to_string(p->q) + " is outside 2..64");
    if (p->n_sites < 1 || p->n_walkers < 1)
        return mc_fail(nullptr, DQMC_ERR_INVALID, f + ": n_sites and n_walkers must be >= 1");
    if (p->n_sites > MAX_SITES)
        return mc_fail(nullptr, DQMC_ERR_INVALID, f + ": n_sites = " + std::to_string(p->n_sites) +
                                                      " exceeds 16384 (the walker's sites must fit in LDS)");
    if (p->z < 1 || p->z > MAX_Z)
        return mc_fail(nullptr, DQMC_ERR_INVALID,
                       f + ": z = " + std::to_string(p->z) + " is outside 1..8 (neighbours per site)");
    if (!p->e_q30 || !p->c_q30 || !p->s_q30)
        return mc_fail(nullptr, DQMC_ERR_INVALID, f + ": e_q30, c_q30 or s_q30 missing");
    const int N = p->n_sites, z = p->z, nb = p->n_bonds, q = p->q;
    std::vector<int> nbr, bonds_h;
    std::string msg;
    if (!mc_tables::lattice_tables(f, N, z, nb, p->series_capacity, p->neighs, p->bonds, nbr, bonds_h, &msg))
        return mc_fail(nullptr, DQMC_ERR_INVALID, msg);
    for (int d = 0; d < q; ++d) {
        if (p->e_q30[d] != p->e_q30[(q - d) % q])
            return mc_fail(nullptr, DQMC_ERR_INVALID, f + ": e_q30[" + std::to_string(d) + "] != e_q30[" +
                                                          std::to_string((q - d) % q) + "]: the table is not symmetric");
        if (p->e_q30[d] > (1LL << 32) || p->e_q30[d] < -(1LL << 32))
            return mc_fail(nullptr, DQMC_ERR_INVALID, f + ": e_q30[" + std::to_string(d) + "] exceeds 2^32 in magnitude");
        if (p->c_q30[d] > (1 << 30) || p->c_q30[d] < -(1 << 30) || p->s_q30[d] > (1 << 30) || p->s_q30[d] < -(1 << 30))
            return mc_fail(nullptr, DQMC_ERR_INVALID,
                           f + ": c_q30 / s_q30 entry " + std::to_string(d) + " exceeds 2^30 in magnitude");
    }
    mc_tables::Colouring colouring;
    if (!mc_tables::colour_tables(f, nbr, N, z, p->colour, p->n_colours, MAX_COLOURS + 1, THREADS, colouring, &msg))
        return mc_fail(nullptr, DQMC_ERR_INVALID, msg);
    if (int rc = mc_check_device(f, p->device_id)) return rc;

    dqmc_qs_handle *h = new dqmc_qs_handle();
    h->N = N;
    h->z = z;
    h->q = q;
    h->W = p->n_walkers;
    h->Nw = (N + 3) / 4;
    h->cap = p->series_capacity;
    h->n_bonds = nb;
    h->device = p->device_id;
    h->nbr_h = nbr;
    h->e_h.assign(p->e_q30, p->e_q30 + q);
    h->confs_h.assign((size_t)h->W, 0ull);
    h->beta_h.assign((size_t)h->W, 0.0);
    h->hash_bonds = mc_hash(bonds_h);
    h->hash_order = mc_blob::hash_pair(mc_hash(p->c_q30, (size_t)q), mc_hash(p->s_q30, (size_t)q));
    h->hash_colour = mc_hash(p->colour, (size_t)N);
    std::vector<int2> cs_h((size_t)q);
    for (int d = 0; d < q; ++d) cs_h[d] = make_int2(p->c_q30[d], p->s_q30[d]);
    auto bail = [&](int rc) { return mc_bail(h, rc); };
    if (int rc = mc_open(h, f)) return bail(rc);
    DevState &d = h->d;
    d.N = N;
    d.Nw = h->Nw;
    d.W = h->W;
    d.q = q;
    d.z = z;
    d.cap = h->cap;
    d.n_bonds = nb;
    const size_t W = h->W;
    int rc = 0;
    if ((rc = mc_alloc(h, &d.conf, (size_t)h->Nw * W)) || (rc = mc_alloc(h, &d.wt, (size_t)q * q * W)) ||
        (rc = mc_alloc(h, &d.key, W)) || (rc = mc_alloc(h, &d.cursor, W)) || (rc = mc_alloc(h, &d.E, W)) ||
        (rc = mc_alloc(h, &d.Mx, W)) || (rc = mc_alloc(h, &d.My, W)) || (rc = mc_alloc(h, &d.sE, W)) ||
        (rc = mc_alloc(h, &d.sE2, W)) || (rc = mc_alloc(h, &d.sM, W)) || (rc = mc_alloc(h, &d.sM2, W)) ||
        (rc = mc_alloc(h, &d.sM4, W)) || (rc = mc_alloc(h, &d.n_meas, W)) || (rc = mc_alloc(h, &d.prop, W)) ||
        (rc = mc_alloc(h, &d.acc, W)) || (rc = mc_alloc(h, &d.n_series, W)) ||
        (rc = mc_alloc(h, &d.ser, (size_t)3 * h->cap * W)) || (rc = mc_alloc(h, &h->site, (size_t)N)) ||
        (rc = mc_alloc(h, &h->rows, (size_t)N * MAX_Z)) || (rc = mc_alloc(h, &h->off, (size_t)MAX_COLOURS + 1)) ||
        (rc = mc_alloc(h, &h->bonds, bonds_h.size())) || (rc = mc_alloc(h, &h->e_q30, (size_t)q)) ||
        (rc = mc_alloc(h, &h->cs_q30, (size_t)q)) || (rc = mc_alloc(h, &h->confs, W)) ||
        (rc = mc_alloc(h, &h->nbr_site, (size_t)N * MAX_Z)) || (rc = mc_alloc(h, &h->ca.prop, W)) ||
        (rc = mc_alloc(h, &h->ca.acc, W)) || (rc = mc_alloc(h, &h->ca.sum_size, W)) ||
        (rc = mc_alloc(h, &h->ca.cursor, W)))
        return bail(rc);
    h->ca.nbr = h->nbr_site;
    h->ca.rate = 0;
    const std::vector<int> nbr_site = mc_tables::padded_rows(nbr, N, z, N);
    std::vector<double> ones((size_t)q * q * W, 1.0);  // beta = 0
    if (hipMemcpyAsync(d.wt, ones.data(), ones.size() * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(h->nbr_site, nbr_site.data(), nbr_site.size() * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        (nb && hipMemcpyAsync(h->bonds, bonds_h.data(), bonds_h.size() * 4, hipMemcpyHostToDevice, h->stream) !=
                   hipSuccess) ||
        hipMemcpyAsync(h->e_q30, h->e_h.data(), (size_t)q * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(h->cs_q30, cs_h.data(), (size_t)q * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
        return bail(mc_fail(h, DQMC_ERR_HIP, f + ": table upload failed"));
    if ((rc = qs_put_colouring(h, colouring, p->n_colours))) return bail(rc);
    if ((rc = qs_launch_observables(h, -1))) return bail(rc);  // all sites in state 0
    if (hipStreamSynchronize(h->stream) != hipSuccess)
        return bail(mc_fail(h, DQMC_ERR_HIP, f + ": device initialisation failed"));
    *out = h;
    return DQMC_OK;
}

int dqmc_qs_destroy(dqmc_qs_handle *h) { return mc_destroy(h); }

int dqmc_qs_seed(dqmc_qs_handle *h, int32_t walker, uint64_t seed)
{
    if (int rc = mc_walker(h, walker, "dqmc_qs_seed")) return rc;
    MCHK(hipSetDevice(h->device));
    if (int rc = mc_put<unsigned long long>(h, h->d.key, 0, walker, seed)) return rc;
    h->confs_h[walker] = 0ull;
    if (int rc = mc_put<unsigned long long>(h, h->ca.cursor, 0, walker, 0ull)) return rc;
    return mc_put<unsigned long long>(h, h->d.cursor, 0, walker, 0ull);
}

int dqmc_qs_set_beta(dqmc_qs_handle *h, int32_t walker, double beta)
{
    if (int rc = mc_walker(h, walker, "dqmc_qs_set_beta")) return rc;
    if (!std::isfinite(beta) || beta < 0.0)
        return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_set_beta: beta must be finite and >= 0");
    const int q = h->q;
    {  // the domain in which no partial acceptance product overflows or vanishes; a refusal changes nothing
        const std::vector<int64_t> e(h->e_h.begin(), h->e_h.end());
        std::string msg;
        if (!mc_tables::qs_beta_in_domain("dqmc_qs_set_beta", beta, h->z, e.data(), q, &msg))
            return mc_fail(h, DQMC_ERR_INVALID, msg);
    }
    std::vector<double> wt((size_t)q * q);
    for (int a = 0; a < q; ++a)
        for (int b = 0; b < q; ++b) {
            const double x = (double)(h->e_h[a] - h->e_h[b]) * Q30_INV;  // exact
            const double y = -beta * x;                                   // one rounding
            wt[(size_t)a * q + b] = exp(y);
        }
    MCHK(hipSetDevice(h->device));
    MCHK(hipMemcpyAsync(h->d.wt + (size_t)walker * q * q, wt.data(), wt.size() * 8, hipMemcpyHostToDevice, h->stream));
    MCHK(hipStreamSynchronize(h->stream));
    h->beta_h[walker] = beta;
    const int R = h->xch.R;  // the exchange tables of the at most two pairs this slot belongs to
    if (R >= 2 && walker % R > 0)
        if (int rc = qs_put_pair_table(h, walker - 1)) return rc;
    if (R >= 2 && walker % R + 1 < R)
        if (int rc = qs_put_pair_table(h, walker)) return rc;
    return DQMC_OK;
}

int dqmc_qs_rand_conf(dqmc_qs_handle *h, int32_t walker)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_qs_rand_conf: null handle");
    if (walker >= h->W) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_rand_conf: walker out of range");
    MCHK(hipSetDevice(h->device));
    MCHK(hipMemcpyAsync(h->confs, h->confs_h.data(), (size_t)h->W * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(qs_rand_conf_kernel, dim3(walker >= 0 ? 1 : h->W), dim3(THREADS), 0, h->stream, h->d,
                       (const unsigned long long *)h->confs, (int)walker);
    MCHK(hipGetLastError());
    if (int rc = qs_launch_observables(h, walker)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    for (int w = 0; w < h->W; ++w)
        if (walker < 0 || w == walker) h->confs_h[w] += 1;
    return DQMC_OK;
}

int dqmc_qs_set_conf(dqmc_qs_handle *h, int32_t walker, const uint8_t *conf)
{
    if (int rc = mc_walker(h, walker, "dqmc_qs_set_conf")) return rc;
    if (!conf) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_set_conf: null conf");
    std::vector<unsigned int> words((size_t)h->Nw, 0u);
    for (int i = 0; i < h->N; ++i) {
        if (conf[i] >= h->q)
            return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_set_conf: the state of site " + std::to_string(i) +
                                                    " (0-based) is not below q");
        words[i >> 2] |= (unsigned int)conf[i] << (8 * (i & 3));
    }
    MCHK(hipSetDevice(h->device));
    MCHK(hipMemcpyAsync(h->d.conf + (size_t)walker * h->Nw, words.data(), words.size() * 4, hipMemcpyHostToDevice,
                        h->stream));
    if (int rc = qs_launch_observables(h, walker)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_qs_get_conf(dqmc_qs_handle *h, int32_t walker, uint8_t *conf)
{
    if (int rc = mc_walker(h, walker, "dqmc_qs_get_conf")) return rc;
    if (!conf) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_get_conf: null conf");
    std::vector<unsigned int> words((size_t)h->Nw, 0u);
    MCHK(hipSetDevice(h->device));
    MCHK(hipMemcpyAsync(words.data(), h->d.conf + (size_t)walker * h->Nw, words.size() * 4, hipMemcpyDeviceToHost,
                        h->stream));
    MCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < h->N; ++i) conf[i] = (uint8_t)(words[i >> 2] >> (8 * (i & 3)));
    return DQMC_OK;
}

int dqmc_qs_set_colouring(dqmc_qs_handle *h, const int32_t *colour, int32_t n_colours)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_qs_set_colouring: null handle");
    mc_tables::Colouring t;
    std::string msg;
    if (!mc_tables::colour_tables("dqmc_qs_set_colouring", h->nbr_h, h->N, h->z, colour, n_colours, MAX_COLOURS + 1, THREADS, t,
                                  &msg))
        return mc_fail(h, DQMC_ERR_INVALID, msg);
    if (int rc = qs_put_colouring(h, t, n_colours)) return rc;
    h->hash_colour = mc_hash(colour, (size_t)h->N);
    return DQMC_OK;
}

int dqmc_qs_sweep(dqmc_qs_handle *h, int32_t n_sweeps, int64_t first_sweep_index, int64_t thermalization,
                  int32_t measure_rate)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_qs_sweep: null handle");
    if (n_sweeps < 0 || measure_rate < 1 || first_sweep_index < 1)
        return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_sweep: n_sweeps >= 0, first_sweep_index >= 1, measure_rate >= 1");
    dqmc_qs_handle::Binner &b = h->bin;
    const int64_t n_meas = mc_tables::measurements_in(first_sweep_index, first_sweep_index + n_sweeps - 1, thermalization,
                                                      measure_rate);
    if (b.on && b.T + n_meas > b.cap)
        return mc_fail(h, DQMC_ERR_STATE, "dqmc_qs_sweep: the measurements of this call would pass the binner's capacity");
    dqmc_qs_handle::Scaling &sc = h->sc;
    if (sc.bin.xs && sc.bin.T + n_meas > b.cap)
        return mc_fail(h, DQMC_ERR_STATE, "dqmc_qs_sweep: the measurements of this call would pass the capacity of the "
                                          "binner's scaling section");
    dqmc_qs_handle::Stiffness &sf = h->st;
    if (sf.bin.xs && sf.bin.T + n_meas > b.cap)
        return mc_fail(h, DQMC_ERR_STATE, "dqmc_qs_sweep: the measurements of this call would pass the capacity of the "
                                          "binner's stiffness section");
    MCHK(hipSetDevice(h->device));
    const double per_sweep = ((double)h->N + QS_SWEEP_OVERHEAD) * std::max(1.0, (double)h->W / QS_RESIDENT_WALKERS);
    const int chunk = (int)std::max(1.0, std::min((double)n_sweeps, std::floor(QS_LAUNCH_BUDGET / per_sweep)));
    const bool cluster = h->ca.rate > 0;
    const size_t lds = sweep_lds_bytes(h->q, h->Nw) + (cluster ? cluster_lds_bytes(h->N) : 0);
    const int k = h->xch.R >= 2 ? h->xch.rate : 0;  // an exchange round after every k-th sweep
    // scaling or stiffness on: a launch also ends at every measured sweep, and the measurement kernels run behind it
    const std::vector<mc_tables::SweepLaunch> launches =
        sc.n_k > 0 || sf.n_dir > 0 ? mc_tables::qs_scaling_cut(n_sweeps, first_sweep_index, thermalization, measure_rate, k, chunk, b.T)
                   : mc_tables::qs_sweep_cut(n_sweeps, first_sweep_index, thermalization, measure_rate, k, chunk, b.T);
    for (const mc_tables::SweepLaunch &l : launches) {
        const long long last = l.first + l.n_sweeps - 1;
        const BinArgs ba = qs_bin_arg(h, l.T_at_start);
#define QS_SWEEP(...)                                                                                                  \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(qs_sweep_kernel<__VA_ARGS__>), dim3(h->W), dim3(h->threads), lds, h->stream, h->d,                \
                       (const int *)h->site, (const int4 *)h->rows, (const int *)h->off, (const long long *)h->e_q30,      \
                       (const int2 *)h->cs_q30, h->C, l.n_sweeps, (long long)l.first, (long long)thermalization,           \
                       (int)measure_rate, h->ca
        // binner off and no measurement handed to a round: the forms of a handle that has neither feature
        if (!b.on && !l.defer_last) {
            if (cluster) QS_SWEEP(true));
            else QS_SWEEP(false));
        } else if (cluster) {
            if (b.on && l.defer_last) QS_SWEEP(true, true, true), ba);
            else if (b.on) QS_SWEEP(true, true, false), ba);
            else QS_SWEEP(true, false, true), ba);
        } else {
            if (b.on && l.defer_last) QS_SWEEP(false, true, true), ba);
            else if (b.on) QS_SWEEP(false, true, false), ba);
            else QS_SWEEP(false, false, true), ba);
        }
#undef QS_SWEEP
        MCHK(hipGetLastError());
        if (k > 0 && last % k == 0) {  // the round of sweep `last`, with that sweep's measurement if it has one
            const int64_t T = l.T_at_start + mc_tables::measurements_in(l.first, last, thermalization, measure_rate) - 1;
            if (int rc = qs_launch_exchange(h, l.defer_last ? 1 : 0, l.defer_last ? T : 0)) return rc;
        }
        if (sc.n_k > 0 && last > thermalization && last % measure_rate == 0)
            if (int rc = qs_launch_scaling(h)) return rc;
        if (sf.n_dir > 0 && last > thermalization && last % measure_rate == 0)
            if (int rc = qs_launch_stiffness(h)) return rc;
    }
    if (b.on) b.T += n_meas;
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_qs_get_stats(dqmc_qs_handle *h, int32_t walker, dqmc_qs_stats *out)
{
    if (int rc = mc_walker(h, walker, "dqmc_qs_get_stats")) return rc;
    if (!out) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_get_stats: null out");
    MCHK(hipSetDevice(h->device));
    const DevState &d = h->d;
    long long E = 0, Mx = 0, My = 0, n_meas = 0, prop = 0, acc = 0, n_series = 0;
    unsigned long long cursor = 0;
    int rc = 0;
    if ((rc = mc_get(h, d.E, 0, walker, &E)) || (rc = mc_get(h, d.Mx, 0, walker, &Mx)) || (rc = mc_get(h, d.My, 0, walker, &My)) ||
        (rc = mc_get(h, d.sE, 0, walker, &out->sum_E)) || (rc = mc_get(h, d.sE2, 0, walker, &out->sum_E2)) ||
        (rc = mc_get(h, d.sM, 0, walker, &out->sum_absM)) || (rc = mc_get(h, d.sM2, 0, walker, &out->sum_M2)) ||
        (rc = mc_get(h, d.sM4, 0, walker, &out->sum_M4)) || (rc = mc_get(h, d.n_meas, 0, walker, &n_meas)) ||
        (rc = mc_get(h, d.prop, 0, walker, &prop)) || (rc = mc_get(h, d.acc, 0, walker, &acc)) ||
        (rc = mc_get(h, d.n_series, 0, walker, &n_series)) || (rc = mc_get(h, d.cursor, 0, walker, &cursor)))
        return rc;
    out->energy_q30 = E;
    out->mx_q30 = Mx;
    out->my_q30 = My;
    out->n_meas = n_meas;
    out->prop_local = prop;
    out->acc_local = acc;
    out->sweeps_drawn = cursor;
    out->confs_drawn = h->confs_h[walker];
    out->n_series = n_series;
    out->n_colours = h->C;
    return DQMC_OK;
}

int dqmc_qs_get_series(dqmc_qs_handle *h, int32_t walker, int64_t *energy_q30, int64_t *mx_q30, int64_t *my_q30,
                       int64_t *n_recorded)
{
    if (int rc = mc_walker(h, walker, "dqmc_qs_get_series")) return rc;
    MCHK(hipSetDevice(h->device));
    long long n = 0;
    if (int rc = mc_get(h, h->d.n_series, 0, walker, &n)) return rc;
    if (n_recorded) *n_recorded = n;
    if (n > 0 && (energy_q30 || mx_q30 || my_q30)) {
        std::vector<long long> rec((size_t)3 * n);
        MCHK(hipMemcpyAsync(rec.data(), h->d.ser + (size_t)walker * h->cap * 3, rec.size() * 8, hipMemcpyDeviceToHost,
                            h->stream));
        MCHK(hipStreamSynchronize(h->stream));
        for (long long k = 0; k < n; ++k) {
            if (energy_q30) energy_q30[k] = rec[3 * k];
            if (mx_q30) mx_q30[k] = rec[3 * k + 1];
            if (my_q30) my_q30[k] = rec[3 * k + 2];
        }
    }
    return DQMC_OK;
}

int dqmc_qs_reset_accumulators(dqmc_qs_handle *h)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_qs_reset_accumulators: null handle");
    MCHK(hipSetDevice(h->device));
    const DevState &d = h->d;
    const size_t W = h->W;
    for (double *p : {d.sE, d.sE2, d.sM, d.sM2, d.sM4}) MCHK(hipMemsetAsync(p, 0, W * 8, h->stream));
    for (long long *p : {d.n_meas, d.n_series}) MCHK(hipMemsetAsync(p, 0, W * 8, h->stream));
    if (int rc = qs_scaling_clear(h)) return rc;
    if (int rc = qs_stiffness_clear(h)) return rc;
    if (int rc = mc_bin_clear(h)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_qs_set_exchange(dqmc_qs_handle *h, int32_t n_replicas, int32_t rate)
{
    int R = 0;
    if (int rc = mc_exchange_ladders(h, "dqmc_qs_set_exchange", n_replicas, rate, &R)) return rc;
    const std::vector<int64_t> e(h->e_h.begin(), h->e_h.end());
    const int J = mc_tables::qs_exchange_bits(h->n_bonds, e.data(), h->q);
    if (R && J > MAX_XJ)
        return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_set_exchange: an energy difference needs " + std::to_string(J) +
                                                " bits, above the 62 a pair's table has");
    MCHK(hipSetDevice(h->device));
    dqmc_qs_handle::Tempering &t = h->xch;
    const size_t W = h->W;
    if (R && !t.sgn) {
        int rc = 0;
        if ((rc = mc_alloc(h, &t.t, (size_t)J * W)) || (rc = mc_alloc(h, &t.sgn, W)) || (rc = mc_alloc(h, &t.replica, W)) ||
            (rc = mc_alloc(h, &t.prop, W)) || (rc = mc_alloc(h, &t.acc, W)))
            return rc;
    }
    t.R = R;
    t.rate = rate;
    t.cursor = 0;
    t.J = J;
    if (t.sgn) {
        MCHK(hipMemsetAsync(t.prop, 0, W * 8, h->stream));
        MCHK(hipMemsetAsync(t.acc, 0, W * 8, h->stream));
        std::vector<int> label(W, 0), sgn(W, 0);
        std::vector<double> tab((size_t)std::max(J, 1) * W, 0.0);
        for (size_t w = 0; R && w < W; ++w) {
            label[w] = (int)(w % R);
            if (w % R + 1 == (size_t)R) continue;  // the last slot of a ladder has no pair of its own
            double col[MAX_XJ];
            qs_pair_table(h, (int)w, col, &sgn[w]);
            for (int j = 0; j < J; ++j) tab[(size_t)j * W + w] = col[j];
        }
        MCHK(hipMemcpyAsync(t.replica, label.data(), W * 4, hipMemcpyHostToDevice, h->stream));
        MCHK(hipMemcpyAsync(t.sgn, sgn.data(), W * 4, hipMemcpyHostToDevice, h->stream));
        if (J > 0) MCHK(hipMemcpyAsync(t.t, tab.data(), (size_t)J * W * 8, hipMemcpyHostToDevice, h->stream));
    }
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_qs_exchange(dqmc_qs_handle *h)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_qs_exchange: null handle");
    if (h->xch.R < 2)
        return mc_fail(h, DQMC_ERR_STATE, "dqmc_qs_exchange: no ladders (dqmc_qs_set_exchange with n_replicas >= 2 first)");
    MCHK(hipSetDevice(h->device));
    if (int rc = qs_launch_exchange(h, 0, 0)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_qs_get_exchange_stats(dqmc_qs_handle *h, int32_t walker, dqmc_qs_exchange_stats *out)
{
    return mc_get_exchange_stats(h, "dqmc_qs_get_exchange_stats", walker, out);
}

int dqmc_qs_binner_enable(dqmc_qs_handle *h, int64_t capacity)
{
    if (int rc = mc_binner_capacity(h, "dqmc_qs_binner_enable", &capacity)) return rc;
    MCHK(hipSetDevice(h->device));
    MCHK(hipStreamSynchronize(h->stream));
    mc_bin_free(h);
    if (int rc = qs_bin_alloc(h, mc_tables::bin_levels(capacity))) {  // with the sections of the features that are on
        mc_bin_free(h);
        return rc;
    }
    MCHK(hipStreamSynchronize(h->stream));
    h->bin.on = true;
    h->bin.cap = capacity;
    return DQMC_OK;
}

int dqmc_qs_binner_size(dqmc_qs_handle *h, int32_t *n_levels, int64_t *n_pushed)
{
    return mc_binner_size(h, "dqmc_qs_binner_size", n_levels, n_pushed);
}

int dqmc_qs_binner_reliable_level(dqmc_qs_handle *h, int32_t *level)
{
    return mc_binner_reliable_level(h, "dqmc_qs_binner_reliable_level", level);
}

int dqmc_qs_binner_get_level(dqmc_qs_handle *h, int32_t walker, int32_t level, double x_sum[6], double x2_sum[6],
                             double xy_sum[3], int64_t *count)
{
    return mc_binner_get_level(h, "dqmc_qs_binner_get_level", mc_blob::SEC_MAIN, nullptr, walker, level, x_sum, x2_sum, xy_sum,
                               count);
}

int dqmc_qs_binner_finish(dqmc_qs_handle *h, int32_t walker, int32_t level, dqmc_qs_binned *out)
{
    return mc_binner_finish(h, "dqmc_qs_binner_finish", mc_blob::SEC_MAIN, nullptr, false, walker, level, out);
}

static const char *const QS_SCALING_OFF = ": the scaling measurement is off (dqmc_qs_set_scaling first)";
static const char *const QS_STIFFNESS_OFF = ": the stiffness measurement is off (dqmc_qs_set_stiffness first)";

int dqmc_qs_set_scaling(dqmc_qs_handle *h, int32_t n_k, const int32_t *cos_q30, const int32_t *sin_q30)
{
    if (n_k < 0 || n_k > SC_MAX_K) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_set_scaling: n_k must be in 0..8 (0 = off)");
    if (n_k > 0 && (!cos_q30 || !sin_q30)) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_set_scaling: null phase table");
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_qs_set_scaling: null handle");
    for (long i = 0; i < (long)n_k * h->N; ++i)
        if (std::abs((long)cos_q30[i]) > (1L << 30) || std::abs((long)sin_q30[i]) > (1L << 30))
            return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_set_scaling: table entry above 2^30 in magnitude");
    MCHK(hipSetDevice(h->device));
    MCHK(hipStreamSynchronize(h->stream));
    dqmc_qs_handle::Scaling &f = h->sc;
    f.bin.free(h);
    mc_release(h, f.cq);
    mc_release(h, f.sq);
    f.n_k = 0;
    if (n_k > 0) {
        const size_t W = h->W, pitch = (size_t)4 * h->Nw, n = (size_t)n_k * pitch;
        int rc = 0;
        if (!f.sS && ((rc = mc_alloc(h, &f.sS, (size_t)SC_MAX_K * W)) || (rc = mc_alloc(h, &f.n_meas, W)))) return rc;
        if ((rc = mc_alloc(h, &f.cq, n)) || (rc = mc_alloc(h, &f.sq, n))) return rc;  // (mc_alloc zeroes the padding)
        MCHK(hipMemcpy2DAsync(f.cq, pitch * 4, cos_q30, (size_t)h->N * 4, (size_t)h->N * 4, n_k, hipMemcpyHostToDevice,
                              h->stream));
        MCHK(hipMemcpy2DAsync(f.sq, pitch * 4, sin_q30, (size_t)h->N * 4, (size_t)h->N * 4, n_k, hipMemcpyHostToDevice,
                              h->stream));
        MCHK(hipStreamSynchronize(h->stream));  // (the tables are the caller's: copied before this returns)
        f.n_k = n_k;
        f.hash = mc_blob::hash_pair(mc_hash(cos_q30, (size_t)n_k * h->N), mc_hash(sin_q30, (size_t)n_k * h->N));
    }
    if (int rc = qs_scaling_clear(h)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    if (h->bin.on) return dqmc_qs_binner_enable(h, h->bin.cap);  // every section empty, the capacity kept
    return DQMC_OK;
}

int dqmc_qs_get_scaling(dqmc_qs_handle *h, int32_t walker, dqmc_qs_scaling *out)
{
    if (int rc = mc_walker(h, walker, "dqmc_qs_get_scaling")) return rc;
    if (!out) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_get_scaling: null out");
    const dqmc_qs_handle::Scaling &f = h->sc;
    *out = dqmc_qs_scaling{};
    if (f.n_k < 1) return DQMC_OK;
    MCHK(hipSetDevice(h->device));
    long long n = 0;
    if (int rc = mc_get(h, f.n_meas, 0, walker, &n)) return rc;
    for (int k = 0; k < f.n_k; ++k)
        if (int rc = mc_get(h, f.sS, k, walker, &out->sum_S[k])) return rc;
    out->n_meas = n;
    out->n_k = f.n_k;
    return DQMC_OK;
}

int dqmc_qs_scaling_binner_get_level(dqmc_qs_handle *h, int32_t walker, int32_t level, double *x_sum, double *x2_sum,
                                     double *xy_sum, int64_t *count)
{
    return mc_binner_get_level(h, "dqmc_qs_scaling_binner_get_level", mc_blob::SEC_SCALING, QS_SCALING_OFF, walker, level,
                               x_sum, x2_sum, xy_sum, count);
}

int dqmc_qs_scaling_binner_finish(dqmc_qs_handle *h, int32_t walker, int32_t level, dqmc_qs_scaling_binned *out)
{
    if (int rc = mc_binner_finish(h, "dqmc_qs_scaling_binner_finish", mc_blob::SEC_SCALING, QS_SCALING_OFF, true, walker, level,
                                  out))
        return rc;
    out->n_k = h->sc.n_k;
    return DQMC_OK;
}

int dqmc_qs_set_stiffness(dqmc_qs_handle *h, int32_t n_dir, int32_t n_classes, const int8_t *slot_class,
                          const int64_t *d1_q30, const int64_t *d2_q30, const double *x)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_qs_set_stiffness: null handle");
    const int N = h->N, z = h->z, q = h->q;
    if (n_dir != 0) {  // everything before the device is touched; a refusal leaves the handle as it was
        std::string msg;
        if (!mc_tables::qs_stiffness_check("dqmc_qs_set_stiffness", N, z, q, n_dir, n_classes, slot_class, d1_q30, d2_q30, x,
                                           &msg))
            return mc_fail(h, DQMC_ERR_INVALID, msg);
    }
    MCHK(hipSetDevice(h->device));
    MCHK(hipStreamSynchronize(h->stream));
    dqmc_qs_handle::Stiffness &f = h->st;
    f.bin.free(h);
    f.n_dir = 0;
    f.n_c = 0;
    if (n_dir > 0) {
        const size_t W = h->W;
        int rc = 0;
        if (!f.sT && ((rc = mc_alloc(h, &f.sT, (size_t)ST_MAX_DIR * W)) || (rc = mc_alloc(h, &f.sJ, (size_t)ST_MAX_DIR * W)) ||
                      (rc = mc_alloc(h, &f.sJ2, (size_t)ST_MAX_DIR * W)) || (rc = mc_alloc(h, &f.n_meas, W)) ||
                      (rc = mc_alloc(h, &f.sI, (size_t)ST_MAX_CLASSES * W)) ||
                      (rc = mc_alloc(h, &f.sK, (size_t)ST_MAX_CLASSES * W)) || (rc = mc_alloc(h, &f.cls, (size_t)N * MAX_Z)) ||
                      (rc = mc_alloc(h, &f.d1, (size_t)q)) || (rc = mc_alloc(h, &f.d2, (size_t)q))))
            return rc;
        std::vector<signed char> cls((size_t)N * MAX_Z, (signed char)-1);  // the rows of nbr_site: slot k of site i at 8 i + k
        for (int i = 0; i < N; ++i)
            for (int k = 0; k < z; ++k) cls[(size_t)i * MAX_Z + k] = (signed char)slot_class[(size_t)i * z + k];
        MCHK(hipMemcpyAsync(f.cls, cls.data(), cls.size(), hipMemcpyHostToDevice, h->stream));
        MCHK(hipMemcpyAsync(f.d1, d1_q30, (size_t)q * 8, hipMemcpyHostToDevice, h->stream));
        MCHK(hipMemcpyAsync(f.d2, d2_q30, (size_t)q * 8, hipMemcpyHostToDevice, h->stream));
        MCHK(hipStreamSynchronize(h->stream));  // (the tables are the caller's: copied before this returns)
        std::memset(f.x, 0, sizeof(f.x));
        for (int m = 0; m < n_dir; ++m)
            for (int c = 0; c < n_classes; ++c) f.x[m][c] = x[(size_t)m * n_classes + c];
        f.n_dir = n_dir;
        f.n_c = n_classes;
        f.hash_twist = mc_blob::hash_pair(mc_hash(d1_q30, (size_t)q), mc_hash(d2_q30, (size_t)q));
        f.hash = mc_blob::hash_pair(mc_hash(slot_class, (size_t)N * z), mc_hash(x, (size_t)n_dir * n_classes));
    }
    if (int rc = qs_stiffness_clear(h)) return rc;
    MCHK(hipStreamSynchronize(h->stream));
    if (h->bin.on) return dqmc_qs_binner_enable(h, h->bin.cap);  // every section empty, the capacity kept
    return DQMC_OK;
}

int dqmc_qs_get_stiffness(dqmc_qs_handle *h, int32_t walker, dqmc_qs_stiffness *out)
{
    if (int rc = mc_walker(h, walker, "dqmc_qs_get_stiffness")) return rc;
    if (!out) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_get_stiffness: null out");
    const dqmc_qs_handle::Stiffness &f = h->st;
    *out = dqmc_qs_stiffness{};
    if (f.n_dir < 1) return DQMC_OK;
    MCHK(hipSetDevice(h->device));
    long long n = 0;
    if (int rc = mc_get(h, f.n_meas, 0, walker, &n)) return rc;
    for (int m = 0; m < f.n_dir; ++m) {
        int rc = 0;
        if ((rc = mc_get(h, f.sT, m, walker, &out->sum_T[m])) || (rc = mc_get(h, f.sJ, m, walker, &out->sum_J[m])) ||
            (rc = mc_get(h, f.sJ2, m, walker, &out->sum_J2[m])))
            return rc;
    }
    out->n_meas = n;
    out->n_dir = f.n_dir;
    return DQMC_OK;
}

int dqmc_qs_get_stiffness_sample(dqmc_qs_handle *h, int32_t walker, int64_t I[8], int64_t K[8])
{
    if (int rc = mc_walker(h, walker, "dqmc_qs_get_stiffness_sample")) return rc;
    if (!I || !K) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_get_stiffness_sample: null output");
    const dqmc_qs_handle::Stiffness &f = h->st;
    for (int c = 0; c < ST_MAX_CLASSES; ++c) I[c] = K[c] = 0;
    if (f.n_dir < 1) return DQMC_OK;
    MCHK(hipSetDevice(h->device));
    for (int c = 0; c < f.n_c; ++c) {
        long long a = 0, b = 0;
        int rc = 0;
        if ((rc = mc_get(h, f.sI, c, walker, &a)) || (rc = mc_get(h, f.sK, c, walker, &b))) return rc;
        I[c] = a;
        K[c] = b;
    }
    return DQMC_OK;
}

int dqmc_qs_stiffness_binner_get_level(dqmc_qs_handle *h, int32_t walker, int32_t level, double *x_sum, double *x2_sum,
                                       double *xy_sum, int64_t *count)
{
    return mc_binner_get_level(h, "dqmc_qs_stiffness_binner_get_level", mc_blob::SEC_STIFFNESS, QS_STIFFNESS_OFF, walker, level,
                               x_sum, x2_sum, xy_sum, count);
}

int dqmc_qs_stiffness_binner_finish(dqmc_qs_handle *h, int32_t walker, int32_t level, dqmc_qs_stiffness_binned *out)
{
    if (int rc = mc_binner_finish(h, "dqmc_qs_stiffness_binner_finish", mc_blob::SEC_STIFFNESS, QS_STIFFNESS_OFF, false, walker,
                                  level, out))
        return rc;
    out->n_dir = h->st.n_dir;
    return DQMC_OK;
}

int dqmc_qs_set_cluster_rate(dqmc_qs_handle *h, int32_t rate)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_qs_set_cluster_rate: null handle");
    if (rate < 0) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_set_cluster_rate: rate must be >= 0");
    if (rate > 0) {
        MCHK(hipSetDevice(h->device));
        if (int rc = qs_reserve_cluster_lds(h, "dqmc_qs_set_cluster_rate")) return rc;
    }
    h->ca.rate = rate;
    return DQMC_OK;
}

int dqmc_qs_cluster_move(dqmc_qs_handle *h, int32_t walker)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_qs_cluster_move: null handle");
    if (walker >= h->W) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_cluster_move: walker out of range");
    MCHK(hipSetDevice(h->device));
    if (int rc = qs_reserve_cluster_lds(h, "dqmc_qs_cluster_move")) return rc;
    const size_t lds = sweep_lds_bytes(h->q, h->Nw) + cluster_lds_bytes(h->N);
    hipLaunchKernelGGL(qs_cluster_move_kernel, dim3(walker >= 0 ? 1 : h->W), dim3(h->threads), lds, h->stream, h->d,
                       (const long long *)h->e_q30, (const int2 *)h->cs_q30, h->ca, (int)walker);
    MCHK(hipGetLastError());
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_qs_get_cluster_stats(dqmc_qs_handle *h, int32_t walker, dqmc_qs_cluster_stats *out)
{
    if (int rc = mc_walker(h, walker, "dqmc_qs_get_cluster_stats")) return rc;
    if (!out) return mc_fail(h, DQMC_ERR_INVALID, "dqmc_qs_get_cluster_stats: null out");
    MCHK(hipSetDevice(h->device));
    long long prop = 0, acc = 0, size = 0;
    unsigned long long m = 0;
    int rc = 0;
    if ((rc = mc_get(h, h->ca.prop, 0, walker, &prop)) || (rc = mc_get(h, h->ca.acc, 0, walker, &acc)) ||
        (rc = mc_get(h, h->ca.sum_size, 0, walker, &size)) || (rc = mc_get(h, h->ca.cursor, 0, walker, &m)))
        return rc;
    out->prop_global = prop;
    out->acc_global = acc;
    out->sum_cluster_size = size;
    out->moves_drawn = m;
    return DQMC_OK;
}

int dqmc_qs_synchronize(dqmc_qs_handle *h)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, "dqmc_qs_synchronize: null handle");
    MCHK(hipSetDevice(h->device));
    MCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

}  // extern "C"

// checkpoint and resume: dqmc_qs_state_size, _export, _import
#include "qs_state.inl"
