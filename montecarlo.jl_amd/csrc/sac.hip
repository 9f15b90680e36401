// sac.hip — the SAC flavor: stochastic analytic continuation (Sandvik, PRB 57, 10287; Beach, cond-mat/0403055; Shao and
// Sandvik, Phys. Rep. 1003) of imaginary-time data, batched over problems and sampling temperatures: the kernels and the
// dqmc_sac_* C ABI.  The reference has nothing of the kind; include/dqmc_hip.h ("the SAC flavor") is the definition, and
// tests/sac_ref.py restates it in numpy.
//
// One workgroup per problem, one wave per replica.  A chain's moves are strictly sequential, and a move is a short
// reduction over the Nt data points: lane l holds res, w and the move's delta for i = l, l + 64, .. (NV = ceil(Nt / 64)
// values, a template parameter, so they are registers), and the sum is the butterfly of the header over the wave.  The
// positions of a workgroup's chains live in LDS as uint16 [R][Nd]; the two table rows of a move come from global memory,
// one contiguous 8 Nt bytes each.  Move d + 1 displaces another delta function than move d, so its rows do not depend on
// move d's outcome: they are requested before move d is decided and waited for after it.  The two uniforms of a move are
// wave-uniform; a block of 32 moves' uniforms is computed by the 64 lanes at once (lane l: move l / 2, t = l & 1) and
// read with v_readlane.
//
// At the end of a sweep: refresh (when due), exchange round (when due), measurement (past thermalisation).  The round
// runs inside the launch: every wave publishes chi2, label and the LDS row of its positions, and leaves res in the
// state array; behind a workgroup barrier both waves of a pair compute the same decision from the same numbers, and on
// a swap each takes the other's row index, chi2, label and res.  A second barrier keeps the next round's publishing behind
// this round's reads.  Barriers occur nowhere else, and every wave of a workgroup runs the same trip counts.
//
// No MFMA, no inline assembly.  Compiled with -ffp-contract=off: the roundings in the header are the ones that run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dqmc_hip.h"
#include "kernels.h"

namespace dqmc_sac {

using dqmc::philox4_uniform;

constexpr int WAVE = 64;
constexpr int MAX_NT = 256, MAX_ND = 4096, MAX_NW = 65535, MAX_R = 16, MAX_WIN = 1 << 24;
constexpr int UBLOCK = 32;  // moves whose uniforms one pass of the wave computes
// a launch runs at most this many moves per chain (the chains of a launch run side by side); dqmc_sac_sweep splits its
// sweeps into launches of at least one sweep each, so that no single kernel holds the GPU for long
constexpr long long LAUNCH_MOVES = 1 << 18;

// what stays with the slot (p, r) besides theta, key, window and the move counter
struct ChainStat {
    double sum, sum2, min, drift;
    long long n_meas, prop, acc, xprop, xacc;
};

struct DevState {
    int P, R, Nt, Nd, Nw;
    const double *g, *w;        // [P][Nt]
    const double *Kt;           // [P][Nw][Nt]
    const double *a;            // [P], norm / Nd
    const double *theta;        // [P R]
    const unsigned long long *key;
    const int *win;
    unsigned long long *m;      // [P R], moves drawn since dqmc_sac_seed
    unsigned short *x;          // [P R][Nd]
    double *res;                // [P R][Nt]
    double *chi2;               // [P R]
    int *label;                 // [P R]
    ChainStat *st;              // [P R]
    unsigned long long *hist;   // [P R][Nw]
};

// LDS of a workgroup: x [R][Nd] uint16, then chi2 [R] double, row [R] int, label [R] int
__host__ __device__ static inline size_t x_bytes(int R, int Nd) { return ((size_t)R * Nd * 2 + 15) / 16 * 16; }
static inline size_t lds_bytes(int R, int Nd) { return x_bytes(R, Nd) + (size_t)R * 16; }
constexpr int MAX_LDS = MAX_R * MAX_ND * 2 + MAX_R * 16;

// what one lane wrote to LDS, every lane of the wave may read afterwards (a wave runs in order; this keeps the compiler
// from moving LDS accesses across it and costs no instruction)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a value every lane holds, as a scalar: what follows from it (addresses, branches, counters) stays out of the VGPRs
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uniform(double v)
{
    return __hiloint2double(uniform(__double2hiint(v)), uniform(__double2loint(v)));
}

__device__ __forceinline__ double lane_value(double v, int src)  // v of lane `src` (wave-uniform)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// p_l <- p_l + p_{l xor off}, off = 32 .. 1: every lane ends with the same sum
__device__ __forceinline__ double butterfly(double p)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, WAVE);
    return p;
}

// res and chi2 of the positions xs[0 .. Nd) from scratch, in the header's order
template <int NV, typename XPtr>
__device__ __forceinline__ double rebuild(const DevState &s, int p, int lane, XPtr xs, double (&res)[NV])
{
    const int Nt = s.Nt;
    const double *__restrict__ Kt = s.Kt + (size_t)p * s.Nw * Nt;
    const double a = s.a[p];
    double S[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) S[v] = 0.0;
    for (int d = 0; d < s.Nd; ++d) {
        const int xo = uniform((int)xs[d]);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int i = lane + WAVE * v;
            if (i < Nt) S[v] = S[v] + Kt[xo * Nt + i];
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int i = lane + WAVE * v;
        double t = 0.0;
        res[v] = 0.0;
        if (i < Nt) {
            res[v] = a * S[v] - s.g[(size_t)p * Nt + i];
            t = (s.w[(size_t)p * Nt + i] * res[v]) * res[v];
        }
        sum = v == 0 ? t : sum + t;
    }
    return uniform(butterfly(sum));
}

// res and chi2 of the chain (p, r), or of every chain of the problem (r < 0: one wave per replica), from x in the state
template <int NV>
__global__ __launch_bounds__(WAVE * MAX_R) void sac_rebuild_kernel(DevState s, int p, int r)
{
    const int lane = threadIdx.x & (WAVE - 1);
    if (r < 0) r = uniform((int)threadIdx.x / WAVE);
    const int c = p * s.R + r;
    double res[NV];
    const double chi2 = rebuild<NV>(s, p, lane, (const unsigned short *)(s.x + (size_t)c * s.Nd), res);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int i = lane + WAVE * v;
        if (i < s.Nt) s.res[(size_t)c * s.Nt + i] = res[v];
    }
    if (lane == 0) s.chi2[c] = chi2;
}

// n sweeps of every chain, global indices first .. first + n - 1; xc = the exchange cursor at the start of the launch
template <int NV>
__global__ __launch_bounds__(WAVE * MAX_R) void sac_sweep_kernel(DevState s, int n, long long first, long long therm,
                                                                 int refresh, int rate, unsigned long long xc)
{
    extern __shared__ __align__(16) unsigned char sac_lds[];
    const int lane = threadIdx.x & (WAVE - 1), r = uniform((int)threadIdx.x / WAVE), p = blockIdx.x;
    const int R = s.R, Nt = s.Nt, Nd = s.Nd, Nw = s.Nw, c = p * R + r;
    unsigned short *xall = (unsigned short *)sac_lds;
    double *xchi = (double *)(sac_lds + x_bytes(R, Nd));
    int *xrow = (int *)(xchi + R), *xlab = xrow + R;
    const double *__restrict__ Kt = s.Kt + (size_t)p * Nw * Nt;

    int row = r;  // the LDS row that holds the positions of the configuration now in this slot
    unsigned short *xs = xall + (size_t)row * Nd;
    for (int d = lane; d < Nd; d += WAVE) xs[d] = s.x[(size_t)c * Nd + d];
    double res[NV], w[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int i = lane + WAVE * v;
        res[v] = i < Nt ? s.res[(size_t)c * Nt + i] : 0.0;
        w[v] = i < Nt ? s.w[(size_t)p * Nt + i] : 0.0;
    }
    const double a = s.a[p], theta = s.theta[c], nwin = (double)(2 * s.win[c] + 1);
    const int win = s.win[c];
    const unsigned long long key = s.key[c];
    unsigned long long m = s.m[c];
    double chi2 = s.chi2[c];
    int label = s.label[c];
    ChainStat st = s.st[c];
    wave_sync();

    for (int k = 0; k < n; ++k) {
        // ---- the sweep: Nd moves, the rows of move d + 1 in flight while move d is decided
        double ublk = 0.0, kn[NV], ko[NV], u1n = 0.0;
        int xnn = 0;
        bool okn = false;
        auto prepare = [&](int d) {
            if (d % UBLOCK == 0) {
                const unsigned long long mm = m + (unsigned long long)(d + (lane >> 1));
                ublk = philox4_uniform(key, (unsigned int)mm, (unsigned int)(mm >> 32), (unsigned int)(lane & 1), 0u);
            }
            const double u0 = lane_value(ublk, 2 * (d % UBLOCK));
            u1n = lane_value(ublk, 2 * (d % UBLOCK) + 1);
            const int xo = uniform((int)xs[d]);
            xnn = xo + uniform((int)floor(u0 * nwin)) - win;
            okn = xnn >= 0 && xnn < Nw;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int i = lane + WAVE * v;
                const bool in = okn && i < Nt;
                kn[v] = in ? Kt[xnn * Nt + i] : 0.0;
                ko[v] = in ? Kt[xo * Nt + i] : 0.0;
            }
        };
        prepare(0);
        for (int d = 0; d < Nd; ++d) {
            double dl[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) dl[v] = a * (kn[v] - ko[v]);
            const int xn = xnn;
            const bool ok = okn;
            const double u1 = u1n;
            if (d + 1 < Nd) prepare(d + 1);
            st.prop += 1;
            if (ok) {
                double sum = 0.0;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const double t = (w[v] * dl[v]) * (2.0 * res[v] + dl[v]);
                    sum = v == 0 ? t : sum + t;
                }
                const double dchi = uniform(butterfly(sum));
                if (dchi <= 0.0 || uniform((int)(u1 < exp(-dchi / (2.0 * theta))))) {
#pragma unroll
                    for (int v = 0; v < NV; ++v) res[v] = res[v] + dl[v];
                    chi2 = chi2 + dchi;
                    if (lane == 0) xs[d] = (unsigned short)xn;
                    st.acc += 1;
                }
            }
            wave_sync();
        }
        m += (unsigned long long)Nd;
        const long long gi = first + k;

        // ---- refresh
        if (refresh > 0 && gi % refresh == 0) {
            const double fresh = rebuild<NV>(s, p, lane, (const unsigned short *)xs, res);
            st.drift = fmax(st.drift, fabs(chi2 - fresh));
            chi2 = fresh;
        }

        // ---- exchange round xc: pairs (q, q + 1), q = xc mod 2
        if (rate > 0 && R >= 2 && gi % rate == 0) {
            const int lo = ((r & 1) == (int)(xc & 1)) ? r : r - 1;  // the lower slot of this wave's pair
            const bool paired = lo >= 0 && lo + 1 < R;
            if (lane == 0) {
                xchi[r] = chi2;
                xrow[r] = row;
                xlab[r] = label;
            }
            if (paired) {
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const int i = lane + WAVE * v;
                    if (i < Nt) s.res[(size_t)c * Nt + i] = res[v];
                }
            }
            __syncthreads();
            if (paired) {
                const int cl = p * R + lo;
                const double q = (1.0 / (2.0 * s.theta[cl]) - 1.0 / (2.0 * s.theta[cl + 1])) * (xchi[lo] - xchi[lo + 1]);
                const bool swap =
                    q >= 0.0 ||
                    uniform((int)(philox4_uniform(s.key[cl], (unsigned int)xc, (unsigned int)(xc >> 32), 0u, 1u) < exp(q)));
                if (r == lo) {
                    st.xprop += 1;
                    st.xacc += swap ? 1 : 0;
                }
                if (swap) {
                    const int o = r == lo ? lo + 1 : lo;  // the partner
                    chi2 = xchi[o];
                    row = xrow[o];
                    label = xlab[o];
                    xs = xall + (size_t)row * Nd;
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const int i = lane + WAVE * v;
                        if (i < Nt) res[v] = s.res[(size_t)(p * R + o) * Nt + i];
                    }
                }
            }
            __syncthreads();
            xc += 1;
        }

        // ---- measurement
        if (gi > therm) {
            for (int d = lane; d < Nd; d += WAVE) atomicAdd(&s.hist[(size_t)c * Nw + xs[d]], 1ull);
            st.sum = st.sum + chi2;
            st.sum2 = st.sum2 + chi2 * chi2;
            st.min = fmin(st.min, chi2);
            st.n_meas += 1;
        }
    }

    // the positions go back in slot order: every row is read by the wave that now owns it
    for (int d = lane; d < Nd; d += WAVE) s.x[(size_t)c * Nd + d] = xs[d];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int i = lane + WAVE * v;
        if (i < Nt) s.res[(size_t)c * Nt + i] = res[v];
    }
    if (lane == 0) {
        s.m[c] = m;
        s.chi2[c] = chi2;
        s.label[c] = label;
        s.st[c] = st;
    }
}

}  // namespace dqmc_sac

using namespace dqmc_sac;

struct dqmc_sac_handle {
    int P = 0, R = 0, Nt = 0, Nd = 0, Nw = 0, device = 0;
    int rate = 0;         // an exchange round after every rate-th sweep, 0: none
    uint64_t cursor = 0;  // rounds since dqmc_sac_set_exchange
    hipStream_t stream = nullptr;
    DevState d{};
    std::vector<void *> allocs;
    std::string err;
};

static thread_local std::string g_sac_create_error;

static int sac_fail(dqmc_sac_handle *h, int code, const std::string &msg)
{
    if (h) h->err = msg;
    else g_sac_create_error = msg;
    return code;
}

#define SCHK(expr)                                                                          \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return sac_fail(h, DQMC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <typename T>
static int sac_alloc(dqmc_sac_handle *h, T **p, size_t count)
{
    void *q = nullptr;
    SCHK(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
    h->allocs.push_back(q);
    SCHK(hipMemsetAsync(q, 0, (count ? count : 1) * sizeof(T), h->stream));
    *p = (T *)q;
    return 0;
}

template <typename T>
static int sac_put(dqmc_sac_handle *h, const T *base, size_t at, const T *v, size_t count)
{
    SCHK(hipMemcpyAsync((void *)(base + at), v, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
    SCHK(hipStreamSynchronize(h->stream));
    return 0;
}

template <typename T>
static int sac_get(dqmc_sac_handle *h, const T *base, size_t at, T *v, size_t count)
{
    SCHK(hipMemcpyAsync(v, base + at, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    SCHK(hipStreamSynchronize(h->stream));
    return 0;
}

static int sac_problem(dqmc_sac_handle *h, int32_t p, const char *fn)
{
    if (!h) return sac_fail(nullptr, DQMC_ERR_INVALID, std::string(fn) + ": null handle");
    if (p < 0 || p >= h->P) return sac_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": problem out of range");
    return 0;
}

static int sac_chain(dqmc_sac_handle *h, int32_t p, int32_t r, const char *fn)
{
    if (int rc = sac_problem(h, p, fn)) return rc;
    if (r < 0 || r >= h->R) return sac_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": replica out of range");
    return 0;
}

static bool sac_theta_ok(double t) { return std::isfinite(t) && t > 0.0; }
static bool sac_window_ok(int32_t w) { return w >= 1 && w <= MAX_WIN; }

// one of the NV forms of a kernel
#define SAC_LAUNCH(kernel, grid, block, lds, ...)                                                       \
    switch ((h->Nt + WAVE - 1) / WAVE) {                                                                \
    case 1: hipLaunchKernelGGL(kernel<1>, grid, block, lds, h->stream, __VA_ARGS__); break;             \
    case 2: hipLaunchKernelGGL(kernel<2>, grid, block, lds, h->stream, __VA_ARGS__); break;             \
    case 3: hipLaunchKernelGGL(kernel<3>, grid, block, lds, h->stream, __VA_ARGS__); break;             \
    default: hipLaunchKernelGGL(kernel<4>, grid, block, lds, h->stream, __VA_ARGS__); break;            \
    }

static int sac_launch_rebuild(dqmc_sac_handle *h, int p, int r)
{
    SAC_LAUNCH(sac_rebuild_kernel, dim3(1), dim3(WAVE * (r < 0 ? h->R : 1)), 0, h->d, p, r);
    SCHK(hipGetLastError());
    SCHK(hipStreamSynchronize(h->stream));
    return 0;
}

static ChainStat sac_clear_sums(ChainStat st)
{
    st.sum = st.sum2 = 0.0;
    st.min = std::numeric_limits<double>::infinity();
    st.n_meas = 0;
    return st;
}

extern "C" {

const char *dqmc_sac_last_error(const dqmc_sac_handle *h) { return h ? h->err.c_str() : g_sac_create_error.c_str(); }

int dqmc_sac_create(const dqmc_sac_params *p, dqmc_sac_handle **out)
{
    if (!p || !out) return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_create: null argument");
    *out = nullptr;
    if (p->n_problems < 1) return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_create: n_problems must be >= 1");
    if (p->n_tau < 1 || p->n_tau > MAX_NT)
        return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_create: n_tau must be in 1..256");
    if (p->n_deltas < 1 || p->n_deltas > MAX_ND)
        return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_create: n_deltas must be in 1..4096");
    if (p->n_omega < 2 || p->n_omega > MAX_NW)
        return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_create: n_omega must be in 2..65535");
    if (p->n_replicas < 1 || p->n_replicas > MAX_R)
        return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_create: n_replicas must be in 1..16");
    if (!sac_window_ok(p->window))
        return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_create: window must be in 1..2^24");
    for (int r = 0; p->theta && r < p->n_replicas; ++r)
        if (!sac_theta_ok(p->theta[r]))
            return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_create: every theta must be finite and > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return sac_fail(nullptr, DQMC_ERR_NO_DEVICE, "dqmc_sac_create: no HIP device visible");
    if (p->device_id < 0 || p->device_id >= ndev)
        return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_create: device_id out of range");

    dqmc_sac_handle *h = new dqmc_sac_handle();
    h->P = p->n_problems;
    h->R = p->n_replicas;
    h->Nt = p->n_tau;
    h->Nd = p->n_deltas;
    h->Nw = p->n_omega;
    h->device = p->device_id;
    auto bail = [&](int rc) {
        g_sac_create_error = h->err;
        dqmc_sac_destroy(h);
        return rc;
    };
    if (hipSetDevice(h->device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(sac_fail(h, DQMC_ERR_HIP, "dqmc_sac_create: cannot open the device"));
    DevState &d = h->d;
    d.P = h->P;
    d.R = h->R;
    d.Nt = h->Nt;
    d.Nd = h->Nd;
    d.Nw = h->Nw;
    const size_t P = h->P, C = P * h->R;
    double *g = nullptr, *w = nullptr, *Kt = nullptr, *a = nullptr, *theta = nullptr;
    unsigned long long *key = nullptr;
    int *win = nullptr;
    int rc = 0;
    if ((rc = sac_alloc(h, &g, P * h->Nt)) || (rc = sac_alloc(h, &w, P * h->Nt)) ||
        (rc = sac_alloc(h, &Kt, P * h->Nw * h->Nt)) || (rc = sac_alloc(h, &a, P)) || (rc = sac_alloc(h, &theta, C)) ||
        (rc = sac_alloc(h, &key, C)) || (rc = sac_alloc(h, &win, C)) || (rc = sac_alloc(h, &d.m, C)) ||
        (rc = sac_alloc(h, &d.x, C * h->Nd)) || (rc = sac_alloc(h, &d.res, C * h->Nt)) ||
        (rc = sac_alloc(h, &d.chi2, C)) || (rc = sac_alloc(h, &d.label, C)) || (rc = sac_alloc(h, &d.st, C)) ||
        (rc = sac_alloc(h, &d.hist, C * h->Nw)))
        return bail(rc);
    d.g = g;
    d.w = w;
    d.Kt = Kt;
    d.a = a;
    d.theta = theta;
    d.key = key;
    d.win = win;
    std::vector<double> th(C);
    std::vector<int> wn(C, p->window), lab(C);
    std::vector<ChainStat> st(C, sac_clear_sums(ChainStat{}));
    for (size_t c = 0; c < C; ++c) {
        th[c] = p->theta ? p->theta[c % h->R] : 1.0;
        lab[c] = (int)(c % h->R);
    }
    if (hipMemcpyAsync(theta, th.data(), C * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(win, wn.data(), C * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(d.label, lab.data(), C * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(d.st, st.data(), C * sizeof(ChainStat), hipMemcpyHostToDevice, h->stream) != hipSuccess)
        return bail(sac_fail(h, DQMC_ERR_HIP, "dqmc_sac_create: state upload failed"));
    // the positions of a workgroup's chains in LDS above the 64 KiB default
    const void *kernels[] = {(const void *)sac_sweep_kernel<1>, (const void *)sac_sweep_kernel<2>,
                             (const void *)sac_sweep_kernel<3>, (const void *)sac_sweep_kernel<4>};
    for (const void *k : kernels)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS) != hipSuccess)
            return bail(sac_fail(h, DQMC_ERR_HIP, "dqmc_sac_create: cannot reserve LDS for the positions"));
    if (hipStreamSynchronize(h->stream) != hipSuccess)
        return bail(sac_fail(h, DQMC_ERR_HIP, "dqmc_sac_create: device initialisation failed"));
    *out = h;
    return DQMC_OK;
}

int dqmc_sac_destroy(dqmc_sac_handle *h)
{
    if (!h) return DQMC_OK;
    if (h->stream) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
    }
    for (void *p : h->allocs) (void)hipFree(p);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return DQMC_OK;
}

int dqmc_sac_set_problem(dqmc_sac_handle *h, int32_t p, const double *g, const double *w, const double *Kt, double norm)
{
    if (int rc = sac_problem(h, p, "dqmc_sac_set_problem")) return rc;
    if (!g || !w || !Kt) return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_set_problem: null argument");
    if (!std::isfinite(norm) || norm <= 0.0)
        return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_set_problem: norm must be finite and > 0");
    for (int i = 0; i < h->Nt; ++i)
        if (!std::isfinite(g[i]) || !std::isfinite(w[i]) || w[i] < 0.0)
            return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_set_problem: g finite, w finite and >= 0");
    for (size_t i = 0; i < (size_t)h->Nw * h->Nt; ++i)
        if (!std::isfinite(Kt[i])) return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_set_problem: Kt must be finite");
    SCHK(hipSetDevice(h->device));
    const double a = norm / (double)h->Nd;
    int rc = 0;
    if ((rc = sac_put(h, h->d.g, (size_t)p * h->Nt, g, (size_t)h->Nt)) ||
        (rc = sac_put(h, h->d.w, (size_t)p * h->Nt, w, (size_t)h->Nt)) ||
        (rc = sac_put(h, h->d.Kt, (size_t)p * h->Nw * h->Nt, Kt, (size_t)h->Nw * h->Nt)) ||
        (rc = sac_put(h, h->d.a, (size_t)p, &a, (size_t)1)))
        return rc;
    return sac_launch_rebuild(h, p, -1);
}

int dqmc_sac_set_theta(dqmc_sac_handle *h, int32_t p, const double *theta)
{
    if (int rc = sac_problem(h, p, "dqmc_sac_set_theta")) return rc;
    if (!theta) return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_set_theta: null argument");
    for (int r = 0; r < h->R; ++r)
        if (!sac_theta_ok(theta[r]))
            return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_set_theta: every theta must be finite and > 0");
    SCHK(hipSetDevice(h->device));
    return sac_put(h, h->d.theta, (size_t)p * h->R, theta, (size_t)h->R);
}

int dqmc_sac_seed(dqmc_sac_handle *h, int32_t p, int32_t r, uint64_t seed)
{
    if (int rc = sac_chain(h, p, r, "dqmc_sac_seed")) return rc;
    SCHK(hipSetDevice(h->device));
    const unsigned long long key = seed, zero = 0;
    if (int rc = sac_put(h, h->d.key, (size_t)p * h->R + r, &key, (size_t)1)) return rc;
    return sac_put<unsigned long long>(h, h->d.m, (size_t)p * h->R + r, &zero, (size_t)1);
}

int dqmc_sac_set_conf(dqmc_sac_handle *h, int32_t p, int32_t r, const uint16_t *x)
{
    if (int rc = sac_chain(h, p, r, "dqmc_sac_set_conf")) return rc;
    if (!x) return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_set_conf: null argument");
    for (int d = 0; d < h->Nd; ++d)
        if (x[d] >= h->Nw) return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_set_conf: position outside the grid");
    SCHK(hipSetDevice(h->device));
    if (int rc = sac_put<unsigned short>(h, h->d.x, ((size_t)p * h->R + r) * h->Nd, x, (size_t)h->Nd)) return rc;
    return sac_launch_rebuild(h, p, r);
}

int dqmc_sac_get_conf(dqmc_sac_handle *h, int32_t p, int32_t r, uint16_t *x)
{
    if (int rc = sac_chain(h, p, r, "dqmc_sac_get_conf")) return rc;
    if (!x) return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_get_conf: null argument");
    SCHK(hipSetDevice(h->device));
    return sac_get<unsigned short>(h, h->d.x, ((size_t)p * h->R + r) * h->Nd, x, (size_t)h->Nd);
}

int dqmc_sac_set_window(dqmc_sac_handle *h, int32_t p, int32_t r, int32_t win)
{
    if (int rc = sac_chain(h, p, r, "dqmc_sac_set_window")) return rc;
    if (!sac_window_ok(win)) return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_set_window: window must be in 1..2^24");
    SCHK(hipSetDevice(h->device));
    const int v = win;
    return sac_put(h, h->d.win, (size_t)p * h->R + r, &v, (size_t)1);
}

int dqmc_sac_set_exchange(dqmc_sac_handle *h, int32_t rate)
{
    if (!h) return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_set_exchange: null handle");
    if (rate < 0) return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_set_exchange: rate must be >= 0");
    SCHK(hipSetDevice(h->device));
    const size_t C = (size_t)h->P * h->R;
    std::vector<ChainStat> st(C);
    std::vector<int> lab(C);
    if (int rc = sac_get(h, h->d.st, 0, st.data(), C)) return rc;
    for (size_t c = 0; c < C; ++c) {
        st[c].xprop = st[c].xacc = 0;
        lab[c] = (int)(c % h->R);
    }
    if (int rc = sac_put(h, h->d.st, 0, st.data(), C)) return rc;
    if (int rc = sac_put(h, h->d.label, 0, lab.data(), C)) return rc;
    h->rate = rate;
    h->cursor = 0;
    return DQMC_OK;
}

int dqmc_sac_sweep(dqmc_sac_handle *h, int32_t n_sweeps, int64_t first_sweep_index, int64_t thermalization,
                   int32_t refresh)
{
    if (!h) return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_sweep: null handle");
    if (n_sweeps < 0 || first_sweep_index < 1 || refresh < 0)
        return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_sweep: n_sweeps >= 0, first_sweep_index >= 1, refresh >= 0");
    SCHK(hipSetDevice(h->device));
    const int chunk = (int)std::max<long long>(1, LAUNCH_MOVES / h->Nd);
    const int k = h->R >= 2 ? h->rate : 0;
    for (int done = 0; done < n_sweeps;) {
        const int n = std::min(chunk, n_sweeps - done);
        const long long first = first_sweep_index + done, last = first + n - 1;
        SAC_LAUNCH(sac_sweep_kernel, dim3(h->P), dim3(WAVE * h->R), lds_bytes(h->R, h->Nd), h->d, n, first,
                   (long long)thermalization, (int)refresh, k, (unsigned long long)h->cursor);
        SCHK(hipGetLastError());
        if (k > 0) h->cursor += (uint64_t)(last / k - (first - 1) / k);  // the rounds the launch ran
        done += n;
    }
    SCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

int dqmc_sac_get_stats(dqmc_sac_handle *h, int32_t p, int32_t r, dqmc_sac_stats *out)
{
    if (int rc = sac_chain(h, p, r, "dqmc_sac_get_stats")) return rc;
    if (!out) return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_get_stats: null out");
    SCHK(hipSetDevice(h->device));
    const size_t c = (size_t)p * h->R + r;
    ChainStat st;
    unsigned long long m = 0;
    int label = 0, win = 0;
    int rc = 0;
    if ((rc = sac_get(h, h->d.st, c, &st, (size_t)1)) || (rc = sac_get(h, h->d.chi2, c, &out->chi2, (size_t)1)) ||
        (rc = sac_get<unsigned long long>(h, h->d.m, c, &m, (size_t)1)) ||
        (rc = sac_get<int>(h, h->d.label, c, &label, (size_t)1)) || (rc = sac_get(h, h->d.win, c, &win, (size_t)1)))
        return rc;
    out->sum_chi2 = st.sum;
    out->sum_chi2_sq = st.sum2;
    out->min_chi2 = st.min;
    out->max_drift = st.drift;
    out->n_meas = st.n_meas;
    out->prop = st.prop;
    out->acc = st.acc;
    out->prop_exchange = st.xprop;
    out->acc_exchange = st.xacc;
    out->replica = label;
    out->moves_drawn = m;
    out->rounds = h->cursor;
    out->window = win;
    return DQMC_OK;
}

int dqmc_sac_get_histogram(dqmc_sac_handle *h, int32_t p, int32_t r, uint64_t *hist)
{
    if (int rc = sac_chain(h, p, r, "dqmc_sac_get_histogram")) return rc;
    if (!hist) return sac_fail(h, DQMC_ERR_INVALID, "dqmc_sac_get_histogram: null argument");
    SCHK(hipSetDevice(h->device));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "histogram entries are 64 bits");
    return sac_get<unsigned long long>(h, h->d.hist, ((size_t)p * h->R + r) * h->Nw, (unsigned long long *)hist,
                                       (size_t)h->Nw);
}

int dqmc_sac_reset_accumulators(dqmc_sac_handle *h)
{
    if (!h) return sac_fail(nullptr, DQMC_ERR_INVALID, "dqmc_sac_reset_accumulators: null handle");
    SCHK(hipSetDevice(h->device));
    const size_t C = (size_t)h->P * h->R;
    std::vector<ChainStat> st(C);
    if (int rc = sac_get(h, h->d.st, 0, st.data(), C)) return rc;
    for (ChainStat &s : st) s = sac_clear_sums(s);
    if (int rc = sac_put(h, h->d.st, 0, st.data(), C)) return rc;
    SCHK(hipMemsetAsync(h->d.hist, 0, C * h->Nw * sizeof(unsigned long long), h->stream));
    SCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}

}  // extern "C"
