// engine.cpp — host side of libdqmc_hip.so: device state of a batch of walkers, the
// propagate state machine of src/flavors/DQMC/stack.jl:502-631 expressed as batched
// kernel launches on one HIP stream, and the C ABI of include/dqmc_hip.h.
//
// All walkers of a handle move in lockstep (same current_slice / direction), so the
// control flow lives on the host and is identical to the reference's; the data of all
// walkers is processed by every launch (grid = units x tiles).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dqmc_hip.h"
#include "hopping_forms.h"
#include "kernels.h"
#include "state_blob.h"
#include <rccl/rccl.h>

using namespace dqmc;
static_assert(HOP_BILAYER_FB == BILAYER_FB, "the table and bilayer.hip agree on the block behind ay");

struct dqmc_comm {
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0, device = 0;
};

static thread_local std::string g_create_error;

struct UTStack;  // unequal-time stack (unequal_time.inl)

struct dqmc_handle {
    dqmc_params p{};
    int n = 0, nb = 1, N = 0, M = 0, s = 0, K = 0, W = 0, units = 0;
    long nn = 0;
    double lambda = 0, epl = 0, eml = 0;
    SweepConsts sc{};
    hipStream_t stream = nullptr;
    KernelSwitches sw;  // read once, when the handle is set up (read_kernel_switches)
    // constants (nb x n x n)
    double *eT = nullptr, *eTinv = nullptr, *eT2 = nullptr, *eTinv2 = nullptr;
    double *eT2T = nullptr;  // transposed copy of eT2: A operand of the daggered slice products in slab.hip
    bool slab = false;       // n == 256 dense path: slice chains and wraps as slab-resident launches
    // the factored form of the hopping exponentials, if they have one (hopping_forms.h: the table, the operand layouts),
    // and the device image of its factors: slice chains and wraps then take the form's kernel instead of slab.hip / the GEMMs
    HopForm form = HopForm::None;
    double *kron_f = nullptr;
    int8_t *conf = nullptr;  // W x (N x M)
    // stack (slot-major): u/t: (K+1) x units x n^2 ; d: (K+1) x units x n
    double *u_stack = nullptr, *t_stack = nullptr, *d_stack = nullptr;
    // slot i of the UDT stack = (su[i], sd[i], st[i]); entry K + 1 is a spare: a slot is rewritten by building the new
    // factors in the spare and swapping the pointers, so the old content stays readable (no load_slot copies)
    std::vector<double *> su, sd, st;
    double *Ul = nullptr, *Ur = nullptr, *Tl = nullptr, *Tr = nullptr, *greens = nullptr, *greens_temp = nullptr;
    double *tmp1 = nullptr, *tmp2 = nullptr, *bufA = nullptr, *bufB = nullptr;
    // scratch of one UDT (udt_AVX_pivot!): V (Householder vectors; hand-over buffer of the two-phase QR before that),
    // W (factored matrix of the cooperative QR, then the compact-WY product), S (V'V), tau, pivot, and what the
    // triangular solves need (winv: inverted 16 x 16 diagonal blocks; ts: n > 256, panel-solved copy of the right-hand
    // side).
    struct QrSet {
        double *V = nullptr, *W = nullptr, *S = nullptr, *tau = nullptr, *winv = nullptr, *ts = nullptr;
        int *pivot = nullptr;
    } qs;
    double *Dl = nullptr, *Dr = nullptr;
    double *greens_alt = nullptr, *lu_img = nullptr;  // decide / apply sweep (sweep_lu.hip)
    bool sweep_fused = true;
    int cus = 0;  // compute units of the device: what the admission rules of the co-resident launch forms count against
    // the last chunk of the latest sweep_spatial, eliminated but not applied to greens (fold_wrap_flush): the next factored
    // wrap of greens applies it, materialize_pending_flush() everywhere else
    struct PendingFlush {
        const double *G = nullptr;  // = greens while pending
        const double *img = nullptr;
        int site0 = 0;
    } pf;
    // the factored wrap in one launch (kron.hip: kron_wrap_kernel): arrival words per unit, never cleared (wrap_launches
    // counts the launches on them); wrap_blocks[pending]: co-resident workgroups of the two forms, 0 = two launches
    unsigned *wrap_cnt = nullptr;
    unsigned wrap_launches = 0;
    int wrap_blocks[2] = {0, 0};
    WalkerRng *rng = nullptr;
    DevStats *stats = nullptr;
    unsigned long long *pc_scratch = nullptr;  // prop_check_kernel: partial maximum + arrival counter per walker
    std::vector<double *> uniforms;  // per walker device arrays
    // The accumulators, one entry per DQMC_RED_* section: the only list of them.  An entry is filled where the section's
    // layout is (re)built (sec_layout: dqmc_create, dqmc_set_pair_directions, dqmc_set_local_targets, ut_sus_layout,
    // td_setup / td_free); the reset, the packed reduction, the binners and the size / get / export entry points read it.
    // A regular entry: acc = [n - 1 sums][sample count], all of it packed (n_red = n), and the binner sees the n - 1
    // sums of one walker's sample (bin_E), which the measurement kernels leave in per_walker.  The irregular ones:
    //   Green's          acc = [G][G.^2][occupation][count]; the binner takes [G][occupation] (bin_E = nb n^2 + nb n)
    //                    from the true G of every unit itself (BIN_SRC_GREENS): no per_walker
    //   correlations     per_walker holds the 4 n_dirs pair sums only, the binner takes the magnetisations from G (BIN_SRC_CORR)
    //   time-displaced   n = E + 1, but the count is not packed (n_red = E): the passes that feed it feed the
    //                    susceptibilities, whose reduced count dqmc_get_reduced hands out with the section
    struct Section {
        double *acc = nullptr, *per_walker = nullptr;
        size_t n = 0, n_red = 0;  // doubles the local getter reports (0: not configured) / that go into the reduction
        long bin_E = 0;
        int bin_mode = BIN_SRC_PLAIN;
    //   sign             [sum of s per DQMC_RED_* section above], no count; packed only while sign weighting is on
    //   thermodynamics   behind the sign section: acc = [10 sums][sum of s][count], its own sum of signs inside; per_walker
    //                    [W][11], read with stride 10, or 11 with sign weighting on (the sample then ends with s_w); its
    //                    binner (DQMC_BIN_THERMODYNAMICS) is sized by hand like a momentum binner (thermo.inl)
    } sec[DQMC_RED_THERMODYNAMICS + 1];
    // correlation measurements (EachSitePairByDistance tables set by the host)
    int n_dirs = 0;
    int *dir_ptr = nullptr, *pair_src = nullptr, *pair_trg = nullptr;
    int K_loc = 0;                  // EachLocalQuadByDistance{K}
    int *trg_of = nullptr;          // [K][n]
    int K_cc = 0;                   // EachLocalQuadBySyncedDistance{K} (current_current_susceptibility)
    std::vector<int> cc_trg_h;      // [K][n]
    std::vector<double> cc_T;       // mc.s.hopping_matrix, nb blocks n x n
    CCPlan cc;
    int current_slice = 0, direction = 0;
    bool prepared = false;
    long long conf_version = 0;     // bumped whenever the HS field changes (mc.last_sweep's role for the UT stack)
    UTStack *ut = nullptr;
    std::string err;
    // timing
    bool timing = false;
    struct Ev { hipEvent_t a, b; int fam; };
    std::vector<Ev> pending;
    std::vector<hipEvent_t> pool;
    double fam_ms[DQMC_K_COUNT] = {0};
    long long fam_n[DQMC_K_COUNT] = {0};
    std::vector<void *> allocs;
    QrCoopWorkspace qr_ws;
    int qrb_sites = 0;  // call sites of udt_AVX_pivot! that take the one-launch blocked form (DQMC_QRB_SITES)
    // checkerboard products with sparse bond-group factors (cb.hip); the dense constants above stay valid
    struct {
        bool on = false;
        int kmax = 0, n_mats = 0;
        double *vals = nullptr, *mu = nullptr, *mu_inv = nullptr;
        int *cols = nullptr;
        int seq[7][32];
        int len[7] = {0, 0, 0, 0, 0, 0, 0};
    } cb;
    // measurement reduction (dqmc_reduce): packed device buffer [sums | maxima | minima]
    double *red_buf = nullptr;
    size_t red_cap = 0;
    dqmc_stats red_stats{};
    bool red_valid = false;
    size_t red_sizes[DQMC_RED_THERMODYNAMICS + 1] = {0, 0, 0, 0, 0, 0, 0};  // packed section sizes of the LAST reduction (dqmc_get_reduced checks against these)
    bool red_td_ok = false;  // the time-displaced and susceptibility sample counts agreed when that reduction was packed
    // logarithmic binners (binner.inl), one per DQMC_BIN_* section: xs, x2 [L][W][E], c [L - 1][W][E], out = finish scratch
    struct Binner {
        bool on = false;
        int E = 0, L = 0;
        int64_t cap = 0, T = 0;  // capacity and pushes so far: count[level] = T >> level for every element
        double *xs = nullptr, *x2 = nullptr, *c = nullptr, *out = nullptr;
    } bin[DQMC_BIN_RESPONSE_END];  // (DQMC_BIN_SIGN + k: the signs pushed with section k = a DQMC_RED_* index; then the momentum binners, the thermodynamics one and the response binners)
    // momentum-space observables (momentum.inl, momentum.hip): n_q == 0: off, nothing allocated.  cos_d / sin_d
    // [n_dirs x n_q] on the device, the host copies for the checkpoint; sample[k]: the per-walker momentum sample
    // [W][E] of binner DQMC_BIN_MOMENTUM_CORRELATIONS + k, allocated with the binner
    struct Momenta {
        int n_q = 0;
        double *cos_d = nullptr, *sin_d = nullptr;
        std::vector<double> cos_h, sin_h;
        double *sample[DQMC_BIN_MOMENTUM_END - DQMC_BIN_MOMENTUM_CORRELATIONS] = {nullptr, nullptr, nullptr};
    } mom;
    // pair channels and the response binners (response.inl, response.hip): n_ch == 0: channels off.  F_d [K_loc^2 x n_ch]
    // on the device, F_h the host copy for the checkpoint; Z [W][n_ch][n_dirs]: the contracted pairing sample, allocated
    // while a pairing response binner is on; sample[k]: [W][E] of binner DQMC_BIN_RESPONSE_PAIRING + k
    struct Response {
        int n_ch = 0;
        double *F_d = nullptr, *Z = nullptr;
        std::vector<double> F_h;
        double *sample[DQMC_BIN_RESPONSE_END - DQMC_BIN_RESPONSE_PAIRING] = {nullptr, nullptr, nullptr};
    } rsp;
    // scalar thermodynamics (thermo.inl, thermo.hip): on == false: off, nothing allocated.  The hopping matrix of
    // dqmc_set_thermodynamics as a neighbour list: the off-diagonal non-zeros of row i of block b at row_ptr[b n + i] ..
    // of col / val, the diagonal in diag; T_hash: FNV-1a 64 of the matrix as it was handed in (the checkpoint compares it)
    struct Thermo {
        bool on = false;
        int *row_ptr = nullptr, *col = nullptr;
        double *val = nullptr, *diag = nullptr;
        double U_s = 0.0;
        uint64_t T_hash = 0;
    } th;
    // Renyi-2 entanglement from walker pairs (entangle.inl, entangle.hip): n_sub == 0: off, nothing allocated.  Not a
    // section: the sums [n_sub][W][W] and the sample count live here.  sub_ptr / sites: the site lists (host copies
    // beside them); img: the compact G_A images, subsystem s at img_off[s]; lad / sg [n_sub][pairs][nb]: log|det| and
    // sign of every pair's M_b; sample: the last sample; fail: pairs whose sample was set to 0
    struct Entangle {
        int n_sub = 0;
        std::vector<int> sub_ptr_h, sites_h;
        std::vector<long> off_h;
        int *sub_ptr = nullptr, *sites = nullptr, *sg = nullptr;
        long *img_off = nullptr;
        double *img = nullptr, *lad = nullptr, *sample = nullptr, *sums = nullptr;
        unsigned long long *fail = nullptr;
        long long count = 0;
    } ent;
    // current response in imaginary time (current_tau.inl, current_tau.hip): every == 0: off, nothing allocated.  Not a
    // section either.  K / n_q: K_cc and the momenta it was set with (the setters of both turn it off); tab
    // [n_dirs][n_q][2]: cos and sin of dqmc_set_momenta, q fastest; x [W][K][n_dirs]: one slice's own ccs sums; kb
    // [W][K]: the pass's bond kinetic energies; sums [W][P]: the per-walker sums over calls
    struct CurrentTau {
        int every = 0, R = 0, K = 0, n_q = 0;
        size_t P = 0;
        double *tab = nullptr, *x = nullptr, *kb = nullptr, *sums = nullptr;
    } ctd;
    // time-displaced recording (unequal_time.inl, tdm.hip): every == 0: off, nothing allocated.  The sample (bin_E doubles
    // per walker in the layout of include/dqmc_hip.h) and the sums are sec[DQMC_RED_TIME_DISPLACED]; src_of [n_dirs][n]
    // only with the fast form
    struct TimeDisplaced {
        int every = 0, what = 0, R = 0;
        bool fast = false;
        bool inj = false;  // the injective form (tdm_greens_inj_kernel): src_of has holes and n_dirs rows per column
        int *src_of = nullptr;
    } td;
    // tau-tau' covariance accumulators (taucov.inl, taucov.hip): bin_size == 0: off, nothing allocated.  Not sections.
    // tcov follows the momentum time-displaced sample (what: mask of DQMC_TD_*; sample [W][sample_E]: its own copy of that
    // sample while the momentum binner is off), ucov the caller's samples.  a, c, s1 [W][S][R], s2 [W][S][R][R]; open:
    // samples in the unfinished bin, nb: closed bins (every walker's: they close together)
    struct TauCov {
        int bin_size = 0, what = 0, R = 0;
        long S = 0, sample_E = 0;
        int64_t open = 0, nb = 0;
        double *a = nullptr, *c = nullptr, *s1 = nullptr, *s2 = nullptr, *sample = nullptr;
    } tcov, ucov;
    // global moves (global_move.inl): per-walker device state, logabsdet / sign per unit of the current field [0] (valid
    // while gm_cache_version == conf_version) and of a proposal [1]; rate / kind of the hook in the update (0 = off)
    GlobalMoveState *gm = nullptr;
    double *gm_lad[2] = {nullptr, nullptr};
    int *gm_sg[2] = {nullptr, nullptr};
    long long gm_cache_version = -1;
    int gm_rate = 0, gm_kind = DQMC_GLOBAL_FLIP_SITE;
    long long gm_updates = 0;  // updates since dqmc_prepare: update u belongs to sweep 1 + u / (2 slices)
    // sign reweighting (global_move.inl, sign.hip): off by default.  sign_sw [W + 2]: s_w of the measurement point in
    // hand as doubles, their sum, the walkers kept (sign_begin writes it in front of every signed sum); sign_fail [W]:
    // samples left out per walker because a unit's sign came out 0
    bool sign_on = false;
    double *sign_sw = nullptr;
    long long *sign_fail = nullptr;
};

// ---------------------------------------------------------------------------
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            h->err = std::string(#expr) + ": " + hipGetErrorString(e_);                                \
            return DQMC_ERR_HIP;                                                                       \
        }                                                                                              \
    } while (0)
#define CHK(expr)                \
    do {                         \
        int rc_ = (expr);        \
        if (rc_ != 0) return rc_; \
    } while (0)

static int fail(dqmc_handle *h, int code, const std::string &msg)
{
    if (h) h->err = msg;
    else g_create_error = msg;
    return code;
}

template <typename T>
static int dalloc(dqmc_handle *h, T **p, size_t count, bool zero = true)
{
    void *q = nullptr;
    HIPCHK(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
    h->allocs.push_back(q);
    if (zero) HIPCHK(hipMemsetAsync(q, 0, (count ? count : 1) * sizeof(T), h->stream));
    *p = (T *)q;
    return 0;
}
// gives a block of dalloc back ahead of dqmc_destroy and nulls the pointer; the stream must be idle
template <typename T>
static void dfree(dqmc_handle *h, T **p)
{
    if (!*p) return;
    auto it = std::find(h->allocs.begin(), h->allocs.end(), (void *)*p);
    if (it != h->allocs.end()) h->allocs.erase(it);
    (void)hipFree((void *)*p);
    *p = nullptr;
}
// (re)builds the layout of section `which` (dqmc_handle::Section; n == 0: not configured): the old buffers go back, the
// new ones start at zero.  `samples`: doubles per walker of per_walker.  The stream must be idle.
static int sec_layout(dqmc_handle *h, int which, size_t n, size_t n_red, long bin_E, size_t samples, int bin_mode = BIN_SRC_PLAIN)
{
    dqmc_handle::Section &s = h->sec[which];
    dfree(h, &s.acc);
    dfree(h, &s.per_walker);
    s = dqmc_handle::Section{};
    // the sum of signs that went with the old sums goes with them
    if (which < DQMC_RED_SIGN && h->sec[DQMC_RED_SIGN].acc)
        HIPCHK(hipMemsetAsync(h->sec[DQMC_RED_SIGN].acc + which, 0, sizeof(double), h->stream));
    if (!n) return 0;
    CHK(dalloc(h, &s.acc, n));
    if (samples) CHK(dalloc(h, &s.per_walker, (size_t)h->W * samples));
    s.n = n; s.n_red = n_red; s.bin_E = bin_E; s.bin_mode = bin_mode;
    return 0;
}

// ---- timing scopes ---------------------------------------------------------
static int timing_drain(dqmc_handle *h)
{
    if (h->pending.empty()) return 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    for (auto &e : h->pending) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
        h->fam_ms[e.fam] += ms;
        h->fam_n[e.fam] += 1;
        h->pool.push_back(e.a);
        h->pool.push_back(e.b);
    }
    h->pending.clear();
    return 0;
}
static hipEvent_t event_get(dqmc_handle *h)  // from the pool of drained events, or a new one
{
    hipEvent_t e;
    if (!h->pool.empty()) { e = h->pool.back(); h->pool.pop_back(); }
    else (void)hipEventCreate(&e);
    return e;
}
struct Timed {
    dqmc_handle *h;
    int fam;
    hipEvent_t a = nullptr, b = nullptr;
    Timed(dqmc_handle *h_, int fam_) : h(h_), fam(fam_)
    {
        if (!h->timing) return;
        a = event_get(h);
        b = event_get(h);
        (void)hipEventRecord(a, h->stream);
    }
    ~Timed()
    {
        if (!h->timing) return;
        (void)hipEventRecord(b, h->stream);
        h->pending.push_back({a, b, fam});
        if (h->pending.size() >= 2048) (void)timing_drain(h);
    }
};

// ---- argument builders -------------------------------------------------------
static GemmArgs gemm_base(dqmc_handle *h, MatRef A, int tA, MatRef B, int tB, double *C)
{
    GemmArgs g{};
    g.M = g.N = g.K = h->n;
    g.n_units = h->units;
    g.nb = h->nb;
    g.A = A;
    g.B = B;
    g.C = C;
    g.strideC = h->nn;
    g.ldc = h->n;
    g.transA = tA;
    g.transB = tB;
    g.kscale = g.colscale = g.rowscale = g.adddiag = vs_none();
    g.row_first = 0;
    g.alpha = 1.0;
    g.ident = 0.0;
    g.beta = 0;
    g.tri = 0;
    return g;
}
static MatRef U_(dqmc_handle *h, const double *p) { return mat(p, h->nn, h->n); }        // per unit
static MatRef C_(dqmc_handle *h, const double *p) { return mat(p, 0, h->n, h->nn); }     // shared constant, per block
// a pair of events for a dispatch-attached (kernel-only) timing, or nulls when timing is off
static void timing_events(dqmc_handle *h, hipEvent_t *a, hipEvent_t *b)
{
    *a = *b = nullptr;
    if (!h->timing) return;
    *a = event_get(h);
    *b = event_get(h);
}
static int timing_push(dqmc_handle *h, hipEvent_t a, hipEvent_t b, int fam)
{
    if (!a) return 0;
    h->pending.push_back({a, b, fam});
    if (h->pending.size() >= 2048) return timing_drain(h);
    return 0;
}
static int run_gemm(dqmc_handle *h, const GemmArgs &g)
{
    // kernel-only duration: the events are attached to the dispatch itself (no launch gap inside)
    hipEvent_t a, b;
    timing_events(h, &a, &b);
    HIPCHK(launch_gemm(g, h->stream, a, b));
    return timing_push(h, a, b, DQMC_K_GEMM);
}
// exp(sign*lambda*conf[:,slice]) for block 0, exp(-sign*lambda*conf) for block 1
// (HubbardModelAttractive.jl:100-110, HubbardModelRepulsive.jl:113-126); slice 1-based
static VecSrc vs_conf(dqmc_handle *h, int slice, int sign)
{
    VecSrc v{};
    v.mode = 2;
    v.conf = h->conf + (long)(slice - 1) * h->N;
    v.conf_stride = (long)h->N * h->M;
    const double a = sign > 0 ? h->epl : h->eml, b = sign > 0 ? h->eml : h->epl;
    v.cpos[0] = a; v.cneg[0] = b;
    v.cpos[1] = b; v.cneg[1] = a;
    return v;
}
static double *uslot(dqmc_handle *h, int i) { return h->su[i]; }
static double *tslot(dqmc_handle *h, int i) { return h->st[i]; }
static double *dslot(dqmc_handle *h, int i) { return h->sd[i]; }
struct Udt { const double *u, *d, *t; };
static Udt slot_ref(dqmc_handle *h, int i) { return Udt{h->su[i], h->sd[i], h->st[i]}; }
static void slot_swap_spare(dqmc_handle *h, int i)
{
    const int sp = h->K + 1;
    std::swap(h->su[i], h->su[sp]); std::swap(h->sd[i], h->sd[sp]); std::swap(h->st[i], h->st[sp]);
}

static int copy_mat(dqmc_handle *h, double *dst, const double *src)
{
    Timed t(h, DQMC_K_MISC);
    HIPCHK(hipMemcpyAsync(dst, src, sizeof(double) * h->units * h->nn, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}
static int copy_vec(dqmc_handle *h, double *dst, const double *src)
{
    Timed t(h, DQMC_K_MISC);
    HIPCHK(hipMemcpyAsync(dst, src, sizeof(double) * h->units * h->n, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}
static int set_identity(dqmc_handle *h, double *A)
{
    Timed t(h, DQMC_K_MISC);
    HIPCHK(launch_set_identity(h->n, h->units, A, h->nn, h->stream));
    return 0;
}
static int set_ones(dqmc_handle *h, double *d)
{
    Timed t(h, DQMC_K_MISC);
    HIPCHK(launch_fill(d, (size_t)h->units * h->n, 1.0, h->stream));
    return 0;
}

// The kernel-selection and test switches, read from the environment once per handle / stand-alone
// primitive call: nothing else reads them (the launchers get them from the handle)
static void read_kernel_switches(dqmc_handle *h)
{
    KernelSwitches &k = h->sw;
    k.qr_noblocked = getenv("DQMC_QR_NOBLOCKED") != nullptr;
    if (const char *e = getenv("DQMC_QRB_SITES")) k.qrb_sites = atoi(e) & 7;
    if (const char *e = getenv("DQMC_QR_TAIL")) k.qr_tail = atoi(e) != 0;
    k.qr_sc1 = getenv("DQMC_QR_SC1") != nullptr;
    k.qr_nocoop = getenv("DQMC_QR_NOCOOP") != nullptr;
    if (const char *e = getenv("DQMC_QR_FORCE_TIMEOUT"))
        k.qr_force_timeout = strncmp(e, "step:", 5) == 0 ? 2 + atoi(e + 5) : (strncmp(e, "extra:", 6) == 0 ? 1000 + atoi(e + 6) : 1);
    k.qr_nopanel = getenv("DQMC_QR_NOPANEL") != nullptr;
    k.trsm_simple = getenv("DQMC_TRSM_SIMPLE") != nullptr;
    k.sweep_split = getenv("DQMC_SWEEP_SPLIT") != nullptr;
    k.flush_ncp2 = getenv("DQMC_FLUSH_NCP2") != nullptr;
    k.no_slab = getenv("DQMC_NO_SLAB") != nullptr;
    k.no_kron = getenv("DQMC_NO_KRON") != nullptr;
    k.no_wrap_flush = getenv("DQMC_NO_WRAP_FLUSH") != nullptr;
    k.wrap_two_launch = getenv("DQMC_WRAP_TWO_LAUNCH") != nullptr;
    k.tdm_general = getenv("DQMC_TDM_GENERAL") != nullptr;
}

// units in whole groups of eight: the XCD block maps launch workgroups for the padded units too, and they take CUs
static int padded_units(const dqmc_handle *h) { return (h->units + 7) / 8 * 8; }
// the one-launch UDT (qrb.hip): eight workgroups per unit, all of them co-resident
static bool udt_blocked_fits(const dqmc_handle *h, int per_cu) { return per_cu >= 1 && padded_units(h) * 8 <= h->cus * per_cu; }
// the fused chunk loop of the site sweep: one elimination workgroup per walker beside the flush workgroups, one per CU
static bool sweep_fused_fits(const dqmc_handle *h)
{
    const int ncp = (h->n % 256 == 0) ? 2 : 1, nt = (h->n % 128 == 0) ? 8 : 4;
    const int flush_blocks = padded_units(h) * (h->n / 64) * (h->n / (16 * nt * ncp));
    return h->W + flush_blocks <= h->cus;
}

static int alloc_qr_workspace(dqmc_handle *h)
{
    // device-side error word (bit 1: a hand-off inside the sweep elimination kernel timed out; bit 0 is no longer set by
    // anything: a cooperative-QR time-out is not an error since round 2, the guarded kernel behind the launch redoes
    // the factorisation and dqmc_qr_fallbacks counts it)
    CHK(dalloc(h, &h->qr_ws.errflag, (size_t)1));
    h->qr_ws.tail = h->sw.qr_tail;
    h->qr_ws.force_sc1 = h->sw.qr_sc1;
    h->qr_ws.no_coop = h->sw.qr_nocoop;
    h->qr_ws.no_panel = h->sw.qr_nopanel;
    h->qr_ws.force_timeout = h->sw.qr_force_timeout;
    if (h->n > 256) return 0;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, h->p.device_id));
    h->cus = prop.multiProcessorCount;
    const size_t slots = (size_t)((h->units + 7) / 8) * 8 * QR_COOP_SLOTS_PER_UNIT;
    CHK(dalloc(h, &h->qr_ws.mailbox, slots * QR_COOP_SLOT));
    CHK(dalloc(h, &h->qr_ws.fb, (size_t)2));
    // co-residency: what the occupancy API reports for the kernel on this device (its ~200 VGPRs admit 2 per CU)
    h->qr_ws.max_blocks = h->cus * qr_coop_blocks_per_cu();
    h->qr_ws.epoch = 0;
    // pre-pivoted blocked UDT in one launch (qrb.hip): n == 256, all eight workgroups of every unit co-resident.
    // DQMC_QR_NOBLOCKED: off; DQMC_QRB_SITES: bit mask of the call sites that use it (1 = slice-sequence builds and every other
    // caller, 2 = first, 4 = second factorisation of calculate_greens_AVX!)
    h->qrb_sites = 0;
    if (h->n == 256 && !h->sw.qr_noblocked) {
        const int per_cu = qrb_blocks_per_cu();
        if (udt_blocked_fits(h, per_cu)) {
            CHK(dalloc(h, (char **)&h->qr_ws.mailbox2, qrb_mailbox_bytes(h->units)));
            h->qr_ws.blk_max_blocks = h->cus * per_cu;
            h->qrb_sites = h->sw.qrb_sites;
        }
    }
    return 0;
}
// The factored wrap in one launch (kron.hip: kron_wrap_kernel): its workgroups wait for each other, so a handle takes it
// only where the occupancy API says that the whole grid is resident at once on this device, for the form with the pending
// chunk (two workgroups per CU by its LDS) and the one without separately.  DQMC_WRAP_TWO_LAUNCH: never.
// The words are allocated if either form fits and wrap_greens_kron asks again per form, so a handle whose grid fits only
// without the chunk mixes one- and two-launch wraps (the same bits either way).  The occupancy figure knows nothing of
// another handle, stream or process on the device: that case is what the bounded poll and the error bit are for.
static int alloc_wrap_handoff(dqmc_handle *h)
{
    if (!hop_row(h->form).one_launch_wrap || h->sw.wrap_two_launch) return 0;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, h->p.device_id));
    h->cus = prop.multiProcessorCount;
    for (int pf = 0; pf < 2; ++pf) h->wrap_blocks[pf] = h->cus * kron_wrap_blocks_per_cu(pf != 0);
    if (kron_wrap_grid(h->units) > std::max(h->wrap_blocks[0], h->wrap_blocks[1])) return 0;
    return dalloc(h, &h->wrap_cnt, (size_t)kron_wrap_grid(h->units) / 16 * KR_CNT_STRIDE);
}
// whether wrap_greens_kron takes the one-launch form, with / without a pending chunk
static bool wrap_one_launch(const dqmc_handle *h, bool pending)
{
    return h->wrap_cnt && hop_row(h->form).one_launch_wrap && kron_wrap_grid(h->units) <= h->wrap_blocks[pending ? 1 : 0];
}
static int check_qr_workspace(dqmc_handle *h)
{
    if (!h->qr_ws.errflag) return 0;
    int e = 0;
    HIPCHK(hipMemcpy(&e, h->qr_ws.errflag, sizeof(int), hipMemcpyDeviceToHost));
    if (e) {  // reported once: the flag is cleared, the data of the failed call is not trustworthy
        HIPCHK(hipMemset(h->qr_ws.errflag, 0, sizeof(int)));
        if (e & 32)
            return fail(h, DQMC_ERR_HIP, "factored wrap (one launch): the hand-off between the workgroups of a unit timed out (is the "
                                         "grid co-resident?  results of this call are invalid; DQMC_WRAP_TWO_LAUNCH=1 selects the "
                                         "two-launch form, which has no hand-off)");
        if (e & 16)
            return fail(h, DQMC_ERR_HIP, "blocked UDT: a hand-off between the workgroups of a matrix timed out (results of this call "
                                         "are invalid; DQMC_QR_NOBLOCKED=1 selects the kernels without that requirement)");
        return fail(h, DQMC_ERR_HIP, (e & 8) ? "site sweep (one launch per slice): a hand-over between workgroups timed out - the grid was "
                                               "not co-resident (results of this call are invalid; the default launch-per-chunk form has no "
                                               "such requirement)"
                                             : "sweep elimination: hand-off timed out (results of this call are invalid)");
    }
    return 0;
}

// ---- UDT (udt_AVX_pivot!, src/linalg/UDT.jl:192-306) ---------------------------
// A is factored (in place, or into q.W by the cooperative kernel).  Q is formed in compact-WY form with GEMMs instead
// of the reference's reflector-by-reflector back accumulation (UDT.jl:250-266):
//   Q = H_1...H_n = I - V S^-1 V',  S = striu(V'V) + diag(1/tau)
// udt_factor: "QR decomposition" loop + D, T (and V for the second half); udt_formq: U = Q from V, tau of the set.
typedef dqmc_handle::QrSet QrSet;
static int udt_factor(dqmc_handle *h, double *A, double *Dout, double *Tout, int apply, QrSet &q)
{
    const int n = h->n;
    const double *F = A;  // where the factored matrix ends up (q.W behind the cooperative QR)
    {
        Timed t(h, DQMC_K_QR);
        // q.V is free until udt_finish writes V: it serves as the hand-over buffer of the two-phase QR
        HIPCHK(launch_qr_pivot(n, h->units, A, h->nn, q.tau, q.pivot, &h->qr_ws, q.W, h->nn, &F, h->stream, q.V, h->nn));
    }
    {
        Timed t(h, DQMC_K_MISC);
        HIPCHK(launch_udt_finish(n, h->units, A, h->nn, F, h->nn, q.pivot, Dout, n, q.V, h->nn, Tout, h->nn, apply,
                                 h->stream));
    }
    return 0;
}
static int udt_formq(dqmc_handle *h, double *Uout, QrSet &q)
{
    const int n = h->n;
    GemmArgs g = gemm_base(h, U_(h, q.V), 1, U_(h, q.V), 0, q.S);
    g.tri = (n % 64 == 0) ? 1 : 0;  // V is unit lower triangular: a third of the k range on average
    CHK(run_gemm(h, g));
    {
        Timed t(h, DQMC_K_TRSM);
        HIPCHK(launch_trsm_right_upper(n, h->units, q.V, h->nn, q.S, h->nn, nullptr, q.tau, n, q.W, h->nn, q.winv, h->sw, h->stream, q.ts));
    }
    g = gemm_base(h, U_(h, q.W), 0, U_(h, q.V), 1, Uout);
    g.alpha = -1.0;
    g.ident = 1.0;
    g.tri = (n % 64 == 0) ? 2 : 0;
    CHK(run_gemm(h, g));
    return 0;
}
// n == 256: the whole of udt_AVX_pivot! in one launch, pivot order fixed up front (qrb.hip).  site: see DQMC_QRB_SITES
static bool udt_is_fused(const dqmc_handle *h, int site) { return (h->qrb_sites >> site) & 1; }
// B != null: Uout = B Q (Uout must not be B)
static int udt_fused(dqmc_handle *h, const double *A, double *Uout, double *Dout, double *Tout, int apply, QrSet &q,
                     const double *B = nullptr)
{
    Timed t(h, DQMC_K_QR);
    HIPCHK(launch_udt_blocked(h->units, A, h->nn, Uout, h->nn, Dout, h->n, Tout, h->nn, q.pivot, &h->qr_ws, apply, h->stream, B,
                              h->nn));
    return 0;
}
static int udt(dqmc_handle *h, double *A, double *Uout, double *Dout, double *Tout, int apply)
{
    if (udt_is_fused(h, 0) && Tout && Tout != A) return udt_fused(h, A, Uout, Dout, Tout, apply, h->qs);
    CHK(udt_factor(h, A, Dout, Tout, apply, h->qs));
    return udt_formq(h, Uout, h->qs);
}
// Out = A[:, pivot of set q] / triu(T) (rdivp!, general.jl:138-166)
static int rdivp_set(dqmc_handle *h, const double *A, const double *T, double *Out, const QrSet &q)
{
    Timed t(h, DQMC_K_TRSM);
    HIPCHK(launch_trsm_right_upper(h->n, h->units, A, h->nn, T, h->nn, q.pivot, nullptr, 0, Out, h->nn, q.winv, h->sw, h->stream, q.ts));
    return 0;
}
static int rdivp(dqmc_handle *h, double *A, const double *T)
{
    return rdivp_set(h, A, T, A, h->qs);
}

// ---- calculate_greens_AVX! (stack.jl:337-393) -----------------------------------
// L = (Ul, Dl, Tl), R = (Ur, Dr, Tr) are only read (they may be stack slots); h->Ul .. h->Tr are the work matrices
// the reference overwrites its six inputs with.  L / R may also BE those work matrices (each is consumed before the
// step that overwrites it).
// a2_copy (optional): receives the matrix handed to the second UDT (:368-376), whose determinant is that of G^-1 up to
// a sign (logdet.hip); the D of that UDT is what the function leaves in h->Dr.
static int calculate_greens_src(dqmc_handle *h, double *out, Udt L, Udt R, double *a2_copy = nullptr)
{
    const int n = h->n;
    QrSet &q = h->qs;
    GemmArgs g = gemm_base(h, U_(h, L.t), 0, U_(h, R.t), 1, out);  // :346-348
    g.colscale = vs_arr(R.d, n);
    g.rowscale = vs_arr(L.d, n);
    CHK(run_gemm(h, g));
    if (udt_is_fused(h, 1)) {
        // :349 and :360 in one launch: T out of place (q.W), and the kernel carries Ul' through the reflectors instead of the
        // identity, so that its "U" is Tl = Ul Q already (Q itself is not used again: :362 overwrites Tr)
        if (L.u == h->Tl) return fail(h, DQMC_ERR_STATE, "calculate_greens: Ul aliases Tl");
        CHK(udt_fused(h, out, h->Tl, h->Dr, q.W, 0, q, L.u));
        CHK(rdivp_set(h, R.u, q.W, h->Ur, q));                             // :361
    } else {
        CHK(udt_factor(h, out, h->Dr, nullptr, 0, q));                     // :349, first half
        CHK(rdivp_set(h, R.u, out, h->Ur, q));                             // :361 (out of place: Ur = R.u[:, p] / T)
        CHK(udt_formq(h, h->Tr, q));                                       // :349, second half
        CHK(run_gemm(h, gemm_base(h, U_(h, L.u), 0, U_(h, h->Tr), 0, h->Tl)));    // :360
    }
    g = gemm_base(h, U_(h, h->Tl), 1, U_(h, h->Ur), 0, h->Tr);         // :362 + :368
    g.adddiag = vs_arr(h->Dr, n);
    CHK(run_gemm(h, g));
    if (a2_copy) CHK(copy_mat(h, a2_copy, h->Tr));
    const double *tlul = h->Tr;  // where Tl Ul of :378 ends up
    if (udt_is_fused(h, 2)) {
        // :376 and :378 in one launch: "U" = Tl Q goes to Ul (free: the reference's Ul = Q is only used in :378)
        CHK(udt_fused(h, h->Tr, h->Ul, h->Dr, q.W, 0, q, h->Tl));
        CHK(rdivp_set(h, h->Ur, q.W, h->Ur, q));                           // :377
        tlul = h->Ul;
    } else {
        CHK(udt_factor(h, h->Tr, h->Dr, nullptr, 0, q));                   // :376
        CHK(rdivp_set(h, h->Ur, h->Tr, h->Ur, q));                         // :377
        CHK(udt_formq(h, h->Ul, q));
        CHK(run_gemm(h, gemm_base(h, U_(h, h->Tl), 0, U_(h, h->Ul), 0, h->Tr)));  // :378
    }
    g = gemm_base(h, U_(h, h->Ur), 0, U_(h, tlul), 1, out);            // :382-391
    g.kscale = vs_inv(h->Dr, n);
    CHK(run_gemm(h, g));
    return 0;
}
static int calculate_greens(dqmc_handle *h, double *out, double *a2_copy = nullptr)
{
    return calculate_greens_src(h, out, Udt{h->Ul, h->Dl, h->Tl}, Udt{h->Ur, h->Dr, h->Tr}, a2_copy);
}

// ---- checkerboard products with sparse factors (slice_matrices.jl:104-222, DQMC.jl:731-750) --------------------
enum { CB_LEFT_B = 0, CB_LEFT_BINV = 1, CB_LEFT_BDAG = 2, CB_RIGHT_B = 3, CB_RIGHT_BINV = 4, CB_RIGHT_ET = 5,
       CB_LEFT_ETINV = 6 };
static int cb_mult(dqmc_handle *h, int which, int slice, const double *X, double *O, const double *qscale)
{
    CbArgs a{};
    a.n = h->n; a.nb = h->nb; a.kmax = h->cb.kmax;
    a.side = (which == CB_RIGHT_B || which == CB_RIGHT_BINV || which == CB_RIGHT_ET) ? 1 : 0;
    a.seq_len = h->cb.len[which];
    for (int i = 0; i < a.seq_len; ++i) a.seq[i] = h->cb.seq[which][i];
    a.vals = h->cb.vals; a.cols = h->cb.cols;
    a.X = X; a.O = O; a.strideX = h->nn;
    a.conf = slice >= 1 ? h->conf + (long)(slice - 1) * h->N : nullptr;
    a.conf_stride = (long)h->N * h->M;
    a.epl = h->epl; a.eml = h->eml;
    switch (which) {
    case CB_LEFT_B: a.pre_conf = +1; a.pre_vec = h->cb.mu; break;
    case CB_LEFT_BINV: a.post_conf = -1; a.post_vec = h->cb.mu_inv; break;
    case CB_LEFT_BDAG: a.post_conf = +1; a.post_vec = h->cb.mu; break;
    case CB_RIGHT_B: a.post_conf = +1; a.post_vec = h->cb.mu; break;
    case CB_RIGHT_BINV: a.pre_conf = -1; a.pre_vec = h->cb.mu_inv; break;
    default: break;
    }
    a.qscale = qscale; a.qstride = h->n;
    hipEvent_t ea, eb;
    timing_events(h, &ea, &eb);
    HIPCHK(launch_cb_apply(a, h->units, h->stream, ea, eb));
    return timing_push(h, ea, eb, DQMC_K_GEMM);
}

// ---- slab-resident product chains (slab.hip) -----------------------------------------
static SlabArgs slab_base(dqmc_handle *h, const double *X0, long x_su, long x_sb, double *out)
{
    SlabArgs a{};
    a.n_units = h->units; a.nb = h->nb; a.nsteps = 0;
    a.X0 = X0; a.x_su = x_su; a.x_sb = x_sb;
    a.out = out; a.out_su = h->nn;
    a.conf_stride = (long)h->N * h->M;
    a.epl = h->epl; a.eml = h->eml;
    return a;
}
static void slab_step_const(dqmc_handle *h, SlabArgs &a, const double *C)  // shared constant, per block
{
    SlabStep &st = a.st[a.nsteps++];
    st = SlabStep{};
    st.A = C; st.su = 0; st.sb = h->nn;
}
static void slab_step_unit(dqmc_handle *h, SlabArgs &a, const double *A)
{
    SlabStep &st = a.st[a.nsteps++];
    st = SlabStep{};
    st.A = A; st.su = h->nn; st.sb = 0;
}
static int run_slab(dqmc_handle *h, const SlabArgs &a)
{
    hipEvent_t ea, eb;
    timing_events(h, &ea, &eb);
    HIPCHK(launch_slab_chain(a, h->stream, ea, eb));
    return timing_push(h, ea, eb, DQMC_K_GEMM);
}

// ---- the same with Kronecker-factored hopping exponentials (kron.hip) -------------
enum { KF_ET2 = 0, KF_ETINV2 = 1, KF_ET2T = 2, KF_ETINV2T = 3 };
static bool use_kron(const dqmc_handle *h) { return h->form != HopForm::None && !h->cb.on; }
// wraps out of place (wrap_greens_slab): the n = 256 slab path and every factored path
static bool oop_wrap(const dqmc_handle *h) { return (h->slab || h->form != HopForm::None) && !h->cb.on; }
// the last chunk of sweep_spatial goes into the first launch of the next wrap (kron.hip) instead of a flush of its own.
// Only with the fused chunk loop (few units: one round of workgroups): every one of the 16 workgroups of a unit reads all of
// C (128 KB) and the image, so the folded launch grows with the units, and at 512 units (config 4) the multi-pass flush it
// replaces is cheaper
static bool fold_wrap_flush(const dqmc_handle *h)
{
    // (a form without a pending-chunk kernel: the stand-alone flush applies the last chunk)
    return use_kron(h) && hop_row(h->form).pending_chunk && h->sweep_fused && !h->sw.no_wrap_flush;
}
// greens as the reference has it: a pending last chunk is applied by the stand-alone flush (out of place through
// greens_alt, which is free between two sweep_spatial calls)
static int materialize_pending_flush(dqmc_handle *h)
{
    if (!h->pf.G) return 0;
    const dqmc_handle::PendingFlush p = h->pf;
    h->pf = dqmc_handle::PendingFlush{};
    if (p.G != h->greens) return fail(h, DQMC_ERR_STATE, "pending sweep update does not belong to greens");
    hipEvent_t a, b;
    timing_events(h, &a, &b);
    HIPCHK(launch_sweep_flush_lu(h->n, h->units, h->greens, h->greens_alt, h->nn, p.site0, 64, p.img, h->sw, h->stream, a, b));
    CHK(timing_push(h, a, b, DQMC_K_FLUSH));
    std::swap(h->greens, h->greens_alt);
    return 0;
}
// greens is about to be recomputed from the UDT stack: a pending chunk need not be applied to it (its HS-field flips are
// in conf already, and the stack is built from conf alone)
static void discard_pending_flush(dqmc_handle *h) { h->pf = dqmc_handle::PendingFlush{}; }
static KronArgs kron_base(dqmc_handle *h, const double *X0, double *out)
{
    KronArgs a{};
    a.n_units = h->units; a.nb = h->nb; a.nsteps = 0;
    a.X0 = X0; a.x_su = h->nn;
    a.out = out; a.out_su = h->nn;
    a.conf_stride = (long)h->N * h->M;
    a.epl = h->epl; a.eml = h->eml;
    return a;
}
static KronStep &kron_step(dqmc_handle *h, KronArgs &a, int which)
{
    KronStep &st = a.st[a.nsteps++];
    st = KronStep{};
    const HopFormRow &row = hop_row(h->form);
    st.ax = h->kron_f + (size_t)which * h->nb * (row.fa + row.fb);
    st.ay = st.ax + (size_t)h->nb * row.fa;
    return st;
}
// the chain launcher of every form, in the order of HopForm (None: run_kron is not reached without a form)
static hipError_t (*const KRON_LAUNCHERS[])(const KronArgs &, hipStream_t, hipEvent_t, hipEvent_t) = {
    nullptr, launch_kron_chain, launch_rect_chain, launch_kron3_chain, launch_bilayer_chain, launch_tri_chain, launch_ttp_chain};
static int run_kron(dqmc_handle *h, const KronArgs &a)
{
    hipEvent_t ea, eb;
    timing_events(h, &ea, &eb);
    HIPCHK(KRON_LAUNCHERS[(int)h->form](a, h->stream, ea, eb));
    return timing_push(h, ea, eb, DQMC_K_GEMM);
}

// ---- slice sequences (stack.jl:272-311, slice_matrices.jl:42-76) -------------------
// The s products of a stack interval only need the HS field of slices that sweep_spatial has already left behind, in
// the order the sweep visits them (up pass: B_l X for l = (idx-1)s+1 .. idx s; down pass: B_l' X for l = idx s ..
// (idx-1)s+1).
static const int8_t *conf_slice(dqmc_handle *h, int slice) { return h->conf + (long)(slice - 1) * h->N; }
static void chain_steps(dqmc_handle *h, SlabArgs &a, int dir, int idx, int t0, int t1)  // products t0 .. t1 - 1
{
    for (int t = t0; t < t1; ++t) {
        SlabStep &st = a.st[a.nsteps];
        if (dir == 1) {
            slab_step_const(h, a, h->eT2);
            st.pre_conf = conf_slice(h, (idx - 1) * h->s + 1 + t);
            st.pre_sign = +1;
        } else {  // B_l' X = eV (eT2' X)
            slab_step_const(h, a, h->eT2T);
            st.post_conf = conf_slice(h, idx * h->s - t);
            st.post_sign = +1;
        }
    }
}
static int wrap_greens_slab(dqmc_handle *h, const double *src, double *dst, int curr_slice, int direction);
// dir = +1: add_slice_sequence_left(idx), reads slot idx - 1, writes slot idx; dir = -1: add_slice_sequence_right(idx),
// reads slot idx, writes slot idx - 1 (idx 1-based as in the reference).  wrap_temp: the up pass's wrap of the old
// Green's function for the propagation check (stack.jl:534-536).
static int add_slice_sequence(dqmc_handle *h, int dir, int idx, bool wrap_temp)
{
    const int src = dir == 1 ? idx - 1 : idx, dst = dir == 1 ? idx : idx - 1;
    const int t0 = 0;
    const double *X = uslot(h, src);
    if (wrap_temp) {
        if (oop_wrap(h)) CHK(wrap_greens_slab(h, h->greens, h->greens_temp, h->current_slice - 1, 1));
    }
    double *out = nullptr;
    if (use_kron(h) && h->s <= SLAB_MAX_STEPS) {  // the same launch with the factored eT2 (kron.hip)
        out = h->bufA;
        KronArgs a = kron_base(h, X, out);
        for (int t = 0; t < h->s; ++t) {
            if (dir == 1) {
                KronStep &st = kron_step(h, a, KF_ET2);
                st.pre_conf = conf_slice(h, (idx - 1) * h->s + 1 + t);
                st.pre_sign = +1;
            } else {  // B_l' X = eV (eT2' X)
                KronStep &st = kron_step(h, a, KF_ET2T);
                st.post_conf = conf_slice(h, idx * h->s - t);
                st.post_sign = +1;
            }
        }
        a.col_d = dslot(h, src); a.col_stride = h->n;  // stack.jl:281 / :305
        CHK(run_kron(h, a));
    }
    else if (h->slab && !h->cb.on && h->s <= SLAB_MAX_STEPS) {  // the (remaining) products in one launch
        out = h->bufA;
        SlabArgs a = slab_base(h, X, h->nn, 0, out);
        chain_steps(h, a, dir, idx, t0, h->s);
        a.col_d = dslot(h, src); a.col_stride = h->n;  // stack.jl:281 / :305
        CHK(run_slab(h, a));
    }
    else for (int t = 0; t < h->s; ++t) {
        const int slice = dir == 1 ? (idx - 1) * h->s + 1 + t : idx * h->s - t;
        out = (t & 1) ? h->bufB : h->bufA;
        if (h->cb.on) {
            CHK(cb_mult(h, dir == 1 ? CB_LEFT_B : CB_LEFT_BDAG, slice, X, out, t == h->s - 1 ? dslot(h, src) : nullptr));
            X = out;
            continue;
        }
        GemmArgs g = gemm_base(h, C_(h, h->eT2), dir == 1 ? 0 : 1, U_(h, X), 0, out);  // (eT2*eV)' = eV*eT2'
        if (dir == 1) g.kscale = vs_conf(h, slice, +1);
        else { g.rowscale = vs_conf(h, slice, +1); g.row_first = 1; }
        if (t == h->s - 1) g.colscale = vs_arr(dslot(h, src), h->n);
        CHK(run_gemm(h, g));
        X = out;
    }
    // new factors into the spare, then slot dst <-> spare: the old slot dst stays readable
    const int sp = h->K + 1;
    if (udt_is_fused(h, 0)) {
        CHK(udt_fused(h, out, uslot(h, sp), dslot(h, sp), h->tmp2, 1, h->qs));
    } else {
        CHK(udt_factor(h, out, dslot(h, sp), h->tmp2, 1, h->qs));
        CHK(udt_formq(h, uslot(h, sp), h->qs));
    }
    CHK(run_gemm(h, gemm_base(h, U_(h, h->tmp2), 0, U_(h, tslot(h, src)), 0, tslot(h, sp))));
    slot_swap_spare(h, dst);
    return 0;
}
static int add_slice_sequence_left(dqmc_handle *h, int idx, bool wrap_temp = false) { return add_slice_sequence(h, +1, idx, wrap_temp); }
static int add_slice_sequence_right(dqmc_handle *h, int idx) { return add_slice_sequence(h, -1, idx, false); }

// wrap_greens! (stack.jl:491-500), out of place, one launch: column slab c of the result is
//   +1:  eT2 (eV (G (eV^-1 eTinv2[:, c])))          -1:  eV^-1 (eTinv2 (G eT2[:, c])) eV[c]
// Factored form (kron.hip): two one-step chains through bufB, each storing its result transposed, so that the right
// product becomes a left product with the transposed factors:
//   +1:  P = eT2 (eV G)           -> bufB = P'        dst = (eTinv2' (eV^-1 P'))'  = P eV^-1 eTinv2
//   -1:  P = eV^-1 (eTinv2 G)     -> bufB = P'        dst = (eV (eT2' P'))'        = P eT2 eV
// On a form with the one-launch wrap (hopping_forms.h) both run in one launch with a hand-off per unit (kron_wrap_kernel) when its whole grid is
// co-resident by the occupancy API (alloc_wrap_handoff); otherwise, and under DQMC_WRAP_TWO_LAUNCH, as two launches.
static int wrap_greens_kron(dqmc_handle *h, const double *src, double *dst, int curr_slice, int direction)
{
    const int8_t *c = conf_slice(h, direction == -1 ? curr_slice - 1 : curr_slice);
    KronArgs a = kron_base(h, src, h->bufB);
    a.transpose_out = 1;
    if (h->pf.G) {  // the sweep's last chunk is applied to the columns of src as the first launch loads them
        if (h->pf.G != src || !hop_row(h->form).pending_chunk) return fail(h, DQMC_ERR_STATE, "wrap of another matrix with a sweep update pending");
        a.pf_img = h->pf.img; a.pf_img_su = (long)sweep_lu_image_doubles(); a.pf_site0 = h->pf.site0;
        h->pf = dqmc_handle::PendingFlush{};
    }
    KronStep &s1 = kron_step(h, a, direction == -1 ? KF_ETINV2 : KF_ET2);
    if (direction == -1) { s1.post_conf = c; s1.post_sign = -1; }
    else { s1.pre_conf = c; s1.pre_sign = +1; }
    if (wrap_one_launch(h, a.pf_img != nullptr)) {
        KronStep &s2 = kron_step(h, a, direction == -1 ? KF_ET2T : KF_ETINV2T);
        if (direction == -1) { s2.post_conf = c; s2.post_sign = +1; }
        else { s2.pre_conf = c; s2.pre_sign = -1; }
        a.wrap_out = dst;
        a.wrap_cnt = h->wrap_cnt;
        a.wrap_target = 16u * (h->wrap_launches + 1);
        a.errflag = h->qr_ws.errflag;
        hipEvent_t ea, eb;
        timing_events(h, &ea, &eb);
        HIPCHK(launch_kron_wrap(a, h->stream, ea, eb));
        ++h->wrap_launches;  // (only a launch that went out adds to the arrival words)
        return timing_push(h, ea, eb, DQMC_K_GEMM);
    }
    CHK(run_kron(h, a));
    KronArgs b = kron_base(h, h->bufB, dst);
    b.transpose_out = 1;
    KronStep &s2 = kron_step(h, b, direction == -1 ? KF_ET2T : KF_ETINV2T);
    if (direction == -1) { s2.post_conf = c; s2.post_sign = +1; }
    else { s2.pre_conf = c; s2.pre_sign = -1; }
    return run_kron(h, b);
}
static int wrap_greens_slab(dqmc_handle *h, const double *src, double *dst, int curr_slice, int direction)
{
    if (use_kron(h)) return wrap_greens_kron(h, src, dst, curr_slice, direction);
    if (direction == -1) {
        const int8_t *c = conf_slice(h, curr_slice - 1);
        SlabArgs a = slab_base(h, h->eT2, 0, h->nn, dst);
        slab_step_unit(h, a, src);
        slab_step_const(h, a, h->eTinv2);
        a.st[1].post_conf = c; a.st[1].post_sign = -1;
        a.col_conf = c; a.col_sign = +1;
        return run_slab(h, a);
    }
    const int8_t *c = conf_slice(h, curr_slice);
    SlabArgs a = slab_base(h, h->eTinv2, 0, h->nn, dst);
    slab_step_unit(h, a, src);
    a.st[0].pre_conf = c; a.st[0].pre_sign = -1;
    slab_step_const(h, a, h->eT2);
    a.st[1].pre_conf = c; a.st[1].pre_sign = +1;
    return run_slab(h, a);
}
static int wrap_greens_inplace(dqmc_handle *h, double *gf, int curr_slice, int direction);
// *gf <- wrapped *gf (the slab path writes into tmp1 and exchanges the two pointers)
static int wrap_greens(dqmc_handle *h, double **gf, int curr_slice, int direction)
{
    if (oop_wrap(h)) {
        CHK(wrap_greens_slab(h, *gf, h->tmp1, curr_slice, direction));
        std::swap(*gf, h->tmp1);
        return 0;
    }
    return wrap_greens_inplace(h, *gf, curr_slice, direction);
}
static int wrap_greens_inplace(dqmc_handle *h, double *gf, int curr_slice, int direction)
{
    if (h->cb.on) {  // both products in place, slab by slab
        const int l = direction == -1 ? curr_slice - 1 : curr_slice;
        CHK(cb_mult(h, direction == -1 ? CB_LEFT_BINV : CB_LEFT_B, l, gf, gf, nullptr));
        CHK(cb_mult(h, direction == -1 ? CB_RIGHT_B : CB_RIGHT_BINV, l, gf, gf, nullptr));
        return 0;
    }
    if (direction == -1) {
        const int l = curr_slice - 1;
        GemmArgs g = gemm_base(h, C_(h, h->eTinv2), 0, U_(h, gf), 0, h->tmp1);  // (eV^-1 eTinv2) * G
        g.rowscale = vs_conf(h, l, -1);
        CHK(run_gemm(h, g));
        g = gemm_base(h, U_(h, h->tmp1), 0, C_(h, h->eT2), 0, gf);              // . * (eT2 eV)
        g.colscale = vs_conf(h, l, +1);
        CHK(run_gemm(h, g));
    } else {
        const int l = curr_slice;
        GemmArgs g = gemm_base(h, C_(h, h->eT2), 0, U_(h, gf), 0, h->tmp1);     // (eT2 eV) * G
        g.kscale = vs_conf(h, l, +1);
        CHK(run_gemm(h, g));
        g = gemm_base(h, U_(h, h->tmp1), 0, C_(h, h->eTinv2), 0, gf);           // . * (eV^-1 eTinv2)
        g.kscale = vs_conf(h, l, -1);
        CHK(run_gemm(h, g));
    }
    return 0;
}

// identity factors in slot `slot`; the old content stays readable in the spare
static int reset_slot(dqmc_handle *h, int slot)
{
    const int sp = h->K + 1;
    CHK(set_identity(h, uslot(h, sp)));
    CHK(set_ones(h, dslot(h, sp)));
    CHK(set_identity(h, tslot(h, sp)));
    slot_swap_spare(h, slot);
    return 0;
}
static int prop_check(dqmc_handle *h)
{
    Timed t(h, DQMC_K_MISC);
    HIPCHK(launch_prop_check(h->n, h->nb, h->W, h->greens_temp, h->greens, h->nn, h->stats, h->pc_scratch, h->stream));
    return 0;
}

// stack.jl:108-159 (the parts with observable effect)
static int init_stack(dqmc_handle *h)
{
    CHK(set_identity(h, h->Ul)); CHK(set_identity(h, h->Ur));
    CHK(set_identity(h, h->Tl)); CHK(set_identity(h, h->Tr));
    CHK(set_ones(h, h->Dl)); CHK(set_ones(h, h->Dr));
    h->current_slice = 0;
    h->direction = 0;
    return 0;
}
// stack.jl:242-255
static int build_stack(dqmc_handle *h)
{
    CHK(reset_slot(h, 0));
    for (int i = 1; i <= h->K; ++i) CHK(add_slice_sequence_left(h, i));
    h->current_slice = h->M + 1;
    h->direction = -1;
    return 0;
}

// stack.jl:502-631
// A sweep update pending on greens (fold_wrap_flush) is taken by the wraps of greens: the plain steps and, at the up
// pass's interval boundaries with the propagation check on, the wrap into greens_temp.  Where greens is recomputed from
// the stack it is dropped (discard_pending_flush), where the old greens is compared it is applied first.
static int propagate(dqmc_handle *h)
{
    const int M = h->M, s = h->s;
    if (h->direction == 1) {
        if (h->current_slice % s == 0) {
            h->current_slice += 1;
            if (h->current_slice == 1) {
                const Udt R = slot_ref(h, 0);   // copyto!(s.Ur, s.u_stack[1]) ... (stack.jl:512-520) without the copies
                CHK(reset_slot(h, 0));
                discard_pending_flush(h);
                CHK(calculate_greens_src(h, h->greens, slot_ref(h, 0), R));
            } else if (1 < h->current_slice && h->current_slice <= M) {
                const int idx = (h->current_slice - 1) / s;
                const Udt R = slot_ref(h, idx);
                // stack.jl:534-536 wraps greens_temp unconditionally; its result is only observable through the
                // check, so the wrap is skipped when the check is off.  (Slab form: out of place, in front of the
                // slice sequence.)
                const bool wt = h->p.check_propagation_error != 0, wt_slab = wt && oop_wrap(h);
                CHK(add_slice_sequence_left(h, idx, wt_slab));  // (wt_slab: its wrap takes a pending update)
                const Udt L = slot_ref(h, idx);
                if (wt && !wt_slab) {
                    CHK(materialize_pending_flush(h));
                    CHK(copy_mat(h, h->greens_temp, h->greens));
                    CHK(wrap_greens(h, &h->greens_temp, h->current_slice - 1, 1));
                }
                if (wt_slab) {
                    // the wrap reads mc.s.greens: the new Green's function goes to the other buffer of the pair
                    // (greens_alt, free between two sweep_spatial calls) instead of waiting for it
                    std::swap(h->greens, h->greens_alt);
                    CHK(calculate_greens_src(h, h->greens, L, R));
                    CHK(prop_check(h));
                    return 0;
                }
                discard_pending_flush(h);
                CHK(calculate_greens_src(h, h->greens, L, R));
                if (h->p.check_propagation_error) CHK(prop_check(h));
            } else {
                CHK(add_slice_sequence_left(h, h->K));
                h->direction = -1;
                h->current_slice = M + 1;
                CHK(propagate(h));
            }
        } else {
            CHK(wrap_greens(h, &h->greens, h->current_slice, 1));
            h->current_slice += 1;
        }
    } else {
        if ((h->current_slice - 1) % s == 0) {
            h->current_slice -= 1;
            if (h->current_slice == M) {
                const Udt L = slot_ref(h, h->K);
                CHK(reset_slot(h, h->K));
                discard_pending_flush(h);
                CHK(calculate_greens_src(h, h->greens, L, slot_ref(h, h->K)));
                CHK(wrap_greens(h, &h->greens, h->current_slice + 1, -1));
            } else if (0 < h->current_slice && h->current_slice < M) {
                const int idx = h->current_slice / s + 1;
                const Udt L = slot_ref(h, idx - 1);
                CHK(add_slice_sequence_right(h, idx));
                const Udt R = slot_ref(h, idx - 1);
                // greens_temp = old Green's function (stack.jl:596-600): exchange the buffers instead of copying
                if (h->p.check_propagation_error) {
                    CHK(materialize_pending_flush(h));
                    std::swap(h->greens_temp, h->greens);
                }
                discard_pending_flush(h);
                CHK(calculate_greens_src(h, h->greens, L, R));
                if (h->p.check_propagation_error) CHK(prop_check(h));
                CHK(wrap_greens(h, &h->greens, h->current_slice + 1, -1));
            } else {
                CHK(add_slice_sequence_right(h, 1));
                h->direction = 1;
                h->current_slice = 0;
                CHK(propagate(h));
            }
        } else {
            CHK(wrap_greens(h, &h->greens, h->current_slice, -1));
            h->current_slice -= 1;
        }
    }
    return 0;
}

// DQMC.jl:546-582
static int sweep_spatial_launches(dqmc_handle *h);
// the fused chunk loop runs where the handle admitted it (dqmc_create) and the chunks are whole
static bool sweep_takes_fused(const dqmc_handle *h) { return h->sweep_fused && h->n % 64 == 0 && h->N >= 128; }
static int sweep_spatial(dqmc_handle *h)
{
    const int l = h->current_slice;
    if (l < 1 || l > h->M) return fail(h, DQMC_ERR_STATE, "sweep_spatial: current_slice outside 1..slices");
    CHK(sweep_spatial_launches(h));
    return 0;
}
static int sweep_spatial_launches(dqmc_handle *h)
{
    const int l = h->current_slice;
    int8_t *cslice = h->conf + (long)(l - 1) * h->N;
    h->conf_version++;
    // decide on the 64 x 64 block (four waves per walker), apply the chunk out of place with MFMA
    CHK(materialize_pending_flush(h));  // (normally consumed by the wrap in between)
    double *cur = h->greens, *alt = h->greens_alt;
    const size_t istr = (size_t)h->units * sweep_lu_image_doubles();

    const long cstr = (long)h->N * h->M;
    hipEvent_t a, b;
    if (sweep_takes_fused(h)) {
        // the elimination of chunk c runs beside the flush of chunk c - 1 (one launch per chunk boundary)
        const int nc = h->N / 64;
        timing_events(h, &a, &b);
        HIPCHK(launch_sweep_lu(h->n, h->nb, h->W, cur, h->nn, cslice, cstr, 0, 64, h->lu_img, h->sc, h->rng, h->stats,
                               h->p.check_sign_problem, h->qr_ws.errflag, h->stream, a, b));
        CHK(timing_push(h, a, b, DQMC_K_SWEEP));
        for (int c = 1; c < nc; ++c) {
            timing_events(h, &a, &b);
            HIPCHK(launch_sweep_fused(h->n, h->nb, h->W, cur, alt, h->nn, cslice, cstr, 64 * c, 64 * (c - 1),
                                      h->lu_img + (size_t)(c & 1) * istr, h->lu_img + (size_t)((c - 1) & 1) * istr, h->sc,
                                      h->rng, h->stats, h->p.check_sign_problem, h->qr_ws.errflag, h->stream, a, b));
            CHK(timing_push(h, a, b, DQMC_K_SWEEP));
            std::swap(cur, alt);
        }
        // the last chunk: left pending for the next wrap (its image slot is not written before the next sweep), or applied
        const double *img_last = h->lu_img + (size_t)((nc - 1) & 1) * istr;
        if (fold_wrap_flush(h)) {
            h->pf = dqmc_handle::PendingFlush{cur, img_last, 64 * (nc - 1)};
        } else {
            timing_events(h, &a, &b);
            HIPCHK(launch_sweep_flush_lu(h->n, h->units, cur, alt, h->nn, 64 * (nc - 1), 64, img_last, h->sw, h->stream, a, b));
            CHK(timing_push(h, a, b, DQMC_K_FLUSH));
            std::swap(cur, alt);
        }
        if (cur != h->greens) std::swap(h->greens, h->greens_alt);
        return 0;
    }
    for (int site0 = 0; site0 < h->N; site0 += 64) {
        const int ns = std::min(64, h->N - site0);
        timing_events(h, &a, &b);
        HIPCHK(launch_sweep_lu(h->n, h->nb, h->W, cur, h->nn, cslice, cstr, site0, ns, h->lu_img, h->sc,
                               h->rng, h->stats, h->p.check_sign_problem, h->qr_ws.errflag, h->stream, a, b));
        CHK(timing_push(h, a, b, DQMC_K_SWEEP));
        timing_events(h, &a, &b);
        HIPCHK(launch_sweep_flush_lu(h->n, h->units, cur, alt, h->nn, site0, ns, h->lu_img, h->sw, h->stream, a, b));
        CHK(timing_push(h, a, b, DQMC_K_FLUSH));
        std::swap(cur, alt);
    }
    if (cur != h->greens) std::swap(h->greens, h->greens_alt);
    return 0;
}

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

const char *dqmc_last_error(const dqmc_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int dqmc_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

int dqmc_create(const dqmc_params *p, dqmc_handle **out)
{
    if (!p || !out) return fail(nullptr, DQMC_ERR_INVALID, "dqmc_create: null argument");
    *out = nullptr;
    if (p->n_sites < 1 || p->slices < 1 || p->safe_mult < 1 || p->n_walkers < 1)
        return fail(nullptr, DQMC_ERR_INVALID, "dqmc_create: n_sites, slices, safe_mult, n_walkers must be >= 1");
    if (p->slices % p->safe_mult != 0)  // stack.jl:115: convert(Int, slices / safe_mult) throws InexactError
        return fail(nullptr, DQMC_ERR_INVALID, "dqmc_create: slices must be divisible by safe_mult");
    if (p->model_kind != DQMC_ATTRACTIVE && p->model_kind != DQMC_REPULSIVE)
        return fail(nullptr, DQMC_ERR_INVALID, "dqmc_create: unknown model_kind");
    if (!p->eT || !p->eTinv || !p->eT2 || !p->eTinv2)
        return fail(nullptr, DQMC_ERR_INVALID, "dqmc_create: hopping exponentials missing");
    if (!(p->U >= 0.0)) return fail(nullptr, DQMC_ERR_INVALID, "dqmc_create: U must be positive");
    const int nb = p->model_kind == DQMC_REPULSIVE ? 2 : 1;
    if (p->n_sites > 1024) return fail(nullptr, DQMC_ERR_INVALID, "dqmc_create: n_sites exceeds 1024 (unsupported)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, DQMC_ERR_NO_DEVICE, "dqmc_create: no HIP device visible");
    if (p->device_id < 0 || p->device_id >= ndev)
        return fail(nullptr, DQMC_ERR_INVALID, "dqmc_create: device_id out of range");

    dqmc_handle *h = new dqmc_handle();
    read_kernel_switches(h);
    h->p = *p;
    h->p.eT = h->p.eTinv = h->p.eT2 = h->p.eTinv2 = nullptr;
    h->N = h->n = p->n_sites;
    h->nb = nb;
    h->M = p->slices;
    h->s = p->safe_mult;
    h->K = h->M / h->s;
    h->W = p->n_walkers;
    h->units = h->W * h->nb;
    h->nn = (long)h->n * h->n;
    // elimination of chunk c beside the flush of chunk c - 1 in one launch (the elimination first applies the previous
    // chunk to its own 64 x 64 block; the flush workgroups take two column passes each, so that at 32 units the whole
    // launch is co-resident, one workgroup per CU): 36 us per chunk against 24 + 17 for the two separate launches.
    // DQMC_SWEEP_SPLIT selects the separate launches.
    // With more units than that the phase is throughput-bound and the separate launches win (config 4 on one GPU,
    // 512 units: 688 vs 715 ms per sweep), so the fused form is used only when its grid fits the CUs.
    h->sweep_fused = false;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, p->device_id) == hipSuccess) h->cus = prop.multiProcessorCount;
    }
    if (!h->sw.sweep_split && h->n % 64 == 0 && h->cus) h->sweep_fused = sweep_fused_fits(h);
    // lambda = acosh(exp(U*dtau/2)) (Attractive.jl:103,118; Repulsive.jl:116,138)
    h->lambda = std::acosh(std::exp(0.5 * p->U * p->delta_tau));
    h->epl = std::exp(h->lambda);
    h->eml = std::exp(-h->lambda);
    for (int ci = 0; ci < 2; ++ci) {
        const double c = ci ? 1.0 : -1.0;
        const double dE = -2.0 * h->lambda * c;
        h->sc.gamma[ci] = std::exp(dE) - 1.0;
        h->sc.ebos[ci] = std::exp(-dE);
        h->sc.dup[ci] = std::exp(dE) - 1.0;
        h->sc.ddn[ci] = std::exp(-dE) - 1.0;
    }
    auto bail = [&](int rc) {
        g_create_error = h->err;
        dqmc_destroy(h);
        return rc;
    };
#define CCHK(expr)                     \
    do {                               \
        int rc__ = (expr);             \
        if (rc__ != 0) return bail(rc__); \
    } while (0)
#define CHIP(expr)                                                        \
    do {                                                                  \
        hipError_t e__ = (expr);                                          \
        if (e__ != hipSuccess) {                                          \
            h->err = std::string(#expr) + ": " + hipGetErrorString(e__);  \
            return bail(DQMC_ERR_HIP);                                    \
        }                                                                 \
    } while (0)
    CHIP(hipSetDevice(p->device_id));
    CHIP(hipStreamCreate(&h->stream));
    const size_t cn = (size_t)nb * h->nn, un = (size_t)h->units * h->nn, uv = (size_t)h->units * h->n;
    CCHK(dalloc(h, &h->eT, cn)); CCHK(dalloc(h, &h->eTinv, cn));
    CCHK(dalloc(h, &h->eT2, cn)); CCHK(dalloc(h, &h->eTinv2, cn));
    CHIP(hipMemcpy(h->eT, p->eT, cn * sizeof(double), hipMemcpyHostToDevice));
    CHIP(hipMemcpy(h->eTinv, p->eTinv, cn * sizeof(double), hipMemcpyHostToDevice));
    CHIP(hipMemcpy(h->eT2, p->eT2, cn * sizeof(double), hipMemcpyHostToDevice));
    CHIP(hipMemcpy(h->eTinv2, p->eTinv2, cn * sizeof(double), hipMemcpyHostToDevice));
    if (h->n == 256 && !h->sw.no_slab) {
        std::vector<double> tr(cn);
        for (int b = 0; b < nb; ++b)
            for (int j = 0; j < h->n; ++j)
                for (int i = 0; i < h->n; ++i) tr[(size_t)b * h->nn + j + (size_t)h->n * i] = p->eT2[(size_t)b * h->nn + i + (size_t)h->n * j];
        CCHK(dalloc(h, &h->eT2T, cn));
        CHIP(hipMemcpy(h->eT2T, tr.data(), cn * sizeof(double), hipMemcpyHostToDevice));
        h->slab = true;
    }
    if (!h->sw.no_kron && (h->slab || h->n != 256)) {
        // the gate forms of this size in the table's order: the first one that takes every block of eT2 and eTinv2 (at
        // n = 256 the factored launches stand in for the slab path's: none without it)
        std::vector<double> img;
        for (HopForm f : {HopForm::Square16, HopForm::Rect32x8, HopForm::Cubic8, HopForm::Bilayer16}) {
            if (hop_row(f).n != h->n || !build_hop_image(f, nb, p->eT2, p->eTinv2, nullptr, img)) continue;
            CCHK(dalloc(h, &h->kron_f, img.size()));
            CHIP(hipMemcpy(h->kron_f, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
            h->form = f;
            break;
        }
    }
    CCHK(dalloc(h, &h->conf, (size_t)h->W * h->N * h->M));
    {
        std::vector<int8_t> ones((size_t)h->W * h->N * h->M, 1);
        CHIP(hipMemcpy(h->conf, ones.data(), ones.size(), hipMemcpyHostToDevice));
    }
    CCHK(dalloc(h, &h->u_stack, (size_t)(h->K + 2) * un));
    CCHK(dalloc(h, &h->t_stack, (size_t)(h->K + 2) * un));
    CCHK(dalloc(h, &h->d_stack, (size_t)(h->K + 2) * uv));
    for (int i = 0; i <= h->K + 1; ++i) {
        h->su.push_back(h->u_stack + (size_t)i * un);
        h->st.push_back(h->t_stack + (size_t)i * un);
        h->sd.push_back(h->d_stack + (size_t)i * uv);
    }
    double **mats[] = {&h->Ul, &h->Ur, &h->Tl, &h->Tr, &h->greens, &h->greens_temp, &h->tmp1,
                       &h->tmp2, &h->bufA, &h->bufB, &h->qs.V, &h->qs.W, &h->qs.S};
    for (auto m : mats) CCHK(dalloc(h, m, un));
    CCHK(dalloc(h, &h->Dl, uv)); CCHK(dalloc(h, &h->Dr, uv)); CCHK(dalloc(h, &h->qs.tau, uv));
    const size_t wn = (size_t)h->units * ((h->n + 15) / 16) * 256;
    CCHK(dalloc(h, &h->qs.winv, wn));
    if (h->n > 256) CCHK(dalloc(h, &h->qs.ts, un));
    CCHK(dalloc(h, &h->qs.pivot, uv));
    CCHK(alloc_qr_workspace(h));
    CCHK(alloc_wrap_handoff(h));
    CCHK(dalloc(h, &h->greens_alt, un));
    CCHK(dalloc(h, &h->lu_img, 2 * (size_t)h->units * sweep_lu_image_doubles()));
    CCHK(dalloc(h, &h->rng, (size_t)h->W));
    CCHK(dalloc(h, &h->stats, (size_t)h->W));
    CCHK(dalloc(h, &h->pc_scratch, 2 * (size_t)h->W));
    CCHK(dalloc(h, &h->gm, (size_t)h->W));
    for (int i = 0; i < 2; ++i) {
        CCHK(dalloc(h, &h->gm_lad[i], (size_t)h->units));
        CCHK(dalloc(h, &h->gm_sg[i], (size_t)h->units));
    }
    {
        std::vector<DevStats> st(h->W);
        for (auto &x : st) {
            x.prop_local = x.acc_local = 0;
            x.negative_probability = {-INFINITY, INFINITY, 0.0, 0};
            x.propagation_error = {-INFINITY, INFINITY, 0.0, 0};
        }
        CHIP(hipMemcpy(h->stats, st.data(), sizeof(DevStats) * h->W, hipMemcpyHostToDevice));
        std::vector<WalkerRng> rg(h->W);
        for (int w = 0; w < h->W; ++w) rg[w] = {(unsigned long long)w, 0ull, nullptr, 0ull, 0};
        CHIP(hipMemcpy(h->rng, rg.data(), sizeof(WalkerRng) * h->W, hipMemcpyHostToDevice));
    }
    h->uniforms.assign(h->W, nullptr);
    {
        const size_t acc_n = 2 * cn + (size_t)nb * h->n + 1;
        CCHK(sec_layout(h, DQMC_RED_GREENS, acc_n, acc_n, (long)(cn + (size_t)nb * h->n), 0, BIN_SRC_GREENS));
        CCHK(sec_layout(h, DQMC_RED_SIGN, DQMC_RED_SIGN, 0, 0, 0));
        CCHK(dalloc(h, &h->sign_sw, (size_t)h->W + 2));
        CCHK(dalloc(h, &h->sign_fail, (size_t)h->W));
    }
    CCHK(init_stack(h));
    CHIP(hipStreamSynchronize(h->stream));
#undef CCHK
#undef CHIP
    *out = h;
    return DQMC_OK;
}

static void ut_free(dqmc_handle *h);
static int binner_reset(dqmc_handle *h);
static int ent_reset(dqmc_handle *h);  // entangle.inl
static int ctd_reset(dqmc_handle *h);  // current_tau.inl
static void ctd_off(dqmc_handle *h);   // (the stream must be idle)
static int ctd_row(dqmc_handle *h, int row, double cc_fac, const double *g0l, const double *gl0, const double *gll,
                   double *add_to, long add_stride, long add_off);
static int ctd_finish(dqmc_handle *h, double cc_fac);
static int tcov_reset(dqmc_handle *h);  // taucov.inl
static void tcov_off(dqmc_handle *h);   // (the stream must be idle)
static int tcov_push(dqmc_handle *h);   // behind mom_push of DQMC_BIN_MOMENTUM_TIME_DISPLACED
int dqmc_destroy(dqmc_handle *h)
{
    if (!h) return DQMC_OK;
    (void)hipSetDevice(h->p.device_id);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto &e : h->pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto e : h->pool) (void)hipEventDestroy(e);
    for (void *q : h->allocs) (void)hipFree(q);
    for (double *u : h->uniforms)
        if (u) (void)hipFree(u);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    ut_free(h);
    delete h;
    return DQMC_OK;
}

#define ENTER(h)                                                        \
    if (!(h)) return DQMC_ERR_INVALID;                                  \
    HIPCHK(hipSetDevice((h)->p.device_id))
#define WALKER_OK(h, w) \
    if ((w) < 0 || (w) >= (h)->W) return fail((h), DQMC_ERR_INVALID, "walker index out of range")

int dqmc_set_conf(dqmc_handle *h, int32_t w, const int8_t *conf)
{
    ENTER(h); WALKER_OK(h, w);
    const size_t sz = (size_t)h->N * h->M;
    for (size_t i = 0; i < sz; ++i)
        if (conf[i] != 1 && conf[i] != -1) return fail(h, DQMC_ERR_INVALID, "conf entries must be +1 or -1");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->conf + (size_t)w * sz, conf, sz, hipMemcpyHostToDevice));
    h->conf_version++;
    return DQMC_OK;
}
int dqmc_get_conf(dqmc_handle *h, int32_t w, int8_t *conf)
{
    ENTER(h); WALKER_OK(h, w);
    const size_t sz = (size_t)h->N * h->M;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(conf, h->conf + (size_t)w * sz, sz, hipMemcpyDeviceToHost));
    return DQMC_OK;
}
int dqmc_set_uniforms(dqmc_handle *h, int32_t w, const double *u, size_t n)
{
    ENTER(h); WALKER_OK(h, w);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->uniforms[w]) { HIPCHK(hipFree(h->uniforms[w])); h->uniforms[w] = nullptr; }
    HIPCHK(hipMalloc((void **)&h->uniforms[w], (n ? n : 1) * sizeof(double)));
    HIPCHK(hipMemcpy(h->uniforms[w], u, n * sizeof(double), hipMemcpyHostToDevice));
    WalkerRng r = {0ull, 0ull, h->uniforms[w], (unsigned long long)n, 0};
    HIPCHK(hipMemcpy(h->rng + w, &r, sizeof(r), hipMemcpyHostToDevice));
    return DQMC_OK;
}
int dqmc_seed(dqmc_handle *h, int32_t w, uint64_t seed)
{
    ENTER(h); WALKER_OK(h, w);
    HIPCHK(hipStreamSynchronize(h->stream));
    WalkerRng r = {(unsigned long long)seed, 0ull, nullptr, 0ull, 0};
    HIPCHK(hipMemcpy(h->rng + w, &r, sizeof(r), hipMemcpyHostToDevice));
    const unsigned long long m0 = 0;  // the move counter of the global-move stream starts anew with the seed
    HIPCHK(hipMemcpy(&h->gm[w].moves_drawn, &m0, sizeof(m0), hipMemcpyHostToDevice));
    return DQMC_OK;
}
int dqmc_uniforms_used(dqmc_handle *h, int32_t w, uint64_t *used)
{
    ENTER(h); WALKER_OK(h, w);
    HIPCHK(hipStreamSynchronize(h->stream));
    WalkerRng r;
    HIPCHK(hipMemcpy(&r, h->rng + w, sizeof(r), hipMemcpyDeviceToHost));
    *used = r.draw;
    return DQMC_OK;
}
int dqmc_get_state(dqmc_handle *h, int32_t *cs, int32_t *dir)
{
    if (!h) return DQMC_ERR_INVALID;
    if (cs) *cs = h->current_slice;
    if (dir) *dir = h->direction;
    return DQMC_OK;
}

static int check_rng(dqmc_handle *h)
{
    std::vector<WalkerRng> rg(h->W);
    HIPCHK(hipMemcpy(rg.data(), h->rng, sizeof(WalkerRng) * h->W, hipMemcpyDeviceToHost));
    for (int w = 0; w < h->W; ++w)
        if (rg[w].exhausted) return fail(h, DQMC_ERR_RNG, "host-supplied uniform stream exhausted");
    return 0;
}
int dqmc_synchronize(dqmc_handle *h)
{
    ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    CHK(timing_drain(h));
    CHK(check_qr_workspace(h));
    return check_rng(h);
}
int dqmc_build_stack(dqmc_handle *h)
{
    ENTER(h);
    CHK(build_stack(h));
    h->prepared = true;
    return dqmc_synchronize(h);
}
int dqmc_prepare(dqmc_handle *h)
{
    ENTER(h);
    CHK(init_stack(h));
    CHK(build_stack(h));
    CHK(propagate(h));
    h->prepared = true;
    h->gm_updates = 0;
    return dqmc_synchronize(h);
}
static int update_hooked(dqmc_handle *h);  // global_move.inl: propagate, the global-move hook (off by default), sweep_spatial
#define NEED_PREPARED(h) \
    if (!(h)->prepared) return fail((h), DQMC_ERR_STATE, "call dqmc_prepare or dqmc_build_stack first")
int dqmc_propagate(dqmc_handle *h)
{
    ENTER(h); NEED_PREPARED(h);
    CHK(propagate(h));
    return dqmc_synchronize(h);
}
int dqmc_sweep_spatial(dqmc_handle *h)
{
    ENTER(h); NEED_PREPARED(h);
    CHK(sweep_spatial(h));
    CHK(materialize_pending_flush(h));  // (the API boundary: greens as the reference has it)
    return dqmc_synchronize(h);
}
int dqmc_update(dqmc_handle *h)
{
    ENTER(h); NEED_PREPARED(h);
    CHK(update_hooked(h));
    CHK(materialize_pending_flush(h));  // (the API boundary: greens as the reference has it)
    return dqmc_synchronize(h);
}
int dqmc_sweep(dqmc_handle *h, int32_t n_sweeps)
{
    ENTER(h); NEED_PREPARED(h);
    for (int i = 0; i < n_sweeps; ++i)
        for (int u = 0; u < 2 * h->M; ++u) CHK(update_hooked(h));
    CHK(materialize_pending_flush(h));  // (the API boundary: greens as the reference has it)
    return dqmc_synchronize(h);
}
int dqmc_update_until_measure(dqmc_handle *h, int32_t *n_updates)
{
    ENTER(h); NEED_PREPARED(h);
    int cnt = 0;
    do {
        CHK(update_hooked(h));
        ++cnt;
    } while (!(h->current_slice == 1 && h->direction == 1));
    if (n_updates) *n_updates = cnt;
    CHK(materialize_pending_flush(h));  // (the API boundary: greens as the reference has it)
    return dqmc_synchronize(h);
}

int dqmc_get_greens_eff(dqmc_handle *h, int32_t w, double *out)
{
    ENTER(h); WALKER_OK(h, w);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->greens + (size_t)w * h->nb * h->nn, sizeof(double) * h->nb * h->nn, hipMemcpyDeviceToHost));
    return DQMC_OK;
}
int dqmc_set_greens_eff(dqmc_handle *h, int32_t w, const double *in)
{
    ENTER(h); WALKER_OK(h, w);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->greens + (size_t)w * h->nb * h->nn, in, sizeof(double) * h->nb * h->nn, hipMemcpyHostToDevice));
    return DQMC_OK;
}
// greens!(mc): temp = greens*eT; out = eTinv*temp (DQMC.jl:721-730); result in tmp2
static int true_greens(dqmc_handle *h, const double *src)
{
    if (h->cb.on) {
        CHK(cb_mult(h, CB_RIGHT_ET, 0, src, h->tmp1, nullptr));
        CHK(cb_mult(h, CB_LEFT_ETINV, 0, h->tmp1, h->tmp2, nullptr));
        return 0;
    }
    CHK(run_gemm(h, gemm_base(h, U_(h, src), 0, C_(h, h->eT), 0, h->tmp1)));
    CHK(run_gemm(h, gemm_base(h, C_(h, h->eTinv), 0, U_(h, h->tmp1), 0, h->tmp2)));
    return 0;
}
int dqmc_get_greens(dqmc_handle *h, int32_t w, double *out)
{
    ENTER(h); WALKER_OK(h, w);
    CHK(true_greens(h, h->greens));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->tmp2 + (size_t)w * h->nb * h->nn, sizeof(double) * h->nb * h->nn, hipMemcpyDeviceToHost));
    return DQMC_OK;
}

// calculate_greens(mc, slice, output) (stack.jl:422-480) for every walker of the handle
static int calculate_greens_from_scratch(dqmc_handle *h, int slice, double *output, double *a2_copy = nullptr)
{
    const int n = h->n, M = h->M, s = h->s;
    // right factor: Ur,Dr,Tr = B(slice+1)' ... B(M)'
    CHK(set_identity(h, h->bufA)); CHK(set_identity(h, h->Ur)); CHK(set_ones(h, h->Dr)); CHK(set_identity(h, h->Tr));
    double *cur = h->bufA, *oth = h->bufB;
    auto chain_step = [&](int k, bool dagger, bool stab, double *D, double *T, double *Ufinal) -> int {
        if (h->cb.on) CHK(cb_mult(h, dagger ? CB_LEFT_BDAG : CB_LEFT_B, k, cur, oth, stab ? D : nullptr));
        else {
            GemmArgs g = dagger ? gemm_base(h, C_(h, h->eT2), 1, U_(h, cur), 0, oth)
                                : gemm_base(h, C_(h, h->eT2), 0, U_(h, cur), 0, oth);
            if (dagger) { g.rowscale = vs_conf(h, k, +1); g.row_first = 1; }
            else g.kscale = vs_conf(h, k, +1);
            if (stab) g.colscale = vs_arr(D, n);
            CHK(run_gemm(h, g));
        }
        std::swap(cur, oth);
        if (stab) {
            // udt(curr_U, D, tmp1); T = tmp1 * T  (stack.jl:441-444)
            CHK(udt(h, cur, Ufinal ? Ufinal : oth, D, h->tmp2, 1));
            if (!Ufinal) std::swap(cur, oth);
            CHK(copy_mat(h, h->tmp1, T));
            CHK(run_gemm(h, gemm_base(h, U_(h, h->tmp2), 0, U_(h, h->tmp1), 0, T)));
        }
        return 0;
    };
    if (slice + 1 <= M) {
        for (int k = M; k >= slice + 1; --k) CHK(chain_step(k, true, k % s == 0, h->Dr, h->Tr, nullptr));
        // final: tmp1 = curr_U*Diagonal(Dr); udt(Ur, Dr, tmp1); Tr = tmp1*Tr
        GemmArgs g = gemm_base(h, U_(h, cur), 0, U_(h, h->qs.S), 0, oth);
        CHK(set_identity(h, h->qs.S));
        g.colscale = vs_arr(h->Dr, n);
        CHK(run_gemm(h, g));
        std::swap(cur, oth);
        CHK(udt(h, cur, h->Ur, h->Dr, h->tmp2, 1));
        CHK(copy_mat(h, h->tmp1, h->Tr));
        CHK(run_gemm(h, gemm_base(h, U_(h, h->tmp2), 0, U_(h, h->tmp1), 0, h->Tr)));
    }
    // left factor: Ul,Dl,Tl = B(slice) ... B(1)
    CHK(set_identity(h, h->bufA)); CHK(set_identity(h, h->Ul)); CHK(set_ones(h, h->Dl)); CHK(set_identity(h, h->Tl));
    cur = h->bufA; oth = h->bufB;
    if (slice >= 1) {
        for (int k = 1; k <= slice; ++k) CHK(chain_step(k, false, k % s == 0, h->Dl, h->Tl, nullptr));
        GemmArgs g = gemm_base(h, U_(h, cur), 0, U_(h, h->qs.S), 0, oth);
        CHK(set_identity(h, h->qs.S));
        g.colscale = vs_arr(h->Dl, n);
        CHK(run_gemm(h, g));
        std::swap(cur, oth);
        CHK(udt(h, cur, h->Ul, h->Dl, h->tmp2, 1));
        CHK(copy_mat(h, h->tmp1, h->Tl));
        CHK(run_gemm(h, gemm_base(h, U_(h, h->tmp2), 0, U_(h, h->tmp1), 0, h->Tl)));
    }
    CHK(calculate_greens(h, output, a2_copy));
    return 0;
}
int dqmc_calculate_greens_at(dqmc_handle *h, int32_t w, int32_t slice, double *out)
{
    ENTER(h); WALKER_OK(h, w);
    if (slice < 0 || slice > h->M) return fail(h, DQMC_ERR_INVALID, "slice out of range 0..slices");
    CHK(calculate_greens_from_scratch(h, slice, h->greens_temp));
    HIPCHK(hipStreamSynchronize(h->stream));
    CHK(check_qr_workspace(h));
    HIPCHK(hipMemcpy(out, h->greens_temp + (size_t)w * h->nb * h->nn, sizeof(double) * h->nb * h->nn,
                     hipMemcpyDeviceToHost));
    return DQMC_OK;
}
// the per-configuration step of replay!(mc) (DQMC.jl:651-653): calculate_greens(mc, slice) into
// mc.s.greens for every walker; current_slice is set like replay! does (DQMC.jl:647)
int dqmc_replay_greens(dqmc_handle *h, int32_t slice)
{
    ENTER(h);
    if (slice < 0 || slice > h->M) return fail(h, DQMC_ERR_INVALID, "slice out of range 0..slices");
    CHK(calculate_greens_from_scratch(h, slice, h->greens));
    h->current_slice = 1;
    h->prepared = true;
    return dqmc_synchronize(h);
}
// compress(mc, model, conf) / decompress (HubbardModel.jl:56-59): Julia BitArray chunks
int dqmc_get_conf_bits(dqmc_handle *h, int32_t w, uint64_t *chunks)
{
    ENTER(h); WALKER_OK(h, w);
    const size_t sz = (size_t)h->N * h->M, nch = (sz + 63) / 64;
    unsigned long long *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, nch * sizeof(unsigned long long)));
    hipError_t e1 = launch_conf_pack(h->conf + (size_t)w * sz, sz, d, h->stream);
    hipError_t e2 = e1 == hipSuccess ? hipStreamSynchronize(h->stream) : e1;
    hipError_t e3 = e2 == hipSuccess ? hipMemcpy(chunks, d, nch * sizeof(unsigned long long), hipMemcpyDeviceToHost) : e2;
    (void)hipFree(d);
    HIPCHK(e3);
    return DQMC_OK;
}
int dqmc_set_conf_bits(dqmc_handle *h, int32_t w, const uint64_t *chunks)
{
    ENTER(h); WALKER_OK(h, w);
    const size_t sz = (size_t)h->N * h->M, nch = (sz + 63) / 64;
    unsigned long long *d = nullptr;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMalloc((void **)&d, nch * sizeof(unsigned long long)));
    hipError_t e1 = hipMemcpy(d, chunks, nch * sizeof(unsigned long long), hipMemcpyHostToDevice);
    hipError_t e2 = e1 == hipSuccess ? launch_conf_unpack(d, sz, h->conf + (size_t)w * sz, h->stream) : e1;
    hipError_t e3 = e2 == hipSuccess ? hipStreamSynchronize(h->stream) : e2;
    (void)hipFree(d);
    HIPCHK(e3);
    h->conf_version++;
    return DQMC_OK;
}

int dqmc_wrap_greens(dqmc_handle *h, int32_t slice, int32_t direction)
{
    ENTER(h);
    if (direction != 1 && direction != -1) return fail(h, DQMC_ERR_INVALID, "direction must be +1 or -1");
    const int l = direction == 1 ? slice : slice - 1;
    if (l < 1 || l > h->M) return fail(h, DQMC_ERR_INVALID, "wrap_greens: slice out of range");
    CHK(wrap_greens(h, &h->greens, slice, direction));
    return dqmc_synchronize(h);
}

static void conv_mag(const DevMagStats &d, dqmc_magstats &o) { o.max = d.max; o.min = d.min; o.sum = d.sum; o.count = d.count; }
int dqmc_get_stats(dqmc_handle *h, int32_t w, dqmc_stats *out)
{
    ENTER(h); WALKER_OK(h, w);
    HIPCHK(hipStreamSynchronize(h->stream));
    DevStats d;
    HIPCHK(hipMemcpy(&d, h->stats + w, sizeof(d), hipMemcpyDeviceToHost));
    out->prop_local = d.prop_local;
    out->acc_local = d.acc_local;
    out->imaginary_probability = {-INFINITY, INFINITY, 0.0, 0};
    conv_mag(d.negative_probability, out->negative_probability);
    conv_mag(d.propagation_error, out->propagation_error);
    return DQMC_OK;
}

// binner.inl: binner_room refuses the call (before anything is accumulated) when the section's binner is full or its
// layout has changed; binner_push_section pushes the samples the measurement kernels have just left on the device
static int binner_room(dqmc_handle *h, int which);
static int binner_push_section(dqmc_handle *h, int which);
// momentum.inl: the transform of the source section's per-walker sample, then its push; mom_off drops the tables and the
// three binners, mom_disable one binner
static int mom_push(dqmc_handle *h, int which);
static void mom_disable(dqmc_handle *h, int which);
static void mom_off(dqmc_handle *h);
// response.inl: the channel contraction / bond kinetic energy, the transform and the push of a response binner;
// resp_disable drops one binner, resp_channels_off the channel table and the two pairing binners
static int resp_push(dqmc_handle *h, int which);
static void resp_disable(dqmc_handle *h, int which);
static void resp_channels_off(dqmc_handle *h);
// global_move.inl: with sign weighting on, s_w of the current fields into sign_sw and their sum into the sign sums of the
// sections about to be fed (DQMC_RED_* indices; sec_b < 0: one section); nothing with it off.  Runs a slice chain unless
// the cache of the current field holds, so it comes in front of true_greens (the chain overwrites tmp1 / tmp2).
static int sign_begin(dqmc_handle *h, int sec_a, int sec_b = -1);
int dqmc_accumulate_greens(dqmc_handle *h)
{
    ENTER(h); NEED_PREPARED(h);
    CHK(binner_room(h, DQMC_BIN_GREENS));
    CHK(sign_begin(h, DQMC_RED_GREENS));
    CHK(true_greens(h, h->greens));
    {
        Timed t(h, DQMC_K_MISC);
        if (h->sign_on)
            HIPCHK(launch_accumulate_signed(h->n, h->nb, h->W, h->tmp2, h->nn, h->sign_sw, h->sec[DQMC_RED_GREENS].acc, h->stream));
        else
            HIPCHK(launch_accumulate(h->n, h->nb, h->W, h->tmp2, h->nn, h->sec[DQMC_RED_GREENS].acc, h->stream));
    }
    if (h->bin[DQMC_BIN_GREENS].on) CHK(binner_push_section(h, DQMC_BIN_GREENS));
    return DQMC_OK;
}
static int cc_setup(dqmc_handle *h);
static int td_setup(dqmc_handle *h, int every, int what);
// EachSitePairByDistance(lattice) (lattice_iterators.jl:157-190) as a direction table
int dqmc_set_pair_directions(dqmc_handle *h, const int32_t *dir_of, int32_t n_dirs)
{
    ENTER(h);
    const int n = h->n;
    if (!dir_of || n_dirs < 1 || n_dirs > n * n) return fail(h, DQMC_ERR_INVALID, "bad direction table");
    std::vector<int> ptr(n_dirs + 1, 0), src((size_t)n * n), trg((size_t)n * n);
    for (int s = 0; s < n; ++s)
        for (int t = 0; t < n; ++t) {
            const int d = dir_of[s + (size_t)n * t];
            if (d < 0 || d >= n_dirs) return fail(h, DQMC_ERR_INVALID, "direction index out of range");
            ptr[d + 1]++;
        }
    for (int d = 0; d < n_dirs; ++d) ptr[d + 1] += ptr[d];
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int s = 0; s < n; ++s)          // the reference's order inside a direction: src outer, trg inner
        for (int t = 0; t < n; ++t) {
            const int d = dir_of[s + (size_t)n * t];
            src[fill[d]] = s;
            trg[fill[d]] = t;
            fill[d]++;
        }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!h->pair_src) {
        CHK(dalloc(h, &h->pair_src, (size_t)n * n));
        CHK(dalloc(h, &h->pair_trg, (size_t)n * n));
    }
    dfree(h, &h->dir_ptr);
    CHK(dalloc(h, &h->dir_ptr, (size_t)n_dirs + 1));
    mom_off(h);  // the phase tables belong to the old directions
    h->n_dirs = n_dirs;
    h->red_valid = false;  // (re)sized: the last reduction is void
    const size_t corr_n = 4 * (size_t)n_dirs + 3 * (size_t)n + 1;
    CHK(sec_layout(h, DQMC_RED_CORRELATIONS, corr_n, corr_n, (long)corr_n - 1, 4 * (size_t)n_dirs, BIN_SRC_CORR));
    HIPCHK(hipMemcpy(h->dir_ptr, ptr.data(), sizeof(int) * (n_dirs + 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->pair_src, src.data(), sizeof(int) * n * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->pair_trg, trg.data(), sizeof(int) * n * n, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->K_cc) CHK(cc_setup(h));  // the current-current tables follow the directions
    if (h->td.every) CHK(td_setup(h, h->td.every, h->td.what));  // and so do the time-displaced rows
    return DQMC_OK;
}
int dqmc_accumulate_correlations(dqmc_handle *h)
{
    ENTER(h); NEED_PREPARED(h);
    if (!h->n_dirs) return fail(h, DQMC_ERR_STATE, "call dqmc_set_pair_directions first");
    CHK(binner_room(h, DQMC_BIN_CORRELATIONS));
    CHK(binner_room(h, DQMC_BIN_MOMENTUM_CORRELATIONS));
    CHK(sign_begin(h, DQMC_RED_CORRELATIONS));
    CHK(true_greens(h, h->greens));
    if (h->sign_on) {
        Timed t(h, DQMC_K_MISC);
        const dqmc_handle::Section &sc = h->sec[DQMC_RED_CORRELATIONS];
        HIPCHK(launch_correlation_pairs(h->n, h->nb, h->p.model_kind, h->W, h->tmp2, h->nn, h->dir_ptr, h->pair_src,
                                        h->pair_trg, h->n_dirs, sc.per_walker, h->stream));
        HIPCHK(launch_corr_reduce_signed(h->n, h->nb, h->p.model_kind, h->W, h->tmp2, h->nn, h->n_dirs, sc.per_walker,
                                         h->sign_sw, sc.acc, h->stream));
    } else {
        Timed t(h, DQMC_K_MISC);
        HIPCHK(launch_correlations(h->n, h->nb, h->p.model_kind, h->W, h->tmp2, h->nn, h->dir_ptr, h->pair_src,
                                   h->pair_trg, h->n_dirs, h->sec[DQMC_RED_CORRELATIONS].per_walker,
                                   h->sec[DQMC_RED_CORRELATIONS].acc, h->stream));
    }
    if (h->bin[DQMC_BIN_CORRELATIONS].on) CHK(binner_push_section(h, DQMC_BIN_CORRELATIONS));
    if (h->bin[DQMC_BIN_MOMENTUM_CORRELATIONS].on) CHK(mom_push(h, DQMC_BIN_MOMENTUM_CORRELATIONS));
    return DQMC_OK;
}
// EachLocalQuadByDistance{K}(lattice) (lattice_iterators.jl:264-318) as a target table
int dqmc_set_local_targets(dqmc_handle *h, const int32_t *trg_of, int32_t K)
{
    ENTER(h);
    const int n = h->n;
    if (!h->n_dirs) return fail(h, DQMC_ERR_STATE, "call dqmc_set_pair_directions first");
    if (!trg_of || K < 1 || K > h->n_dirs) return fail(h, DQMC_ERR_INVALID, "bad target table");
    for (size_t i = 0; i < (size_t)n * K; ++i)
        if (trg_of[i] < -1 || trg_of[i] >= n) return fail(h, DQMC_ERR_INVALID, "target index out of range");
    HIPCHK(hipStreamSynchronize(h->stream));
    resp_channels_off(h);  // the channel table belongs to the old targets
    h->K_loc = K;
    h->red_valid = false;
    dfree(h, &h->trg_of);
    CHK(dalloc(h, &h->trg_of, (size_t)n * K));
    const size_t pc_n = (size_t)h->n_dirs * K * K + 1;
    CHK(sec_layout(h, DQMC_RED_PAIRING, pc_n, pc_n, (long)pc_n - 1, pc_n - 1));
    HIPCHK(hipMemcpy(h->trg_of, trg_of, sizeof(int) * n * K, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}
int dqmc_accumulate_pairing(dqmc_handle *h)
{
    ENTER(h); NEED_PREPARED(h);
    if (!h->K_loc) return fail(h, DQMC_ERR_STATE, "call dqmc_set_local_targets first");
    CHK(binner_room(h, DQMC_BIN_PAIRING));
    CHK(binner_room(h, DQMC_BIN_RESPONSE_PAIRING));
    CHK(sign_begin(h, DQMC_RED_PAIRING));
    CHK(true_greens(h, h->greens));
    if (h->sign_on) {
        Timed t(h, DQMC_K_MISC);
        const dqmc_handle::Section &sc = h->sec[DQMC_RED_PAIRING];
        HIPCHK(launch_pairing_pairs(h->n, h->nb, h->W, h->tmp2, h->nn, h->dir_ptr, h->pair_src, h->pair_trg, h->n_dirs,
                                    h->K_loc, h->trg_of, sc.per_walker, h->stream));
        HIPCHK(launch_reduce_signed(h->W, sc.bin_E, 1.0, sc.per_walker, h->sign_sw, sc.acc, h->stream));
    } else {
        Timed t(h, DQMC_K_MISC);
        HIPCHK(launch_pairing(h->n, h->nb, h->W, h->tmp2, h->nn, h->dir_ptr, h->pair_src, h->pair_trg, h->n_dirs,
                              h->K_loc, h->trg_of, h->sec[DQMC_RED_PAIRING].per_walker, h->sec[DQMC_RED_PAIRING].acc,
                              h->stream));
    }
    if (h->bin[DQMC_BIN_PAIRING].on) CHK(binner_push_section(h, DQMC_BIN_PAIRING));
    if (h->bin[DQMC_BIN_RESPONSE_PAIRING].on) CHK(resp_push(h, DQMC_BIN_RESPONSE_PAIRING));
    return DQMC_OK;
}
int dqmc_reset_accumulators(dqmc_handle *h)
{
    ENTER(h);
    h->red_valid = false;  // (the last reduction no longer describes the accumulators)
    for (const auto &s : h->sec)
        if (s.n) HIPCHK(hipMemsetAsync(s.acc, 0, s.n * sizeof(double), h->stream));
    CHK(binner_reset(h));
    CHK(ent_reset(h));
    CHK(ctd_reset(h));
    CHK(tcov_reset(h));
    return DQMC_OK;
}

// ---- size / host get / device export of a section's sums (dqmc_handle::Section) --------------------------------------
static const char *const SEC_NEED[] = {nullptr, "call dqmc_set_pair_directions first", "call dqmc_set_local_targets first",
                                       "nothing accumulated", "call dqmc_set_time_displaced first", nullptr,
                                       "call dqmc_set_thermodynamics first"};
static int sec_size(dqmc_handle *h, int which, size_t *n)
{
    if (!h || !n) return DQMC_ERR_INVALID;
    *n = h->sec[which].n;
    return DQMC_OK;
}
static int sec_get(dqmc_handle *h, int which, double *host_out)
{
    const dqmc_handle::Section &s = h->sec[which];
    if (!s.n) return fail(h, DQMC_ERR_STATE, SEC_NEED[which]);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(host_out, s.acc, s.n * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
static int sec_export(dqmc_handle *h, int which, void *device_out)
{
    const dqmc_handle::Section &s = h->sec[which];
    if (!s.n) return fail(h, DQMC_ERR_STATE, SEC_NEED[which]);
    HIPCHK(hipMemcpyAsync(device_out, s.acc, s.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}
int dqmc_accumulator_size(dqmc_handle *h, size_t *n) { return sec_size(h, DQMC_RED_GREENS, n); }
int dqmc_get_accumulators(dqmc_handle *h, double *host_out) { ENTER(h); return sec_get(h, DQMC_RED_GREENS, host_out); }
int dqmc_export_accumulators(dqmc_handle *h, void *device_out) { ENTER(h); return sec_export(h, DQMC_RED_GREENS, device_out); }
int dqmc_correlations_size(dqmc_handle *h, size_t *n) { return sec_size(h, DQMC_RED_CORRELATIONS, n); }
int dqmc_get_correlations(dqmc_handle *h, double *host_out) { ENTER(h); return sec_get(h, DQMC_RED_CORRELATIONS, host_out); }
int dqmc_export_correlations(dqmc_handle *h, void *device_out) { ENTER(h); return sec_export(h, DQMC_RED_CORRELATIONS, device_out); }
int dqmc_pairing_size(dqmc_handle *h, size_t *n) { return sec_size(h, DQMC_RED_PAIRING, n); }
int dqmc_get_pairing(dqmc_handle *h, double *host_out) { ENTER(h); return sec_get(h, DQMC_RED_PAIRING, host_out); }
int dqmc_export_pairing(dqmc_handle *h, void *device_out) { ENTER(h); return sec_export(h, DQMC_RED_PAIRING, device_out); }

#include "unequal_time.inl"
#include "binner.inl"
#include "momentum.inl"
#include "taucov.inl"
#include "global_move.inl"
#include "thermo.inl"
#include "response.inl"
#include "entangle.inl"
#include "current_tau.inl"
#include "checkpoint.inl"

// ---------------------------------------------------------------------------
// Measurement reduction over ranks: every accumulator the handle keeps and the DQMCAnalysis
// counters, as ONE packed device buffer of doubles [sums | maxima | minima]:
//   sums   = acc (G, G.^2, occupation, count), correlations, pairing, susceptibilities, time-displaced rows (each if
//            configured), the sums of signs (with sign weighting on), the thermodynamics section (if configured), then prop_local, acc_local, negative_probability {sum, count}, propagation_error {sum, count}
//   maxima = negative_probability.max, propagation_error.max      minima = the two .min
// (MagnitudeStats, DQMC.jl:4-47).  dqmc_reduce runs three ncclAllReduce (sum / max / min) on the handle's stream;
// a host-side collective (MPI from Julia, gloo in the tests) can do the same through export / import.
static const size_t RED_STAT_SUMS = 6;
static size_t red_nsum(dqmc_handle *h)
{
    size_t n = RED_STAT_SUMS;
    for (const auto &s : h->sec) n += s.n_red;
    return n;
}
static int red_pack(dqmc_handle *h)
{
    const size_t nsum = red_nsum(h), tot = nsum + 4;
    if (h->red_cap < tot) {
        HIPCHK(hipStreamSynchronize(h->stream));  // (the old buffer goes back)
        dfree(h, &h->red_buf);
        h->red_cap = 0;
        CHK(dalloc(h, &h->red_buf, tot));
        h->red_cap = tot;
    }
    size_t off = 0;
    for (int i = 0; i <= DQMC_RED_THERMODYNAMICS; ++i) {
        const dqmc_handle::Section &s = h->sec[i];
        if (s.n_red)
            HIPCHK(hipMemcpyAsync(h->red_buf + off, s.acc, s.n_red * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        off += s.n_red;
        h->red_sizes[i] = s.n_red;
    }
    // the time-displaced sums went without their sample count: the passes that feed them feed the susceptibilities, whose
    // count stands for both (dqmc_get_reduced hands it out with the section) - if the two local counts agree
    h->red_td_ok = false;
    const dqmc_handle::Section &td = h->sec[DQMC_RED_TIME_DISPLACED], &sus = h->sec[DQMC_RED_SUSCEPTIBILITIES];
    if (td.n) {
        double c_td = 0.0, c_sus = 0.0;
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(&c_td, td.acc + td.n - 1, sizeof(double), hipMemcpyDeviceToHost));
        if (sus.n) HIPCHK(hipMemcpy(&c_sus, sus.acc + sus.n - 1, sizeof(double), hipMemcpyDeviceToHost));
        h->red_td_ok = c_td == c_sus;
    }
    // counters of the local walkers, reduced on the host in walker order
    std::vector<DevStats> st(h->W);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(st.data(), h->stats, sizeof(DevStats) * h->W, hipMemcpyDeviceToHost));
    double tail[RED_STAT_SUMS + 4] = {0, 0, 0, 0, 0, 0, -INFINITY, -INFINITY, INFINITY, INFINITY};
    for (const auto &x : st) {
        tail[0] += (double)x.prop_local;
        tail[1] += (double)x.acc_local;
        tail[2] += x.negative_probability.sum;
        tail[3] += (double)x.negative_probability.count;
        tail[4] += x.propagation_error.sum;
        tail[5] += (double)x.propagation_error.count;
        tail[6] = std::fmax(tail[6], x.negative_probability.max);
        tail[7] = std::fmax(tail[7], x.propagation_error.max);
        tail[8] = std::fmin(tail[8], x.negative_probability.min);
        tail[9] = std::fmin(tail[9], x.propagation_error.min);
    }
    HIPCHK(hipMemcpy(h->red_buf + off, tail, sizeof(tail), hipMemcpyHostToDevice));
    return 0;
}
// The reduced sums stay in red_buf (read with dqmc_get_reduced): the handle's own accumulators keep the LOCAL sums, so
// that the reduction can be repeated every measure_rate sweeps (DQMC.jl:429-436) - writing the global sums back into
// them would count the earlier samples once per rank again at the next reduction.
static int red_unpack(dqmc_handle *h)
{
    const size_t off = red_nsum(h) - RED_STAT_SUMS;
    double tail[RED_STAT_SUMS + 4];
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(tail, h->red_buf + off, sizeof(tail), hipMemcpyDeviceToHost));
    dqmc_stats &r = h->red_stats;
    r.prop_local = (int64_t)std::llround(tail[0]);
    r.acc_local = (int64_t)std::llround(tail[1]);
    r.imaginary_probability = {-INFINITY, INFINITY, 0.0, 0};
    r.negative_probability = {tail[6], tail[8], tail[2], (int64_t)std::llround(tail[3])};
    r.propagation_error = {tail[7], tail[9], tail[4], (int64_t)std::llround(tail[5])};
    h->red_valid = true;
    return 0;
}
int dqmc_comm_unique_id(void *id128)
{
    if (!id128) return DQMC_ERR_INVALID;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return fail(nullptr, DQMC_ERR_HIP, "ncclGetUniqueId failed");
    std::memcpy(id128, &id, sizeof(id));
    return DQMC_OK;
}
int dqmc_comm_init(const void *id128, int32_t nranks, int32_t rank, int32_t device_id, dqmc_comm **out)
{
    if (!id128 || !out || nranks < 1 || rank < 0 || rank >= nranks) return fail(nullptr, DQMC_ERR_INVALID, "dqmc_comm_init: bad arguments");
    *out = nullptr;
    if (hipSetDevice(device_id) != hipSuccess) return fail(nullptr, DQMC_ERR_NO_DEVICE, "dqmc_comm_init: hipSetDevice failed");
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    dqmc_comm *c = new dqmc_comm();
    c->nranks = nranks; c->rank = rank; c->device = device_id;
    const ncclResult_t r = ncclCommInitRank(&c->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        delete c;
        return fail(nullptr, DQMC_ERR_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    }
    *out = c;
    return DQMC_OK;
}
int dqmc_comm_destroy(dqmc_comm *c)
{
    if (!c) return DQMC_OK;
    if (c->comm) (void)ncclCommDestroy(c->comm);
    delete c;
    return DQMC_OK;
}
int dqmc_reduce_size(dqmc_handle *h, size_t *n_doubles)
{
    if (!h || !n_doubles) return DQMC_ERR_INVALID;
    *n_doubles = red_nsum(h) + 4;
    return DQMC_OK;
}
int dqmc_reduce(dqmc_handle *h, dqmc_comm *comm)
{
    ENTER(h);
    CHK(red_pack(h));
    if (comm && comm->comm) {
        if (comm->device != h->p.device_id) return fail(h, DQMC_ERR_INVALID, "dqmc_reduce: communicator bound to another device");
        const size_t nsum = red_nsum(h);
        ncclResult_t r = ncclGroupStart();
        if (r == ncclSuccess) r = ncclAllReduce(h->red_buf, h->red_buf, nsum, ncclDouble, ncclSum, comm->comm, h->stream);
        if (r == ncclSuccess) r = ncclAllReduce(h->red_buf + nsum, h->red_buf + nsum, 2, ncclDouble, ncclMax, comm->comm, h->stream);
        if (r == ncclSuccess) r = ncclAllReduce(h->red_buf + nsum + 2, h->red_buf + nsum + 2, 2, ncclDouble, ncclMin, comm->comm, h->stream);
        const ncclResult_t r2 = ncclGroupEnd();
        if (r != ncclSuccess || r2 != ncclSuccess)
            return fail(h, DQMC_ERR_HIP, std::string("ncclAllReduce: ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
    }
    CHK(red_unpack(h));
    return DQMC_OK;
}
// host-mediated variant: pack -> host buffer (reduce it with any collective: sums first, then 2 maxima, 2 minima)
int dqmc_reduce_export(dqmc_handle *h, double *host_out)
{
    ENTER(h);
    CHK(red_pack(h));
    HIPCHK(hipMemcpy(host_out, h->red_buf, (red_nsum(h) + 4) * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
int dqmc_reduce_import(dqmc_handle *h, const double *host_in)
{
    ENTER(h);
    if (h->red_cap < red_nsum(h) + 4) return fail(h, DQMC_ERR_STATE, "call dqmc_reduce_export first");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->red_buf, host_in, (red_nsum(h) + 4) * sizeof(double), hipMemcpyHostToDevice));
    CHK(red_unpack(h));
    return DQMC_OK;
}
// section `which` of the last reduction: 0 Green's-function sums (dqmc_accumulator_size doubles), 1 correlations,
// 2 pairing, 3 susceptibilities (sizes as the local getters report), 4 the time-displaced rows: the E packed sums, then
// the reduced sample count of the susceptibilities (dqmc_time_displaced_size doubles), 5 the sums of signs, 6 thermodynamics
int dqmc_get_reduced(dqmc_handle *h, int32_t which, double *host_out)
{
    ENTER(h);
    if (!host_out || which < 0 || which > DQMC_RED_THERMODYNAMICS) return fail(h, DQMC_ERR_INVALID, "dqmc_get_reduced: bad arguments");
    if (!h->red_valid) return fail(h, DQMC_ERR_STATE, "call dqmc_reduce first");
    size_t off = 0;
    for (int i = 0; i < which; ++i) off += h->sec[i].n_red;
    const size_t cnt = h->sec[which].n_red;
    if (cnt == 0) return fail(h, DQMC_ERR_STATE, "dqmc_get_reduced: this accumulator is not configured");
    for (int i = 0; i <= DQMC_RED_THERMODYNAMICS; ++i)  // (sizes as they are NOW against the sizes that were packed)
        if (h->sec[i].n_red != h->red_sizes[i])
            return fail(h, DQMC_ERR_STATE, "accumulators were reconfigured after the last reduction: call dqmc_reduce again");
    if (h->red_cap < red_nsum(h) + 4) return fail(h, DQMC_ERR_STATE, "call dqmc_reduce first");
    if (which == DQMC_RED_TIME_DISPLACED && !h->red_td_ok)
        return fail(h, DQMC_ERR_STATE, "time-displaced and susceptibility sample counts differed at the last reduction: "
                                       "call dqmc_reset_accumulators after dqmc_set_time_displaced");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(host_out, h->red_buf + off, cnt * sizeof(double), hipMemcpyDeviceToHost));
    if (which == DQMC_RED_TIME_DISPLACED) {  // the susceptibilities are packed right in front: their last double is the count
        host_out[cnt] = 0.0;
        if (h->sec[DQMC_RED_SUSCEPTIBILITIES].n_red)
            HIPCHK(hipMemcpy(host_out + cnt, h->red_buf + off - 1, sizeof(double), hipMemcpyDeviceToHost));
    }
    return DQMC_OK;
}
int dqmc_get_reduced_stats(dqmc_handle *h, dqmc_stats *out)
{
    if (!h || !out) return DQMC_ERR_INVALID;
    if (!h->red_valid) return fail(h, DQMC_ERR_STATE, "call dqmc_reduce first");
    *out = h->red_stats;
    return DQMC_OK;
}


// Factors from the host (include/dqmc_hip.h): the triangular 16 x 16 lattice's hopping exponentials as three 16 x 16 factors
// per matrix, the t-t' square lattice's as four.  They are checked against the handle's own eT2 / eTinv2 (tri_factor_ok,
// ttp_factor_ok) before the handle takes them; a failed check leaves it as it was.
static int set_host_factors(dqmc_handle *h, const double *f, HopForm form, const std::string &name)
{
    ENTER(h);
    if (!f) return fail(h, DQMC_ERR_INVALID, name + ": null factors");
    if (h->n != 256) return fail(h, DQMC_ERR_INVALID, name + ": n_sites must be 256");
    if (h->prepared) return fail(h, DQMC_ERR_STATE, name + ": call before dqmc_prepare");
    if (!h->slab || h->cb.on || h->sw.no_kron || h->form != HopForm::None) return DQMC_OK;  // a path that does not take them: kept
    const int nb = h->nb;
    std::vector<double> E((size_t)2 * nb * h->nn), img;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(E.data(), h->eT2, sizeof(double) * nb * h->nn, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(E.data() + (size_t)nb * h->nn, h->eTinv2, sizeof(double) * nb * h->nn, hipMemcpyDeviceToHost));
    int b = 0;
    if (!build_hop_image(form, nb, E.data(), E.data() + (size_t)nb * h->nn, f, img, &b))
        return fail(h, DQMC_ERR_INVALID, name + ": the factors do not reproduce eT2 / eTinv2 of block " + std::to_string(b) + " within 256 ulp");
    CHK(dalloc(h, &h->kron_f, img.size()));
    HIPCHK(hipMemcpy(h->kron_f, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
    h->form = form;
    return DQMC_OK;
}
int dqmc_set_triangular_factors(dqmc_handle *h, const double *f) { return set_host_factors(h, f, HopForm::Tri16, "dqmc_set_triangular_factors"); }
int dqmc_set_square_tp_factors(dqmc_handle *h, const double *f) { return set_host_factors(h, f, HopForm::Ttp16, "dqmc_set_square_tp_factors"); }

// CheckerboardTrue with the bond-group factors kept sparse on the device (stack.jl:185-235): `n_mats` factors in ELL
// form (vals / cols [n_mats][n][kmax], 0-based columns, padding val 0), the diagonal exp(-+dtau mu) per block and
// seven factor sequences (order: B, B^-1, B', X B, X B^-1, X eT, eTinv X; entries index the factor list).
int dqmc_set_checkerboard(dqmc_handle *h, int32_t kmax, int32_t n_mats, const double *vals, const int32_t *cols,
                          const double *mu, const double *mu_inv, const int32_t *seqs /* [7][32] */,
                          const int32_t *lens /* [7] */)
{
    ENTER(h);
    if (kmax < 1 || kmax > 64 || n_mats < 1 || !vals || !cols || !mu || !mu_inv || !seqs || !lens)
        return fail(h, DQMC_ERR_INVALID, "dqmc_set_checkerboard: bad arguments");
    const size_t cnt = (size_t)n_mats * h->n * kmax;
    for (size_t i = 0; i < cnt; ++i)
        if (cols[i] < 0 || cols[i] >= h->n) return fail(h, DQMC_ERR_INVALID, "dqmc_set_checkerboard: column index out of range");
    for (int q = 0; q < 7; ++q) {
        if (lens[q] < 0 || lens[q] > 32) return fail(h, DQMC_ERR_INVALID, "dqmc_set_checkerboard: sequence too long");
        for (int i = 0; i < lens[q]; ++i)
            if (seqs[q * 32 + i] < 0 || seqs[q * 32 + i] >= n_mats)
                return fail(h, DQMC_ERR_INVALID, "dqmc_set_checkerboard: factor index out of range");
    }
    // the slab kernel keeps two images of n x (width + 1) doubles in LDS; refused before anything is allocated or changed
    if (!cb_slab_width(h->n, nullptr))
        return fail(h, DQMC_ERR_INVALID, "dqmc_set_checkerboard: n_sites = " + std::to_string(h->n) + " is beyond the sparse form: its "
                                         "narrowest slab (8 columns) needs 160 n bytes of the 163840 B of LDS, i.e. n_sites <= 1024; "
                                         "the handle keeps the dense constants");
    HIPCHK(hipStreamSynchronize(h->stream));
    CHK(dalloc(h, &h->cb.vals, cnt));
    CHK(dalloc(h, &h->cb.cols, cnt));
    CHK(dalloc(h, &h->cb.mu, (size_t)h->nb * h->n));
    CHK(dalloc(h, &h->cb.mu_inv, (size_t)h->nb * h->n));
    HIPCHK(hipMemcpy(h->cb.vals, vals, cnt * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->cb.cols, cols, cnt * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->cb.mu, mu, (size_t)h->nb * h->n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->cb.mu_inv, mu_inv, (size_t)h->nb * h->n * sizeof(double), hipMemcpyHostToDevice));
    h->cb.kmax = kmax; h->cb.n_mats = n_mats;
    for (int q = 0; q < 7; ++q) {
        h->cb.len[q] = lens[q];
        for (int i = 0; i < lens[q]; ++i) h->cb.seq[q][i] = seqs[q * 32 + i];
    }
    h->cb.on = true;
    return DQMC_OK;
}

// [sparse on, kmax, slab width, dynamic LDS bytes] of the checkerboard products; zeros on the dense constants
int dqmc_checkerboard_plan(dqmc_handle *h, int32_t out[4])
{
    if (!h || !out) return DQMC_ERR_INVALID;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!h->cb.on) return DQMC_OK;
    size_t lds = 0;
    out[0] = 1;
    out[1] = h->cb.kmax;
    out[2] = cb_slab_width(h->n, &lds);
    out[3] = (int32_t)lds;
    return DQMC_OK;
}
// diagnostic: one cb_mult of every unit on buffers of its own (no Monte-Carlo state is read but the HS field, none written)
int dqmc_checkerboard_apply(dqmc_handle *h, int32_t which, int32_t slice, const double *X, const double *qscale,
                            int32_t in_place, double *out)
{
    ENTER(h);
    if (!h->cb.on) return fail(h, DQMC_ERR_STATE, "dqmc_checkerboard_apply: the handle has no sparse checkerboard");
    if (!X || !out) return fail(h, DQMC_ERR_INVALID, "dqmc_checkerboard_apply: null matrix");
    if (which < CB_LEFT_B || which > CB_LEFT_ETINV) return fail(h, DQMC_ERR_INVALID, "dqmc_checkerboard_apply: which must be 0..6");
    const bool conf_scaled = which <= CB_RIGHT_BINV;  // (the two greens() sandwiches take no slice)
    if (conf_scaled && (slice < 1 || slice > h->M)) return fail(h, DQMC_ERR_INVALID, "dqmc_checkerboard_apply: slice out of range");
    const size_t cnt = (size_t)h->units * h->nn, qcnt = (size_t)h->units * h->n;
    struct Bufs {
        double *x = nullptr, *o = nullptr, *q = nullptr;
        ~Bufs() { (void)hipFree(x); (void)hipFree(o); (void)hipFree(q); }
    } b;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMalloc((void **)&b.x, cnt * sizeof(double)));
    if (!in_place) HIPCHK(hipMalloc((void **)&b.o, cnt * sizeof(double)));
    HIPCHK(hipMemcpy(b.x, X, cnt * sizeof(double), hipMemcpyHostToDevice));
    if (qscale) {
        HIPCHK(hipMalloc((void **)&b.q, qcnt * sizeof(double)));
        HIPCHK(hipMemcpy(b.q, qscale, qcnt * sizeof(double), hipMemcpyHostToDevice));
    }
    double *dst = in_place ? b.x : b.o;
    CHK(cb_mult(h, which, conf_scaled ? slice : 0, b.x, dst, b.q));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, dst, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}

// the device error word as it stands (not cleared): 0 unless a bounded wait inside a kernel ran out since the last call that
// reported it (bit 1: sweep elimination hand-off, bit 4: one-launch UDT hand-off, bit 5: one-launch wrap hand-off)
int dqmc_device_errors(dqmc_handle *h, int32_t *word)
{
    ENTER(h);
    if (!word) return DQMC_ERR_INVALID;
    *word = 0;
    if (!h->qr_ws.errflag) return DQMC_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(word, h->qr_ws.errflag, sizeof(int), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
// what the handle decided about its co-resident launch forms when it was set up (nothing is launched): [units, units in
// whole groups of eight, CUs, one-launch UDT call sites, workgroups the one-launch UDT may use (0: not admitted), workgroups
// the cooperative QR may use, cooperative QR admitted for these units, fused chunk loop, workgroups the one-launch wrap may
// use without / with a pending chunk, one-launch wrap admitted without / with a pending chunk]
int dqmc_launch_plan(dqmc_handle *h, int32_t out[12])
{
    if (!h || !out) return DQMC_ERR_INVALID;
    out[0] = h->units;
    out[1] = padded_units(h);
    out[2] = h->cus;
    out[3] = h->qrb_sites;
    out[4] = h->qr_ws.blk_max_blocks;
    out[5] = h->qr_ws.max_blocks;
    out[6] = qr_coop_grid(h->n, h->units, &h->qr_ws) != 0;
    out[7] = sweep_takes_fused(h);
    for (int pf = 0; pf < 2; ++pf) {
        out[8 + pf] = h->wrap_blocks[pf];
        out[10 + pf] = wrap_one_launch(h, pf != 0);
    }
    return DQMC_OK;
}
// which call sites of udt_AVX_pivot! take the one-launch pre-pivoted form (bit 0: slice-sequence builds and every other caller,
// bit 1 / 2: first / second factorisation of calculate_greens_AVX!); 0 = the pivoted multi-launch form everywhere
int dqmc_udt_one_launch_sites(dqmc_handle *h, int32_t *mask)
{
    if (!h || !mask) return DQMC_ERR_INVALID;
    *mask = h->qrb_sites;
    return DQMC_OK;
}

// diagnostics: cooperative-QR launches whose hand-offs timed out and were redone by the single-workgroup kernel
int dqmc_kron_hopping(dqmc_handle *h, int32_t *on)
{
    ENTER(h);
    if (!on) return DQMC_ERR_INVALID;
    *on = use_kron(h) ? 1 : 0;
    return DQMC_OK;
}

int dqmc_qr_fallbacks(dqmc_handle *h, int64_t *count)
{
    ENTER(h);
    if (!count) return DQMC_ERR_INVALID;
    *count = 0;
    if (!h->qr_ws.fb) return DQMC_OK;
    int fb[2] = {0, 0};
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(fb, h->qr_ws.fb, sizeof(fb), hipMemcpyDeviceToHost));
    *count = fb[1];
    return DQMC_OK;
}

int dqmc_timing_enable(dqmc_handle *h, int32_t on)
{
    ENTER(h);
    CHK(timing_drain(h));
    h->timing = on != 0;
    for (int i = 0; i < DQMC_K_COUNT; ++i) { h->fam_ms[i] = 0; h->fam_n[i] = 0; }
    return DQMC_OK;
}
int dqmc_timing_get(dqmc_handle *h, double *ms, int64_t *launches)
{
    ENTER(h);
    CHK(timing_drain(h));
    for (int i = 0; i < DQMC_K_COUNT; ++i) {
        if (ms) ms[i] = h->fam_ms[i];
        if (launches) launches[i] = h->fam_n[i];
    }
    return DQMC_OK;
}

// ---------------------------------------------------------------------------
// stand-alone batched primitives (host in / host out)
// ---------------------------------------------------------------------------
namespace {
// the primitive entry points run on a throw-away handle of their own (dqmc_handle hh)
static int scratch_init(dqmc_handle *h, int device_id, int n, int batch)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, DQMC_ERR_NO_DEVICE, "no HIP device visible");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, DQMC_ERR_INVALID, "device_id out of range");
    if (n < 1 || n > 1024 || batch < 1) return fail(nullptr, DQMC_ERR_INVALID, "n must be 1..1024 and batch >= 1");
    read_kernel_switches(h);
    h->p.device_id = device_id;
    h->n = h->N = n;
    h->nb = 1;
    h->W = h->units = batch;
    h->nn = (long)n * n;
    HIPCHK(hipSetDevice(device_id));
    HIPCHK(hipStreamCreate(&h->stream));
    return 0;
}
static void scratch_free(dqmc_handle *h)
{
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void *q : h->allocs) (void)hipFree(q);
    h->allocs.clear();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = nullptr;
}
}  // namespace

#define SCHK(expr)                                   \
    do {                                             \
        int rc_ = (expr);                            \
        if (rc_ != 0) {                              \
            g_create_error = h->err.empty() ? g_create_error : h->err; \
            scratch_free(h);                         \
            return rc_;                              \
        }                                            \
    } while (0)
#define SHIP(expr)                                                       \
    do {                                                                 \
        hipError_t e_ = (expr);                                          \
        if (e_ != hipSuccess) {                                          \
            g_create_error = std::string(#expr) + ": " + hipGetErrorString(e_); \
            scratch_free(h);                                             \
            return DQMC_ERR_HIP;                                         \
        }                                                                \
    } while (0)

int dqmc_vmul(int32_t device_id, int32_t n, int32_t batch, int32_t ta, int32_t tb, const double *A, const double *B,
              double *C)
{
    dqmc_handle hh; dqmc_handle *h = &hh;
    SCHK(scratch_init(h, device_id, n, batch));
    const size_t un = (size_t)batch * h->nn;
    double *dA, *dB, *dC;
    SCHK(dalloc(h, &dA, un, false)); SCHK(dalloc(h, &dB, un, false)); SCHK(dalloc(h, &dC, un));
    SHIP(hipMemcpy(dA, A, un * sizeof(double), hipMemcpyHostToDevice));
    SHIP(hipMemcpy(dB, B, un * sizeof(double), hipMemcpyHostToDevice));
    SCHK(run_gemm(h, gemm_base(h, U_(h, dA), ta != 0, U_(h, dB), tb != 0, dC)));
    SHIP(hipStreamSynchronize(h->stream));
    SHIP(hipMemcpy(C, dC, un * sizeof(double), hipMemcpyDeviceToHost));
    scratch_free(h);
    return DQMC_OK;
}

static int scratch_udt_bufs(dqmc_handle *h)
{
    const size_t un = (size_t)h->units * h->nn, uv = (size_t)h->units * h->n;
    CHK(dalloc(h, &h->qs.V, un)); CHK(dalloc(h, &h->qs.W, un)); CHK(dalloc(h, &h->qs.S, un));
    CHK(dalloc(h, &h->qs.tau, uv)); CHK(dalloc(h, &h->qs.pivot, uv));
    CHK(dalloc(h, &h->qs.winv, (size_t)h->units * ((h->n + 15) / 16) * 256));
    CHK(alloc_qr_workspace(h));
    return 0;
}

int dqmc_udt_pivot(int32_t device_id, int32_t n, int32_t batch, double *U, double *D, double *T, int64_t *pivot,
                   int32_t apply)
{
    dqmc_handle hh; dqmc_handle *h = &hh;
    SCHK(scratch_init(h, device_id, n, batch));
    const size_t un = (size_t)batch * h->nn, uv = (size_t)batch * n;
    double *dU, *dD, *dT, *dTo;
    SCHK(dalloc(h, &dU, un)); SCHK(dalloc(h, &dD, uv)); SCHK(dalloc(h, &dT, un, false)); SCHK(dalloc(h, &dTo, un));
    SCHK(scratch_udt_bufs(h));
    SHIP(hipMemcpy(dT, T, un * sizeof(double), hipMemcpyHostToDevice));
    SCHK(udt(h, dT, dU, dD, dTo, apply != 0));
    SHIP(hipStreamSynchronize(h->stream));
    SCHK(check_qr_workspace(h));
    SHIP(hipMemcpy(U, dU, un * sizeof(double), hipMemcpyDeviceToHost));
    SHIP(hipMemcpy(D, dD, uv * sizeof(double), hipMemcpyDeviceToHost));
    // (the one-launch form writes T out of place also for Val(false))
    SHIP(hipMemcpy(T, (apply || udt_is_fused(h, 0)) ? dTo : dT, un * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<int> piv(uv);
    SHIP(hipMemcpy(piv.data(), h->qs.pivot, uv * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < uv; ++i) pivot[i] = (int64_t)piv[i] + 1;
    scratch_free(h);
    return DQMC_OK;
}

int dqmc_logdet_matrices(int32_t device_id, int32_t n, int32_t batch, double *A, int64_t strideA, double *D,
                         int64_t strideD, double *logabsdet, int32_t *sign)
{
    dqmc_handle hh; dqmc_handle *h = &hh;
    SCHK(scratch_init(h, device_id, n, batch));
    if (!A || !D || !logabsdet || !sign || strideA < h->nn || strideD < n) {
        scratch_free(h);
        return fail(nullptr, DQMC_ERR_INVALID, "dqmc_logdet_matrices: null array, strideA < n * n or strideD < n");
    }
    const size_t ua = (size_t)batch * strideA, ud = (size_t)batch * strideD;
    double *dA, *dD, *dL;
    int *dS;
    SCHK(dalloc(h, &dA, ua, false)); SCHK(dalloc(h, &dD, ud, false)); SCHK(dalloc(h, &dL, batch)); SCHK(dalloc(h, &dS, batch));
    SHIP(hipMemcpy(dA, A, ua * sizeof(double), hipMemcpyHostToDevice));
    SHIP(hipMemcpy(dD, D, ud * sizeof(double), hipMemcpyHostToDevice));
    SHIP(launch_logdet(n, batch, dA, strideA, dD, strideD, dL, dS, h->stream));
    SHIP(hipStreamSynchronize(h->stream));
    SHIP(hipMemcpy(A, dA, ua * sizeof(double), hipMemcpyDeviceToHost));
    SHIP(hipMemcpy(D, dD, ud * sizeof(double), hipMemcpyDeviceToHost));
    SHIP(hipMemcpy(logabsdet, dL, batch * sizeof(double), hipMemcpyDeviceToHost));
    static_assert(sizeof(int) == sizeof(int32_t), "sign buffer");
    SHIP(hipMemcpy(sign, dS, batch * sizeof(int), hipMemcpyDeviceToHost));
    scratch_free(h);
    return DQMC_OK;
}

int dqmc_rdivp(int32_t device_id, int32_t n, int32_t batch, double *A, const double *T, const int64_t *pivot)
{
    dqmc_handle hh; dqmc_handle *h = &hh;
    SCHK(scratch_init(h, device_id, n, batch));
    const size_t un = (size_t)batch * h->nn, uv = (size_t)batch * n;
    double *dA, *dT;
    SCHK(dalloc(h, &dA, un, false)); SCHK(dalloc(h, &dT, un, false)); SCHK(dalloc(h, &h->qs.pivot, uv));
    SCHK(dalloc(h, &h->qs.winv, (size_t)h->units * ((h->n + 15) / 16) * 256));
    std::vector<int> piv(uv);
    for (size_t i = 0; i < uv; ++i) {
        if (pivot[i] < 1 || pivot[i] > n) { scratch_free(h); return fail(nullptr, DQMC_ERR_INVALID, "pivot entry out of range"); }
        piv[i] = (int)(pivot[i] - 1);
    }
    SHIP(hipMemcpy(dA, A, un * sizeof(double), hipMemcpyHostToDevice));
    SHIP(hipMemcpy(dT, T, un * sizeof(double), hipMemcpyHostToDevice));
    SHIP(hipMemcpy(h->qs.pivot, piv.data(), uv * sizeof(int), hipMemcpyHostToDevice));
    SCHK(rdivp(h, dA, dT));
    SHIP(hipStreamSynchronize(h->stream));
    SHIP(hipMemcpy(A, dA, un * sizeof(double), hipMemcpyDeviceToHost));
    scratch_free(h);
    return DQMC_OK;
}

int dqmc_calculate_greens(int32_t device_id, int32_t n, int32_t batch, const double *Ul, const double *Dl,
                          const double *Tl, const double *Ur, const double *Dr, const double *Tr, double *G)
{
    dqmc_handle hh; dqmc_handle *h = &hh;
    SCHK(scratch_init(h, device_id, n, batch));
    const size_t un = (size_t)batch * h->nn, uv = (size_t)batch * n;
    double *dG;
    SCHK(dalloc(h, &h->Ul, un, false)); SCHK(dalloc(h, &h->Ur, un, false)); SCHK(dalloc(h, &h->Tl, un, false));
    SCHK(dalloc(h, &h->Tr, un, false)); SCHK(dalloc(h, &h->Dl, uv, false)); SCHK(dalloc(h, &h->Dr, uv, false));
    SCHK(dalloc(h, &dG, un));
    SCHK(scratch_udt_bufs(h));
    SHIP(hipMemcpy(h->Ul, Ul, un * sizeof(double), hipMemcpyHostToDevice));
    SHIP(hipMemcpy(h->Ur, Ur, un * sizeof(double), hipMemcpyHostToDevice));
    SHIP(hipMemcpy(h->Tl, Tl, un * sizeof(double), hipMemcpyHostToDevice));
    SHIP(hipMemcpy(h->Tr, Tr, un * sizeof(double), hipMemcpyHostToDevice));
    SHIP(hipMemcpy(h->Dl, Dl, uv * sizeof(double), hipMemcpyHostToDevice));
    SHIP(hipMemcpy(h->Dr, Dr, uv * sizeof(double), hipMemcpyHostToDevice));
    SCHK(calculate_greens(h, dG));
    SHIP(hipStreamSynchronize(h->stream));
    SCHK(check_qr_workspace(h));
    SHIP(hipMemcpy(G, dG, un * sizeof(double), hipMemcpyDeviceToHost));
    scratch_free(h);
    return DQMC_OK;
}

int dqmc_mfma_f64_peak(int32_t device_id, int32_t iters, double *tflops)
{
    dqmc_handle hh; dqmc_handle *h = &hh;
    SCHK(scratch_init(h, device_id, 16, 1));
    double *sink;
    SCHK(dalloc(h, &sink, 16));
    hipDeviceProp_t prop;
    SHIP(hipGetDeviceProperties(&prop, device_id));
    // 8 waves per CU = 2 per SIMD, the occupancy of the GEMM launches at 32 units (DQMC_PROBE_WG_PER_CU: other occupancies)
    const int blocks = prop.multiProcessorCount * (getenv("DQMC_PROBE_WG_PER_CU") ? atoi(getenv("DQMC_PROBE_WG_PER_CU")) : 2);
    hipEvent_t a, b;
    SHIP(hipEventCreate(&a)); SHIP(hipEventCreate(&b));
    SHIP(launch_mfma_peak(iters / 8 + 1, blocks, sink, h->stream));  // warm up
    SHIP(hipEventRecord(a, h->stream));
    SHIP(launch_mfma_peak(iters, blocks, sink, h->stream));
    SHIP(hipEventRecord(b, h->stream));
    SHIP(hipStreamSynchronize(h->stream));
    float ms = 0.f;
    SHIP(hipEventElapsedTime(&ms, a, b));
    const double flops = (double)blocks * 4.0 /*waves*/ * (double)iters * 4.0 /*mfma*/ * 2.0 * 16 * 16 * 4;
    *tflops = flops / (ms * 1e-3) / 1e12;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    scratch_free(h);
    return DQMC_OK;
}

}  // extern "C"
