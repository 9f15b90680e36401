// kernels.h — launch interfaces of the gfx950 DQMC kernels (internal to libdqmc_hip.so).
//
// Data model: a "unit" is one n x n problem = (walker, block); unit = walker*nb + block.
// Every per-unit matrix is column-major with leading dimension ld and lives at
// base + unit*stride_unit + (unit % nb)*stride_blk  (stride_unit = 0 for the hopping
// exponentials, which are shared by all walkers and indexed by block only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dqmc {

// A length-n vector per unit that is either stored (d) or derived on the fly from
// the HS field: exp(±lambda*conf[i,l]) takes only two values
// (HubbardModelAttractive.jl:100-110, HubbardModelRepulsive.jl:113-126).
struct VecSrc {
    int mode;  // 0 = none (1.0), 1 = d[i], 2 = conf-derived, 3 = 1.0/d[i],
               // 4 = min(1, d[i]) (vmin!), 5 = 1/max(1, d[i]) (vmaxinv!, general.jl:90-117)
    const double *d;
    long stride;          // per unit
    const int8_t *conf;   // conf + walker*conf_stride + i  (already offset to the slice)
    long conf_stride;     // per walker
    double cpos[2], cneg[2];  // value for conf=+1 / conf=-1, per block
};
static inline VecSrc vs_none() { VecSrc v = {}; v.mode = 0; return v; }
static inline VecSrc vs_arr(const double *d, long stride) { VecSrc v = {}; v.mode = 1; v.d = d; v.stride = stride; return v; }
static inline VecSrc vs_inv(const double *d, long stride) { VecSrc v = {}; v.mode = 3; v.d = d; v.stride = stride; return v; }
static inline VecSrc vs_min1(const double *d, long stride) { VecSrc v = {}; v.mode = 4; v.d = d; v.stride = stride; return v; }
static inline VecSrc vs_maxinv(const double *d, long stride) { VecSrc v = {}; v.mode = 5; v.d = d; v.stride = stride; return v; }
#ifdef __HIPCC__
__device__ __forceinline__ double vs_get(const VecSrc &v, int unit, int nb, int i)
{
    if (v.mode == 1) return v.d[(long)unit * v.stride + i];
    if (v.mode == 3) return 1.0 / v.d[(long)unit * v.stride + i];
    if (v.mode == 2) {
        const int w = unit / nb, b = unit - w * nb;
        const int8_t c = v.conf[(long)w * v.conf_stride + i];
        return c > 0 ? v.cpos[b] : v.cneg[b];
    }
    if (v.mode == 4) return fmin(1.0, v.d[(long)unit * v.stride + i]);
    if (v.mode == 5) return 1.0 / fmax(1.0, v.d[(long)unit * v.stride + i]);
    return 1.0;
}
#endif

struct MatRef {
    const double *p;
    long stride_unit, stride_blk;
    int ld;
};
static inline MatRef mat(const double *p, long su, int ld, long sb = 0) { MatRef m = {p, su, sb, ld}; return m; }

// C[u] = beta*C[u] + epi( alpha * opA(A[u]) * diag(kscale) * opB(B[u]) ) + ident*I + diag(adddiag)
// epi applies colscale (index n) and rowscale (index m); row_first selects the order.
struct GemmArgs {
    int M, N, K;
    int n_units, nb;
    MatRef A, B;
    double *C; long strideC; int ldc;
    int transA, transB;
    VecSrc kscale, colscale, rowscale, adddiag;
    int row_first;
    double alpha;   // scale of the product
    double ident;   // added on the diagonal
    int beta;       // 0: overwrite, 1: accumulate into C
    // structure of the compact-WY operands (V = unit lower triangular Householder vectors with explicit zeros, M = N = K):
    //   1: C = V' V, only the 64 x 64 tiles on and above the diagonal are computed, k >= max(m0, n0) (the rest of the
    //      sum is zero; the triangle below the diagonal tiles is left untouched: nothing reads it)
    //   2: C = A V', k < n0 + 64 (V[n, k] = 0 for k > n)
    // (measured at 32 units, n = 256: no change of the launch time - 24.4 us either way: the launch lasts as long as
    // its full-k tiles, and those run at the chip's sustained fp64 MFMA rate, 45.7 TF/s = 23.5 us per 2 n^3 x 32; the
    // skipped work only saves power.  A k-tile of 32 instead of 16 did not change it either.)
    int tri;
};
// start/stop (optional): events that take the dispatch's own begin/end timestamps (hipExtLaunchKernelGGL),
// i.e. the kernel-only duration a profiler's kernel trace reports
hipError_t launch_gemm(const GemmArgs &g, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// Chain of left products on a column slab kept in LDS (slab.hip; n = 256 only, ld = 256):
//   X_s = post_s (.) (A_s (pre_s (.) X_{s-1})), out = X_nsteps (.) colscale;  pre/post = exp(sign lambda conf[row]) or none
constexpr int SLAB_MAX_STEPS = 10;
struct SlabStep {
    const double *A; long su, sb;        // A_s at A + unit su + block sb (su = 0: shared constant)
    const int8_t *pre_conf; int pre_sign;    // conf pointers already offset to the slice; null = no scaling
    const int8_t *post_conf; int post_sign;
};
struct SlabArgs {
    int n_units, nb, nsteps;
    SlabStep st[SLAB_MAX_STEPS];
    const double *X0; long x_su, x_sb;   // X_0 (per unit, or a shared constant with x_su = 0)
    double *out; long out_su;            // must not alias X0 or any per-unit A_s
    const double *col_d; long col_stride;  // final column scaling by an array (per unit), or
    const int8_t *col_conf; int col_sign;  // by exp(sign lambda conf[col]), or none
    long conf_stride;                    // per walker
    double epl, eml;
};
hipError_t launch_slab_chain(const SlabArgs &a, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// The same chains with A_s in one of the factored forms of hopping_forms.h, each with a kernel of its own (below); the
// form's operand layout behind ax / ay is described once, at the table there
struct KronStep {
    const double *ax, *ay;               // the two operand sets of A_s, all blocks (HopFormRow: fa / fb doubles per block)
    const int8_t *pre_conf; int pre_sign;    // conf pointers already offset to the slice; null = no scaling
    const int8_t *post_conf; int post_sign;
};
struct KronArgs {
    int n_units, nb, nsteps;
    KronStep st[SLAB_MAX_STEPS];
    const double *X0; long x_su;         // X_0 per unit
    double *out; long out_su;            // must not alias X0
    const double *col_d; long col_stride;  // final column scaling by an array (per unit), or none
    int transpose_out;                   // store the result transposed
    long conf_stride;                    // per walker
    double epl, eml;
    // pending rank-64 update of X_0 (launch_kron_chain / launch_kron_wrap only): the last chunk of a sweep, eliminated but not yet applied to G.  When
    // pf_img is set, X_0 is first replaced by X_0 + (X_0[:, c] - E) X Y X_0[c, :] (c = pf_site0 .. + 63, the chunk's image
    // at pf_img + unit * pf_img_su): what sweep_flush_lu_kernel would have written (kron.hip).  Null: no update.
    const double *pf_img; long pf_img_su;
    int pf_site0;
    // launch_kron_wrap only: st[1] goes from out into wrap_out; arrival word of unit u at wrap_cnt[KR_CNT_STRIDE u], which
    // reaches wrap_target (16 x the one-launch wraps on these words so far, this one included) when the unit's first step
    // is stored; errflag: the device error word (bit 5: that wait ran out)
    double *wrap_out;
    unsigned *wrap_cnt; unsigned wrap_target;
    int *errflag;
};
hipError_t launch_kron_chain(const KronArgs &a, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// wrap_greens! at n = 256 in one launch (kron.hip: kron_wrap_kernel): nsteps = 2, both results stored transposed.  Every
// workgroup waits for the 15 others of its unit, so the caller launches it only when kron_wrap_grid(n_units) workgroups are
// co-resident: kron_wrap_blocks_per_cu (the occupancy API, with / without the pending chunk) x compute units.
constexpr int KR_CNT_STRIDE = 32;  // arrival words on 128-byte lines of their own
inline int kron_wrap_grid(int n_units) { return (n_units + 7) / 8 * 8 * 16; }  // whole groups of eight units (XCD placement)
int kron_wrap_blocks_per_cu(bool pending);
hipError_t launch_kron_wrap(const KronArgs &a, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// The same chains at n = 512 = 8 x 8 x 8 sites with A_s = Ez (x) Exy (kron3.hip): ax / ay are the operand images of
// Exy (64 x 64, block b at + 4096 b) and of I2 (x) Ez (block b at + 256 b) described there
hipError_t launch_kron3_chain(const KronArgs &a, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// The same chains on the triangular 16 x 16 lattice (n = 256) with A_s = (Fy (x) Fx) Ed (tri.hip): ax = Fx and ay = Fy of
// block b at + 256 b, and Fd (applied along the diagonals x - y = const) at ay + 256 (nb + b)
hipError_t launch_tri_chain(const KronArgs &a, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// The same chains on the t-t' square 16 x 16 lattice (n = 256) with A_s = (Fy (x) Fx) Ed Ea (ttp.hip): ax, ay and Fd as for
// launch_tri_chain, and Fa (applied along the anti-diagonals x + y = const) at ay + 256 (2 nb + b)
hipError_t launch_ttp_chain(const KronArgs &a, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// The same chains on the two-layer square 16 x 16 x 2 lattice (n = 512) with A_s = Ez (x) Ey (x) Ex (bilayer.hip): ax = Ex of
// block b at + 256 b; ay = Ey of block b at + BILAYER_FB b, with the 2 x 2 Ez (column-major) behind it at + 256
constexpr int BILAYER_FB = 264;
hipError_t launch_bilayer_chain(const KronArgs &a, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// The same chains on the rectangular 32 x 8 lattice (n = 256, site x + 32 y) with A_s = Ey (x) Ex of unequal factors
// (rect.hip): ax = Ex (32 x 32, column-major) of block b at + 1024 b, ay = Ey (8 x 8) of block b at + 64 b
hipError_t launch_rect_chain(const KronArgs &a, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// Column-pivoted Householder QR, in place (udt_AVX_pivot! "QR decomposition" loop,
// src/linalg/UDT.jl:212-246).  On exit A holds R on/above the diagonal and the
// Householder vectors below it (unit diagonal implied), tau[n], pivot[n] (0-based:
// column j of the factored matrix is original column pivot[j]).
// Workspace of the cooperative (8 workgroups per matrix) QR: mailbox of n_units x 2 x 8 slots of
// QR_COOP_SLOT doubles (tagged packets), an error flag (bounded spins), a launch counter.
// Kernel-selection and test switches (environment).  Each handle, and each stand-alone primitive call, reads them once
// when it is set up (read_kernel_switches(), engine.cpp) and keeps its own copy; the launchers get them as arguments
// (or through the QR workspace) and never read the environment.  So a handle's kernels cannot change during its life,
// whatever another handle or thread does.
struct KernelSwitches {
    bool qr_noblocked = false;    // DQMC_QR_NOBLOCKED: no one-launch pre-pivoted UDT (qrb.hip)
    int qrb_sites = 7;            // DQMC_QRB_SITES: call sites that take it (bit mask, see alloc_qr_workspace)
    bool qr_tail = true;          // DQMC_QR_TAIL=0: no hand-over to qr_tail_kernel at n == 256
    bool qr_sc1 = false;          // DQMC_QR_SC1: write-through (agent-scope) packet stores regardless of placement
    bool qr_nocoop = false;       // DQMC_QR_NOCOOP: single-workgroup QR kernels only
    int qr_force_timeout = 0;     // DQMC_QR_FORCE_TIMEOUT (QrCoopWorkspace::force_timeout)
    bool qr_nopanel = false;      // DQMC_QR_NOPANEL: streaming QR instead of the panel kernel for n > 256
    bool trsm_simple = false;     // DQMC_TRSM_SIMPLE: substitution kernel instead of the MFMA solves
    bool sweep_split = false;     // DQMC_SWEEP_SPLIT: elimination and flush as separate launches
    bool flush_ncp2 = false;      // DQMC_FLUSH_NCP2: the separate flush always in its multi-pass form
    bool no_slab = false;         // DQMC_NO_SLAB: no slab-resident product chains (slab.hip)
    bool no_kron = false;         // DQMC_NO_KRON: dense slab chains even where the hopping factorises (kron.hip)
    bool no_wrap_flush = false;   // DQMC_NO_WRAP_FLUSH: the last chunk of a sweep as a stand-alone flush, not in the wrap
    bool wrap_two_launch = false; // DQMC_WRAP_TWO_LAUNCH: the factored wrap at n = 256 as two one-step launches
    bool tdm_general = false;     // DQMC_TDM_GENERAL: the pair-list kernel for the Green's rows of every table (tdm.hip)
};

constexpr int QR_COOP_SLOT = 528;  // 264 packets of 16 bytes
constexpr int QR_COOP_SLOTS_PER_UNIT = 16;  // 2 parities x 8 parts (qr_coop_kernel)
struct QrCoopWorkspace {
    double *mailbox = nullptr;
    int *errflag = nullptr;
    int *fb = nullptr;    // [0] launch epoch of the last cooperative launch that timed out, [1] fallbacks taken
    unsigned long long epoch = 0;
    int max_blocks = 0;   // launch the cooperative kernel only if its grid fits (co-residency)
    // switches, copied from the handle's KernelSwitches when the workspace is set up:
    bool tail = true;       // n == 256: steps 128.. on one CU per matrix (qr_tail_kernel)
    int force_sc1 = 0;      // write-through (agent-scope) packet stores regardless of placement
    int no_coop = 0;        // single-workgroup kernels only
    bool no_panel = false;  // streaming kernel instead of the panel kernel for n > 256
    int force_timeout = 0;  // test hook: 1 = every cooperative launch gives up at once;
                            // "step:<j>" -> 2 + j: part 3 of every matrix stops publishing at step j (bounded spins run out)
    // pre-pivoted blocked UDT (qrb.hip, n == 256): its own mailbox; blk_max_blocks = co-resident workgroups (0 = off)
    double *mailbox2 = nullptr;
    int blk_max_blocks = 0;
};
// udt_AVX_pivot! (UDT.jl:192-306) at n == 256 in one launch: U, D, T = D^-1 R (pivot applied or not, out of place), pivot
// (0-based positions -> original columns).  Pivot order = descending norm of the input columns (qrb.hip).
// B (optional, n_units x strideB, must not alias U): U receives B Q instead of Q (the product the reference forms right behind
// the decomposition in calculate_greens_AVX!, stack.jl:360 / :378)
hipError_t launch_udt_blocked(int n_units, const double *A, long strideA, double *U, long strideU, double *D, long strideD,
                              double *T, long strideT, int *pivot, QrCoopWorkspace *ws, int apply_pivot, hipStream_t s,
                              const double *B = nullptr, long strideB = 0);
size_t qrb_mailbox_bytes(int n_units);
int qrb_blocks_per_cu();
// ws may be null: single-workgroup kernels only
// W (n_units x strideW, may be null): output of the cooperative kernel, which leaves A intact so that a time-out of
// its hand-offs can be recovered by the single-workgroup kernel launched (guarded) behind it; *factored tells where
// the factored matrix is (W or A)
// X (n_units x strideX, may be null): hand-over buffer of the two-phase factorisation at n == 256 (cooperative steps
// 0..63, then one CU per matrix, qr_tail_kernel); its contents are scratch
hipError_t launch_qr_pivot(int n, int n_units, double *A, long strideA, double *tau, int *pivot,
                           QrCoopWorkspace *ws, double *W, long strideW, const double **factored, hipStream_t s,
                           double *X = nullptr, long strideX = 0);
int qr_coop_blocks_per_cu();
// grid of the cooperative kernel for n_units matrices, 0 where launch_qr_pivot takes a single-workgroup kernel instead
int qr_coop_grid(int n, int n_units, const QrCoopWorkspace *ws);

// After launch_qr_pivot: D = |diag R| (UDT.jl:268-272); V = unit-lower Householder
// vectors (n x n, explicit zeros/ones); T = D^-1 R:
//   apply_pivot = 1: Tout[i, pivot[j]] = R[i,j]/D[i], zero elsewhere (UDT.jl:283-297), out of place
//   apply_pivot = 0: A[i,j] *= 1/D[i] for j >= i in place, below-diagonal left dirty (UDT.jl:298-306)
// F = the factored matrix (A itself for the in-place kernels)
hipError_t launch_udt_finish(int n, int n_units, double *A, long strideA, const double *F, long strideF,
                             const int *pivot, double *D, long strideD, double *V, long strideV, double *Tout,
                             long strideT, int apply_pivot, hipStream_t s);

// X = gather(A)[:, pivot] * triu(T)^-1 written to Out (rdivp!, src/linalg/general.jl:138-166).
// pivot may be null (identity).  If dmul != null the diagonal of T is ignored and
// column j is multiplied by dmul[j] instead of divided by T[j,j] (used with the
// compact-WY triangle, whose inverse diagonal is tau).
hipError_t launch_trsm_right_upper(int n, int n_units, const double *A, long strideA, const double *T,
                                   long strideT, const int *pivot, const double *dmul, long strideV,
                                   double *Out, long strideOut, double *winv, const KernelSwitches &sw,
                                   hipStream_t s, double *scratch = nullptr);
// winv: n_units * ceil(n/16) * 256 doubles of scratch for the inverted diagonal blocks (n <= 256 path);
// nullptr selects the substitution kernel; scratch: n_units x strideOut doubles for the panelled MFMA solve of n > 256
// (without it the substitution kernel is used there); sw.trsm_simple: the substitution kernel everywhere

// sweep_spatial (DQMC.jl:546-582): the constants of the local updates, the walkers' random streams and counters
struct SweepConsts {
    // per conf value index ci = (conf>0): attractive gamma (Attractive.jl:121) and
    // exp(-dE_boson); repulsive Delta_up, Delta_dn (Repulsive.jl:139-141)
    double gamma[2], ebos[2], dup[2], ddn[2];
};
struct WalkerRng {           // device-resident, one per walker
    unsigned long long seed;
    unsigned long long draw;       // draws consumed (philox counter or array cursor)
    const double *uniforms;        // non-null: host-supplied stream
    unsigned long long n_uniforms;
    int exhausted;
};
struct DevMagStats { double max, min, sum; long long count; };
struct DevStats {
    long long prop_local, acc_local;
    DevMagStats negative_probability, propagation_error;
};
#ifdef __HIPCC__
__device__ __forceinline__ double philox_uniform(unsigned long long seed, unsigned long long index)
{
    unsigned int c0 = (unsigned int)index, c1 = (unsigned int)(index >> 32), c2 = 0u, c3 = 0u;
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
    const unsigned long long hi = c0 >> 5, lo = c1 >> 6;
    return (double)((hi << 26) | lo) * (1.0 / 9007199254740992.0);
}

// the same generator and uniform with all four counter words given: philox4_uniform(seed, low32(i), high32(i), 0, 0)
// equals philox_uniform(seed, i); the Ising cluster move draws from c2 = 1 (ising.hip)
__device__ __forceinline__ double philox4_uniform(unsigned long long seed, unsigned int c0, unsigned int c1,
                                                  unsigned int c2, unsigned int c3)
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
    const unsigned long long hi = c0 >> 5, lo = c1 >> 6;
    return (double)((hi << 26) | lo) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ void magstats_push(DevMagStats &s, double value)
{
    const double v = log10(fabs(value));
    s.max = fmax(s.max, v);
    s.min = fmin(s.min, v);
    s.sum += v;
    s.count += 1;
}
#endif
// One chunk of 64 sites of the current slice as a decide / apply pair (sweep_lu.hip): sweep_lu_kernel eliminates the
// 64 x 64 block G[c, c] with one wave per walker (decisions, HS field, counters) and leaves register images of the
// triangular factors (sweep_lu_image_doubles() doubles per unit); sweep_flush_lu_kernel applies the chunk to G out of
// place (Gout = Gin + T R0).  No limit on n_blocks * n_sites.
size_t sweep_lu_image_doubles();
// Layout of that image (doubles per unit): [U pair tiles 6][L pair tiles 6][PT 4][Q 4], each a 16 x 16 tile as 4 accumulator
// registers x 64 lanes of v_mfma_f64_16x16x4_f64 (register r of lane (g, ci) = element [4 r + g][ci]), then x[64].  U pair
// (K, J), K < J: block Uu_KJ of the eliminated strict upper triangle; L pair (K, J): block L_JK of the strict lower one;
// PT_J: (I - X_J Uu_JJ)^-1; Q_J: (I - L_JJ X_J)^-1 (X = diag(x); tools/proto/lu_sweep_proto.py: PT_J is the transpose of its
// PT[J], Q_J its Q[J]).  Taken as the A operand, register q of a tile is the B-side transpose (A[ci][4 q + g] = [4 q + g][ci]).
constexpr int LU_TILE = 256;
constexpr int LU_OFF_U = 0, LU_OFF_L = 6 * LU_TILE, LU_OFF_PT = 12 * LU_TILE, LU_OFF_Q = 16 * LU_TILE;
constexpr int LU_IMG = 20 * LU_TILE;
constexpr int LU_STRIDE = LU_IMG + 64;
__host__ __device__ constexpr int lu_pair(int K, int J)  // K < J: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
{
    return K == 0 ? J - 1 : (K == 1 ? J + 1 : 5);
}
hipError_t launch_sweep_lu(int n, int nb, int n_walkers, const double *G, long strideG, int8_t *conf_slice,
                           long conf_stride, int site0, int nsites, double *img, SweepConsts sc, WalkerRng *rng,
                           DevStats *stats, int check_sign, int *errflag, hipStream_t s,
                           hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// elimination of chunk `site0` beside the flush of the previous chunk `site0p` (one launch; n % 64 == 0)
hipError_t launch_sweep_fused(int n, int nb, int n_walkers, const double *Gin, double *Gout, long strideG,
                              int8_t *conf_slice, long conf_stride, int site0, int site0p, double *img,
                              const double *imgp, SweepConsts sc, WalkerRng *rng, DevStats *stats, int check_sign,
                              int *errflag, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// sw.flush_ncp2: the multi-pass form that more units than CUs take anyway
hipError_t launch_sweep_flush_lu(int n, int n_units, const double *Gin, double *Gout, long strideG, int site0,
                                 int nsites, const double *img, const KernelSwitches &sw, hipStream_t s,
                                 hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// Checkerboard products with sparse bond-group factors (cb.hip): O = post . F_last ... F_first . pre . X on the rows
// (side 0) or columns (side 1) of X; factor m in ELL form vals / cols [m][n][kmax]; the diagonal scalings are the
// conf-derived exp(+-lambda s) (sign +1 / -1, 0 = none) and / or a stored vector per block (mu); qscale scales the
// other index (the Diagonal(D) of add_slice_sequence_left/right).
struct CbArgs {
    int n, nb, side, kmax, seq_len;
    int seq[32];
    const double *vals;
    const int *cols;
    const double *X;
    double *O;
    long strideX;
    const int8_t *conf;   // already offset to the slice
    long conf_stride;
    double epl, eml;
    int pre_conf, post_conf;
    const double *pre_vec, *post_vec;   // [nb][n] or null
    const double *qscale;               // [units][qstride] or null
    long qstride;
};
hipError_t launch_cb_apply(const CbArgs &a, int n_units, hipStream_t s, hipEvent_t start = nullptr,
                           hipEvent_t stop = nullptr);
// slab width (32, 16 or 8 values of the index that is not mixed) cb_apply_kernel takes at n, and its dynamic LDS bytes;
// 0 when not even 8 columns fit CB_LDS_MAX
constexpr size_t CB_LDS_MAX = 160 * 1024;
int cb_slab_width(int n, size_t *lds_bytes);

// small helpers
hipError_t launch_set_identity(int n, int count, double *A, long stride, hipStream_t s);
hipError_t launch_fill(double *p, size_t n, double v, hipStream_t s);
// elementwise helpers of the unequal-time path: A = Diagonal(d) (copyto!(A, Diagonal(d))), A += B (rvadd!),
// O = A - I (vsub!, general.jl:67-85), d = f(d) in place with f given by the VecSrc mode
hipError_t launch_set_diag(int n, int nb, int units, double *A, long stride, VecSrc d, hipStream_t s);
hipError_t launch_mat_add(double *A, const double *B, size_t count, hipStream_t s);
hipError_t launch_sub_identity(int n, int units, double *O, const double *A, long stride, hipStream_t s);
hipError_t launch_vec_map(int n, int nb, int units, double *dst, long stride, VecSrc src, hipStream_t s);
hipError_t launch_scale_mat(int n, int nb, int units, double *O, const double *A, long stride, VecSrc row, VecSrc col,
                            int row_first, hipStream_t s);
// per walker max|A-B| over its nb blocks; pushes log10 into stats.propagation_error if > 1e-7
// scratch: 2 zero-initialised words per walker (partial maximum, arrival counter; left zeroed by every launch)
hipError_t launch_prop_check(int n, int nb, int n_walkers, const double *A, const double *B,
                             long stride_unit, DevStats *stats, unsigned long long *scratch, hipStream_t s);
// acc += sum over walkers of G, G.^2, 1-diag(G); layout documented in include/dqmc_hip.h
hipError_t launch_accumulate(int n, int nb, int n_walkers, const double *G, long stride_unit,
                             double *acc, hipStream_t s);
hipError_t launch_mfma_peak(int iters, int blocks, double *sink, hipStream_t s);
// equal-time correlations (cdc, sdc_x/y/z per direction; mx, my, mz per site), summed over walkers:
// acc layout [cdc nd][sdc_x nd][sdc_y nd][sdc_z nd][mx n][my n][mz n][count]
hipError_t launch_correlations(int n, int nb, int model, int n_walkers, const double *G, long stride_unit,
                               const int *dir_ptr, const int *pair_src, const int *pair_trg, int n_dirs,
                               double *per_walker, double *acc, hipStream_t s);
// pc_kernel over EachLocalQuadByDistance{K}: trg_of[src + n*k] = target of src in direction k (< K), -1 if none;
// per_walker [walkers][n_dirs*K*K], acc [n_dirs*K*K + 1] (Julia layout [dir12, dir1, dir2], then the sample count)
hipError_t launch_pairing(int n, int nb, int n_walkers, const double *G, long stride_unit, const int *dir_ptr,
                          const int *pair_src, const int *pair_trg, int n_dirs, int K, const int *trg_of,
                          double *per_walker, double *acc, hipStream_t s);
// susceptibilities: one time slice of the packed kernels added to per_walker [walkers][4*n_dirs (+ n_dirs*K*K)]
// ([cds][sds_x][sds_y][sds_z][ps]); the reduce multiplies by delta_tau and adds the sample count
hipError_t launch_sus_slice(int n, int nb, int model, int n_walkers, const double *G00, const double *G0l,
                            const double *Gl0, const double *Gll, long stride_unit, const int *dir_ptr,
                            const int *pair_src, const int *pair_trg, int n_dirs, int K, const int *trg_of,
                            double *per_walker, long per_stride, hipStream_t s);
hipError_t launch_sus_reduce(int n_walkers, long total, double factor, const double *per_walker, double *acc,
                             hipStream_t s);
// current_current_susceptibility (cc.hip): target table trg[k][s] (-1 if none) and, per block b, the hopping
// entries tst[b][k][s] = T_b[s, trg] and tts[b][k][s] = T_b[trg, s].  bsum [walkers][K][n] holds the G00 factor of
// the pass.  The fast path (fast = true; chosen by the host) needs n_dirs == n and, for every s1, a different dir12
// for every s2 (dsel[s1][s2] = dir12); the chunk tables describe the LDS panels (see cc.hip).
constexpr int CC_KMAX = 8;  // largest K of the fast path
struct CCPlan {
    int K = 0;
    const int *trg = nullptr;
    const double *tst = nullptr, *tts = nullptr;
    double *bsum = nullptr;
    bool fast = false;
    int C = 0, umax = 0, nchunks = 0, chunks_per_wg = 0, n_wg = 0, threads = 0;
    size_t lds_bytes = 0;
    const int *dsel = nullptr, *rows = nullptr, *ucnt = nullptr, *slot = nullptr;
    double *partial = nullptr;  // [walkers][n_wg][K][n] (fast path), [walkers][K][n_dirs] (general kernel)
};
hipError_t launch_cc_b(int n, int nb, int n_walkers, int K, double afac, const double *G00, long stride_unit,
                       const int *trg, const double *tst, const double *tts, double *bsum, hipStream_t s);
// one time slice added to per_walker[w][offset + dir12 + n_dirs*k] (already divided by n)
hipError_t launch_cc_slice(const CCPlan &p, int n, int nb, int n_walkers, double afac, double xfac,
                           const double *G0l, const double *Gl0, const double *Gll, long stride_unit,
                           const int *dir_ptr, const int *pair_src, const int *pair_trg, int n_dirs,
                           double *per_walker, long per_stride, long offset, hipStream_t s);
// time-displaced recording (tdm.hip): row `row` of every walker's sample per_walker[w][per_stride], written, not added.
// Green's rows: Gl0[b][row][d] at ((0 nb + b) R + row) n_dirs + d and G0l[b][row][d] at ((1 nb + b) R + row) n_dirs + d,
// each (1/n) sum over the pairs of direction d; fast = one lane per direction over src_of[d + n j] (needs n_dirs == n and
// a complete table), else the pair lists.  minus_identity: G0l - I in the place of G0l (row 0).
hipError_t launch_tdm_greens(bool fast, int n, int nb, int n_walkers, int R, int row, int minus_identity,
                             const double *Gl0, const double *G0l, long stride_unit, const int *src_of,
                             const int *dir_ptr, const int *pair_src, const int *pair_trg, int n_dirs,
                             double *per_walker, long per_stride, hipStream_t s);
// the injective form of the Green's rows: src_of[d + n_dirs j] with -1 where column j has no source in direction d (every
// source and every target meets a direction at most once, n_dirs <= 2 n; chosen by the host where the fast form's Latin
// square test fails); rows of n_dirs entries
hipError_t launch_tdm_greens_inj(int n, int n_dirs, int nb, int n_walkers, int R, int row, int minus_identity,
                                 const double *Gl0, const double *G0l, long stride_unit, const int *src_of,
                                 double *per_walker, long per_stride, hipStream_t s);
// density rows: the per-slice values of sus_pairs_kernel at offset + (q R + row) n_dirs + d, q = CDC, SDCx, SDCy, SDCz
hipError_t launch_tdm_density(int n, int nb, int model, int n_walkers, int R, int row, int minus_identity,
                              const double *G00, const double *G0l, const double *Gl0, const double *Gll,
                              long stride_unit, const int *dir_ptr, const int *pair_src, const int *pair_trg, int n_dirs,
                              double *per_walker, long per_stride, long offset, hipStream_t s);
// logarithmic binning (binner.hip).  Where a push reads its W x E samples: PLAIN = scale * src[w][e]; GREENS = the true
// G of every unit and the occupation 1 - G_ii; CORR = src [w][4 n_dirs] followed by mx, my (zero) and mz from G.
// State: xs, x2 [L][W][E], c [L - 1][W][E]; lmax = trailing 1-bits of the number of pushes so far (< L).
enum { BIN_SRC_PLAIN = 0, BIN_SRC_GREENS = 1, BIN_SRC_CORR = 2 };
struct BinPush {
    int mode = BIN_SRC_PLAIN;
    const double *src = nullptr, *G = nullptr;
    long stride_unit = 0;
    int n = 0, nb = 1, model = 0, n_dirs = 0;
    double scale = 1.0;
    // sign reweighting: s_w per walker (sign.hip).  The GREENS and CORR sources, which read G themselves, then take the
    // signed kernel and push s_w x (0 for s_w = 0); a PLAIN source has been signed where it was written.
    const double *sw = nullptr;
};
hipError_t launch_binner_push(const BinPush &p, int W, int E, int L, int lmax, double *xs, double *x2, double *c,
                              hipStream_t s);
// out [8 E + 1]: mean, std_error, std_error_walkers, tau, sum mean_w, sum mean_w^2, sum varN_w(level), sum varN_w(0), W
hipError_t launch_binner_finish(int W, int E, long T, int level, const double *xs, const double *x2, double *out,
                                hipStream_t s);
// the lattice Fourier transform of a segment of every walker's sample (momentum.hip): for w < n_walkers, row < rows,
// q < n_q:  Y[w y_stride + y_off + row n_q + q] = scale * sum_d X[w x_stride + x_off + row n_dirs + d] tab[d + n_dirs q],
// d in ascending order.  sw != nullptr: the launch also writes Y[w y_stride + sign_at] = sw[w].
struct MomentumArgs {
    const double *X = nullptr, *tab = nullptr, *sw = nullptr;
    double *Y = nullptr;
    long x_stride = 0, x_off = 0, y_stride = 0, y_off = 0, sign_at = 0;
    int rows = 0, n_dirs = 0, n_q = 0;
    double scale = 1.0;
};
hipError_t launch_momentum(const MomentumArgs &a, int n_walkers, hipStream_t s);
// log|det| and sign of I + B_M ... B_1 per unit (logdet.hip): logabsdet = sum_i log D2[i] with D2 the D of the second
// udt_AVX_pivot! of calculate_greens_AVX! (stack.jl:376), sign = sign det A2 of the matrix that UDT factors, from an LU
// with partial pivoting of the copy in A2 (n_units x strideA, destroyed).  One workgroup per unit, fixed summation order.
hipError_t launch_logdet(int n, int n_units, double *A2, long strideA, const double *D2, long strideD, double *logabsdet,
                         int *sign, hipStream_t s);
// DQMC global moves (logdet.hip): per walker, device-resident.  m = moves_drawn is the walker's move counter, the Philox
// counter words of u(m, t) are (t, low32(m), 1, high32(m)).
struct GlobalMoveState {
    unsigned long long moves_drawn;
    long long prop_global, acc_global;
    long long dS;        // sum(conf) - sum(conf') of the pending proposal
    double last_p;       // weight ratio of the latest move
    int active, site, last_accepted, pad_;
};
// kind 0: conf -> -conf, 1: conf[site, :] -> -conf[site, :] with site = min(N - 1, floor(u(m, 0) N)).  walker < 0: all.
hipError_t launch_gm_propose(int N, int M, int n_walkers, int kind, int walker, int8_t *conf, WalkerRng *rng,
                             GlobalMoveState *gm, hipStream_t s);
// accept iff p > 1 || u(m, 1) < p (the uniform drawn only when p <= 1); accepted walkers copy (lad_prop, sg_prop) into
// (lad_cur, sg_cur), rejected ones get their field back
hipError_t launch_gm_decide(int N, int M, int nb, int n_walkers, int kind, double lambda, int check_sign, int8_t *conf,
                            WalkerRng *rng, GlobalMoveState *gm, DevStats *stats, double *lad_cur, int *sg_cur,
                            const double *lad_prop, const int *sg_prop, hipStream_t s);
// sign reweighting (sign.hip).  sw [n_walkers + 2]: s_w as a double (+1, -1, 0: left out), sum_w s_w, walkers kept.
// launch_sign_prepare builds it from the per-unit signs sg [n_walkers][nb] (nullptr: all +1), counts the walkers left
// out in failures [n_walkers] and adds sum_w s_w to *sum_a and, if given, *sum_b.  The signed sums add s_w x_w in the
// order of their unsigned counterparts (launch_accumulate; the reduce steps of launch_correlations, launch_pairing and
// launch_sus_reduce, whose per_walker input they rewrite in place as s_w x_w) and count the walkers kept.
hipError_t launch_sign_prepare(int nb, int n_walkers, const int *sg, double *sw, long long *failures, double *sum_a,
                               double *sum_b, hipStream_t s);
hipError_t launch_accumulate_signed(int n, int nb, int n_walkers, const double *G, long stride_unit, const double *sw,
                                    double *acc, hipStream_t s);
hipError_t launch_corr_reduce_signed(int n, int nb, int model, int n_walkers, const double *G, long stride_unit,
                                     int n_dirs, double *per_walker, const double *sw, double *acc, hipStream_t s);
hipError_t launch_reduce_signed(int n_walkers, long total, double factor, double *per_walker, const double *sw,
                                double *acc, hipStream_t s);
// the pair sums of launch_correlations / launch_pairing alone (per_walker written, acc untouched)
hipError_t launch_correlation_pairs(int n, int nb, int model, int n_walkers, const double *G, long stride_unit,
                                    const int *dir_ptr, const int *pair_src, const int *pair_trg, int n_dirs,
                                    double *per_walker, hipStream_t s);
hipError_t launch_pairing_pairs(int n, int nb, int n_walkers, const double *G, long stride_unit, const int *dir_ptr,
                                const int *pair_src, const int *pair_trg, int n_dirs, int K, const int *trg_of,
                                double *per_walker, hipStream_t s);
// scalar thermodynamics (thermo.hip): the ten elements of include/dqmc_hip.h "thermodynamics" per walker from the true G
// of every unit (G + (w nb + b) stride_unit), written to per_walker[w][per_stride], then the sums into acc
// [10 sums][sum of signs][count].  The hopping matrix comes as a neighbour list: the off-diagonal non-zeros T_ij of row i
// of block b at row_ptr[b n + i] .. row_ptr[b n + i + 1] of col / val, the diagonal in tdiag [nb n].  sw: nullptr, or
// sign.hip's [n_walkers + 2]; then per_walker is rewritten as s_w x, per_walker[w][10] = s_w (per_stride >= 11) and
// acc[10] is left to launch_sign_prepare.
constexpr int DQMC_THERMO_ELEMENTS_K = 10;
hipError_t launch_thermodynamics(int n, int nb, int n_walkers, const double *G, long stride_unit, const int *row_ptr,
                                 const int *col, const double *val, const double *tdiag, double U_s, double *per_walker,
                                 long per_stride, const double *sw, double *acc, hipStream_t s);
// entanglement (entangle.hip; include/dqmc_hip.h "entanglement").  launch_entanglement_gather: G_A and its transpose of
// every (subsystem, unit) from the true G of every unit (G + u stride_unit) into img + img_off[s] + u 2 na^2, sites
// [sub_ptr[s] .. sub_ptr[s + 1]) of `sites`.  launch_entanglement_pairs, one subsystem: lad / sg [n_pairs][nb] get
// sum log|pivot| and sign of det M_b of every pair (w < w', w-major), then sample[W w + w'] = x(w, w') and sums += sample;
// *failures counts the pairs whose sample was set to 0.  entanglement_prepare raises the pair kernel's dynamic LDS limit
// for the largest subsystem (above 64 sites the image is dynamic: entanglement_lds_bytes).
constexpr int DQMC_ENT_MAX_SITES_K = 128;
size_t entanglement_lds_bytes(int na);
hipError_t entanglement_prepare(int na_max);
hipError_t launch_entanglement_gather(int n, int n_units, int n_sub, const double *G, long stride_unit, const int *sub_ptr,
                                      const int *sites, const long *img_off, double *img, hipStream_t s);
hipError_t launch_entanglement_pairs(int na, int nb, int n_walkers, const double *img, double *lad, int *sg, double *sample,
                                     double *sums, unsigned long long *failures, hipStream_t s);
// response.hip: the symmetry-channel contraction of every walker's pairing sample, in front of launch_momentum:
//   Z[w z_stride + c n_dirs + d] = sum_kk F[kk + KK c] X[w x_stride + x_off + d + n_dirs kk],  kk ascending, c < n_ch <= 8
hipError_t launch_pair_channels(int n_dirs, int KK, int n_ch, int n_walkers, const double *X, long x_stride, long x_off,
                                const double *F, double *Z, long z_stride, hipStream_t s);
// and the bond kinetic energy of the current-target columns from the true G of every unit (G + (w nb + b) stride_unit):
//   out[w out_stride + out_off + k] = (fac / n) sum_src [trg >= 0] sum_b tts[b n K + src + n k] (delta_{src,trg} - G_b[src + n trg]),
// trg = trg_of[src + n k], tts = T_b[trg, src] as cc_setup stores it; sw: nullptr, or sign.hip's s_w, then out is s_w x
hipError_t launch_bond_kinetic(int n, int nb, int K, int n_walkers, double fac, const double *G, long stride_unit,
                               const int *trg_of, const double *tts, const double *sw, double *out, long out_stride,
                               long out_off, hipStream_t s);
// current_tau.hip: row `r` of the imaginary-time-resolved current-current recording from one slice's own sums
// x [n_walkers][K][n_dirs] (launch_cc_slice into a zeroed buffer), tab [n_dirs][n_q][2] = (cos, sin) of q . r_d:
//   sums[w sums_stride + off_c + k n_q + q] += s_w sum_d tab[2 (q + n_q d)]     x[(w K + k) n_dirs + d],  d ascending,
//   sums[w sums_stride + off_s + k n_q + q] += s_w sum_d tab[2 (q + n_q d) + 1] x[(w K + k) n_dirs + d]
// (sw == nullptr: s_w = 1; s_w == 0: the walker is left out), and, with add_to != nullptr,
//   add_to[w add_stride + add_off + k n_dirs + d] += x[(w K + k) n_dirs + d]
hipError_t launch_current_tau_row(int n_dirs, int n_q, int K, int n_walkers, const double *x, const double *tab,
                                  const double *sw, double *sums, long sums_stride, long off_c, long off_s,
                                  double *add_to, long add_stride, long add_off, hipStream_t s);
// the end of a recorded pass: sums[w sums_stride + tail + .] = [kbond: K][sum of s_w][samples kept][samples left out]
// take kb [n_walkers][K] (launch_bond_kinetic's, s_w x already), s_w, and one count
hipError_t launch_current_tau_finish(int K, int n_walkers, const double *kb, const double *sw, double *sums,
                                     long sums_stride, long tail, hipStream_t s);
// taucov.hip: one push into the tau-tau' covariance state of n_series series of every walker.  Series sl < n_series of
// this launch is (j, q) = (sl / n_q, sl % n_q); its R values are X[w x_walker + x_off + j j_stride + r r_stride + q] and its
// state a, c, s1 [n_walkers][S][R], s2 [n_walkers][S][R][R] at series series0 + sl of the S the accumulator holds.
// a += x; with close != 0: b = a / bin_size, c = b if first, d = b - c, s1 += d, s2[r][r'] += d[r] d[r'], a = 0.
constexpr int TAUCOV_THREADS = 256;
constexpr int TAUCOV_MAX_R = 2048;   // a series' d lives in LDS (16 KiB)
constexpr int TAUCOV_SMALL_R = 16;   // up to here TAUCOV_SMALL_SPB series share a workgroup, one wave each
constexpr int TAUCOV_SMALL_SPB = 4;
struct TauCovPush {
    const double *X = nullptr;
    long x_walker = 0, x_off = 0, j_stride = 0, r_stride = 0;
    int n_q = 1, R = 0;
    long n_series = 0, series0 = 0, S = 0;
    int close = 0, first = 0;
    double bin_size = 1.0;
    double *a = nullptr, *c = nullptr, *s1 = nullptr, *s2 = nullptr;
};
hipError_t launch_taucov_push(const TauCovPush &p, int n_walkers, hipStream_t s);
// HS field <-> Julia BitArray chunks (compress / decompress, HubbardModel.jl:56-59)
hipError_t launch_conf_pack(const int8_t *conf, size_t n_elem, unsigned long long *chunks, hipStream_t s);
hipError_t launch_conf_unpack(const unsigned long long *chunks, size_t n_elem, int8_t *conf, hipStream_t s);

}  // namespace dqmc
