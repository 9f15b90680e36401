/*
 * dqmc_hip.h — C ABI of libdqmc_hip.so, the MI355X (gfx950) DQMC sweep engine.
 *
 * The reference (ffreyer/MonteCarlo.jl) has no FFI: its plugin surface is Julia
 * dispatch on `Stack <: AbstractDQMCStack` (src/flavors/DQMC/DQMC.jl:133-136,
 * stack.jl:108,242).  This ABI is what a `HIPDQMCStack <: AbstractDQMCStack`
 * would `ccall` (binding text in INTEGRATION.md).  Every entry point names the
 * reference function/state it stands in for.  All paths are relative to the
 * reference repository root.
 *
 * Conventions
 *  - every function returns 0 on success or a negative dqmc_status; the message
 *    is available from dqmc_last_error().  No C++ exception crosses the ABI.
 *  - matrices are IEEE fp64, column-major, exactly as Julia `Matrix{Float64}`;
 *    the HS field is `Array{Int8,2}` (n_sites x slices, column-major, values ±1);
 *    pivots are Int64 and 1-based as in Julia.
 *  - the caller owns every host buffer; the library owns all device memory.
 *  - numerical events (propagation instability, negative determinant ratio) are
 *    counters, not errors, as in the reference (DQMC.jl:4-47).
 *  - a handle drives one device from one host thread.
 *  - "unit" = (walker, block): attractive model 1 block per walker, repulsive
 *    model 2 blocks (spin up / down, src/linalg/blockdiagonal.jl:13-36).  Buffers
 *    documented as "per walker" hold n_blocks consecutive n x n matrices.
 */
#ifndef DQMC_HIP_H
#define DQMC_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dqmc_handle dqmc_handle;

typedef enum {
    DQMC_OK = 0,
    DQMC_ERR_INVALID = -1,  /* bad argument (Julia: error()/@assert, e.g. stack.jl:173) */
    DQMC_ERR_HIP = -2,      /* HIP runtime error */
    DQMC_ERR_NO_DEVICE = -3,
    DQMC_ERR_STATE = -4,    /* call order violated (e.g. sweep before prepare) */
    DQMC_ERR_RNG = -5       /* host-supplied uniform stream exhausted */
} dqmc_status;

enum { DQMC_ATTRACTIVE = 0, DQMC_REPULSIVE = 1 };

/* DQMCParameters (DQMC.jl:52-125) + the model fields the hot path reads
 * (HubbardModelAttractive.jl:26-39, HubbardModelRepulsive.jl:24-41) + the
 * host-computed hopping exponentials (stack.jl:167-181). */
typedef struct {
    int32_t n_sites;                 /* length(lattice) */
    int32_t model_kind;              /* DQMC_ATTRACTIVE / DQMC_REPULSIVE */
    int32_t slices;                  /* mc.p.slices, must be divisible by safe_mult (stack.jl:115) */
    int32_t safe_mult;               /* mc.p.safe_mult */
    int32_t n_walkers;               /* independent Markov chains batched on this device */
    int32_t device_id;
    int32_t check_propagation_error; /* mc.p.check_propagation_error */
    int32_t check_sign_problem;      /* mc.p.check_sign_problem */
    double delta_tau;                /* mc.p.delta_tau */
    double U;                        /* model.U (>= 0, sign carried by model_kind) */
    /* n_blocks consecutive n x n col-major matrices each; copied at create */
    const double *eT;                /* hopping_matrix_exp             = exp(-dtau/2 T) */
    const double *eTinv;             /* hopping_matrix_exp_inv         = exp(+dtau/2 T) */
    const double *eT2;               /* hopping_matrix_exp_squared     */
    const double *eTinv2;            /* hopping_matrix_exp_inv_squared */
    /* dqmc_create tests each block of eT2 and eTinv2 for a Kronecker form when no checkerboard is set and DQMC_NO_KRON
     * is unset; the test is max|E - product of the factors| <= 256 DBL_EPSILON max|E| with E[0,0] > 0.
     *  - n_sites == 256 (dense slab path): E = Ey (x) Ex, the periodic 16 x 16 square lattice (site x + 16 y), with
     *    Ex = E[0:16, 0:16], Ey = E[0::16, 0::16] / E[0,0].
     *  - n_sites == 256, when a block fails that test: E = Ey (x) Ex with unequal factors, the periodic 32 x 8
     *    rectangular lattice (site x + 32 y), with Ex = E[0:32, 0:32], Ey = E[0::32, 0::32][0:8, 0:8] / E[0,0].  That
     *    orientation only: 8 x 32 and 64 x 4 keep the dense path.  Wraps are two launches and the sweep's last chunk is
     *    applied by a flush of its own, as on the triangular path.
     *  - n_sites == 512: E = Ez (x) Ey (x) Ex, the periodic 8 x 8 x 8 cubic lattice (site x + 8 y + 64 z), with
     *    Ex = E[0:8, 0:8], Ey = E[0::8, 0::8][0:8, 0:8] / E[0,0], Ez = E[0::64, 0::64] / E[0,0].
     *  - n_sites == 512, when a block fails that test: E = Ez (x) Ey (x) Ex with a 2 x 2 Ez, the periodic two-layer
     *    16 x 16 x 2 square lattice with interlayer hopping t_perp (site x + 16 y + 256 z, z the layer), with
     *    Ex = E[0:16, 0:16], Ey = E[0::16, 0::16][0:16, 0:16] / E[0,0], Ez = E[0::256, 0::256] / E[0,0].  The two-layer
     *    lattice is factored at L = 16 only; next-nearest-neighbour hopping is not defined on it.
     * When every block passes, slice products and wraps apply the factors instead of the dense matrix
     * (dqmc_kron_hopping reports it); the difference is rounding of the exponential, far inside the 1e-10 tolerance on G.
     * Any other size or hopping keeps the dense products.  The triangular 16 x 16 lattice, which is no Kronecker product,
     * takes its factors through dqmc_set_triangular_factors. */
} dqmc_params;

/* MagnitudeStats (DQMC.jl:4-31): log10 magnitudes */
typedef struct {
    double max, min, sum;
    int64_t count;
} dqmc_magstats;

/* DQMCAnalysis (DQMC.jl:36-47) for one walker */
typedef struct {
    int64_t prop_local, acc_local;
    dqmc_magstats imaginary_probability; /* always empty: the Hubbard models are real (HubbardModel.jl:52) */
    dqmc_magstats negative_probability;
    dqmc_magstats propagation_error;
} dqmc_stats;

/* ---- lifetime ---------------------------------------------------------- */
/* DQMC(model; ...) + init!(mc) + initialize_stack (DQMC.jl:250-289,337-341; stack.jl:108-159) */
int dqmc_create(const dqmc_params *p, dqmc_handle **out);
int dqmc_destroy(dqmc_handle *h);
/* message of the last failing call on this handle (h may be NULL: create errors) */
const char *dqmc_last_error(const dqmc_handle *h);
/* number of visible HIP devices (0 if none); never fails */
int dqmc_device_count(void);

/* ---- state ------------------------------------------------------------- */
/* mc.conf (HubbardModel.jl:4-5,46-48); conf is n_sites x slices Int8 */
int dqmc_set_conf(dqmc_handle *h, int32_t walker, const int8_t *conf);
int dqmc_get_conf(dqmc_handle *h, int32_t walker, int8_t *conf);
/* compress(mc, model, conf) = BitArray(conf .== 1) and decompress = 2c .- 1 (HubbardModel.jl:56-59,
 * used by ConfigRecorder, src/configurations.jl:24-43): the chunks of Julia's BitArray, element i
 * (1-based column-major) in bit (i-1)%64 of chunk (i-1)/64; ceil(n_sites*slices/64) chunks */
int dqmc_get_conf_bits(dqmc_handle *h, int32_t walker, uint64_t *chunks);
int dqmc_set_conf_bits(dqmc_handle *h, int32_t walker, const uint64_t *chunks);
/* RNG feeding `rand() < p` (DQMC.jl:573).  Test mode: a host-supplied uniform
 * stream consumed with the reference's conditional rule (only when p <= 1). */
int dqmc_set_uniforms(dqmc_handle *h, int32_t walker, const double *u, size_t n);
/* Production mode: Philox4x32-10 counter stream, counter = draw index, key = seed */
int dqmc_seed(dqmc_handle *h, int32_t walker, uint64_t seed);
/* number of uniforms consumed so far by a walker */
int dqmc_uniforms_used(dqmc_handle *h, int32_t walker, uint64_t *used);
/* mc.s.current_slice, mc.s.direction (stack.jl:30-31); identical for all walkers */
int dqmc_get_state(dqmc_handle *h, int32_t *current_slice, int32_t *direction);

/* ---- the sweep loop ---------------------------------------------------- */
/* init!, build_stack, propagate (DQMC.jl:412-414) */
int dqmc_prepare(dqmc_handle *h);
/* build_stack only (stack.jl:242-255) */
int dqmc_build_stack(dqmc_handle *h);
/* propagate(mc) (stack.jl:502-631) */
int dqmc_propagate(dqmc_handle *h);
/* sweep_spatial(mc) (DQMC.jl:546-582) with propose_local / accept_local!
 * (HubbardModelAttractive.jl:113-155, HubbardModelRepulsive.jl:128-232) */
int dqmc_sweep_spatial(dqmc_handle *h);
/* update(mc, i) = propagate + sweep_spatial (DQMC.jl:523-538) */
int dqmc_update(dqmc_handle *h);
/* n_sweeps x (2*slices x update), the loop body of run! (DQMC.jl:420-437)
 * without measurements.  Asynchronous work is complete on return. */
int dqmc_sweep(dqmc_handle *h, int32_t n_sweeps);
/* updates until current_slice == 1 && direction == +1 — the measurement point
 * of run! (DQMC.jl:425-436); *n_updates receives the number of updates run */
int dqmc_update_until_measure(dqmc_handle *h, int32_t *n_updates);
/* wait for all queued device work of this handle */
int dqmc_synchronize(dqmc_handle *h);

/* ---- Green's functions -------------------------------------------------- */
/* mc.s.greens: effective G at current_slice, n_blocks x (n x n) */
int dqmc_get_greens_eff(dqmc_handle *h, int32_t walker, double *out);
int dqmc_set_greens_eff(dqmc_handle *h, int32_t walker, const double *in);
/* greens(mc) = eTinv * mc.s.greens * eT (DQMC.jl:721-730) */
int dqmc_get_greens(dqmc_handle *h, int32_t walker, double *out);
/* calculate_greens(mc, slice) from scratch (stack.jl:422-480); runs for all
 * walkers, returns the chosen walker's G.  Overwrites Ul..Tr, curr_U, tmp1/2
 * like the reference; does not touch mc.s.greens or the stack slots. */
int dqmc_calculate_greens_at(dqmc_handle *h, int32_t walker, int32_t slice, double *out);
/* the per-configuration step of replay!(mc) (DQMC.jl:647-653): calculate_greens(mc, slice) from
 * scratch into mc.s.greens for every walker (replay! uses slice = 0), current_slice <- 1 */
int dqmc_replay_greens(dqmc_handle *h, int32_t slice);
/* wrap_greens!(mc, mc.s.greens, slice, direction) on all walkers (stack.jl:491-500) */
int dqmc_wrap_greens(dqmc_handle *h, int32_t slice, int32_t direction);

/* ---- analysis ----------------------------------------------------------- */
int dqmc_get_stats(dqmc_handle *h, int32_t walker, dqmc_stats *out);

/* ---- global moves ----------------------------------------------------------------------------------------------
 * The reference reserves them and leaves them unsupported: DQMCParameters has global_moves and global_rate
 * (DQMC.jl:53-54, 72-73), DQMCAnalysis has prop_global and acc_global (DQMC.jl:40-42), and update(mc, i) carries the
 * hook, commented out (DQMC.jl:526-532).  Here a move changes the whole HS field or one site's time line and is
 * accepted with the ratio of the fermion determinants, from log|det(I + B_M ... B_1)| and its sign per block.
 *
 * calculate_greens_AVX! (stack.jl:337-393) forms G^-1 = (Ul U1) A2 (T1 Ur'), A2 being the matrix of its second
 * udt_AVX_pivot! (:368-376).  With D = |diag R|, T = D^-1 R P' (UDT.jl:270-277) every U is orthogonal and every T has
 * a triangular diagonal of +-1, so log|det G^-1| = sum_i log D2_i (D2 the D of that second UDT), and sign det G^-1 =
 * sign det A2: the chains Ul Dl Tl and Ur Dr Tr are products of B_l = eT2 eV(l) (slice_matrices.jl:23-39), each of
 * positive determinant.  The sign of det A2 comes from an LU with partial pivoting of a copy of A2 (csrc/logdet.hip). */
/* logabsdet[w * n_blocks + b] and sign[...] (+1 / -1; 0: A2 singular or not finite) of I + B_M ... B_1 for the current
 * field of every walker, from scratch: the slice chain of calculate_greens(mc, 0) (stack.jl:422-480).  Overwrites
 * Ul..Tr, curr_U, tmp1/2 like dqmc_calculate_greens_at; does not touch mc.s.greens, the stack slots or current_slice.
 * A unit's values do not depend on the other units of the handle. */
int dqmc_logdet(dqmc_handle *h, double *logabsdet, int32_t *sign);
enum { DQMC_GLOBAL_FLIP_ALL = 0,    /* conf -> -conf */
       DQMC_GLOBAL_FLIP_SITE = 1 }; /* conf[i, :] -> -conf[i, :], i = min(N - 1, floor(u(m, 0) N)) (0-based) */
/* One global move of `walker`, or of every walker when walker < 0 (the place of global_move(mc, mc.model, mc.conf),
 * DQMC.jl:530).  Weight ratio p, from propose_local's conventions: attractive (HubbardModelAttractive.jl:113-127, bosonic
 * weight exp(-lambda sum conf), determinant squared) p = exp(lambda (sum conf - sum conf') + 2 (logabsdet' - logabsdet));
 * repulsive (HubbardModelRepulsive.jl:128-156) p = sign_up' sign_dn' sign_up sign_dn exp(sum_b (logabsdet'_b -
 * logabsdet_b)).  Accepted iff p > 1 || u(m, 1) < p, the uniform drawn only when p <= 1 (DQMC.jl:573); p < 0 is rejected
 * and, with check_sign_problem, pushed to negative_probability (DQMC.jl:562-563).  u(m, t) is Philox4x32-10 with key =
 * the walker's seed and counter words (t, low32(m), 1, high32(m)), m = the walker's moves since dqmc_seed (as
 * dqmc_mc_global_move); the local stream (words 2 and 3 zero) and dqmc_uniforms_used are not touched.  In
 * dqmc_set_uniforms mode the move consumes the host stream instead, in this order: the site uniform (FLIP_SITE only),
 * then the acceptance uniform if p <= 1; these do count in dqmc_uniforms_used.
 * Proposal, decision, the field of each walker and the counters stay on the device.  On return every walker of the
 * handle is in the state dqmc_prepare leaves for its field (accepted: the new one, rejected: the old one): the stack
 * rebuilt, mc.s.greens at current_slice = slices, direction = -1.  The logabsdet of the current field is kept between
 * moves and recomputed when the field has changed in between.  Cost: two slice chains (one if the cache holds) plus
 * dqmc_prepare's stack build.  DQMC_ERR_STATE before dqmc_prepare, DQMC_ERR_INVALID for an unknown kind. */
int dqmc_global_move(dqmc_handle *h, int32_t kind, int32_t walker);
/* mc.p.global_rate with mc.p.global_moves (DQMC.jl:53-54): from now on dqmc_update, dqmc_sweep and
 * dqmc_update_until_measure run one move of `kind` per walker where the reference's hook stands (DQMC.jl:526-532): behind
 * the propagate that reaches current_slice == slices && direction == -1, in front of that slice's sweep_spatial, in
 * every sweep whose index is a multiple of rate.  The sweep index of an update is 1 + (updates since dqmc_prepare) /
 * (2 slices).  rate 0 = off (the default): the sweep is then exactly the one of a handle without global moves.
 * DQMC_ERR_INVALID for rate < 0 or an unknown kind. */
int dqmc_set_global_rate(dqmc_handle *h, int32_t rate, int32_t kind);
/* DQMCAnalysis prop_global / acc_global (DQMC.jl:40-42) of one walker and its move counter m */
typedef struct {
    int64_t prop_global, acc_global;
    uint64_t moves_drawn;
} dqmc_global_stats;
int dqmc_get_global_stats(dqmc_handle *h, int32_t walker, dqmc_global_stats *out);
/* The latest move the walker took part in: its weight ratio p as the device computed it (NaN: a singular or non-finite
 * A2), the decision (1 accepted, 0 rejected) and the site of a FLIP_SITE move (0 for FLIP_ALL).  Before the walker's
 * first move: p = 0, accepted = 0, site = 0. */
int dqmc_get_global_last(dqmc_handle *h, int32_t walker, double *p, int32_t *accepted, int32_t *site);

/* ---- sign reweighting -------------------------------------------------------------------------------------------
 * The reference only reports the sign problem: a negative ratio is pushed to negative_probability (DQMC.jl:562-563) and
 * the measurements go on adding the bare sample (generic.jl:207-215).  Where the weight w of a field is not positive -
 * the repulsive model away from half filling or on a frustrated lattice - that is the average under |w|, not under w.
 * Like the global moves this is a defined extension, off by default: with it on, every accumulator and every binner
 * takes s O in the place of O, s = the sign of the field, next to the sum of s, and <O> = <O s> / <s>.
 * s_w = prod_b sign_b of walker w, sign_b as dqmc_logdet returns it.  The determinant does not change under a cyclic
 * rotation of the slices, so s_w belongs to the field, not to current_slice.  It is taken from the values kept for the
 * global moves (one slice chain when the field has changed since, none otherwise: the dqmc_accumulate_* calls of one
 * measurement point share it).  The attractive model's weight is a square: s_w = +1, no chain is run.  The evaluation
 * leaves the Markov chain alone, as dqmc_logdet does: mc.s.greens, the stack slots, current_slice, the RNG cursors.
 * A unit whose sign comes out 0 (A2 singular or not finite): the walker's sample is left out of every section fed by
 * that call - it is not read, not added with weight 0 to a count - and the walker's counter of dqmc_get_sign_failures
 * goes up by one.  (Its binners, which advance in step for all walkers, take 0 for s x and for s: a pair that changes
 * neither sum of the ratio.)
 * With weighting on: [sum G] becomes [sum s G], [sum G.^2] [sum s G.^2], the occupation [sum s (1 - G_ii)], and so on
 * for every section of "measurement accumulators" ... "time-displaced recording" below; each section's last double stays
 * the plain number of samples (walkers kept).  Walkers are added in the order of the unsigned sums, so that with every
 * s_w = +1 all sums and all binner levels are bit for bit those of a handle with weighting off.  With weighting off
 * nothing is evaluated or launched, and every size, layout and result is that of a handle without it. */
/* on != 0 / 0.  DQMC_ERR_STATE if any section or binner holds samples (dqmc_reset_accumulators first): signed and
 * unsigned sums never mix.  The sums of signs start at zero. */
int dqmc_set_sign_weighting(dqmc_handle *h, int32_t on);
int dqmc_get_sign_weighting(dqmc_handle *h, int32_t *on);
/* s_w (+1 / -1; 0: see above) of every walker's current field, n_walkers entries; works with weighting off too */
int dqmc_get_sign(dqmc_handle *h, int32_t *sign /* n_walkers */);
/* samples left out per walker since dqmc_create (n_walkers entries; dqmc_reset_accumulators does not clear them) */
int dqmc_get_sign_failures(dqmc_handle *h, int64_t *count /* n_walkers */);
/* The section DQMC_RED_SIGN: one sum of s per DQMC_RED_* section in front of it, in enum order (the sections are fed at
 * different times, so each has its own denominator): DQMC_RED_SIGN doubles, no trailing count - a section's own last
 * double is that.  Entry k grows by sum_w s_w with every call that feeds section k (dqmc_accumulate_susceptibilities
 * feeds DQMC_RED_SUSCEPTIBILITIES and, with recording on, DQMC_RED_TIME_DISPLACED); it returns to zero with
 * dqmc_reset_accumulators and when section k is laid out anew.  All zero while weighting is off. */
int dqmc_sign_sums_size(dqmc_handle *h, size_t *n_doubles);
int dqmc_get_sign_sums(dqmc_handle *h, double *host_out);
int dqmc_export_sign_sums(dqmc_handle *h, void *device_out);

/* ---- measurement accumulators (stand-in for push!(LogBinner, greens(mc)),
 * measurements/generic.jl:207-215,260-263).  dqmc_accumulate_greens adds, for
 * every walker of this handle, the true G, G.^2 and the occupation 1-G_ii into
 * device-side sums.  Layout of the accumulator (doubles):
 *   [0 .. B*n*n)            sum G          (B = n_blocks)
 *   [B*n*n .. 2*B*n*n)      sum G.^2
 *   [2*B*n*n .. +B*n)       sum (1 - G_ii)
 *   last                    number of samples                                 */
int dqmc_accumulate_greens(dqmc_handle *h);
int dqmc_accumulator_size(dqmc_handle *h, size_t *n_doubles);
int dqmc_reset_accumulators(dqmc_handle *h);
/* copy accumulators to a host buffer, or device-to-device into a caller-owned
 * device buffer (e.g. a torch tensor that is then all-reduced over RCCL) */
int dqmc_get_accumulators(dqmc_handle *h, double *host_out);
int dqmc_export_accumulators(dqmc_handle *h, void *device_out);

/* ---- equal-time correlation measurements on the device ----------------------
 * cdc_kernel, sdc_{x,y,z}_kernel over EachSitePairByDistance and m{x,y,z}_kernel over EachSite
 * (measurements/measurements.jl:51-190, generic.jl:325-330; HubbardModelAttractive.jl:219-246).
 * dir_of[src + n*trg] (0-based) is the direction index of a pair as produced by
 * EachSitePairByDistance(lattice) (src/lattices/lattice_iterators.jl:157-190).  Accumulator layout:
 *   [cdc n_dirs][sdc_x n_dirs][sdc_y n_dirs][sdc_z n_dirs][mx n][my n][mz n][samples]
 * every pair quantity already divided by n_sites as finish! does (generic.jl:283-286);
 * dqmc_reset_accumulators clears these sums too. */
int dqmc_set_pair_directions(dqmc_handle *h, const int32_t *dir_of, int32_t n_dirs);
int dqmc_accumulate_correlations(dqmc_handle *h);
int dqmc_correlations_size(dqmc_handle *h, size_t *n_doubles);
int dqmc_get_correlations(dqmc_handle *h, double *host_out);
int dqmc_export_correlations(dqmc_handle *h, void *device_out);

/* pc_kernel over EachLocalQuadByDistance{K} (measurements/measurements.jl:199-214, generic.jl:287-290,
 * 341-349, src/lattices/lattice_iterators.jl:258-318; HubbardModelAttractive.jl:243-245):
 * trg_of[src + n*k] (0-based, -1 = none) is the site reached from src in the k-th shortest direction,
 * k < K, i.e. the (dir, trg) lists the iterator builds from EachSitePairByDistance.  Accumulator layout:
 * [n_dirs x K x K] in Julia's column-major order of output[dir12, dir1, dir2], already divided by
 * n_sites, then [samples].  Requires dqmc_set_pair_directions. */
int dqmc_set_local_targets(dqmc_handle *h, const int32_t *trg_of, int32_t K);
int dqmc_accumulate_pairing(dqmc_handle *h);
int dqmc_pairing_size(dqmc_handle *h, size_t *n_doubles);
int dqmc_get_pairing(dqmc_handle *h, double *host_out);
int dqmc_export_pairing(dqmc_handle *h, void *device_out);

/* ---- unequal-time Green's functions -------------------------------------------
 * UnequalTimeStack and its users (src/flavors/DQMC/unequal_time_stack.jl), for all walkers of the
 * handle at once; the sweep state (mc.s.greens, the DQMC stack, current_slice) is not disturbed.
 * The stacks are rebuilt lazily after the HS field has changed (the role of mc.last_sweep, :164-169).
 * Results stay on the device in three n x n x units buffers: `which` = 0 holds G(k,l) of
 * dqmc_ut_greens / the GreensIterator, or G0l of the CombinedGreensIterator; 1 = Gl0; 2 = Gll. */
/* build_stack(mc, mc.ut_stack) (:106-160) */
int dqmc_ut_build_stack(dqmc_handle *h);
/* stack inspection for tests (test/flavortests_DQMC.jl:75-96): which 0 forward, 1 backward, 2 inverse;
 * idx 0-based slot; per walker nb*n*n (U, T) and nb*n (D) doubles */
int dqmc_ut_get_stack(dqmc_handle *h, int32_t w, int32_t which, int32_t idx, double *U, double *D, double *T);
/* calculate_greens(mc, slice1, slice2) (:288-303; full1 :447-530, full2 :534-605) with 0 <= slices <=
 * slices; effective != 0 returns the stack's effective G, 0 applies _greens! (DQMC.jl:721-730) like
 * greens(mc, k, l) (:260-287) */
int dqmc_ut_greens(dqmc_handle *h, int32_t slice1, int32_t slice2, int32_t effective);
int dqmc_ut_get(dqmc_handle *h, int32_t w, int32_t which, double *host_out);
int dqmc_ut_export(dqmc_handle *h, int32_t which, void *device_out /* units*n*n doubles */);
/* GreensIterator(mc, :, l, recalculate) (:644-715): begin computes G(l <- l); each next advances k by one
 * and returns it in *k (-1 when exhausted); result in buffer 0 */
int dqmc_greens_iterator_begin(dqmc_handle *h, int32_t l, int32_t recalculate);
int dqmc_greens_iterator_next(dqmc_handle *h, int32_t *k);
/* CombinedGreensIterator(mc, recalculate) (:746-883): needs current_slice == 1; each next returns
 * l = 1..slices in *l (-1 when exhausted) with (G0l, Gl0, Gll) in buffers 0, 1, 2 */
int dqmc_combined_iterator_begin(dqmc_handle *h, int32_t recalculate);
int dqmc_combined_iterator_next(dqmc_handle *h, int32_t *l);

/* Susceptibilities on the device: apply!(::CombinedGreensIterator, ...) (measurements/generic.jl:226-243)
 * for charge_density_susceptibility, spin_density_susceptibility(:x, :y, :z) and, when
 * dqmc_set_local_targets has been called, pairing_susceptibility (measurements.jl:57-58,142-144,207;
 * packed kernels :76-92,158-192,215-219; HubbardModelAttractive.jl:226-249): the sum over l = 1..slices
 * of kernel(G00, G0l, Gl0, Gll), times delta_tau / n_sites as finish! does.  Needs current_slice == 1
 * and dqmc_set_pair_directions.  Accumulator layout:
 *   [cds n_dirs][sds_x n_dirs][sds_y n_dirs][sds_z n_dirs][ps n_dirs x K x K][ccs, see below][samples]
 * dqmc_reset_accumulators clears these sums too. */
int dqmc_accumulate_susceptibilities(dqmc_handle *h, int32_t recalculate);
int dqmc_susceptibilities_size(dqmc_handle *h, size_t *n_doubles);
int dqmc_get_susceptibilities(dqmc_handle *h, double *host_out);
int dqmc_export_susceptibilities(dqmc_handle *h, void *device_out);

/* current_current_susceptibility (measurements.jl:257-317; attractive override HubbardModelAttractive.jl:250-266)
 * over EachLocalQuadBySyncedDistance{K} (lattice_iterators.jl:360-467): trg_of[src + n*k] = 0-based target of src
 * in direction k < K (-1 if none), as for dqmc_set_local_targets; T = mc.s.hopping_matrix, model_kind's number of
 * n x n column-major blocks (copied).  Needs dqmc_set_pair_directions first.  Once set, every
 * dqmc_accumulate_susceptibilities also sums cc_kernel(G00, G0l, Gl0, Gll) in the same CombinedGreensIterator pass,
 * times delta_tau / n_sites (generic.jl:291-294), and the susceptibility layout above gains a section in front of
 * the sample count:
 *   [cds][sds_x][sds_y][sds_z][ps n_dirs x K_pc x K_pc if local targets][ccs n_dirs x K_cc][samples]
 * ccs in Julia's column-major order of output[dir12, dir_ii].  The reference's identity terms stay out as in
 * measurements.jl:295-309.  dqmc_current_targets_fast_path reports whether the lattice took the LDS kernel
 * (n_dirs == n_sites, one direction per (src1, src2) for each src1, K <= 8) or the general one.
 * dqmc_current_targets_plan reports the launch plan of the LDS kernel (host code only, for tests and tools):
 *   out = [fast, C sources per chunk, umax panel rows, chunks, chunks per workgroup, workgroups per walker,
 *          threads per workgroup, dynamic LDS bytes];
 * all zero when no targets are set or the general kernel is taken. */
int dqmc_set_current_targets(dqmc_handle *h, const int32_t *trg_of, int32_t K, const double *T);
int dqmc_current_targets_fast_path(dqmc_handle *h, int32_t *fast);
int dqmc_current_targets_plan(dqmc_handle *h, int32_t out[8]);

/* ---- time-displaced recording: G(r, tau) and the tau-resolved charge / spin correlations ---------------------------
 * The reference has no such measurement: GreensAt{k,l} gives one (k, l) matrix and its susceptibilities integrate over l
 * (generic.jl:226-243).  Like the global moves this is a defined extension.  Recording is a setting of the handle, as
 * dqmc_set_current_targets is: once set, every dqmc_accumulate_susceptibilities pass also keeps, in the same pass, rows
 * of what its packed kernels see at the slices l = 0, every, 2 every, ..., slices.
 * dqmc_set_time_displaced(h, every, what): every == 0 turns recording off (the default; `what` is then ignored and
 * nothing stays allocated).  Otherwise every >= 1 with slices % every == 0 (so that the row l = slices, tau = beta,
 * exists) and `what` a non-empty mask of DQMC_TD_GREENS | DQMC_TD_DENSITY; anything else returns DQMC_ERR_INVALID and
 * the handle keeps its setting.  Needs dqmc_set_pair_directions (DQMC_ERR_STATE without it); a later
 * dqmc_set_pair_directions rebuilds the layout for the new table.  Every successful call starts the sums at zero.
 * Rows r = 0 .. R-1, R = 1 + slices / every; row r belongs to l = r every, tau = l delta_tau.  Row 0 takes the packed
 * tuple (G00, G0l, Gl0, Gll) = (G00, G00 - I, G00, G00) with G00 = greens!(mc): the -I is the tau -> 0+ limit of
 * G(0, tau) = -<c^dagger(tau) c(0)>, and with it the packed charge and spin kernels are the equal-time kernels term by
 * term (measurements.jl:60-73 against :75-92).  Rows r >= 1 take the tuple the CombinedGreensIterator yields at l.
 * Per-walker sample = element order of the binner section (d fastest, then r, then the block b; N = n_sites):
 *   [if GREENS : Gl0[b][r][d] = (1/N) sum over the pairs (i, j) of direction d of Gl0_b[i, j]    n_blocks R n_dirs
 *                G0l[b][r][d] = (1/N) sum over the pairs (i, j) of direction d of G0l_b[i, j]    n_blocks R n_dirs]
 *   [if DENSITY: CDC[r][d] SDCx[r][d] SDCy[r][d] SDCz[r][d]                                      4 R n_dirs]
 * The DENSITY entries are the per-slice values whose sum over l, times delta_tau, is the cds / sds of the
 * susceptibility layout: divided by N, no delta_tau.  The accumulator has the same layout, holds the sum of the samples
 * over walkers and calls, and ends with [samples]; dqmc_reset_accumulators clears it.
 * Every value is stored from a sum in a fixed order (no atomics): two passes on the same state give the same bits and a
 * walker's sample does not depend on the other walkers.  The Green's rows take one of three kernels (csrc/tdm.hip):
 * where n_dirs == n_sites and every source and every target meets each direction exactly once (translation-invariant
 * tables) a lane owns a direction and walks the columns through a table src_of[d + n_dirs j] built here from dir_of, so
 * that a wave reads within one column (fast = 1); where that test fails but every source and every target still meets
 * a direction at most once and n_dirs <= 2 n_sites (a lattice with a two-site basis: the honeycomb has 3 n / 2
 * directions, n or n / 2 pairs each) the same walk runs over a src_of with -1 where a column has no source in a direction
 * (fast = 2, the injective form); every other table, or any table under DQMC_TDM_GENERAL=1 (read at dqmc_create), takes
 * the pair lists (fast = 0).  The three differ in summation order only.  The division is by N = n_sites in all of them,
 * whatever the pair count of a direction.  dqmc_time_displaced_plan: out = [rows R, every, what, fast (2 / 1 / 0)], all
 * zero when off.
 * With recording off nothing is allocated or launched and every result is bit for bit that of a handle without it; with
 * recording on the pass leaves the susceptibility accumulators, mc.s.greens, the stacks, the HS field and the RNG
 * cursors bit for bit as without. */
enum { DQMC_TD_GREENS = 1, DQMC_TD_DENSITY = 2 };
int dqmc_set_time_displaced(dqmc_handle *h, int32_t every, int32_t what);
/* doubles of the accumulator, sample count included (0 when recording is off) */
int dqmc_time_displaced_size(dqmc_handle *h, size_t *n_doubles);
int dqmc_get_time_displaced(dqmc_handle *h, double *host_out);
int dqmc_export_time_displaced(dqmc_handle *h, void *device_out);
int dqmc_time_displaced_plan(dqmc_handle *h, int32_t out[4]);   /* [rows R, every, what, fast] */

/* ---- error bars: logarithmic binning per walker on the device ------------------------------------------------
 * The observable of a DQMCMeasurement is a BinningAnalysis LogBinner (measurements/generic.jl:35-39, default capacity
 * _default_capacity :68-88), and mean / var / std_error / tau are answered from it (generic.jl:58-61,
 * Measurements.jl:85-88).  Here there is one binner per (walker, scalar element) of a section, L = ceil(log2(capacity +
 * 1)) levels, state on the device as [level][walker][element] for each of x_sum, x2_sum and the one-value compressor:
 * (3 L - 1) * n_walkers * n_elements doubles per section (the top level has no compressor).  push(x), with t pushes
 * before it: for l = 0, 1, ...: x_sum[l] += x, x2_sum[l] += x^2; if bit l of t is 0, keep x in the compressor and stop,
 * else x = (compressor[l] + x) / 2 and go on.  count[l] = floor(T / 2^l) after T pushes, the same for every element:
 * kept on the host.  Per level, n = count[l]: var = x2_sum/(n-1) - x_sum^2/(n(n-1)), varN = var/n, std_error =
 * sqrt(max(varN, 0)), tau = (varN(l)/varN(0) - 1)/2, mean = x_sum[0]/count[0]; NaN errors below two samples.  The
 * reliable level is the last one with count >= 32 (level 0 if there is none).
 * The W walkers of a handle are independent chains: mean = sum_w mean_w / W, std_error = sqrt(sum_w varN_w(l)) / W,
 * tau = (sum_w varN_w(l) / sum_w varN_w(0) - 1)/2, and a second estimate that needs no binning, std_error_walkers =
 * sqrt(sum_w (mean_w - mean)^2 / (W (W - 1))) (NaN for W = 1).
 * Sections and their element order (the accumulator layouts above without the trailing sample count):
 *   DQMC_BIN_GREENS            [G: B*n*n][1 - G_ii: B*n]   (no G.^2 block: the binner supersedes it)
 *   DQMC_BIN_CORRELATIONS      [cdc][sdc_x][sdc_y][sdc_z][mx][my][mz]
 *   DQMC_BIN_PAIRING           [n_dirs x K x K]
 *   DQMC_BIN_SUSCEPTIBILITIES  [cds][sds_x][sds_y][sds_z][ps if local targets][ccs if current targets]
 *   DQMC_BIN_USER              n_elements samples per walker supplied by the caller
 *   DQMC_BIN_TIME_DISPLACED    the per-walker sample of "time-displaced recording" above (pushed by
 *                              dqmc_accumulate_susceptibilities, which checks the room of both of its sections first)
 * Once a section is enabled, its dqmc_accumulate_* call also pushes every walker's sample, read in place from the
 * buffers the measurement kernels leave behind, after those kernels and on the same stream; the accumulators receive
 * exactly what they receive without a binner.  A push beyond the capacity fails with DQMC_ERR_STATE before anything is
 * accumulated (the reference: OverflowError).  dqmc_reset_accumulators clears the binners too.  With no binner enabled
 * nothing is allocated or launched. */
enum { DQMC_BIN_GREENS = 0, DQMC_BIN_CORRELATIONS = 1, DQMC_BIN_PAIRING = 2, DQMC_BIN_SUSCEPTIBILITIES = 3,
       DQMC_BIN_USER = 4 };
/* (an enum of its own: the five sections above are a closed list for hosts that enumerate them).  Enabling it needs
 * dqmc_set_time_displaced and dqmc_prepare.  Memory: (3 L - 1) n_walkers E doubles, E = (2 n_blocks + 4) R n_dirs with
 * both parts - choose `every` and the capacity with that in mind. */
enum { DQMC_BIN_TIME_DISPLACED = 5 };
/* LogBinner(zero, capacity = capacity) for every walker and element of a measurement section (generic.jl:39);
 * capacity 0 = 100000.  The section's measurement must be configured (pair directions, local / current targets; the
 * susceptibilities also need dqmc_prepare); if its layout changes afterwards, enable again.  Enabling again starts anew. */
/* With sign weighting on, every section pushes s_w x, and s_w itself goes into a one-element binner of its own per
 * section, DQMC_BIN_SIGN + k for the section with DQMC_RED_* index k (sections are pushed at different times, so each has
 * its own push count).  It is made with the section's binner (dqmc_binner_enable, or dqmc_set_sign_weighting for the
 * binners enabled before it), has its capacity and push count, and is read like any other binner; it cannot be enabled
 * on its own.  The error of a ratio <O s> / <s> is the host's to form, from level 0 of both (dqmc.py: signed()). */
enum { DQMC_BIN_SIGN = 6 };
int dqmc_binner_enable(dqmc_handle *h, int32_t which, int64_t capacity);
/* elements per walker, levels and pushes so far (length(obs), BinningAnalysis' count at level 0) */
int dqmc_binner_size(dqmc_handle *h, int32_t which, size_t *n_elements, int32_t *n_levels, int64_t *n_pushed);
/* the level std_error(obs) and tau(obs) use (generic.jl:60-61): the last one with at least 32 entries */
int dqmc_binner_reliable_level(dqmc_handle *h, int32_t which, int32_t *level);
/* x_sum and x2_sum (n_elements doubles each, either may be NULL) and the count of one level of one walker */
int dqmc_binner_get_level(dqmc_handle *h, int32_t which, int32_t walker, int32_t level,
                          double *x_sum, double *x2_sum, int64_t *count);
/* mean(m), std_error(m), tau(m) (generic.jl:58-61) over the walkers of the handle at `level` (< 0: the reliable one),
 * plus the cross-walker error; host buffers of n_elements doubles, any may be NULL */
int dqmc_binner_finish(dqmc_handle *h, int32_t which, int32_t level,
                       double *mean, double *std_error, double *std_error_walkers, double *tau);
/* the additive moments behind dqmc_binner_finish into a caller-owned device buffer of 4 * n_elements + 1 doubles:
 * [sum_w mean_w][sum_w mean_w^2][sum_w varN_w(level)][sum_w varN_w(0)][W].  A multi-rank host sums the whole buffer over
 * its ranks (same level everywhere) and applies the formulas above with W = the last entry. */
int dqmc_binner_export_moments(dqmc_handle *h, int32_t which, int32_t level, void *device_out);
/* a binner over samples the caller computes on the device (an observable of its own): create, then push a device
 * buffer [n_walkers][n_elements] per sample.  The buffer must be complete when the call is made; the call returns when
 * it has been read. */
int dqmc_binner_user_create(dqmc_handle *h, int64_t n_elements, int64_t capacity);
int dqmc_binner_user_push(dqmc_handle *h, const double *device_samples);

/* ---- momentum-space observables: S(q), chi(q), G(k, tau) with error bars ----------------------------------------
 * The reference measures per direction only; users of a Hubbard DQMC report the lattice Fourier transforms.  Like the
 * time-displaced recording this is a defined extension.  The transform is linear, so the momentum-space MEANS are the
 * host's to form from the existing accumulators and a phase table (dqmc.py: structure_factors, static_susceptibilities,
 * momentum_time_displaced) and need nothing here.  Their ERROR BARS need the covariances between directions, which no
 * binner keeps: so the transform is applied to every walker's sample on the device and the result is binned.
 * dqmc_set_momenta(h, n_q, cos_tab, sin_tab): the tables are [n_dirs x n_q] doubles, d fastest (element d + n_dirs q),
 * and are copied to the device.  n_q == 0 turns the feature off and frees everything (the default; the tables are then
 * ignored); otherwise 1 <= n_q <= n_dirs and both tables non-NULL, anything else returns DQMC_ERR_INVALID and the
 * handle keeps its setting.  Needs dqmc_set_pair_directions (DQMC_ERR_STATE without it); a later
 * dqmc_set_pair_directions turns momenta off, because the tables no longer fit.  Every successful call frees the three
 * binners below; the caller enables them again.
 * The engine attaches no meaning to the tables.  The convention of this header and of dqmc.py: C[d, q] = cos(q . r_d),
 * S[d, q] = sin(q . r_d) with r_d the displacement of direction d, pos[src] - pos[trg] under the minimum image
 * (EachSitePairByDistance.directions), so that sum_d e^{-i q . r_d} X[d] = Cpart[q] - i Spart[q] with
 *   Cpart[q] = sum_d X[d] C[d, q],  Spart[q] = sum_d X[d] S[d, q],  d in ascending order (csrc/momentum.hip).
 * The three binner sections, enabled with dqmc_binner_enable(h, which, capacity) and read with dqmc_binner_size,
 * _reliable_level, _get_level, _finish and _export_moments like any other; per-walker sample, q fastest:
 *   DQMC_BIN_MOMENTUM_CORRELATIONS      fed by dqmc_accumulate_correlations: [Sc][Sx][Sy][Sz], n_q each: Cpart of cdc,
 *                                       sdc_x, sdc_y, sdc_z.  E = 4 n_q
 *   DQMC_BIN_MOMENTUM_SUSCEPTIBILITIES  fed by dqmc_accumulate_susceptibilities: [chi_c][chi_x][chi_y][chi_z], n_q each:
 *                                       Cpart of cds, sds_x, sds_y, sds_z, times delta_tau as that section's binner
 *                                       takes them.  E = 4 n_q.  Needs dqmc_prepare, as its source does
 *   DQMC_BIN_MOMENTUM_TIME_DISPLACED    fed by dqmc_accumulate_susceptibilities while recording is on; needs
 *                                       dqmc_set_time_displaced.  If GREENS: [Gl0 C][Gl0 S][G0l C][G0l S], each
 *                                       n_blocks R n_q (q fastest, then r, then the block): Cpart and Spart of the rows
 *                                       Gl0[b][r][.] and G0l[b][r][.]; if DENSITY: [CDC][SDCx][SDCy][SDCz], each R n_q,
 *                                       Cpart only.  E = (4 n_blocks + 4) R n_q with both parts
 * The density-type rows take the cosine only: their Wick expressions are symmetric under i <-> j, so X[d] = X[-d] in
 * every sample and the sine part is rounding noise.  The pairing and current-current sums (ps, ccs) have binners of their
 * own: "pair structure factors and superfluid stiffness" below.
 * Memory per binner: (3 L - 1) n_walkers E doubles, as for every section: a momentum binner over n_q momenta is n_q /
 * n_dirs (Green's rows: 2 n_q / n_dirs) of the real-space one.
 * A momentum binner is pushed on the handle's stream behind the source section's kernels, whether or not the source
 * section's own binner is enabled; the room of every binner of a call is checked before anything is accumulated
 * (DQMC_ERR_STATE when a capacity would be passed); dqmc_reset_accumulators clears them.  The sample is the transform of
 * exactly what the source section's binner receives.  Enabling one before dqmc_set_momenta (the time-displaced one:
 * before dqmc_set_time_displaced) returns DQMC_ERR_STATE; dqmc_set_momenta or, for the time-displaced one,
 * dqmc_set_time_displaced called afterwards disables it.
 * Sign weighting: the sources are s_w x already where the transform reads them, and the momentum sample has one more
 * element at its end, s_w itself (E grows by 1: dqmc_binner_size reports it), so that the host forms <s O~> / <s> and
 * its jackknife over the walkers from level 0 of this one binner; there is no DQMC_BIN_SIGN + k for these sections.
 * dqmc_set_sign_weighting re-creates the momentum binners that were enabled before it, empty, with their capacities.
 * Every output element is one dot product summed in a fixed order with no atomics: a second pass on the same state gives
 * the same bits, and a walker's sample depends neither on n_walkers nor on the other rows.  There is no DQMC_RED_*
 * section for momenta: with no momentum binner enabled nothing is allocated beyond the two tables, nothing is launched,
 * and every result, reduction buffer and state blob is byte for byte that of a handle that never called
 * dqmc_set_momenta.  dqmc_momenta_plan: out = [n_q, n_dirs, tile rows, tile columns of the kernel], zeros when off. */
enum { DQMC_BIN_MOMENTUM_CORRELATIONS = 11, DQMC_BIN_MOMENTUM_SUSCEPTIBILITIES = 12, DQMC_BIN_MOMENTUM_TIME_DISPLACED = 13,
       DQMC_BIN_MOMENTUM_END = 14 };
int dqmc_set_momenta(dqmc_handle *h, int32_t n_q, const double *cos_tab, const double *sin_tab);
int dqmc_momenta_plan(dqmc_handle *h, int32_t out[4]);   /* [n_q, n_dirs, tile rows, tile cols], zeros when off */

/* ---- tau-tau' covariance of G(k, tau) and of the tau-resolved correlations ----------------------------------------
 * A binner keeps each element's own variance.  An analytic continuation of G(k, tau) needs the covariance between the
 * time slices of one momentum, which no binner holds: data of one Markov chain are strongly correlated between
 * neighbouring tau.  The reference has no such measurement; this is a defined extension.
 * A SERIES is the R values along tau of one (row group, block or channel, q) of the DQMC_BIN_MOMENTUM_TIME_DISPLACED
 * sample above.  dqmc_set_tau_covariance(h, bin_size, what): `what` is a non-empty mask of DQMC_TD_GREENS (the [Gl0 C]
 * rows, Re G(k, tau): series b n_q + q, b < n_blocks) and DQMC_TD_DENSITY ([CDC][SDCx][SDCy][SDCz]: series
 * (channel) n_q + q behind the Green's series, if any), S = (n_blocks [GREENS] + 4 [DENSITY]) n_q series in all; bin_size
 * >= 1 consecutive samples are averaged into one bin.  bin_size == 0 turns it off and frees everything (the default).
 * DQMC_ERR_INVALID for bin_size < 0 or a mask that is empty or has other bits; DQMC_ERR_STATE before dqmc_set_momenta or
 * dqmc_set_time_displaced, for rows the recording does not hold, and with sign weighting on (the sample is then s x, and
 * the covariance of a ratio is another estimator); the handle keeps its setting.  Whatever frees the momentum
 * time-displaced binner (dqmc_set_momenta, dqmc_set_pair_directions, dqmc_set_time_displaced) turns it off, and so does
 * switching sign weighting on.  The momentum binner itself need not be enabled: the accumulator then runs the same
 * transform into a sample of its own.
 * State per walker w and series s: the open bin's sum a[R], a shift c[R], S1[R], S2[R][R] (row-major, full), and the
 * number of closed bins.  Once per dqmc_accumulate_susceptibilities pass, on the handle's stream behind the momentum
 * binner's push, with x the series of the pass's sample:
 *     a += x;  and when the pass is the bin_size-th of its bin:
 *     b = a / bin_size;  c = b if it is the walker's first bin;  d = b - c;  S1 += d;  S2[r][r'] += d[r] d[r'];  a = 0.
 * The samples of an unfinished bin are part of no result.  The mean of the bins is c + S1 / nb and their scatter matrix
 * S2 - S1 S1^T / nb (dqmc.py: tau_covariance_from_moments pools walkers and ranks).  The shift is part of the definition:
 * G(k, tau) is O(1) with errors of 1e-3 and below, so the unshifted sum of products minus the product of means would
 * cancel six and more digits, and an eigendecomposition that keeps modes down to 1e-10 of the largest would weight that
 * loss by 1 / lambda.  With the shift the sums hold deviations only.
 * Every stored value is one accumulator, updated once per closed bin in ascending order with no atomics: the state
 * depends on the walker's samples only, a second run gives the same bits, and S2 is exactly symmetric (the two products
 * commute).  csrc/taucov.hip: one workgroup per (walker, series), four series per workgroup for R <= 16; a pass that
 * closes no bin touches R doubles per series, a closing one streams S2 once (2 R^2 doubles per series).  R <= 2048.
 * Memory: n_walkers S (R^2 + 3 R) doubles, and the n_walkers E doubles of the sample.  A failed allocation returns the
 * HIP error and leaves the feature off.  dqmc_tau_covariance_plan: out = [bin_size, S, R, bytes, closed bins], zeros when
 * off.  dqmc_tau_covariance_get copies the moments to the host: n_bins [n_walkers], shift, S1 [n_walkers][S][R], S2
 * [n_walkers][S][R][R]; any may be NULL; DQMC_ERR_STATE when off.  dqmc_reset_accumulators clears everything, the open
 * bin and the shifts included.  The moments are not part of the state blob: a checkpoint of a handle with the
 * accumulator on would lose them, and the host refuses to write one (dqmc.py: save).  With the accumulator off nothing is
 * allocated or launched, and every result, reduction buffer and state blob is byte for byte that of a handle that never
 * called dqmc_set_tau_covariance; with it on every other result still is.
 * The same kernel on samples of the caller's (an observable of its own), as dqmc_binner_user_create / _push:
 * dqmc_user_covariance(h, n_series, R, bin_size) (bin_size == 0: off; DQMC_ERR_INVALID for n_series < 1, R < 1,
 * R > 2048, bin_size < 0), then per sample dqmc_user_covariance_push with a device buffer [n_walkers][n_series][R],
 * complete when the call is made; the call returns when it has been read.  _plan and _get as above. */
int dqmc_set_tau_covariance(dqmc_handle *h, int32_t bin_size, int32_t what);
int dqmc_tau_covariance_plan(dqmc_handle *h, int64_t out[5]);
int dqmc_tau_covariance_get(dqmc_handle *h, int64_t *n_bins, double *shift, double *S1, double *S2);
int dqmc_user_covariance(dqmc_handle *h, int64_t n_series, int32_t R, int32_t bin_size);
int dqmc_user_covariance_push(dqmc_handle *h, const double *device_samples);
int dqmc_user_covariance_plan(dqmc_handle *h, int64_t out[5]);
int dqmc_user_covariance_get(dqmc_handle *h, int64_t *n_bins, double *shift, double *S1, double *S2);

/* ---- measurement reduction over ranks -------------------
 * One process (or thread) per GPU; walkers never interact, the only collective is the reduction of the measurement
 * sums every `measure_rate` sweeps (DQMC.jl:429-436).  dqmc_reduce packs EVERY accumulator of the handle (Green's
 * function sums, correlations, pairing, susceptibilities - whichever are configured) and the DQMCAnalysis counters
 * of its walkers (prop_local, acc_local, MagnitudeStats sum / count / max / min, DQMC.jl:4-47) into one device
 * buffer [sums | 2 maxima | 2 minima] and runs ncclAllReduce (sum, max, min) over RCCL on the handle's stream.
 * The global sums are read with dqmc_get_reduced (section by section, same layouts and sizes as the local getters)
 * and the global counters with dqmc_get_reduced_stats.  The handle's own accumulators are NOT modified - they keep
 * the local sums - so the reduction may be repeated at every measurement interval (each call reduces the sums
 * accumulated so far since the last dqmc_reset_accumulators).
 * comm == NULL reduces over the walkers of this handle only.  A host that brings its own collective (MPI from
 * Julia, gloo in this repository's tests) uses dqmc_reduce_export -> reduce (sums, then maxima, then minima; layout
 * above) -> dqmc_reduce_import instead. */
typedef struct dqmc_comm dqmc_comm;
/* ncclGetUniqueId on rank 0 (128 bytes), to be broadcast by the host's own means */
int dqmc_comm_unique_id(void *id128);
/* ncclCommInitRank on device_id (collective: every rank calls it with the same id) */
int dqmc_comm_init(const void *id128, int32_t nranks, int32_t rank, int32_t device_id, dqmc_comm **out);
int dqmc_comm_destroy(dqmc_comm *c);
int dqmc_reduce(dqmc_handle *h, dqmc_comm *comm);
int dqmc_reduce_size(dqmc_handle *h, size_t *n_doubles /* sums + 4 */);
int dqmc_reduce_export(dqmc_handle *h, double *host_out);
int dqmc_reduce_import(dqmc_handle *h, const double *host_in);
enum { DQMC_RED_GREENS = 0, DQMC_RED_CORRELATIONS = 1, DQMC_RED_PAIRING = 2, DQMC_RED_SUSCEPTIBILITIES = 3 };
/* With recording on (dqmc_set_time_displaced) the E = dqmc_time_displaced_size - 1 sums are packed behind the
 * susceptibilities, in front of the counters: dqmc_reduce_size grows by exactly E; with recording off the buffer is byte
 * for byte the one above.  The sample count is not packed a second time: the passes that record are the passes that feed
 * the susceptibilities, so dqmc_get_reduced(DQMC_RED_TIME_DISPLACED) returns [E reduced sums][reduced susceptibility
 * samples], dqmc_time_displaced_size doubles.  It returns DQMC_ERR_STATE when the two local counts differed at the
 * reduction, i.e. recording was (re)set after susceptibility passes with no dqmc_reset_accumulators since. */
enum { DQMC_RED_TIME_DISPLACED = 4 };
/* With sign weighting on (dqmc_set_sign_weighting) the DQMC_RED_SIGN sums of signs are packed behind the time-displaced
 * rows, in front of the counters: dqmc_reduce_size grows by exactly DQMC_RED_SIGN; with weighting off the buffer is byte
 * for byte the one above and dqmc_get_reduced(DQMC_RED_SIGN) returns DQMC_ERR_STATE. */
enum { DQMC_RED_SIGN = 5 };
int dqmc_get_reduced(dqmc_handle *h, int32_t which, double *host_out);
int dqmc_get_reduced_stats(dqmc_handle *h, dqmc_stats *out);

/* ---- thermodynamics ---------------------------------------------------------------------------------------------------
 * Energy, filling, double occupancy, local moment and the fluctuations behind the compressibility and the uniform spin
 * susceptibility, as ten scalars per sample.  The reference has no such measurement: its `occupation` is the per-site
 * vector of the Green's section, and <n_up n_dn>, <N^2>, <Mz^2> are products of Green's elements inside one sample, which
 * the mean G does not give.  Off by default; a handle that never calls dqmc_set_thermodynamics launches, packs and saves
 * exactly what it did before this section existed.
 * Notation: G_s the true equal-time Green's function of block s for one walker's field (dqmc_get_greens; G_ij =
 * <c_i c+_j>), for the attractive model (one block) G_up = G_dn = G and spin sums count the block twice; T_s the hopping
 * matrix of block s (mc.s.hopping_matrix, -mu on its diagonal); N = n_sites; n_s,i = 1 - G_s,ii; U_s = +U for the
 * repulsive model, -U for the attractive one: the interaction is U_s sum_i (n_up,i - 1/2)(n_dn,i - 1/2).
 *   0 n_up   (1/N) sum_i n_up,i                      1 n_dn   (1/N) sum_i n_dn,i
 *   2 n      n_up + n_dn                             3 D      (1/N) sum_i n_up,i n_dn,i
 *   4 m2     n - 2 D  (the local moment <(n_up - n_dn)^2>)
 *   5 E_kin  (1/N) sum_s sum_{i != j} T_s,ij (-G_s,ji)
 *   6 E_int  U_s (D - n/2 + 1/4)
 *   7 E      (1/N) sum_s sum_ij T_s,ij (delta_ij - G_s,ji) + E_int     (the -mu n term is in)
 *   8 N2     (1/N) [ (sum_s sum_i n_s,i)^2 + sum_s sum_ij (delta_ij - G_s,ji) G_s,ij ]  = <N^2> / N
 *   9 Mz2    (1/N) [ (sum_i (n_up,i - n_dn,i))^2 + sum_s sum_ij (delta_ij - G_s,ji) G_s,ij ]  = <(sum_i n_up,i - n_dn,i)^2> / N
 * 8 and 9 use the Wick contraction of cdc_kernel / sdc_z_kernel (measurements.jl:60-74, 180-186) summed over all pairs.
 * The linear combinations 2, 4, 6, 7 are elements of their own so that a binner gives their error bars without a
 * covariance.  The host derives kappa = beta (<N2> - N <n>^2) and chi_s = beta <Mz2> / 4.
 * The section DQMC_RED_THERMODYNAMICS: [10 sums][sum of s][sample count], DQMC_THERMO_ELEMENTS + 2 doubles.  It carries
 * its own sum of signs, so the DQMC_RED_SIGN section keeps its five entries; the sum of s equals the count while sign
 * weighting is off, and with it on the ten sums are sums of s_w x_w, a walker whose sign is 0 is left out of all twelve
 * and counted in dqmc_get_sign_failures.  dqmc_reset_accumulators zeroes it, dqmc_set_sign_weighting refuses while it
 * holds samples, and dqmc_reduce packs it behind the sums of signs (dqmc_get_reduced(DQMC_RED_THERMODYNAMICS)).
 * The binner DQMC_BIN_THERMODYNAMICS (dqmc_binner_enable, after dqmc_set_thermodynamics): E = 10, or with sign weighting
 * on E = 11, the sample being [s_w x_w][s_w] as for the momentum binners, so that the jackknife of <x s> / <s> has its
 * denominator in the same binner; there is no DQMC_BIN_SIGN + k for it.  Switching sign weighting makes it again, empty,
 * with its capacity.
 * A walker's sample is summed in a fixed order without atomics: the same bits in every run and for any n_walkers.
 * Checkpoint: see "checkpoint and resume", format versions 3 and 4. */
enum { DQMC_RED_THERMODYNAMICS = 6 };
enum { DQMC_BIN_THERMODYNAMICS = 14 };  /* = DQMC_BIN_MOMENTUM_END: behind the momentum binners */
enum { DQMC_THERMO_ELEMENTS = 10 };
/* The reference has no such measurement.  T: mc.s.hopping_matrix as dqmc_set_current_targets takes it, n_blocks matrices
 * n x n, column-major; the engine keeps it as a per-row neighbour list.  NULL turns the section off again: its sums and
 * its binner go.  DQMC_ERR_INVALID for a non-finite entry or a row with more than 64 off-diagonal non-zeros, and the
 * handle keeps its setting.  A call with a matrix empties the section and drops its binner. */
int dqmc_set_thermodynamics(dqmc_handle *h, const double *T);
/* The reference has no such measurement.  One sample per walker from the true G of the current fields, at the place
 * dqmc_accumulate_greens is called.  DQMC_ERR_STATE before dqmc_prepare or dqmc_set_thermodynamics. */
int dqmc_accumulate_thermodynamics(dqmc_handle *h);
/* size / host copy / device copy of the section, as for the other sections (0 doubles while it is off) */
int dqmc_thermodynamics_size(dqmc_handle *h, size_t *n_doubles);
int dqmc_get_thermodynamics(dqmc_handle *h, double *host_out);
int dqmc_export_thermodynamics(dqmc_handle *h, void *device_out);

/* ---- pair structure factors and superfluid stiffness: P_c(q), its susceptibility, Lambda_kk(q), the bond kinetic energy ----
 * The reference measures the pairing sums per (direction, k1, k2) and the current-current sums per (direction, k) only
 * and leaves the superfluid stiffness as a comment (measurements.jl:223-256).  Like the momentum binners this is a
 * defined extension, and like them it exists for the ERROR BARS: the means are host transforms of the existing sums
 * (dqmc.py: pair_structure_factors, pair_susceptibilities, current_response, superfluid_stiffness).
 * dqmc_set_pair_channels(h, n_ch, F): F is [K*K x n_ch] doubles, kk = k1 + K k2 fastest (element kk + K*K c), K the K of
 * dqmc_set_local_targets; the engine attaches no meaning to it (dqmc.py: F[kk, c] = f_c[k1] f_c[k2], f_c the weights of
 * symmetry channel c over the local-target directions).  Needs dqmc_set_local_targets (DQMC_ERR_STATE without it).
 * n_ch == 0 turns the channels off and frees everything (F is then ignored); 1 <= n_ch <= 8 with F non-NULL turns them
 * on; anything else returns DQMC_ERR_INVALID and the handle keeps its setting.  A later dqmc_set_local_targets turns them
 * off.  Every successful call frees the two pairing binners below.
 * With Cpart / Spart the transforms of dqmc_set_momenta, per-walker samples, q fastest:
 *   DQMC_BIN_RESPONSE_PAIRING                 fed by dqmc_accumulate_pairing: [P cos: n_ch n_q][P sin: n_ch n_q], the Cpart
 *                                             and Spart of Z[c][d] = sum_kk F[kk, c] X[d + n_dirs kk], kk ascending, X the
 *                                             pairing sample.  E = 2 n_ch n_q.  Needs the channels and the momenta
 *   DQMC_BIN_RESPONSE_PAIRING_SUSCEPTIBILITY  the same of the ps part of the susceptibility sample, times delta_tau as
 *                                             that section's binner takes it; fed by dqmc_accumulate_susceptibilities.
 *                                             Needs dqmc_prepare as well
 *   DQMC_BIN_RESPONSE_CURRENT                 fed by dqmc_accumulate_susceptibilities: [Lambda cos: K_cc n_q][Lambda sin:
 *                                             K_cc n_q][kbond: K_cc]: the Cpart and Spart of the K_cc rows ccs[. + n_dirs k]
 *                                             times delta_tau, then the bond kinetic energy of the same sample,
 *                                               kbond[k] = (1/N) sum_src [trg >= 0] sum_sigma T_sigma[trg, src]
 *                                                          (delta_{src,trg} - G_sigma[src, trg]),   trg = trg_of[src + n k],
 *                                             with G the G00 of the pass and trg_of, T those of dqmc_set_current_targets;
 *                                             the spin sum counts the attractive model's one block twice, as E_kin of
 *                                             "thermodynamics" does.  E = 2 K_cc n_q + K_cc.  Needs dqmc_set_current_targets,
 *                                             the momenta and dqmc_prepare
 * Sign convention of the stiffness (fixed on free fermions, tests/response_ref.py): with k_x = kbond[+x] + kbond[-x]
 * (negative) and C_xx(q) = the Cpart of the row k = +x as this binner holds it.  The reference's cc_kernel sums <J J> of
 * J = T c+ c - h.c. without the factor i of the current j = i J, so ccs carries i^2 = -1: C_xx(q) <= 0, and its
 * longitudinal limit C_xx(q_x -> 0, q_y = 0) tends to +k_x.  The current response of the stiffness formula is
 * Lambda_xx(q) = -C_xx(q), whose longitudinal limit tends to -k_x > 0:
 *   rho_s = (-k_x - Lambda_xx(q_x = 0, q_y -> 0)) / 4 = (-k_x + C_xx(q_x = 0, q_y -> 0)) / 4,
 *   Drude weight = -k_x - Lambda_xx(q_x -> 0, q_y = 0) = -k_x + C_xx(q_x -> 0, q_y = 0).
 * ccs and this binner's sample stay as cc_kernel gives them; the minus sign is the host's (dqmc.py: superfluid_stiffness).
 * Everything else is as for the momentum binners: enabled with dqmc_binner_enable (DQMC_ERR_STATE when the momenta or the
 * source's configuration is missing), pushed on the handle's stream behind the source's kernels whether or not the source's
 * own binner is on, the room of every binner of a call checked before anything is accumulated, cleared by
 * dqmc_reset_accumulators, read with dqmc_binner_size, _reliable_level, _get_level, _finish and _export_moments.
 * dqmc_set_momenta and dqmc_set_pair_directions free all three, dqmc_set_pair_channels and dqmc_set_local_targets the two
 * pairing ones, dqmc_set_current_targets the current one.  With sign weighting the sources are s_w x already (kbond is
 * multiplied by s_w here), the sample gains a trailing s_w and dqmc_set_sign_weighting re-creates the binners empty.
 * Every element is one sum in a fixed order with no atomics: a second pass gives the same bits, and a walker's sample does
 * not depend on n_walkers.  There is no DQMC_RED_* section: with none of the three binners enabled nothing is launched and
 * every accumulator, reduction buffer and state blob is byte for byte that of a handle that never called
 * dqmc_set_pair_channels.  Memory per binner: (3 L - 1) n_walkers E doubles.  Checkpoint: format versions 5 - 8. */
enum { DQMC_BIN_RESPONSE_PAIRING = 15, DQMC_BIN_RESPONSE_PAIRING_SUSCEPTIBILITY = 16, DQMC_BIN_RESPONSE_CURRENT = 17,
       DQMC_BIN_RESPONSE_END = 18 };
int dqmc_set_pair_channels(dqmc_handle *h, int32_t n_ch, const double *F /* [K*K x n_ch], kk fastest */);
int dqmc_response_plan(dqmc_handle *h, int32_t out[4]);  /* [n_ch, K, K_cc, n_q], zeros where unset */

/* ---- entanglement: the second Renyi entropy from walker pairs ------------------------------------------------------
 * The reference, a single-chain code, has no such measurement: it needs independent Markov chains at the same
 * parameters, which is what the walker batch is.  Grover's estimator (T. Grover, PRL 111, 130402): for a subsystem
 * A = (a_0 .. a_{N_A - 1}) of distinct 0-based sites, taken in the order given, and every pair of walkers w < w',
 *   M_b(w, w') = I - G_A^(w,b) - G_A^(w',b) + 2 G_A^(w,b) G_A^(w',b)                      (N_A x N_A)
 *   x(w, w')   = prod_b det M_b(w, w')       repulsive model (two blocks: up, down)
 *   x(w, w')   = (det M_0(w, w'))^2          attractive model (both spin species share the one block)
 * G_A^(w,b)[i, j] = G^(w,b)[a_i, a_j], G the true equal-time Green's function that dqmc_accumulate_greens sums
 * (dqmc_get_greens).  One sample is the strictly upper triangle of the W x W matrix x, one matrix per subsystem, element
 * (w, w') at W w + w'; the lower triangle and the diagonal are 0.  Tr rho_A^2 is the mean of x over pairs and samples,
 * S_2(A) = -log Tr rho_A^2 (dqmc.py: entanglement_from_pair_sums, with the delete-one-walker jackknife).
 * det M_b comes from an elimination with partial pivoting in the pivot order of dqmc_logdet's sign (largest magnitude,
 * lowest row among equals) as sign and sum of log|pivot|; x = sign exp(sum).  Every sum and pivot choice is taken in a
 * fixed order: x(w, w') depends on the two walkers' G alone, not on W, the other subsystems or the launch shape.  A pair
 * with a zero or non-finite pivot (or a non-finite x) gives the sample 0 and is counted in `failures`.
 * Limits: 1 <= N_A <= DQMC_ENT_MAX_SITES (M is eliminated in the LDS of one workgroup), at most DQMC_ENT_MAX_SUBSYSTEMS
 * subsystems, W >= 2.  Sign weighting: the signed estimator needs s_w s_w' and <s>^2 and is NOT implemented; with sign
 * weighting on dqmc_accumulate_entanglement returns DQMC_ERR_STATE.  Each handle pairs its own walkers only; there is no
 * reduction over ranks (purities of ranks combine as count-weighted means on the host).
 * The sums are NOT a DQMC_RED_* section: dqmc_accumulator_size, dqmc_reduce_size, the packed reduction and the state blob
 * are those of a handle without the measurement, whether it is on or off, and with it off nothing is allocated or
 * launched.  The checkpoint carries the sums in the file's preamble (dqmc.py: save / load, dqmc_set_entanglement_sums). */
enum { DQMC_ENT_MAX_SITES = 128, DQMC_ENT_MAX_SUBSYSTEMS = 64 };
/* The reference has no such measurement.  Subsystem s is sites[sub_ptr[s] .. sub_ptr[s + 1]), sub_ptr[0] = 0.  n_sub = 0
 * turns the measurement off and frees everything (the pointers are then ignored).  DQMC_ERR_INVALID for n_sub < 0 or
 * above DQMC_ENT_MAX_SUBSYSTEMS, an empty list, more than DQMC_ENT_MAX_SITES sites, a duplicate site or a site outside
 * [0, n_sites): the handle keeps its setting.  DQMC_ERR_STATE for a handle with fewer than two walkers.  A successful
 * call starts with zero sums. */
int dqmc_set_entanglement(dqmc_handle *h, int32_t n_sub, const int32_t *sub_ptr /* [n_sub + 1] */, const int32_t *sites);
/* n_sub W W + 2 doubles: [sums: n_sub x W x W][sample count][failures]; 0 while the measurement is off */
int dqmc_entanglement_size(dqmc_handle *h, size_t *n_doubles);
/* The reference has no such measurement.  One sample from the true G of the current fields, at any point where
 * dqmc_accumulate_greens is allowed.  DQMC_ERR_STATE before dqmc_prepare or dqmc_set_entanglement and with sign
 * weighting on. */
int dqmc_accumulate_entanglement(dqmc_handle *h);
/* the sums, the count and the failures (n = dqmc_entanglement_size); the last sample alone (n = n_sub W W; zeros before
 * the first one).  dqmc_reset_accumulators zeroes the sums, the count and the failures. */
int dqmc_get_entanglement(dqmc_handle *h, double *host_out, size_t n);
int dqmc_get_entanglement_sample(dqmc_handle *h, double *host_out, size_t n);
/* puts back what dqmc_get_entanglement handed out (the checkpoint's way in); the count and the failures must be
 * non-negative integers, DQMC_ERR_INVALID otherwise */
int dqmc_set_entanglement_sums(dqmc_handle *h, const double *host_in, size_t n);

/* ---- current response in imaginary time: Lambda(q, tau) ---------------------------------------------------------------
 * The reference has no such measurement.  DQMC_BIN_RESPONSE_CURRENT holds the current-current sums integrated over all
 * slices, i.e. Lambda(q, i omega = 0) only.  This opt-in recording keeps the per-slice values that the susceptibility pass
 * computes anyway, transformed to momentum space, as PER-WALKER sums over calls, so that the host can form
 * Lambda(q, i omega_m), the Drude weight D / pi = -k_x - Lambda_xx(q = 0, i omega_m -> 0) and the dc-conductivity proxy
 * (beta^2 / pi) Lambda_xx(q = 0, beta / 2) with delete-one-walker jackknife errors (dqmc.py: current_time_displaced,
 * current_matsubara, drude_weight, dc_conductivity).
 * dqmc_set_current_time_displaced(h, every): every == 0 turns the recording off and frees everything (the default);
 * every >= 1 with slices % every == 0 turns it on with rows r = 0 .. R - 1, R = 1 + slices / every, tau_r = r every
 * delta_tau; anything else returns DQMC_ERR_INVALID and the handle keeps its setting.  Needs dqmc_set_pair_directions,
 * dqmc_set_current_targets, dqmc_set_momenta and dqmc_prepare (DQMC_ERR_STATE without them); a later call of any of the
 * first three turns it off.  Every successful call starts with zero sums; dqmc_reset_accumulators and
 * dqmc_set_sign_weighting zero them too.  From then on every dqmc_accumulate_susceptibilities pass adds one sample.
 * Per walker, q fastest, then k, then r (P = 2 R K_cc n_q + K_cc + 3 doubles):
 *   [C: R x K_cc x n_q][S: R x K_cc x n_q][kbond: K_cc][sum of s_w][samples kept][samples left out]
 *   C[r][k][q] = sum_d cos(q . r_d) x_r[d + n_dirs k],   S[r][k][q] = sum_d sin(q . r_d) x_r[d + n_dirs k],   d ascending,
 * with the tables of dqmc_set_momenta and x_r what cc_kernel gives for the packed tuple of slice l = r every, summed over
 * the quads of a direction and divided by N as ccs is: no delta_tau, the attractive model's factors as in the pass, so
 * delta_tau sum_{l = 1 .. slices} x_l is the ccs sample.  Row 0 takes (G00, G00 - I, G00, G00), the tau -> 0+ convention
 * of the time-displaced recording above.  kbond is exactly that of DQMC_BIN_RESPONSE_CURRENT.  With sign weighting every
 * entry is s_w times the above, a walker with s_w = 0 adds nothing and is counted as left out; with it off the sum of
 * s_w is the number of samples kept.  The values stay as cc_kernel gives them (C <= 0 on the diagonal); Lambda = -C is
 * the host's sign, as for the stiffness.
 * At a recorded slice the ccs kernels write the slice's sums into a zeroed scratch, one kernel (current_tau.hip)
 * contracts it with both tables and then adds it to the susceptibility sample: that sample, its sums, every binner fed by
 * them, mc.s.greens, the stacks, the field and the RNG cursors are bit for bit those of a pass without the recording.
 * Every stored value is one sum in a fixed order with no atomics: a second pass on the same state adds the same bits, and
 * a walker's sample does not depend on n_walkers.  Not a DQMC_RED_* section, no binner, nothing in the packed reduction
 * or the state blob: with it off nothing is allocated or launched.  Each handle records its own walkers; ranks combine on
 * the host (count-weighted).  The checkpoint carries the setting and the sums in the file's preamble (dqmc.py: save /
 * load, dqmc_set_current_time_displaced_sums). */
int dqmc_set_current_time_displaced(dqmc_handle *h, int32_t every);
int dqmc_current_time_displaced_plan(dqmc_handle *h, int32_t out[4]);  /* [R, every, K_cc, n_q], zeros while off */
/* n_walkers P doubles, walker after walker; 0 while the recording is off */
int dqmc_current_time_displaced_size(dqmc_handle *h, size_t *n_doubles);
int dqmc_get_current_time_displaced(dqmc_handle *h, double *host_out);
/* puts back what dqmc_get_current_time_displaced handed out (the checkpoint's way in); the two sample counts of every
 * walker must be non-negative integers, DQMC_ERR_INVALID otherwise */
int dqmc_set_current_time_displaced_sums(dqmc_handle *h, const double *host_in);

/* ---- checkpoint and resume ---------------------------------------------------------------------------------------
 * save / load / resume! (FileIO.jl:38-156, DQMC.jl:463-477, 797-924) for the state that lives on the device.  Like the
 * global moves this is a defined extension of the ABI: the reference writes a JLD file from host objects; here the engine
 * hands out and takes back one blob, and the file around it is the host's (dqmc.py: save / load).
 * Saved is what cannot be recomputed: the HS field, the RNG cursors, the counters and every measurement sum.  Not saved:
 * mc.s.greens, the UDT stack, Ul .. Tr, a pending sweep update, the logabsdet / sign cache, the unequal-time stack (all
 * follow from the field: resume! rebuilds them through run!'s init!, build_stack, propagate, DQMC.jl:412-414), reduced
 * buffers (dqmc_reduce), timing counters and host-supplied uniform streams.
 * The blob is little-endian with fixed-width fields; doubles are IEEE bit patterns.
 *   header (560 bytes)
 *     u64 magic "DQMCSTA1"   u32 format version (1)   u32 header bytes
 *     char[16] dqmc_build_source_hash of the exporting library, zero padded (informational, never checked)
 *     i32 n_sites, model_kind, slices, safe_mult, n_walkers, n_blocks      f64 delta_tau, U
 *     u64 n[6]      doubles of the accumulator of each DQMC_RED_* section, 0 = not configured
 *     u64 n_red[6]  doubles of its part of the reduction buffer
 *     11 binners (DQMC_BIN_GREENS .. DQMC_BIN_TIME_DISPLACED, then DQMC_BIN_SIGN + k): i32 on, E, L, pad   i64 capacity, T
 *     i32 time-displaced every, what, R     i32 sign weighting on     i32 global rate, global kind
 *     i64 updates since dqmc_prepare (the global-move schedule)     u64 FNV-1a 64 of the header bytes in front of it
 *   payload, in this order, nothing between the parts
 *     the HS field: per walker the ceil(n_sites slices / 64) u64 chunks of dqmc_get_conf_bits
 *     per walker (u64 seed, u64 draw): the Philox key and cursor of dqmc_seed / dqmc_uniforms_used
 *     per walker i64 prop_local, acc_local, then negative_probability and propagation_error as (f64 max, min, sum, i64 count)
 *     per walker u64 moves_drawn, i64 prop_global, acc_global, i64 pending dS, f64 last p, i32 active, site, accepted, pad
 *     per walker i64 dqmc_get_sign_failures
 *     the accumulator of every configured section in DQMC_RED_* order, the sums of signs included (n doubles each)
 *     x_sum [L][W][E], x2_sum [L][W][E], compressor [L - 1][W][E] of every enabled binner in the order of the header
 * The binner's T and the update count are state and come back with the payload; every other header field describes how
 * the handle is configured and must be the same on both sides.
 * Format version 2: the header has room for exactly the eleven binners above, so a handle with a momentum binner enabled
 * (DQMC_BIN_MOMENTUM_*) writes version 2: the version-1 header (its version field reads 2) and payload, followed by an
 * extension; a handle with none enabled writes the version-1 blob unchanged, whether or not momenta are set.
 *   extension
 *     i32 n_q, n_dirs     3 binners (DQMC_BIN_MOMENTUM_CORRELATIONS ..): i32 on, E, L, pad   i64 capacity, T
 *     cos_tab, sin_tab: n_dirs n_q doubles each
 *     x_sum, x2_sum, compressor of every enabled momentum binner, as above
 *     u64 FNV-1a 64 of all extension bytes in front of it
 * dqmc_state_import takes both versions.  The extension is validated like the header, before the first write: its size,
 * its checksum (which covers the binner arrays too), then n_q, n_dirs and the binner shapes against the importing
 * handle's, then the tables byte for byte against the handle's own; a version-1 blob is refused by a handle with a
 * momentum binner enabled.
 * Format versions 3 and 4: a handle with the thermodynamics section configured (dqmc_set_thermodynamics) writes the
 * version-1 blob with version field 3, or the version-2 blob with version field 4, followed by one more extension; a
 * handle without the section writes version 1 or 2 unchanged, byte for byte.
 *   thermodynamics extension
 *     u64 n (12), n_red     1 binner (DQMC_BIN_THERMODYNAMICS): i32 on, E, L, pad   i64 capacity, T
 *     u64 FNV-1a 64 of the bytes of the hopping matrix handed to dqmc_set_thermodynamics     f64 U_s
 *     the section's n doubles     x_sum, x2_sum, compressor of the binner if enabled
 *     u64 FNV-1a 64 of all bytes of this extension in front of it
 * It is validated like the others before the first write; a version 3 / 4 blob is refused by a handle without the
 * section and a version 1 / 2 blob by a handle with it, the field named ("section thermodynamics n").
 * Format versions 5 - 8: a handle with a response binner enabled (DQMC_BIN_RESPONSE_*) writes the version 1 - 4 blob it
 * would write without them, its version field raised by 4, followed by a third extension; a handle with none enabled
 * writes versions 1 - 4 unchanged, byte for byte, whether or not pair channels are set.
 *   response extension
 *     i32 n_ch, K, K_cc, pad     3 binners (DQMC_BIN_RESPONSE_PAIRING ..): i32 on, E, L, pad   i64 capacity, T
 *     F: K K n_ch doubles (none while the channels are off)
 *     x_sum, x2_sum, compressor of every enabled response binner     u64 FNV-1a 64 of all extension bytes in front of it
 * It is validated like the others before the first write (the F table byte for byte against the handle's); a version
 * 5 - 8 blob is refused by a handle with no response binner and a version 1 - 4 blob by a handle with one, the binner
 * named ("binner response_pairing on"). */
/* bytes of the blob of this handle as it is configured now */
int dqmc_state_size(dqmc_handle *h, size_t *n_bytes);
/* The blob into host_out (n_bytes = dqmc_state_size).  Only at the measurement point, current_slice == 1 && direction ==
 * +1, where dqmc_update_until_measure returns (and dqmc_sweep when it started there); DQMC_ERR_STATE anywhere else, and
 * when a walker runs on a dqmc_set_uniforms stream (a test device the blob does not carry).  Only copies are made: no
 * kernel is launched and no buffer of the handle is written, so the chain's future is bit for bit that of a handle that
 * was never exported. */
int dqmc_state_export(dqmc_handle *h, void *host_out, size_t n_bytes);
/* Takes a blob into a handle created with the same dqmc_params and configured the same way (pair directions, local and
 * current targets, time-displaced setting, binners with the same capacities, sign weighting, global rate and kind; the
 * susceptibility section laid out if it was, e.g. by dqmc_susceptibilities_size).  A bad magic, an unknown version, a
 * damaged header, any configuration field that differs and a buffer shorter or longer than the header describes return
 * DQMC_ERR_INVALID with dqmc_last_error naming the first offending field; everything is checked before the first write,
 * so a refused call leaves the handle as it was.
 * On success the payload is restored, the stack and mc.s.greens are rebuilt from the field (init_stack, build_stack, then
 * the propagates of a down pass with no sweep in between) and the handle stands at the measurement point, prepared.  The
 * last reduction is void, the logabsdet / sign cache invalid, the unequal-time stack rebuilt on its next use.  Every walker
 * is on the Philox stream of its saved (seed, draw) afterwards: a walker of the importing handle that ran on a
 * dqmc_set_uniforms stream leaves it (the handle keeps the buffer until dqmc_destroy or the next dqmc_set_uniforms).
 * The checksum protects the header only: the payload is taken as it comes, as dqmc_set_conf_bits and the other setters
 * take their arguments (its one index, the site of a walker's latest global move, is checked against n_sites), and a
 * payload damaged in transit with its sizes intact is not noticed.  The rebuilt
 * G differs from the propagated one it replaces by rounding: a resumed chain agrees with the uninterrupted one as device
 * and oracle agree, not to the bit.  Exact are: the payload through export and import, the exporting chain's future,
 * and the futures of two imports of one blob. */
int dqmc_state_import(dqmc_handle *h, const void *host_in, size_t n_bytes);

/* ---- batched linalg primitives (unit parity with test/slice_matrices.jl) --
 * host in / host out, `batch` independent n x n problems, run on device_id.  */
/* vmul! family (src/linalg/general.jl:7-56): C = op(A)*op(B); transa/transb 0|1 */
int dqmc_vmul(int32_t device_id, int32_t n, int32_t batch, int32_t transa, int32_t transb,
              const double *A, const double *B, double *C);
/* udt_AVX_pivot!(U, D, T, pivot, temp, Val(apply)) (src/linalg/UDT.jl:192-306);
 * T holds the input on entry and T on exit.  The reference's contracts hold (test/slice_matrices.jl:202-234:
 * U unitary, U*Diagonal(D)*T = input resp. U*D*UpperTriangular(T)*P = input with P[i, pivot[i]] = 1).  At n = 256 and up to
 * 32 matrices the pivot order is the descending order of the INPUT's column norms (one-launch blocked factorisation), not the
 * step-by-step search of UDT.jl:212-246: D is then not sorted; DQMC_QR_NOBLOCKED=1 selects the reference's rule. */
int dqmc_udt_pivot(int32_t device_id, int32_t n, int32_t batch, double *U, double *D, double *T,
                   int64_t *pivot, int32_t apply_pivot);
/* The kernel behind dqmc_logdet on matrices of the caller's: unit u has its n x n column-major matrix at A + u * strideA
 * (strideA >= n * n) and n positive numbers at D + u * strideD (strideD >= n); logabsdet[u] = sum_i log D[u][i] in the
 * kernel's fixed order, sign[u] = the sign of det A[u] from an LU with partial pivoting (the largest magnitude on or
 * below the diagonal, the lowest row among equals), 0 for a zero or non-finite pivot.  A and D come back as the device
 * left them: the matrices overwritten by the elimination at n > 64, everything between the units untouched. */
int dqmc_logdet_matrices(int32_t device_id, int32_t n, int32_t batch, double *A, int64_t strideA, double *D,
                         int64_t strideD, double *logabsdet, int32_t *sign);
/* Diagnostic (like dqmc_logdet_matrices): impose the per-unit signs that "sign reweighting" works from, sign[w * n_blocks +
 * b], each -1, 0 or +1.  Real fields give a negative sign only where a search finds one and never a sign of 0; this reaches
 * the signed sums, and the path of a walker that is left out, at any shape.  The call first brings the cache of the current
 * field up to date (one slice chain unless it holds: the kept logabsdet stay the true ones) and then overwrites the kept
 * per-unit signs; the cache still counts as that of the current field.  From then on dqmc_get_sign and every signed
 * dqmc_accumulate_* see the imposed signs, until something invalidates the cache: any update or sweep, dqmc_set_conf /
 * dqmc_set_conf_bits, a global move, dqmc_state_import, and dqmc_logdet, which recomputes from scratch.  No other
 * Monte-Carlo state is changed.  A global move taken while an override is in force would use the imposed signs in its
 * weight ratio: a test must not do that.  DQMC_ERR_INVALID for a null pointer or a value outside {-1, 0, +1}, DQMC_ERR_STATE
 * before dqmc_prepare and on the attractive model (sign +1 by construction, no array behind it); a refused call changes
 * nothing. */
int dqmc_impose_unit_signs(dqmc_handle *h, const int32_t *sign /* n_walkers * n_blocks */);
/* rdivp!(A, T, O, pivot) (src/linalg/general.jl:138-166) */
int dqmc_rdivp(int32_t device_id, int32_t n, int32_t batch, double *A, const double *T,
               const int64_t *pivot);
/* calculate_greens_AVX! (src/flavors/DQMC/stack.jl:337-393) */
int dqmc_calculate_greens(int32_t device_id, int32_t n, int32_t batch, const double *Ul,
                          const double *Dl, const double *Tl, const double *Ur, const double *Dr,
                          const double *Tr, double *G);

/* CheckerboardTrue (DQMC(m; checkerboard=true), DQMC.jl:250-263) with the bond-group factors kept SPARSE on the
 * device: chkr_hop_half[g], chkr_hop[1], their inverses (and the adjoints, as separate factors) of
 * init_checkerboard_matrices (stack.jl:185-235) in ELL form - vals / cols [n_mats][n_sites][kmax], 0-based columns,
 * padding entries val = 0 - plus chkr_mu / chkr_mu_inv per block [n_blocks][n_sites] and seven factor sequences
 * (each up to 32 indices into the factor list, applied first to last):
 *   0 B X   (multiply_slice_matrix_left!, slice_matrices.jl:104-124)     3 X B    (:125-149)
 *   1 B^-1 X (:150-171)                                                   4 X B^-1 (:172-196)
 *   2 B' X  (multiply_daggered_slice_matrix_left!, :197-222)              5 X eT, 6 eTinv X (greens(), DQMC.jl:731-750)
 * Right products take the factors' transposes (rows of H' = columns of H).  After this call the propagation path
 * applies these sequences slab by slab in LDS instead of dense GEMMs with the multiplied-out constants (which
 * dqmc_create still needs: the unequal-time path uses them).
 * The slab is 32 values of the index that is not mixed up to n_sites = 256, 16 up to 568 and 8 above: two images of
 * n_sites x (width + 1) doubles and two scaling vectors must fit the 160 KiB of LDS of a compute unit, which 8 columns
 * (160 n_sites bytes) do up to n_sites = 1024, the ceiling of dqmc_create.  A size that no width fits is refused with
 * DQMC_ERR_INVALID before anything is allocated: the handle keeps the dense constants and stays usable. */
int dqmc_set_checkerboard(dqmc_handle *h, int32_t kmax, int32_t n_mats, const double *vals, const int32_t *cols,
                          const double *mu, const double *mu_inv, const int32_t *seqs, const int32_t *lens);
/* out = [1, kmax, slab width (32, 16 or 8), dynamic LDS bytes of a product] with a sparse checkerboard, else zeros */
int dqmc_checkerboard_plan(dqmc_handle *h, int32_t out[4]);
/* Diagnostic (like dqmc_vmul): exactly the launch the propagation path issues for sequence `which` (0..6, the order
 * above) at HS slice `slice` (1..slices; ignored by sequences 5 and 6), for every unit of the handle, on device buffers
 * of its own.  X and out are host arrays [n_walkers * n_blocks][n_sites][n_sites], column-major per unit.  qscale
 * (NULL: none) is [n_walkers * n_blocks][n_sites] and multiplies the result along the index that is not mixed: columns
 * for the left products (the D of a stabilisation step), rows for the right ones.  in_place != 0 hands the kernel one
 * buffer as source and destination, as the wrap does.  No Monte-Carlo state is written.  DQMC_ERR_STATE without a
 * sparse checkerboard, DQMC_ERR_INVALID for another `which` or a slice outside 1..slices for sequences 0..4. */
int dqmc_checkerboard_apply(dqmc_handle *h, int32_t which, int32_t slice, const double *X, const double *qscale,
                            int32_t in_place, double *out);

/* The cooperative QR with the reference's pivot rule (n < 256, or 33..64 units at n = 256; 8 workgroups per matrix, bounded
 * hand-off spins) leaves its input intact; if a launch times out (CUs held by another stream for longer than the spins allow),
 * the guarded single-workgroup kernel launched behind it redoes the factorisation, so results stay valid.  This counter reports
 * how often that happened.  (The one-launch UDT has no second path: its time-outs fail the call, see dqmc_device_errors.) */
int dqmc_qr_fallbacks(dqmc_handle *h, int64_t *count);
/* 1 when slice products and wraps apply eT2 / eTinv2 in factored form (Kronecker products of 16 x 16 factors or of an 8 x 8 and a
 * 32 x 32 factor at n = 256, 8 x 8 factors or the two-layer 2 x 2 (x) 16 x 16 (x) 16 x 16 form at n = 512, see dqmc_params; the triangular 16 x 16 lattice's three factors, see
 * dqmc_set_triangular_factors; the t-t' square 16 x 16 lattice's four factors, see dqmc_set_square_tp_factors), else 0 */
int dqmc_kron_hopping(dqmc_handle *h, int32_t *on);
/* The periodic 16 x 16 TriangularLattice (n_sites = 256, site x + 16 y; hopping along X = x + 1, Y = y + 1 and D = XY,
 * triangular.jl:60-78) in three-factor form.  X, Y and D commute, so exp(-a T) = e^{a mu} f(X) f(Y) f(XY) with
 * f = exp(a t (S + S')) on a 16-ring, and each of eT2 and eTinv2 is E = (Fy (x) Fx) Ed, where Ed applies Fd along each
 * diagonal x - y = u: (Ed v)(x, y) = sum_y' Fd[y, y'] v(x - y + y', y').  f holds, per block, [eT2: Fx Fy Fd][eTinv2: Fx
 * Fy Fd], each a 16 x 16 column-major matrix (1536 doubles per block).
 * The handle checks them against its own eT2 / eTinv2: E[0,0] > 0 and max|E - P| <= 256 DBL_EPSILON max|E| for
 * P = (Fy (x) Fx) Ed and for the two orders the kernel applies, Fx Ed Fy and Fy Ed Fx.  When every block passes, slice
 * products and wraps apply the three factors (tri.hip; dqmc_kron_hopping reports 1) and the sweep's last chunk is applied
 * by the stand-alone flush.  Returns DQMC_ERR_INVALID for factors that fail the check or n_sites != 256, DQMC_ERR_STATE
 * after dqmc_prepare / dqmc_build_stack / dqmc_replay_greens; in both cases the handle keeps its path and stays usable.
 * A handle on a path that does not take them (DQMC_NO_KRON or DQMC_NO_SLAB set, a checkerboard, or a square lattice's
 * Kronecker factors already taken) returns DQMC_OK and keeps its path. */
int dqmc_set_triangular_factors(dqmc_handle *h, const double *f);
/* The periodic 16 x 16 SquareLattice with next-nearest-neighbour hopping t' (n_sites = 256, site x + 16 y; hopping t along
 * X = x + 1 and Y = y + 1, t' along D = XY and A = X Y^-1) in four-factor form.  An extension: the reference's Hubbard
 * models have nearest-neighbour hopping only.  X, Y, D and A commute, so exp(-a T) = e^{a mu} f_t(X) f_t(Y) f_t'(D) f_t'(A)
 * with f_s = exp(a s (S + S')) on a 16-ring, and each of eT2 and eTinv2 is E = (Fy (x) Fx) Ed Ea, where Ed applies Fd
 * along each diagonal x - y = u and Ea applies Fa along each anti-diagonal x + y = w:
 *   (Ed v)(x, y) = sum_y' Fd[y, y'] v(x - y + y', y')        (Ea v)(x, y) = sum_y' Fa[y, y'] v(x + y - y', y')
 * f holds, per block, [eT2: Fx Fy Fd Fa][eTinv2: Fx Fy Fd Fa], each a 16 x 16 column-major matrix (2048 doubles per
 * block); mu is folded into Fx.
 * The handle checks them against its own eT2 / eTinv2: E[0,0] > 0 and max|E - P| <= 256 DBL_EPSILON max|E| for
 * P = (Fy (x) Fx) Ed Ea and for the four orders the kernel applies, Fx Ea Ed Fy, Fy Ea Ed Fx, Fy Ed Ea Fx and Fx Ed Ea Fy.
 * When every block passes, slice products and wraps apply the four factors (ttp.hip; dqmc_kron_hopping reports 1) and, as
 * on the triangular path, the sweep's last chunk is applied by the stand-alone flush and a wrap is two launches.  Returns
 * DQMC_ERR_INVALID for factors that fail the check or n_sites != 256, DQMC_ERR_STATE after dqmc_prepare /
 * dqmc_build_stack / dqmc_replay_greens; in both cases the handle keeps its path and stays usable.  A handle on a path
 * that does not take them (DQMC_NO_KRON or DQMC_NO_SLAB set, a checkerboard, or Kronecker or triangular factors already
 * taken) returns DQMC_OK and keeps its path. */
int dqmc_set_square_tp_factors(dqmc_handle *h, const double *f);
/* which call sites of udt_AVX_pivot! (UDT.jl:192-306) this handle serves with the one-launch pre-pivoted factorisation:
 * bit 0 add_slice_sequence_left/right (stack.jl:272-311) and other callers, bit 1 / bit 2 the two factorisations of
 * calculate_greens_AVX! (stack.jl:349, :376); 0 = the reference's pivot rule everywhere (n != 256, > 32 units, DQMC_QR_NOBLOCKED) */
int dqmc_udt_one_launch_sites(dqmc_handle *h, int32_t *mask);
/* Read-only diagnostic: which of the launch forms that need co-resident workgroups this handle took when it was set up,
 * from the variables the launchers themselves read; nothing is launched.  A unit is one walker x one block; the block maps
 * launch whole groups of eight units.
 *   out[0]  units                                   out[1]  units in whole groups of eight
 *   out[2]  compute units of the device             out[3]  dqmc_udt_one_launch_sites
 *   out[4]  workgroups the one-launch UDT may use (compute units x occupancy; 0: not admitted, or n_sites != 256)
 *   out[5]  workgroups the cooperative QR may use   out[6]  1: the cooperative QR is admitted for out[0] units
 *           (n_sites <= 256; it runs at the call sites out[3] leaves to it), 0: single-workgroup QR kernels
 *   out[7]  1: site sweep with the fused chunk loop (elimination beside the previous chunk's flush), 0: launch per chunk
 *   out[8], out[9]    workgroups the one-launch factored wrap may use without / with a pending sweep chunk
 *   out[10], out[11]  1: the factored wrap is one launch without / with a pending chunk, 0: two launches (or no factored wrap;
 *           always 0 with the triangular lattice's three factors and the t-t' square lattice's four) */
int dqmc_launch_plan(dqmc_handle *h, int32_t out[12]);
/* device error word as it stands (0 = no bounded wait inside a kernel has run out); no reference counterpart: the reference
 * has no concurrent workgroups (diagnostic next to DQMCAnalysis, src/flavors/DQMC/DQMC.jl:35-47) */
int dqmc_device_errors(dqmc_handle *h, int32_t *word);
/* commit the library was built from ("<short hash>[+]"); used by bench.py to tell fresh profile files from stale ones */
const char *dqmc_build_commit(void);
/* hash of the kernel sources the library was built from (csrc/Makefile: SOURCE_HASH); commits that leave the kernels alone
 * leave it alone - this is what decides whether a committed profile still describes the library */
const char *dqmc_build_source_hash(void);

/* ---- the classical MC flavor with the IsingModel ---------------------------------------------------------------
 * MC(model; ...) (src/flavors/MC/MC.jl:16-80) with IsingModel (src/models/Ising/IsingModel.jl) for n_walkers
 * independent Markov chains on one device, one lane per walker (csrc/ising.hip).  A walker's stream is the Philox4x32-10
 * counter stream of dqmc_seed: key = seed, counter = draw index.  sweep(mc) (MC.jl:316-333) visits sites 1..N in order,
 * dE = 2 s_i sum_{j in neighs[:, i]} s_j (IsingModel.jl:85-101), and accepts iff dE <= 0 || u < exp(-beta dE), with a
 * uniform drawn only when dE > 0; exp(-beta dE) is a per-walker table computed on the host (dqmc_mc_set_beta).
 * Limits: n_sites <= 16384, 1 <= z <= 8.  Errors come from dqmc_mc_last_error. */
typedef struct dqmc_mc_handle dqmc_mc_handle;

typedef struct {
    int32_t n_sites;         /* length(lattice(m)) */
    int32_t z;               /* neighbours per site: size(l.neighs, 1) */
    int32_t n_walkers;       /* independent chains batched on this device */
    int32_t device_id;
    int32_t n_bonds;         /* size(l.bonds, 1) */
    int32_t series_capacity; /* per-walker measurements recorded as a time series (0 = none) */
    const int64_t *neighs;   /* l.neighs as is: z x n_sites, column-major, 1-based (lattices/abstract.jl:56-66) */
    const int64_t *bonds;    /* l.bonds[:, 1:2]: n_bonds x 2, column-major, 1-based (abstract.jl:33-38, neighbors(l)) */
} dqmc_mc_params;

/* MCAnalysis (MC.jl:1-11) and the sums behind IsingEnergyMeasurement / IsingMagnetizationMeasurement
 * (models/Ising/measurements.jl:13-94) for one walker; the sums are exact integers held in fp64 */
typedef struct {
    int64_t energy;        /* model.energy[] */
    int64_t magnetization; /* sum(mc.conf) */
    double sum_E, sum_E2, sum_absM, sum_M2;
    int64_t n_meas;        /* measurements summed since the last dqmc_mc_reset_accumulators */
    int64_t prop_local, acc_local;
    uint64_t uniforms_used; /* draws consumed from the walker's stream */
    int64_t n_series;       /* measurements recorded in the series, <= series_capacity */
} dqmc_mc_stats;

/* MC(m; ...) + init! (MC.jl:50-80): validates the arguments, then the device (no device: DQMC_ERR_NO_DEVICE) */
int dqmc_mc_create(const dqmc_mc_params *p, dqmc_mc_handle **out);
int dqmc_mc_destroy(dqmc_mc_handle *h);
/* message of the last failing call on this handle (h may be NULL: create errors) */
const char *dqmc_mc_last_error(const dqmc_mc_handle *h);
/* mc.p.beta (MCParameters, MC.jl:24) of one walker: the threshold table exp(-beta 2k), k = 1..8, computed on the host;
 * beta finite and >= 0 */
int dqmc_mc_set_beta(dqmc_mc_handle *h, int32_t walker, double beta);
/* the walker's stream: key = seed, cursor at draw 0 */
int dqmc_mc_seed(dqmc_mc_handle *h, int32_t walker, uint64_t seed);
/* mc.conf = rand(MC, m) (IsingModel.jl:83): site i takes the walker's next uniform, u < 0.5 -> -1; then init!
 * (energy(mc, m, conf), IsingModel.jl:24).  walker < 0: every walker */
int dqmc_mc_rand_conf(dqmc_mc_handle *h, int32_t walker);
/* mc.conf as Int8 +-1 in site order; set_conf recomputes energy and magnetization and leaves the cursor alone */
int dqmc_mc_set_conf(dqmc_mc_handle *h, int32_t walker, const int8_t *conf);
int dqmc_mc_get_conf(dqmc_mc_handle *h, int32_t walker, int8_t *conf);
/* BitArray(conf .== 1) chunks as dqmc_get_conf_bits: ceil(n_sites / 64) uint64 */
int dqmc_mc_get_conf_bits(dqmc_mc_handle *h, int32_t walker, uint64_t *chunks);
/* n_sweeps x sweep(mc) with the measurement rule of run! (MC.jl:262-283): after global sweep index
 * i = first_sweep_index, first_sweep_index + 1, ... measure iff i > thermalization && i % measure_rate == 0.
 * Split into launches of bounded work; complete on return. */
int dqmc_mc_sweep(dqmc_mc_handle *h, int32_t n_sweeps, int64_t first_sweep_index, int64_t thermalization,
                  int32_t measure_rate);
int dqmc_mc_get_stats(dqmc_mc_handle *h, int32_t walker, dqmc_mc_stats *out);
/* per-measurement E and |M| (the Observable series of measure!, measurements.jl:30-37,75-81), n_series entries each;
 * either buffer may be NULL */
int dqmc_mc_get_series(dqmc_mc_handle *h, int32_t walker, int32_t *energy, int32_t *abs_magnetization,
                       int64_t *n_recorded);
/* clear the measurement sums and series of every walker (MCAnalysis counters stay) */
int dqmc_mc_reset_accumulators(dqmc_mc_handle *h);
/* Wolff cluster move, global_move(mc, m::IsingModel, conf) (IsingModel.jl:104-140) with m.energy[] = energy(mc, m,
 * conf).  Seed site min(N - 1, floor(u(m, 0) N)); the directed slot (i, k) (0-based site i, k < z) joins
 * neighs[k, i] iff the two spins are equal and u(m, 1 + 8 i + k) < 1 - exp(-2 beta) (computed on the host by
 * dqmc_mc_set_beta); the cluster (the sites reachable from the seed through such slots, one site at least) is flipped,
 * accepted = cluster size > 1, then energy and magnetization are recomputed.  u(m, t) is Philox4x32-10 with key = the
 * walker's seed and counter words (t, low32(m), 1, high32(m)); m counts the walker's cluster moves since
 * dqmc_mc_seed.  The local stream (counter words 2 and 3 zero) is not touched. */
/* mc.p.global_rate with mc.p.global_moves (MC.jl:22-23, 233-236): from now on dqmc_mc_sweep runs one global_move per
 * walker after every sweep whose global index is a multiple of rate, before that sweep's measurement.  0 = off (the
 * default); rate >= 0 */
int dqmc_mc_set_global_rate(dqmc_mc_handle *h, int32_t rate);
/* one global_move (IsingModel.jl:104-140) of one walker, or of every walker when walker < 0; it takes no measurement */
int dqmc_mc_global_move(dqmc_mc_handle *h, int32_t walker);
/* MCAnalysis prop_global / acc_global (MC.jl:1-11, 234-235) of one walker, with the sum of the cluster sizes and the
 * move cursor m */
typedef struct {
    int64_t prop_global, acc_global, sum_cluster_size;
    uint64_t moves_drawn;
} dqmc_mc_global_stats;
int dqmc_mc_get_global_stats(dqmc_mc_handle *h, int32_t walker, dqmc_mc_global_stats *out);
/* Replica exchange (parallel tempering) between the walkers of one handle.  The reference has no such move; like the
 * cluster move this is a defined extension.  The walkers form n_walkers / R ladders of R consecutive slots.  Slot w keeps
 * what belongs to its temperature: beta and its tables, the Philox key and both cursors, the sums, series and binner,
 * and every counter.  An accepted exchange swaps the configurations of two neighbouring slots of a ladder: the spins,
 * energy, magnetization and the replica label (at first the slot's index within its ladder).  So dqmc_mc_get_stats(w)
 * and the binner of w stay "at beta_w"; a replica wanders over the slots.  The handle keeps an exchange cursor x, the
 * number of rounds since dqmc_mc_set_exchange.  Round x tries the pairs (i, i + 1) of every ladder with ladder-local
 * i = x (mod 2) and i + 1 < R.  For the slots (a, b = a + 1) of a pair: d = (E_a - E_b) / 2 (an integer, E = n_bonds mod 2
 * for every configuration) and db = beta_a - beta_b in fp64 on the host; the betas need not be monotone.  The pair
 * swaps if db == 0, d == 0, or db and d have the same sign.  Otherwise p = 1.0, then p = p * q[j] for every set bit j of
 * |d| in ascending order, with q[j] = exp(-2 |db| 2^j) a per-pair table of J entries (2^J > n_bonds, J <= 17) from the
 * host's libm, rebuilt by dqmc_mc_set_beta for the two pairs a slot belongs to; the pair swaps iff u < p, where
 * u = Philox4x32-10 with the key of slot a and counter words (low32(x), high32(x), 2, 0), formed only when it decides.
 * This is a third domain: the local stream has words 2 and 3 zero, the cluster move has word 2 = 1.  Neither of their
 * cursors moves.  There is no exp on the device and a product of doubles is exactly rounded, so every decision can be
 * reproduced bit for bit.  p differs from exp(2 db d) by the rounding of at most 17 factors and 16 products, about
 * 20 ulp: that relative error of the acceptance probability is the size of the deviation from exact detailed balance
 * (a chain that used p for both directions of every pair would be exact; the rule is symmetric in a and b).  Per slot a,
 * prop_exchange / acc_exchange count the tries and swaps of the pair (a, a + 1); the last slot of a ladder stays 0. */
/* n_replicas = R >= 2 defines the ladders (n_walkers % R != 0: DQMC_ERR_INVALID); 0 or 1: none.  rate = k > 0: from now
 * on dqmc_mc_sweep runs one round after every sweep whose global index is a multiple of k, after that sweep's cluster
 * move if it has one and before its measurement; rate 0 (or no ladders): dqmc_mc_sweep runs none and behaves as on a
 * handle that never had exchange (with R >= 2 dqmc_mc_exchange still works).  Resets the cursor, the labels and the
 * exchange counters.  The results do not depend on how a run is split into calls of dqmc_mc_sweep. */
int dqmc_mc_set_exchange(dqmc_mc_handle *h, int32_t n_replicas, int32_t rate);
/* one round at the cursor by hand (a launch of its own); it takes no measurement.  Without ladders: DQMC_ERR_STATE */
int dqmc_mc_exchange(dqmc_mc_handle *h);
/* the exchange counters of the pair (walker, walker + 1), the label of the replica now in the slot, and the cursor */
typedef struct {
    int64_t prop_exchange, acc_exchange;
    int64_t replica;
    uint64_t rounds;
} dqmc_mc_exchange_stats;
int dqmc_mc_get_exchange_stats(dqmc_mc_handle *h, int32_t walker, dqmc_mc_exchange_stats *out);
/* 1: dqmc_mc_sweep runs its rounds inside the sweep kernel (64 % R == 0: a ladder never straddles a wave; the spins
 * change columns in LDS), except a round that follows a cluster move; 0: every round is a launch of its own on the state
 * in device memory (any other R), or dqmc_mc_sweep runs no rounds */
int dqmc_mc_exchange_fused(dqmc_mc_handle *h, int32_t *fused);
/* Checkerboard sweeps: the local update of one walker spread over a whole workgroup.  sweep(mc) of the reference is
 * sequential, so this is another Markov chain: like the cluster move and replica exchange a defined extension, opt-in,
 * on a Philox domain of its own.  A colouring gives every site a colour c_i in [0, C), C <= 16, such that no site shares
 * its colour with any entry of its neighs column (a repeated neighbour is fine and counts twice in dE, as on
 * SquareLattice(2); a site that lists itself as a neighbour cannot be coloured: DQMC_ERR_INVALID).  A checkerboard sweep
 * of a walker visits the colours 0 .. C - 1 in order; within a colour every site i (0-based) is decided from the
 * configuration as it stood when the colour began: dE = 2 s_i sum_k s_{neighs[k, i]}, accepted iff dE <= 0 ||
 * u_cb(s, i) < thr[dE / 2 - 1] with the per-walker table exp(-beta 2k) of dqmc_mc_set_beta, compared in fp64 (no exp on
 * the device).  u_cb(s, i) is Philox4x32-10 with the slot's key and counter words (i, low32(s), 3, high32(s)), where s
 * counts the checkerboard sweeps the slot has run since dqmc_mc_seed: a fourth domain (word 2 is 0 for the local stream,
 * 1 for the cluster move, 2 for exchange).  It matters only where dE > 0 and is formed only there; uniforms_used, the
 * move cursor and the exchange cursor do not move.  The sites of a colour share no bond, so the outcome is one
 * configuration whatever order the device takes them in, dE is additive within a colour, and E and M stay exact
 * integers: a host restatement reproduces every sweep bit for bit.  prop_local += n_sites per sweep, acc_local counts
 * the accepted sites.  Everything else keeps its place: sweep i is followed by its cluster move, its exchange round
 * (always a launch of its own in this mode: dqmc_mc_exchange_fused answers 0), its measurement and its FSS measurement;
 * an exchange leaves s with the slot, like every other cursor.  Each colour pass is a product of commuting single-site
 * Metropolis kernels, each of which satisfies detailed balance, so the sweep leaves the Boltzmann weight invariant. */
#define DQMC_MC_UPDATE_SEQUENTIAL   0
#define DQMC_MC_UPDATE_CHECKERBOARD 1
/* kind 0 (the default): the sequential sweep, exactly as on a handle that never heard of this call (colour is ignored).
 * kind 1: checkerboard sweeps with the caller's colouring, colour[i] in [0, n_colours), 1 <= n_colours <= 16 (copied).
 * It is validated on the host before the device is touched: DQMC_ERR_INVALID names the offending pair of sites, and the
 * handle stays as it was.  May be called at any time between sweeps; it touches neither the configurations, the sums
 * nor any cursor (only dqmc_mc_seed zeroes sweeps_drawn). */
int dqmc_mc_set_update(dqmc_mc_handle *h, int32_t kind, const int32_t *colour /* n_sites, NULL for kind 0 */,
                       int32_t n_colours);
typedef struct {
    int32_t kind, n_colours; /* n_colours = 0 in sequential mode */
    uint64_t sweeps_drawn;   /* the slot's checkerboard sweep cursor s */
} dqmc_mc_update_stats;
int dqmc_mc_get_update(dqmc_mc_handle *h, int32_t walker, dqmc_mc_update_stats *out);
int dqmc_mc_synchronize(dqmc_mc_handle *h);

/* ---- error bars of the MC flavor: one logarithmic binner per walker, pushed inside the sweep --------------------
 * measure! of IsingEnergyMeasurement / IsingMagnetizationMeasurement pushes E, E^2, |M| and M^2 into Observables
 * (models/Ising/measurements.jl:30-35,72-78), and finish! takes their means (:37-42,80-85).  Here
 * every walker has one binner over the four elements [E, E2, M, M2] (M = |M|) under the contract of "error bars" above:
 * L = ceil(log2(capacity + 1)) levels; per level and walker x_sum[4], x2_sum[4], a one-value compressor [4] (none on the
 * top level) and the cross sums xy_sum[2] of the pairs (E, E2) and (M, M2), which take the product of the pair's two
 * level-l values wherever x2_sum[l] takes the squares.  Device layout [level][element][walker].  All walkers measure at
 * the same sweeps, so the push count T and count[l] = floor(T / 2^l) are host integers.  Per level, n = count[l]:
 * varN as above, covN = (xy_sum/(n-1) - x_sum y_sum/(n(n-1)))/n, NaN below two samples; this is what the error of
 * C = beta^2/N (<E2> - <E>^2) and chi = beta/N (<M2> - <M>^2) (measurements.jl:40,83) needs:
 * var(C) = (beta^2/N)^2 (varN(E2) - 4 <E> covN(E, E2) + 4 <E>^2 varN(E)).
 * Once enabled, dqmc_mc_sweep pushes every measurement it takes, in the sweep kernel itself (and right after the
 * cluster move for a measurement that follows one); the sums, series and chains are exactly those of a handle without
 * a binner.  dqmc_mc_sweep counts the measurements of a call beforehand: if they would pass the capacity it returns
 * DQMC_ERR_STATE and nothing has run (the reference: OverflowError of push!).  dqmc_mc_reset_accumulators clears the
 * binner and its count; dqmc_mc_global_move takes no measurement and pushes nothing.  With the binner off nothing is
 * allocated and the launches are those of a handle that never had one. */
/* LogBinner(zero, capacity = capacity) behind each Observable (measurements/generic.jl:39; capacity 0 = 100000,
 * generic.jl:68-88).  Enabling again starts anew. */
int dqmc_mc_binner_enable(dqmc_mc_handle *h, int64_t capacity);
/* levels and pushes so far (length of the Observables measure! pushes into, measurements.jl:30-35); either may be NULL */
int dqmc_mc_binner_size(dqmc_mc_handle *h, int32_t *n_levels, int64_t *n_pushed);
/* the level std_error and tau use (generic.jl:60-61): the last one with count >= 32, else 0 */
int dqmc_mc_binner_reliable_level(dqmc_mc_handle *h, int32_t *level);
/* the sums of one level of one walker in element order [E, E2, M, M2] / pair order [(E, E2), (M, M2)] and the level's
 * count; any output may be NULL */
int dqmc_mc_binner_get_level(dqmc_mc_handle *h, int32_t walker, int32_t level,
                             double x_sum[4], double x2_sum[4], double xy_sum[2], int64_t *count);
/* mean, std_error^2 and tau of the Observables of one walker (generic.jl:58-61; mean(m.E), mean(m.E2) of finish!,
 * measurements.jl:38-39,81-82) and the covariances behind the errors of C and chi (measurements.jl:40,83) */
typedef struct {
    double mean[4];   /* x_sum[0] / count[0] */
    double varN[4];   /* at `level`; std_error = sqrt(max(varN, 0)) */
    double varN0[4];  /* at level 0 */
    double tau[4];    /* (varN / varN0 - 1) / 2 */
    double covN[2];   /* at `level`, pairs (E, E2) and (M, M2) */
    int64_t count;    /* count[level] */
    int32_t level;    /* the level used */
} dqmc_mc_binned;
/* level < 0: the reliable level */
int dqmc_mc_binner_finish(dqmc_mc_handle *h, int32_t walker, int32_t level, dqmc_mc_binned *out);

/* ---- finite-size-scaling observables of the MC flavor: M^4 and the structure factor S(k) ------------------------
 * The reference measures E and M only (models/Ising/measurements.jl); this is a defined extension, like the cluster
 * move and replica exchange.  The Binder cumulant U4 = 1 - <M^4>/(3 <M^2>^2) and the second-moment correlation length
 * xi = sqrt(S(0)/S(k) - 1)/(2 sin(|k|/2)), S(0) = <M^2>/N, need two functions of the configuration at the moment of
 * measurement, which is never kept:
 *   phase tables  the host passes n_k wave vectors (0 <= n_k <= 8) as fixed-point tables int32 [n_k][N], site order as
 *                 dqmc_mc_get_conf: cos_q30[k][i] = llround(cos(k . r_i) 2^30) and sin_q30[k][i] likewise.  n_k = 0
 *                 measures M^4 only.
 *   per measurement and walker
 *                 Fc_k = sum_i s_i cos_q30[k][i], Fs_k = sum_i s_i sin_q30[k][i] in 64-bit integers (|F| <= 2^14 2^30 =
 *                 2^44: exact, whatever the order of the additions; a numpy int64 sum reproduces them),
 *                 S_k = ((double)Fc (double)Fc + (double)Fs (double)Fs) * inv, inv = 1.0 / ((double)N * 2^60) (the
 *                 conversions are exact, the rest is three or four fp64 roundings depending on contraction: device and
 *                 host agree to a few ulp, not to the bit),
 *                 M4 = m2 * m2 with m2 = (double)(M M) (exact), one rounding: M4 and its running sum are bit-exact.
 *                 The entries are off by at most 2^-31 relative to the unit phase, which puts the quantisation bias of
 *                 S_k below 2^-29 relative to N (the largest value S_k takes), far under any statistical error.
 *   when          exactly where and when E and |M| of that measurement are taken: the same configuration, after that
 *                 sweep's cluster move and exchange round.  Under replica exchange the values belong to the slot ("at
 *                 beta_w"), like the other sums.
 * Per walker: sum_M4, sum_S[8] and an n_meas of their own (FSS may be switched on mid-run).  With the binner enabled a
 * second section "FSS" of its own arrays, under the same level / compressor scheme as the section above: elements
 * [M2, M4, S_0 .. S_{n_k - 1}] (M2 = M M), cross sums of the pairs (M2, M4) and (M2, S_k), device layout
 * [level][element][walker].  The four-element section, its getters and its pushes are as they are without FSS, and
 * so are the chains, the sums and the draws: with FSS on, dqmc_mc_sweep ends a launch at every measured sweep and
 * launches one measurement kernel behind it, on the state the sweep's last kernel left in device memory. */
/* n_k >= 0: FSS on with these tables (copied; either may be NULL when n_k == 0); n_k = -1: off (the default).  Resets
 * the FSS sums; if the binner is enabled it starts anew with every section empty and its capacity kept.
 * DQMC_ERR_INVALID for n_k > 8, n_k < -1, a NULL table with n_k > 0 (these two are checked before the handle), or an
 * entry above 2^30 in magnitude. */
int dqmc_mc_set_fss(dqmc_mc_handle *h, int32_t n_k, const int32_t *cos_q30, const int32_t *sin_q30);
typedef struct {
    int64_t n_meas;    /* FSS measurements summed since dqmc_mc_set_fss / dqmc_mc_reset_accumulators */
    int32_t n_k;       /* -1: FSS is off (then everything else is 0) */
    double sum_M4;
    double sum_S[8];   /* entries at and above n_k are 0 */
} dqmc_mc_fss;
int dqmc_mc_get_fss(dqmc_mc_handle *h, int32_t walker, dqmc_mc_fss *out);
/* the sums of one level of one walker of the FSS section: x_sum and x2_sum hold 2 + n_k elements [M2, M4, S_0 ..],
 * xy_sum 1 + n_k pairs [(M2, M4), (M2, S_0) ..]; any output may be NULL.  DQMC_ERR_STATE without binner or FSS. */
int dqmc_mc_fss_binner_get_level(dqmc_mc_handle *h, int32_t walker, int32_t level, double *x_sum, double *x2_sum,
                                 double *xy_sum, int64_t *count);
/* as dqmc_mc_binned, for the FSS section: entries at and above 2 + n_k (covN: 1 + n_k) are 0 */
typedef struct {
    double mean[10];   /* [M2, M4, S_0 ..] */
    double varN[10];   /* at `level` */
    double varN0[10];  /* at level 0 */
    double tau[10];
    double covN[9];    /* at `level`, pairs (M2, M4), (M2, S_0) .. */
    int64_t count;
    int32_t level;
    int32_t n_k;
} dqmc_mc_fss_binned;
/* level < 0: the reliable level (the last one with count >= 32, else 0) */
int dqmc_mc_fss_binner_finish(dqmc_mc_handle *h, int32_t walker, int32_t level, dqmc_mc_fss_binned *out);

/* ---- the classical MC flavor with q-state models: Potts and clock ------------------------------------------------
 * The reference's MC flavor is a plugin surface (energy, propose_local, accept_local!) with the IsingModel as its one
 * model; the q-state models, their update and their order parameter are a defined extension, and this comment is the
 * definition (tests/qstate_ref.py restates it).  A handle family of its own (csrc/qstate.hip): nothing of dqmc_mc_*
 * takes part.  fl(.) is one IEEE fp64 rounding; the object file is compiled with -ffp-contract=off, so no product is
 * fused into a sum.
 *
 * Model.  Site variable s_i in {0 .. q - 1}, 2 <= q <= 64, and a pair-energy table e[d] over d = (s_i - s_j) mod q with
 * e[d] = e[(q - d) mod q]: E = -J sum_bonds e[(s_i - s_j) mod q] over the undirected bonds table.  Potts: e[d] = delta_{d,0};
 * clock: e[d] = cos(2 pi d / q).  The host passes three fixed-point tables, e_q30[d] = llround(J e[d] 2^30) (int64,
 * |e_q30| <= 2^32, symmetric), c_q30[s] = llround(cos(2 pi s / q) 2^30) and s_q30[s] = llround(sin(2 pi s / q) 2^30)
 * (int32, magnitude <= 2^30).  A walker's energy is the exact int64 E_int = -sum_bonds e_q30[d] (|E_int| <= 2^16 2^32)
 * and its order parameter the exact int64 pair (Mx, My) = sum_i (c_q30[s_i], s_q30[s_i]) (magnitude <= 2^44); integer
 * sums are exact in any order, so the device's reductions and a numpy int64 sum agree.  For q = 2, My = 0.
 *
 * Uniforms.  P(key; c0, c1, c2, c3) is Philox4x32-10 with key = the walker's seed; its output words (o0, o1, o2, o3) give
 * two uniforms by the conversion of philox4_uniform (csrc/kernels.h): u1 = (((o0 >> 5) << 26) | (o1 >> 6)) 2^-53 and
 * u2 = (((o2 >> 5) << 26) | (o3 >> 6)) 2^-53.  Domain word c2 = 4: the sweep, P(key; i, low32(s), 4, high32(s)) for site
 * i (0-based) in the walker's sweep s, the number of sweeps the walker has run since dqmc_qs_seed.  Domain word c2 = 5:
 * the initial configuration, P(key; i, low32(r), 5, high32(r)), r = the dqmc_qs_rand_conf calls the walker has had since
 * dqmc_qs_seed; site i takes min(q - 1, (int)fl(u1 q)), u2 is not used.  (Words 0..3 are the Ising flavor's domains.)
 *
 * Sweep.  One workgroup per walker; the sites as bytes and the walker's weight table in LDS.  A colouring gives every
 * site a colour in [0, C), C <= 16, such that no site shares its colour with any entry of its neighs column (a repeated
 * neighbour is fine and counts twice, as on SquareLattice(2); a site that lists itself cannot be coloured).  A sweep
 * visits the colours 0 .. C - 1 in order; within a colour every site is decided from the configuration as it stood
 * when the colour began.  For site i with state s, one call P gives (u1, u2):
 *   proposal    t = (s + 1 + min(q - 2, (int)fl(u1 (q - 1)))) mod q: uniform over the other states, the flip for q = 2
 *   for k = 0 .. z - 1, j = neighs[k, i]: a_k = (s - s_j) mod q, b_k = (t - s_j) mod q
 *   dE_int      = sum_k (e_q30[a_k] - e_q30[b_k]) in int64: exactly the change of E_int
 *   p           = 1.0, then p = fl(p w[a_k][b_k]) for k = 0 .. z - 1 in order, with the walker's table
 *                 w[a][b] = exp(fl(-beta fl((double)(e_q30[a] - e_q30[b]) 2^-30))), q^2 doubles from the host's libm
 *                 (dqmc_qs_set_beta); no exp on the device, only exactly rounded products
 *   accept iff  dE_int <= 0 || u2 < p
 * Both uniforms are formed for every site, whatever it decides: the sweep cursor alone positions the stream.  The sites
 * of a colour share no bond, so the outcome is one configuration whatever order the device takes them in and dE_int is
 * additive within a colour: a host restatement reproduces every sweep bit for bit.  prop_local += n_sites per sweep,
 * acc_local counts the accepted sites.  The proposal is symmetric and each single-site kernel accepts with
 * min(1, p(s -> t)); p(s -> t) p(t -> s) = 1 and p = exp(-beta dE) hold up to the rounding of z factors and z - 1
 * products, about z ulp of p (|p exp(beta dE) - 1| <= (2 z - 1) 2^-53 to first order, plus libm's error per factor):
 * that relative error of the acceptance probability is the size of the deviation from exact detailed balance.  A
 * colour pass is a product of commuting single-site Metropolis kernels, so the sweep leaves the Boltzmann weight of
 * E_int 2^-30 invariant to that accuracy.
 * Domain of beta.  The decision u2 < p is consulted exactly where dE_int > 0, so a partial product that left the finite
 * range would corrupt it: inf times a later factor accepts an uphill move whose true p is small, 0 or NaN rejects one
 * whose true p is moderate.  Every partial product is the exponential of a sum of at most z exponents, each within
 * beta range of zero, range = (max_d e_q30[d] - min_d e_q30[d]) 2^-30 (exact in fp64).  dqmc_qs_set_beta therefore
 * accepts beta iff fl(fl(beta z) range) <= 700: then every partial product lies in [e^-700, e^700], finite, non-zero
 * and normal (e^-700 = 1e-304 > DBL_MIN, e^700 < DBL_MAX), and the rounding of at most 8 factors cannot move it across
 * either edge.  A beta outside is refused with DQMC_ERR_INVALID; the message names beta, z, the range and the bound,
 * and the walker's beta, table and exchange tables stay as they were.  (|J e| = 4 of both signs and z = 8: beta <= 10.9;
 * Potts with J = 1 on a square lattice: beta <= 175.)  The exchange tables need no such guard: their products have
 * factors <= 1 only and can do no worse than underflow monotonically to 0, a correct "reject".
 *
 * Measurement.  After the sweep with global index i (first_sweep_index, first_sweep_index + 1, ..) iff
 * i > thermalization && i % measure_rate == 0 (the rule of dqmc_mc_sweep), inside the kernel, in this order of operations:
 *   e = (double)E_int 2^-30, x = (double)Mx 2^-30, y = (double)My 2^-30 (exact: conversions below 2^53, powers of two)
 *   m2 = fl(fl(x x) + fl(y y))
 *   sum_E += e, sum_E2 += fl(e e), sum_M2 += m2, sum_M4 += fl(m2 m2), sum_absM += sqrt(m2), n_meas += 1
 * each sum one rounding per measurement, in the order of the measurements.  numpy reproduces all of them bit for bit
 * except sum_absM where the device's fp64 sqrt is not the correctly rounded one: that sum is compared at 1e-13 relative.
 * While fewer than series_capacity measurements are recorded, (E_int, Mx, My) is appended to the walker's series.
 * U4 = 1 - <M^4> / (2 <M^2>^2) is the Binder cumulant of a two-component order parameter (0 in the disordered phase).
 * The results do not depend on how a run is split into calls of dqmc_qs_sweep.
 *
 * Cluster move (dqmc_qs_set_cluster_rate, dqmc_qs_cluster_move).  A cluster move in Wolff's embedding: for a symmetric
 * table the reflection s -> (r - s) mod q maps the difference d of a bond to -d when both ends are reflected, so it is a
 * symmetry of every bond; reflecting one end takes the bond from difference a to difference b at the cost
 * e[a] - e[b].  For Potts models this is the Wolff move (clusters of equal states, bond probability 1 - exp(-beta J)),
 * for clock models Wolff's reflection restricted to the q lattice axes.  Domain word c2 = 6; m is the walker's move
 * cursor, the cluster moves since dqmc_qs_seed (which sets it to 0): P(key; t, low32(m), 6, high32(m)) gives (u1, u2).
 * The sweep and configuration streams are not touched.
 *   seed        t = 0: i0 = min(N - 1, (int)fl(u1 N)), N = n_sites
 *   reflection  r = (2 s_i0 + 1 + min(q - 2, (int)fl(u2 (q - 1)))) mod q: uniform over the q - 1 reflections that move
 *               the seed's state, the flip for q = 2
 *   slot (i, k) the directed slot of site i (0-based) and k < z uses t = 1 + 8 i + k and u1 only.  With j = neighs[k, i]
 *               and the states as they stood before the move: a = (s_i - s_j) mod q, b = (r - s_i - s_j) mod q; the slot
 *               is active iff e_q30[a] > e_q30[b] && u1 < fl(1.0 - w[a][b]), with the walker's table w
 *   cluster     C = the sites reachable from i0 through active slots (i0 itself at least).  The set does not depend on
 *               the order in which slots are examined; a slot is drawn only where it is needed, and the stream is
 *               addressed by (m, i, k), not by position
 *   move        s_i <- (r - s_i) mod q for every i in C
 *   dE_int      = sum_{i in C} sum_k [neighs[k, i] not in C] (e_q30[a] - e_q30[b]) in int64: bonds inside C do not
 *               change by the symmetry of e, a repeated neighbour counts twice as in the local rule, and on
 *               TriangularLattice the running E stays "bonds energy of the start plus neighbour differences"
 *   dMx, dMy    = sum_{i in C} (c_q30, s_q30)[new] - (c_q30, s_q30)[old]: integers, exact in any order
 *   counters    prop_global += 1, acc_global += (|C| > 1), sum_cluster_size += |C|, moves_drawn = m + 1
 * The move is never rejected.  With p = fl(1 - w[a][b]) = 1 - exp(-beta (e[a] - e[b])) up to the rounding of one table
 * entry and one subtraction, the probability of growing C and not growing it across its boundary differs between a
 * configuration and its image by the factor exp(-beta dE) to about one ulp per boundary slot: detailed balance for the
 * Boltzmann weight of E_int 2^-30, to the accuracy the sweep has.  With cluster rate k > 0 the sweep with global index
 * i runs one move per walker iff i % k == 0, in the order sweep i, its move, its measurement; rate 0 (the default)
 * leaves every stream, sum and launch as without the feature.  The results do not depend on how a run is split into
 * calls of dqmc_qs_sweep, nor on the number of walkers in the handle.
 *
 * Replica exchange (dqmc_qs_set_exchange, dqmc_qs_exchange).  As dqmc_mc_set_exchange: the walkers form n_walkers / R
 * ladders of R consecutive slots.  Slot w keeps what belongs to its temperature: beta and its table w[q][q], the key, the
 * sweep cursor s, the move cursor m and the conf cursor r, the sums, the series, the binner and every counter.  An
 * accepted exchange of the pair (a, b = a + 1) swaps the configurations (the Nw = ceil(N / 4) words), E_int, Mx, My and a
 * replica label, which starts as the slot's index within its ladder.  The handle keeps an exchange cursor x, the rounds
 * since dqmc_qs_set_exchange; round x tries the pairs with ladder-local i = x (mod 2), i + 1 < R.
 *   d           = E_a - E_b, an exact int64 in units of 2^-30
 *   db          = beta_a - beta_b in fp64 on the host; the betas need not be monotone
 *   swap if     db == 0, d == 0, or db and d have the same sign
 *   otherwise   p = 1.0, then p = fl(p t[j]) for every set bit j of |d| in ascending order, with the per-pair table
 *               t[j] = exp(-fl(|db| 2^(j - 30))), j < J, from the host's libm (the scaling by a power of two is exact, so
 *               exp sees one rounded argument; no exp on the device).  J is the smallest integer with
 *               2^J > 2 n_bonds max_d |e_q30[d]| >= |d|: 50 at the create-time limits (2^16 bonds, |e_q30| <= 2^32); a
 *               handle whose J would exceed 62 is refused (DQMC_ERR_INVALID).  dqmc_qs_set_beta rebuilds the tables of
 *               the at most two pairs a slot belongs to.
 *   swap iff    u < p, u = u1 of P(key_a; 0, low32(x), 7, high32(x)): domain word c2 = 7, a fourth q-state domain (4 the
 *               sweep, 5 the configuration, 6 the cluster move).  No other cursor moves.
 *   counters    per slot a: prop_exchange / acc_exchange count the tries and swaps of the pair (a, a + 1); the last slot
 *               of a ladder stays 0
 * Every decision can be reproduced bit for bit.  p differs from exp(db d) by the error of libm and one rounding per
 * factor and one per product: at most about 2 J ulp, |p exp(-db d) - 1| <= 2 J 2^-53 to first order with a correctly
 * rounded exp.  That relative error of the acceptance probability is the size of the deviation from exact detailed
 * balance (a chain that used p for both directions of every pair would be exact; the rule is symmetric in a and b).
 *
 * Order inside a sweep.  The sweep with global index i runs, in this order: its colour passes; its cluster move iff
 * cluster rate > 0 && i % cluster rate == 0; its exchange round iff exchange rate k > 0 && R >= 2 && i % k == 0; its
 * measurement by the rule above, of every slot, on the configuration the slot then holds.  The measurement of a sweep
 * with a round is taken by the exchange kernel.  Results do not depend on how a run is split into dqmc_qs_sweep calls.
 *
 * Binner (dqmc_qs_binner_enable).  One logarithmic binner per walker under the contract of "error bars" above, pushed
 * wherever a measurement is taken, behind the sums and the series record.  Six elements [E, E2, |M|, M2, M2, M4] with
 * the values the sums use: e, fl(e e), sqrt(m2), m2, m2, fl(m2 m2); M2 is kept twice so that pair p is the elements
 * (2 p, 2 p + 1): (E, E2), (|M|, M2), (M2, M4), whose cross sums xy_sum[3] take the product of the pair's two level-l
 * values wherever x2_sum[l] takes the squares.  L = ceil(log2(capacity + 1)) levels, a one-value compressor per element
 * below the top level, device layout [level][element][walker]; all walkers measure at the same sweeps, so the push
 * count T and count[l] = T >> l are host integers, and the level a push stops at is the number of trailing 1-bits of T.
 * varN, covN, tau and the reliable level are those of dqmc_mc_binned.  A dqmc_qs_sweep whose measurements would pass
 * the capacity returns DQMC_ERR_STATE and nothing has run.  dqmc_qs_reset_accumulators clears the binner and its count.
 * The sums, series and chains are exactly those of a handle without a binner.  The elements with a square root (|M|,
 * and the cross sum of (|M|, M2)) inherit the device's sqrt and compare at 1e-13 relative, all others bit for bit.
 *
 * Scaling (dqmc_qs_set_scaling).  The structure factor of the two-component order parameter m_i = (cos theta_i,
 * sin theta_i), theta = 2 pi s / q: S(k) = (|sum_i cos theta_i e^{i k . r_i}|^2 + |sum_i sin theta_i e^{i k . r_i}|^2) / N =
 * sum_ij m_i . m_j cos(k . (r_i - r_j)) / N, the transform of the correlation function, at up to 8 wave vectors, for the
 * second-moment correlation length xi = sqrt(S(0)/S(k) - 1)/(2 sin(|k|/2)), S(0) = <M2>/N (tests/qstate_scaling_ref.py
 * restates this part).
 *   phase tables  the host passes n_k wave vectors, 1 <= n_k <= 8, as int32 cos_q30[n_k][N] and sin_q30[n_k][N], site
 *                 order as dqmc_qs_get_conf: cos_q30[k][i] = llround(cos(k . r_i) 2^30) and the sine likewise, magnitude
 *                 <= 2^30 (the tables of dqmc_mc_set_fss).
 *   exact part    per measurement, walker and k, for every state t < q: Ac[t] = sum_{i: s_i = t} cos_q30[k][i] and
 *                 As[t] = sum_{i: s_i = t} sin_q30[k][i] in int64 (|.| <= 2^14 2^30 = 2^44: exact in any order), over the N
 *                 sites only: the zero bytes that pad a walker's last configuration word are no sites of state 0.
 *   fp64 part     u[t] A[t] can reach 2^74 and has no exact integer home, so the contraction over t is fp64 in a fixed
 *                 order.  For (u, A) = (c_q30, Ac), (c_q30, As), (s_q30, Ac), (s_q30, As) in this order:
 *                 F = +0.0; for t = 0 .. q - 1: F = fl(F + fl((double)u[t] (double)A[t])) (both conversions exact), giving
 *                 F1 .. F4.  S_k = fl(fl(fl(fl(fl(F1 F1) + fl(F2 F2)) + fl(F3 F3)) + fl(F4 F4)) inv) with
 *                 inv = 1.0 / ((double)N 2^120) from the host (N 2^120 is exact: one rounding).  numpy reproduces S_k and
 *                 its running sum bit for bit.  F1 + i F2 and F3 + i F4 are the transforms of the two components; the
 *                 complex number sum_i e^{i theta_i} e^{i k . r_i} = (F1 - F4) + i (F2 + F3) is another quantity, whose
 *                 square differs from S_k N by 2 (F2 F3 - F1 F4): zero on average, not per configuration.  For q = 2,
 *                 s_q30 = 0 and F3 = F4 = 0 exactly.  At
 *                 k = 0 (cos_q30 = 2^30, sin_q30 = 0) S_k N equals m2 of "Measurement" up to rounding, in the units of
 *                 sum_M2.  The table entries are off by at most 2^-31 each: |S_k - S(k)| <~ 2^-29 N.
 *   when          exactly where the sweep's measurement is taken by the rule of "Measurement", on the configuration E
 *                 and M are taken from: by "Order inside a sweep" after the cluster move and the exchange round.  Under
 *                 replica exchange the value belongs to the slot ("at beta_w").
 *   sums          per walker sum_S[8] (each += S_k, one rounding per measurement, in the order of the measurements) and
 *                 an n_meas of its own: the feature may be switched on mid-run.  dqmc_qs_reset_accumulators clears them.
 *   binner        with the binner enabled, a second section over the elements [M2, S_0 .. S_{n_k - 1}] under the level /
 *                 compressor scheme of the first: M2 is the m2 the first section gets, cross sums xy_sum[n_k] of the pairs
 *                 (M2, S_k), device layout [level][element][walker], a push count of its own.  The six-element section,
 *                 its getters and its pushes are as they are without the feature.  dqmc_qs_set_scaling with a binner
 *                 enabled restarts the binner with every section empty and its capacity kept; the capacity check of
 *                 dqmc_qs_sweep covers both sections.  No element has a square root: all compare bit for bit.
 * The measurement is a kernel of its own (csrc/qs_scaling.inl) that dqmc_qs_sweep launches behind every measured sweep,
 * behind the exchange kernel where that sweep has a round, on the configuration in device memory; with the feature on,
 * a launch of the sweep kernel additionally ends at every measured sweep (mc_tables.h, qs_scaling_cut).  The chains, the
 * sums, the series, the draws and the first binner section are those of a handle without the feature, and with
 * n_k = 0 (the default) so is every launch.  Results do not depend on how a run is split into dqmc_qs_sweep calls.
 *
 * Stiffness (dqmc_qs_set_stiffness).  The helicity modulus (spin stiffness) of a model whose pair energy is a function
 * e(theta_i - theta_j) of an angle theta = 2 pi s / q.  Under a uniform twist phi along the unit vector e_mu the bond
 * (i, j) gets the energy -J e(theta_i - theta_j - phi x_b), x_b = e_mu . (r_j - r_i) at minimum image, and
 *   Upsilon_mu = (1/N) d^2F/dphi^2 at phi = 0 = (<T_mu> - beta <J_mu^2>) / N,
 *   T_mu = sum_b x_b^2 d2[(s_i - s_j) mod q],  J_mu = sum_b x_b d1[(s_i - s_j) mod q],
 * d1 the first and d2 the second derivative of the pair energy with respect to the angle (clock model:
 * d1[d] = J sin(2 pi d / q), d2[d] = J cos(2 pi d / q)).  Z(phi) is a smooth function of phi even with discrete spins, so
 * the formula is an identity of the q^N-state sum (tests/qstate_stiffness_ref.py restates this part and checks it by
 * enumeration).
 *   twist tables  int64 d1_q30[q] and d2_q30[q] = llround(. 2^30), magnitude <= 2^32; d1 exactly antisymmetric,
 *                 d1[(q - d) % q] == -d1[d] (so d1[0] = 0, and d1[q/2] = 0 for even q), d2 exactly symmetric: both computed
 *                 for d <= q / 2 and mirrored, as e_q30.
 *   slot classes  a directed slot is a pair (i, k), k < z, with j = neighs[k, i].  The host passes int8 slot_class, z x
 *                 n_sites in the layout of neighs: -1 (the slot is not counted) or a class c < n_c <= 8.  A class is a bond
 *                 displacement vector; the host counts every undirected neighbour pair once, in the orientation whose
 *                 displacement is the class vector.  The engine validates ranges only: which slots are counted is the
 *                 host's definition.
 *   exact part    per measurement, walker and class, int64: I_c = sum_{(i, k) of class c} d1_q30[(s_i - s_j) mod q] and
 *                 K_c likewise with d2_q30 (|.| <= 2^17 2^32 = 2^49: exact in any order).  The padding bytes of a
 *                 walker's last configuration word are no sites.
 *   fp64 part     for each direction mu < n_dir <= 4 with the host's projections double x[n_dir][n_c], in this order and
 *                 with no product fused into a sum: G = +0.0, for c = 0 .. n_c - 1: G = fl(G + fl(x[mu][c] (double)I_c));
 *                 F = +0.0, for c = 0 .. n_c - 1: F = fl(F + fl(fl(x[mu][c] x[mu][c]) (double)K_c)); J_mu = fl(G 2^-30),
 *                 T_mu = fl(F 2^-30), J2_mu = fl(J_mu J_mu).  numpy reproduces all three bit for bit.
 *   when          exactly where E and M are measured, on that configuration: after the cluster move and the exchange
 *                 round ("at beta_w" under replica exchange).  If scaling is on as well, the scaling kernel runs first.
 *   sums          per walker sum_T[4], sum_J[4], sum_J2[4], one rounding each per measurement in measurement order, and
 *                 an n_meas of its own (the feature may be switched on mid-run).  dqmc_qs_reset_accumulators clears them.
 *                 I_c and K_c of the last sample stay readable (dqmc_qs_get_stiffness_sample).
 *   binner        with the binner enabled, a third section over the 2 n_dir elements [T_0, J2_0, T_1, J2_1, ..] under the
 *                 level / compressor scheme of the first: pair p is the elements (2 p, 2 p + 1) with one cross sum
 *                 xy_sum[p], device layout [level][element][walker], a push count of its own.  dqmc_qs_set_stiffness with
 *                 a binner enabled restarts the binner with every section empty and its capacity kept; the capacity check
 *                 of dqmc_qs_sweep covers every section.  No element has a square root: all compare bit for bit.
 * The measurement is a kernel of its own (csrc/qs_stiffness.inl) behind every measured sweep, under the launch cut of
 * "Scaling" (one cut, two trailing kernels with both features on).  The chains, the sums, the series, the draws and the
 * other binner sections are those of a handle without the feature, and with n_dir = 0 (the default) so is every launch.
 *
 * Limits: n_sites <= 16384, 1 <= z <= 8, 2 <= q <= 64, n_colours <= 16.  Errors come from dqmc_qs_last_error. */
typedef struct dqmc_qs_handle dqmc_qs_handle;

typedef struct {
    int32_t n_sites;         /* length(lattice) */
    int32_t z;               /* neighbours per site: size(l.neighs, 1) */
    int32_t q;               /* states per site */
    int32_t n_walkers;       /* independent chains batched on this device */
    int32_t device_id;
    int32_t n_bonds;         /* size(l.bonds, 1) */
    int32_t series_capacity; /* per-walker measurements recorded as a series (0 = none) */
    int32_t n_colours;       /* C */
    const int64_t *neighs;   /* l.neighs: z x n_sites, column-major, 1-based */
    const int64_t *bonds;    /* l.bonds[:, 1:2]: n_bonds x 2, column-major, 1-based */
    const int64_t *e_q30;    /* [q] */
    const int32_t *c_q30;    /* [q] */
    const int32_t *s_q30;    /* [q] */
    const int32_t *colour;   /* [n_sites], each in [0, n_colours) */
} dqmc_qs_params;

typedef struct {
    int64_t energy_q30, mx_q30, my_q30;  /* E_int, Mx, My of the configuration now in the slot */
    double sum_E, sum_E2, sum_absM, sum_M2, sum_M4;
    int64_t n_meas;                      /* measurements summed since the last dqmc_qs_reset_accumulators */
    int64_t prop_local, acc_local;
    uint64_t sweeps_drawn, confs_drawn;  /* the cursors s and r */
    int64_t n_series;                    /* measurements recorded in the series, <= series_capacity */
    int32_t n_colours;
} dqmc_qs_stats;

/* Everything is validated on the host before the device is touched; DQMC_ERR_INVALID names the offender: q outside
 * 2..64, n_sites above 16384, z outside 1..8, an index out of range, e_q30[d] != e_q30[(q - d) mod q] or an entry above
 * 2^32 in magnitude, a c_q30 / s_q30 entry above 2^30 in magnitude, and the colouring as dqmc_qs_set_colouring.  Then
 * the device (none: DQMC_ERR_NO_DEVICE).  Every walker starts with seed 0, beta 0 (w = 1) and all sites in state 0. */
int dqmc_qs_create(const dqmc_qs_params *p, dqmc_qs_handle **out);
int dqmc_qs_destroy(dqmc_qs_handle *h);
/* message of the last failing call on this handle (h may be NULL: create errors) */
const char *dqmc_qs_last_error(const dqmc_qs_handle *h);
/* the walker's stream: key = seed, the cursors s, r and m at 0 (the configuration stays) */
int dqmc_qs_seed(dqmc_qs_handle *h, int32_t walker, uint64_t seed);
/* beta finite and >= 0: builds the walker's table w on the host */
int dqmc_qs_set_beta(dqmc_qs_handle *h, int32_t walker, double beta);
/* the initial configuration at the walker's cursor r (walker < 0: every walker), then E_int, Mx, My from scratch */
int dqmc_qs_rand_conf(dqmc_qs_handle *h, int32_t walker);
/* the states in site order, each < q (else DQMC_ERR_INVALID, nothing changed); set_conf recomputes E_int, Mx and My and
 * leaves the cursors alone */
int dqmc_qs_set_conf(dqmc_qs_handle *h, int32_t walker, const uint8_t *conf);
int dqmc_qs_get_conf(dqmc_qs_handle *h, int32_t walker, uint8_t *conf);
/* another colouring from now on (copied): colour[i] in [0, n_colours), 1 <= n_colours <= 16.  Validated on the host
 * before the device is touched: DQMC_ERR_INVALID names the offending site or pair of sites, and the handle stays as it
 * was.  Between sweeps at any time; configurations, sums and cursors stay. */
int dqmc_qs_set_colouring(dqmc_qs_handle *h, const int32_t *colour, int32_t n_colours);
/* n_sweeps sweeps of every walker with the measurement rule above.  Split into launches of bounded work; complete on
 * return. */
int dqmc_qs_sweep(dqmc_qs_handle *h, int32_t n_sweeps, int64_t first_sweep_index, int64_t thermalization,
                  int32_t measure_rate);
int dqmc_qs_get_stats(dqmc_qs_handle *h, int32_t walker, dqmc_qs_stats *out);
/* the recorded (E_int, Mx, My), n_series entries each; any buffer may be NULL */
int dqmc_qs_get_series(dqmc_qs_handle *h, int32_t walker, int64_t *energy_q30, int64_t *mx_q30, int64_t *my_q30,
                       int64_t *n_recorded);
/* clear the measurement sums and series of every walker (prop_local, acc_local and the cursors stay) */
int dqmc_qs_reset_accumulators(dqmc_qs_handle *h);
int dqmc_qs_synchronize(dqmc_qs_handle *h);

typedef struct {
    int64_t prop_global, acc_global; /* cluster moves made, and those with |C| > 1 */
    int64_t sum_cluster_size;        /* sum of |C| over the moves */
    uint64_t moves_drawn;            /* the move cursor m */
} dqmc_qs_cluster_stats;
/* one cluster move per walker behind every sweep whose global index is a multiple of rate, before its measurement;
 * rate >= 0 (else DQMC_ERR_INVALID), 0 = none (the default).  The first rate > 0 reserves the larger LDS of the sweep
 * kernel with moves (DQMC_ERR_HIP and a message if the device refuses it; the rate then stays as it was). */
int dqmc_qs_set_cluster_rate(dqmc_qs_handle *h, int32_t rate);
/* one cluster move of the walker by hand, or of every walker (walker < 0), at its cursor m; E_int, Mx and My follow, no
 * measurement is taken.  Works at any rate. */
int dqmc_qs_cluster_move(dqmc_qs_handle *h, int32_t walker);
/* (dqmc_qs_seed puts moves_drawn back to 0; dqmc_qs_reset_accumulators leaves all four alone, as it leaves prop_local) */
int dqmc_qs_get_cluster_stats(dqmc_qs_handle *h, int32_t walker, dqmc_qs_cluster_stats *out);

/* n_replicas = R >= 2 defines the ladders (n_walkers % R != 0: DQMC_ERR_INVALID; so is a handle whose J would exceed
 * 62); 0 or 1: none.  rate = k > 0: from now on dqmc_qs_sweep runs one round after every sweep whose global index is a
 * multiple of k, in the order of "Order inside a sweep"; rate 0 (or no ladders): dqmc_qs_sweep runs none and behaves as
 * on a handle that never had exchange (with R >= 2 dqmc_qs_exchange still works).  Resets the cursor, the labels and the
 * exchange counters. */
int dqmc_qs_set_exchange(dqmc_qs_handle *h, int32_t n_replicas, int32_t rate);
/* one round at the cursor by hand (a launch of its own); it takes no measurement.  Without ladders: DQMC_ERR_STATE */
int dqmc_qs_exchange(dqmc_qs_handle *h);
/* the exchange counters of the pair (walker, walker + 1), the label of the replica now in the slot, and the cursor */
typedef struct {
    int64_t prop_exchange, acc_exchange;
    int64_t replica;
    uint64_t rounds;
} dqmc_qs_exchange_stats;
int dqmc_qs_get_exchange_stats(dqmc_qs_handle *h, int32_t walker, dqmc_qs_exchange_stats *out);
/* a binner per walker for `capacity` measurements (0 = 100000, at most 2^40); enabling again starts anew */
int dqmc_qs_binner_enable(dqmc_qs_handle *h, int64_t capacity);
/* levels and pushes so far; either may be NULL.  This and the calls below: DQMC_ERR_STATE without a binner */
int dqmc_qs_binner_size(dqmc_qs_handle *h, int32_t *n_levels, int64_t *n_pushed);
/* the last level with count >= 32, else 0 */
int dqmc_qs_binner_reliable_level(dqmc_qs_handle *h, int32_t *level);
/* the sums of one level of one walker in element order [E, E2, |M|, M2, M2, M4] / pair order [(E, E2), (|M|, M2),
 * (M2, M4)] and the level's count; any output may be NULL */
int dqmc_qs_binner_get_level(dqmc_qs_handle *h, int32_t walker, int32_t level,
                             double x_sum[6], double x2_sum[6], double xy_sum[3], int64_t *count);
typedef struct {
    double mean[6];   /* x_sum[0] / count[0] */
    double varN[6];   /* at `level`; std_error = sqrt(max(varN, 0)) */
    double varN0[6];  /* at level 0 */
    double tau[6];    /* (varN / varN0 - 1) / 2 */
    double covN[3];   /* at `level`, pairs (E, E2), (|M|, M2) and (M2, M4) */
    int64_t count;    /* count[level] */
    int32_t level;    /* the level used */
} dqmc_qs_binned;
/* level < 0: the reliable level */
int dqmc_qs_binner_finish(dqmc_qs_handle *h, int32_t walker, int32_t level, dqmc_qs_binned *out);

/* "Scaling" above.  n_k in 1..8: the measurement on with these tables (copied); n_k = 0: off (the default; the tables
 * are not looked at).  Resets the scaling sums; if the binner is enabled it starts anew with every section empty and
 * its capacity kept.  DQMC_ERR_INVALID for n_k outside 0..8, a NULL table with n_k > 0 (these two are checked before the
 * handle), or an entry above 2^30 in magnitude; the handle then stays as it was. */
int dqmc_qs_set_scaling(dqmc_qs_handle *h, int32_t n_k, const int32_t *cos_q30 /* [n_k][n_sites] */,
                        const int32_t *sin_q30 /* [n_k][n_sites] */);
typedef struct {
    int64_t n_meas;    /* scaling measurements summed since dqmc_qs_set_scaling / dqmc_qs_reset_accumulators */
    int32_t n_k;       /* 0: the measurement is off (then everything else is 0) */
    double sum_S[8];   /* entries at and above n_k are 0 */
} dqmc_qs_scaling;
int dqmc_qs_get_scaling(dqmc_qs_handle *h, int32_t walker, dqmc_qs_scaling *out);
/* the sums of one level of one walker of the scaling section: x_sum and x2_sum hold 1 + n_k elements [M2, S_0 ..],
 * xy_sum n_k pairs [(M2, S_0) ..]; any output may be NULL.  DQMC_ERR_STATE without a binner or with the measurement off. */
int dqmc_qs_scaling_binner_get_level(dqmc_qs_handle *h, int32_t walker, int32_t level, double *x_sum, double *x2_sum,
                                     double *xy_sum, int64_t *count);
/* as dqmc_qs_binned, for the scaling section: entries at and above 1 + n_k (covN: n_k) are 0 */
typedef struct {
    double mean[9];    /* [M2, S_0 ..] */
    double varN[9];    /* at `level` */
    double varN0[9];   /* at level 0 */
    double tau[9];
    double covN[8];    /* at `level`, pairs (M2, S_0) .. */
    int64_t count;
    int32_t level;
    int32_t n_k;
} dqmc_qs_scaling_binned;
/* level < 0: the reliable level (the last one with count >= 32, else 0) */
int dqmc_qs_scaling_binner_finish(dqmc_qs_handle *h, int32_t walker, int32_t level, dqmc_qs_scaling_binned *out);

/* "Stiffness" above.  n_dir in 1..4: the measurement on with these tables (copied); n_dir = 0: off (the default; nothing
 * else is looked at).  Resets the stiffness sums; if the binner is enabled it starts anew with every section empty and
 * its capacity kept.  Everything is checked before the device is touched: DQMC_ERR_INVALID for n_dir outside 0..4,
 * n_classes outside 1..8, a NULL table, a class outside -1..n_classes-1, a d1_q30 that is not antisymmetric or a d2_q30
 * that is not symmetric, an entry of either above 2^32 in magnitude, or an x that is not finite; the handle then stays
 * as it was. */
int dqmc_qs_set_stiffness(dqmc_qs_handle *h, int32_t n_dir, int32_t n_classes,
                          const int8_t *slot_class /* z x n_sites, column-major as neighs */,
                          const int64_t *d1_q30 /* [q] */, const int64_t *d2_q30 /* [q] */,
                          const double *x /* [n_dir][n_classes] */);
typedef struct {
    int64_t n_meas;     /* stiffness measurements summed since dqmc_qs_set_stiffness / dqmc_qs_reset_accumulators */
    int32_t n_dir;      /* 0: the measurement is off (then everything else is 0) */
    double sum_T[4];    /* entries at and above n_dir are 0 */
    double sum_J[4];
    double sum_J2[4];
} dqmc_qs_stiffness;
int dqmc_qs_get_stiffness(dqmc_qs_handle *h, int32_t walker, dqmc_qs_stiffness *out);
/* I_c and K_c of the walker's last measurement (entries at and above n_classes, and everything with the measurement
 * off or before the first measurement, are 0) */
int dqmc_qs_get_stiffness_sample(dqmc_qs_handle *h, int32_t walker, int64_t I[8], int64_t K[8]);
/* the sums of one level of one walker of the stiffness section: x_sum and x2_sum hold 2 n_dir elements
 * [T_0, J2_0, T_1, J2_1 ..], xy_sum n_dir pairs [(T_0, J2_0) ..]; any output may be NULL.  DQMC_ERR_STATE without a
 * binner or with the measurement off. */
int dqmc_qs_stiffness_binner_get_level(dqmc_qs_handle *h, int32_t walker, int32_t level, double *x_sum, double *x2_sum,
                                       double *xy_sum, int64_t *count);
/* as dqmc_qs_binned, for the stiffness section: entries at and above 2 n_dir (covN: n_dir) are 0 */
typedef struct {
    double mean[8];    /* [T_0, J2_0, T_1, J2_1 ..] */
    double varN[8];    /* at `level` */
    double varN0[8];   /* at level 0 */
    double tau[8];
    double covN[4];    /* at `level`, pairs (T_mu, J2_mu) */
    int64_t count;
    int32_t level;
    int32_t n_dir;
} dqmc_qs_stiffness_binned;
/* level < 0: the reliable level (the last one with count >= 32, else 0) */
int dqmc_qs_stiffness_binner_finish(dqmc_qs_handle *h, int32_t walker, int32_t level, dqmc_qs_stiffness_binned *out);

/* ---- checkpoint and resume of the classical MC flavor ---------------------------------------------------------------
 * save / load (FileIO.jl covers the MC flavor as well as DQMC) for the state of a dqmc_mc_handle or a dqmc_qs_handle.  As
 * for DQMC ("checkpoint and resume") the engine hands out and takes back one blob and the file around it is the host's
 * (mc.py: save / load).  Every piece of chain state lives in global memory between launches, every decision is integer or
 * exact, and the results do not depend on how a run is cut into sweep calls, so a handle that imported a blob continues
 * BYTE FOR BYTE as the exporting one would have: there is no "measurement point", a handle may be exported between any two
 * calls, and nothing is rebuilt.  The format (csrc/mc_blob.h) is one of its own; the DQMC blob is untouched by it.
 * The blob is little-endian with fixed-width fields; doubles are IEEE bit patterns.
 *   header
 *     u64 magic "DQMCMCS1"   u32 format version (1)   u32 header bytes
 *     char[16] dqmc_build_source_hash of the exporting library, zero padded (carried, never checked)
 *     the configuration: i32 engine kind (0 Ising, 1 q-state), n_sites, z, q (0: Ising), n_walkers, series_capacity,
 *       n_bonds, update kind, n_colours (0 while sequential), cluster / global rate, exchange n_replicas, exchange rate,
 *       n_k of FSS (-1 = off) / scaling (0 = off), stiffness n_dir, n_classes
 *       3 binner sections (main, FSS / scaling, stiffness): i32 on   i64 capacity   i32 L, n_elem, n_pairs, n_comp
 *       u64 FNV-1a 64 of: the neighbour table, the bonds table, e_q30, (c_q30, s_q30), the twist tables (d1_q30, d2_q30),
 *       the colouring, the per-walker betas, the k-vector phase tables, the stiffness slot classes and projections; each as
 *       the handle got it, 0 where it has none
 *     u32 records   u32 0   per record: u32 tag, u32 element bytes, u64 elements, u64 byte offset in the blob
 *   payload: the records' arrays in the order of the table, each 8-byte aligned
 *     the configurations (Ising: the bit-packed u32 words [ceil(n_sites / 32)][W]; q-state: byte states [W][4 ceil(n_sites / 4)])
 *     per walker: the Philox key; the cursors (sweep or draw, conf, cluster or Wolff move, checkerboard sweeps_drawn); the
 *     running E, M (Ising) or E_int, Mx, My (q-state); the sums of E, E2, |M|, M2 (q-state: M4) and n_meas; prop / acc of
 *     the local and of the cluster moves and sum_cluster_size; n_series and the series
 *     with ladders: the replica labels and per-pair prop / acc
 *     with FSS / scaling: sum_M4 (Ising), sum_S and their n_meas;  with stiffness: sum_T, sum_J, sum_J2, their n_meas and
 *     the last sample I, K
 *     xs, x2, xy, c of every binner section that is on
 *     u64 x 4: T of the three binner sections, the exchange cursor
 *   u64 FNV-1a 64 of every byte in front of it
 * The running energy is restored, not recomputed.  Tables that follow from the configuration (the acceptance weights of
 * beta, the exchange pair tables and signs, the colour-sorted site tables) are not in the blob: the handle has them.
 * Import checks, in this order and before its first write: the buffer holds a header; magic; version; the size the header
 * implies against n_bytes; the checksum; every configuration field against the handle (the first that differs is named
 * under *_last_error); the ranges of the state (every T <= capacity, n_series <= series_capacity, q-state bytes < q with zero
 * padding behind site n_sites, Ising padding bits zero, the replica labels a permutation within each ladder).  A refused
 * import returns DQMC_ERR_INVALID and leaves the handle exactly as it was: an export before and after gives the same
 * bytes.  Resuming on another walker count or with changed tables is refused by these checks.
 * dqmc_*_state_size: the bytes of the blob the handle would export now.  dqmc_*_state_export: synchronizes the handle's
 * stream and copies into `host_out` (n_bytes must be the size, else DQMC_ERR_INVALID); it changes nothing.
 * dqmc_*_state_import: validates on the host, copies to the device and sets the host-side state (the binner sections' T,
 * the exchange cursor, the q-state conf cursors).  A null handle: DQMC_ERR_INVALID. */
int dqmc_mc_state_size(dqmc_mc_handle *h, size_t *n_bytes);
int dqmc_mc_state_export(dqmc_mc_handle *h, void *host_out, size_t n_bytes);
int dqmc_mc_state_import(dqmc_mc_handle *h, const void *host_in, size_t n_bytes);
int dqmc_qs_state_size(dqmc_qs_handle *h, size_t *n_bytes);
int dqmc_qs_state_export(dqmc_qs_handle *h, void *host_out, size_t n_bytes);
int dqmc_qs_state_import(dqmc_qs_handle *h, const void *host_in, size_t n_bytes);

/* ---- the SAC flavor: stochastic analytic continuation -----------------------------------------------------------
 * A(omega) from imaginary-time data by sampling (Sandvik, PRB 57, 10287; Beach, cond-mat/0403055; Shao and Sandvik,
 * Phys. Rep. 1003), batched over P independent problems (momenta) and R sampling temperatures each (csrc/sac.hip).
 * The reference has nothing of the kind: like the cluster move and replica exchange this is a defined extension, and
 * this comment is the definition (tests/sac_ref.py restates it).  fl(.) is one IEEE fp64 rounding; the object file is
 * compiled with -ffp-contract=off, so no product is fused into a sum.
 *
 * A problem p < P has Nt data points g[i], weights w[i] = 1 / sigma_i^2 and a kernel table Kt[j][i], j < Nw, stored
 * grid-major (the Nt values of one grid point are contiguous).  The host has rotated g and Kt into the eigenbasis of the
 * covariance; the device never sees a covariance.  The spectrum is Nd delta functions of equal amplitude
 * a = fl(norm / Nd) at integer grid positions x[d].  Limits: 1 <= Nt <= 256, 1 <= Nd <= 4096, 2 <= Nw <= 65535.
 *
 * A chain is (p, r), r < R <= 16, with sampling temperature theta[p][r] > 0.  Its state is x[Nd] (uint16), the residual
 * res[i] = a sum_d Kt[x_d][i] - g[i], chi2 = sum_i w_i res_i^2 and a move counter m (moves since dqmc_sac_seed).  Its
 * uniform u(m, t), t in {0, 1}, is Philox4x32-10 made into a uniform as philox4_uniform (csrc/kernels.h) does, with
 * key = the chain's seed and counter words (low32(m), high32(m), t, 0).  Both uniforms of a move are consumed whatever
 * the move does, so m alone positions the stream.
 *
 * The lane sum L(t) of t[0 .. Nt): p_l = t[l] + t[l + 64] + .. in increasing index for l < 64, entries at and above Nt
 * being +0.0 (with one entry per lane p_l is that entry); then p_l <- p_l + p_{l xor off} for off = 32, 16, 8, 4, 2, 1;
 * L = p_0.  In numpy: pad to a multiple of 64, add the rows of the [.][64] image in order, then
 * while len(p) > 1: h = len(p) // 2; p = p[:h] + p[h:].
 *
 * A sweep makes Nd moves, d = 0 .. Nd - 1 in order; move d has counter m and leaves m + 1:
 *   x' = x_d + (int)floor(fl(u(m, 0) (2 win + 1))) - win, win >= 1 the chain's window.  x' outside [0, Nw): rejected.
 *   Otherwise D_i = fl(a fl(Kt[x'][i] - Kt[x_d][i])), t_i = fl(fl(w_i D_i) fl(fl(2 res_i) + D_i)), dchi = L(t);
 *   accept iff dchi <= 0 || u(m, 1) < exp(fl(-dchi / fl(2 theta))) (the exponential only when dchi > 0; the device's exp
 *   and the host's may differ in the last bit, which decides with probability ~1e-16 per move);
 *   on accept res_i <- fl(res_i + D_i), chi2 <- fl(chi2 + dchi), x_d <- x'.
 * prop counts every move, acc the accepted ones, both from the creation of the handle.
 *
 * After the sweep with global index i (first_sweep_index, first_sweep_index + 1, ..), in this order:
 *  - refresh, iff refresh > 0 && i % refresh == 0: S_i = Kt[x_0][i] + Kt[x_1][i] + .. added in increasing d from +0.0,
 *    res_i = fl(fl(a S_i) - g_i), fresh = L(fl(fl(w_i res_i) res_i)); max_drift = max(max_drift, |chi2 - fresh|), then
 *    chi2 = fresh.  dqmc_sac_set_problem and dqmc_sac_set_conf build res and chi2 the same way.
 *  - an exchange round, iff rate > 0 && R >= 2 && i % rate == 0.  The handle keeps a cursor X, the rounds since
 *    dqmc_sac_set_exchange.  Round X tries the pairs (r, r + 1) of every problem with r = X (mod 2), r + 1 < R:
 *    q = fl(fl(fl(1 / fl(2 theta_r)) - fl(1 / fl(2 theta_{r+1}))) fl(chi2_r - chi2_{r+1})); the pair swaps iff
 *    q >= 0 || u < exp(q), u = Philox4x32-10 with the key of slot r and counter words (low32(X), high32(X), 0, 1): a
 *    domain of its own (the moves have word 3 = 0), formed only when it decides.  As in dqmc_mc_set_exchange theta,
 *    seed, move counter, window, sums, histogram and counters stay with the slot (p, r); the configuration (x, res,
 *    chi2) and a replica label (at first r) move.  prop_exchange / acc_exchange of slot r count the tries and swaps of
 *    the pair (r, r + 1).
 *  - a measurement, iff i > thermalization: hist[x_d] += 1 for every d (uint64), sum_chi2 += chi2,
 *    sum_chi2_sq += fl(chi2 chi2), min_chi2 = min(min_chi2, chi2), n_meas += 1.
 * A chain's results depend on its own problem, ladder and seeds only: not on P, not on the other problems, and not on
 * how n_sweeps is split over calls of dqmc_sac_sweep.  Errors come from dqmc_sac_last_error. */
typedef struct dqmc_sac_handle dqmc_sac_handle;

typedef struct {
    int32_t n_problems;  /* P */
    int32_t n_tau;       /* Nt */
    int32_t n_deltas;    /* Nd */
    int32_t n_omega;     /* Nw */
    int32_t n_replicas;  /* R */
    int32_t device_id;
    int32_t window;      /* every chain's window at first, in 1..2^24 */
    const double *theta; /* R values every problem's ladder starts with; NULL: 1.0 */
} dqmc_sac_params;

typedef struct {
    double chi2;                            /* of the configuration now in the slot */
    double sum_chi2, sum_chi2_sq, min_chi2; /* over the measurements; min_chi2 = +inf while n_meas == 0 */
    double max_drift;                       /* largest |running chi2 - rebuilt chi2| a refresh has seen */
    int64_t n_meas, prop, acc, prop_exchange, acc_exchange;
    int64_t replica;                        /* label of the configuration now in the slot */
    uint64_t moves_drawn;                   /* m */
    uint64_t rounds;                        /* the handle's exchange cursor */
    int32_t window;
} dqmc_sac_stats;

/* validates the arguments, then the device (no device: DQMC_ERR_NO_DEVICE), as dqmc_mc_create.  Every chain starts with
 * x = 0, seed 0, m = 0, label r; the tables are zero until dqmc_sac_set_problem */
int dqmc_sac_create(const dqmc_sac_params *p, dqmc_sac_handle **out);
int dqmc_sac_destroy(dqmc_sac_handle *h);
/* message of the last failing call on this handle (h may be NULL: create errors) */
const char *dqmc_sac_last_error(const dqmc_sac_handle *h);
/* g[Nt], w[Nt] (finite, >= 0), Kt[Nw][Nt] and norm > 0 of problem p; rebuilds res and chi2 of its R chains */
int dqmc_sac_set_problem(dqmc_sac_handle *h, int32_t p, const double *g, const double *w, const double *Kt, double norm);
/* the R sampling temperatures of problem p, each finite and > 0; they need not be monotone */
int dqmc_sac_set_theta(dqmc_sac_handle *h, int32_t p, const double *theta);
/* the chain's stream: key = seed, m = 0 */
int dqmc_sac_seed(dqmc_sac_handle *h, int32_t p, int32_t r, uint64_t seed);
/* x[Nd], every entry < Nw; set_conf rebuilds res and chi2 and leaves m, the label and every sum alone */
int dqmc_sac_set_conf(dqmc_sac_handle *h, int32_t p, int32_t r, const uint16_t *x);
int dqmc_sac_get_conf(dqmc_sac_handle *h, int32_t p, int32_t r, uint16_t *x);
/* the chain's window, in 1..2^24 (it may exceed Nw) */
int dqmc_sac_set_window(dqmc_sac_handle *h, int32_t p, int32_t r, int32_t win);
/* rate = k > 0: dqmc_sac_sweep runs one round after every sweep whose global index is a multiple of k; 0: none.
 * Resets the cursor, the labels and the exchange counters */
int dqmc_sac_set_exchange(dqmc_sac_handle *h, int32_t rate);
/* n_sweeps sweeps of every chain with global indices first_sweep_index (>= 1) ..; refresh >= 0 (0: never).  Split into
 * launches of bounded work; complete on return */
int dqmc_sac_sweep(dqmc_sac_handle *h, int32_t n_sweeps, int64_t first_sweep_index, int64_t thermalization,
                   int32_t refresh);
int dqmc_sac_get_stats(dqmc_sac_handle *h, int32_t p, int32_t r, dqmc_sac_stats *out);
/* hist[Nw] of the slot (p, r) */
int dqmc_sac_get_histogram(dqmc_sac_handle *h, int32_t p, int32_t r, uint64_t *hist);
/* clears hist, sum_chi2, sum_chi2_sq, min_chi2 and n_meas of every chain; the chains, prop, acc, the exchange counters
 * and max_drift stay */
int dqmc_sac_reset_accumulators(dqmc_sac_handle *h);

/* ---- instrumentation ------------------------------------------------------ */
/* Per-kernel-family device time accumulated with HIP events on the handle's
 * stream when enabled (off by default; used by bench.py's roofline leg). */
enum { DQMC_K_GEMM = 0, DQMC_K_QR = 1, DQMC_K_TRSM = 2, DQMC_K_SWEEP = 3, DQMC_K_MISC = 4, DQMC_K_FLUSH = 5,
       DQMC_K_COUNT = 6 };
int dqmc_timing_enable(dqmc_handle *h, int32_t on);
int dqmc_timing_get(dqmc_handle *h, double *ms /* DQMC_K_COUNT */, int64_t *launches /* DQMC_K_COUNT */);
/* fp64 MFMA micro-benchmark: issues `iters` dependent-free v_mfma_f64_16x16x4_f64
 * per wave on every CU, returns achieved TFLOP/s (confirms the roofline peak) */
int dqmc_mfma_f64_peak(int32_t device_id, int32_t iters, double *tflops);

#ifdef __cplusplus
}
#endif
#endif
