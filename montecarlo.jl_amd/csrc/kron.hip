// kron.hip — slice-matrix chains and wraps with the hopping exponential applied in Kronecker-factored form (n = 256).
//
// On the periodic 16 x 16 SquareLattice (site i = x + 16 y) every hopping exponential is, up to rounding, a Kronecker
// product A = Ay (x) Ax of two 16 x 16 matrices (hopping_forms.h: kron_split checks it at handle creation).  A column v of
// 256 entries, read as the 16 x 16 matrix V[x][y] = v[x + 16 y], then gives (A v) = vec(Ax V Ay^T): two 16-contractions,
// 8 v_mfma_f64_16x16x4_f64 per column instead of the 64 of the dense product.
//
//   X_s = post_s (.) ( A_s * ( pre_s (.) X_{s-1} ) ),  s = 1 .. nsteps,    out = X_nsteps (.) col_d   (or its transpose)
//
// with the argument conventions and scaling placement of slab.hip.  Used for
//   * add_slice_sequence_left/right (stack.jl:272-311): the safe_mult products B_l X / B_l' X;
//   * wrap_greens! (stack.jl:491-500) as two one-step chains with transposed stores (engine.cpp: wrap_greens_kron): in one
//     launch with a hand-off per unit where the grid is co-resident (kron_wrap_kernel), else as two launches.
//
// Layout.  A wave holds a column as one MFMA accumulator tile (4 doubles per lane): register r of lane (g = lane >> 4,
// c = lane & 15) is V[a = g + 4 r][b = c], where (a, b) = (y, x) or (x, y) by step parity.  Register q of that tile is
// also the B operand of k-block q of a product that sums over a, so P = Fa V needs no data movement; P^T goes through
// LDS once (a 16 x 17 tile per column), and Q = Fb P^T leaves the tile with its roles swapped.  So each step is one
// transpose, and the parity alternates: (y, x) at the start, where a load of one register is 64 consecutive doubles.
// Columns are independent: a workgroup (4 waves x KR_NC columns) owns 16 consecutive columns through all steps, and
// nothing crosses workgroups.  The result is staged in LDS and stored as whole 128-byte lines, as is or transposed.
//
// Pending chunk (KronArgs::pf_img, the first chain of a wrap behind a sweep).  The sweep leaves its last chunk c of 64
// sites eliminated but not applied: G' = G + T R0 with T = C X Y, C = G[:, c] - E, Y = (I - Uu X)^-1 (I - L X)^-1,
// R0 = G[c, :] (sweep_lu.hip).  A workgroup owns whole columns j, so it forms G'[:, j] = G[:, j] + C R^[:, j] with
// R^ = X Y R0 re-associated onto the rows (the stand-alone flush solves on the columns of C instead):
//   XV_J = X_J Q_J (R0_J + sum_{K<J} L_JK XV_K),   R^_J = PT_J (XV_J + X_J sum_{K>J} Uu_JK R^_K)
// (blocks of 16 sites, image tiles as in kernels.h, each taken as the A operand of its own matrix), then 256 x 64 x 16 of
// MFMA with C read from G.  R0 is register (site0 / 64) of the X_0 tiles already loaded.
#include "factored_common.h"

namespace dqmc {

constexpr int KR_N = 256;
constexpr int KR_NC = 4;                 // columns per wave
constexpr int KR_COLS = 4 * KR_NC;       // columns per workgroup
constexpr int KR_TLD = 17;               // row stride of a transpose tile (doubles)
constexpr int KR_SLD = 18;               // row stride of the transposed staging image (doubles; even: 16-byte reads)
constexpr int KR_LDS_T = 4 * KR_NC * 16 * KR_TLD;  // transpose tiles of the four waves
constexpr int KR_LDS_S = KR_N * KR_SLD;            // staging image of the result (>= KR_COLS * KR_N)
constexpr int KR_LDS = KR_LDS_T > KR_LDS_S ? KR_LDS_T : KR_LDS_S;
// pending chunk (kr_apply_pending): the 20 image tiles as row-major 16 x 17 matrices, x, R0 [column][site] (stride 65);
// behind the transpose tiles, the update [column][entry] (stride 257), written once the image is no longer read
constexpr int KR_PF_TS = 16 * 17;
constexpr int KR_PF_IMG = 0, KR_PF_X = 20 * KR_PF_TS, KR_PF_R0 = KR_PF_X + 64, KR_PF_RLD = 65;
constexpr int KR_PF_D = KR_LDS_T, KR_PF_DLD = 257;
constexpr int KR_LDS_PF = KR_PF_D + KR_COLS * KR_PF_DLD;  // 67 712 bytes: two workgroups per CU
static_assert(KR_PF_R0 + KR_COLS * KR_PF_RLD <= KR_LDS_PF && KR_LDS <= KR_LDS_PF, "pending-chunk LDS layout");

#define KR_GLOBAL __attribute__((address_space(1)))
typedef const KR_GLOBAL double *kr_gcdp;
typedef double kr_d2 __attribute__((ext_vector_type(2)));
typedef const KR_GLOBAL kr_d2 *kr_gcd2p;
typedef unsigned kr_u4 __attribute__((ext_vector_type(4)));

#ifdef KR_STAMPS  // diagnostic build only (tools/kr_stamps.py): per workgroup of the pending-chunk launch, cycle stamps of wave 0
                  // (inside kr_chain only of the chain that applies the chunk: the second chain of kron_wrap_kernel stamps nothing)
__device__ long long *kr_stamp_ptr = nullptr;
#define KR_STAMP(k)                                                                                   \
    do {                                                                                              \
        if (PF && threadIdx.x == 0 && kr_stamp_ptr)                                                   \
            kr_stamp_ptr[16 * blockIdx.x + (k)] = (long long)__builtin_amdgcn_s_memtime();            \
    } while (0)
#define KR_STAMP_RT(k)                                                                                \
    do {                                                                                              \
        if (PF && threadIdx.x == 0 && kr_stamp_ptr)                                                   \
            kr_stamp_ptr[16 * blockIdx.x + (k)] = (long long)__builtin_amdgcn_s_memrealtime();        \
    } while (0)
extern "C" int dqmc_debug_kr_stamps(void *devptr)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(kr_stamp_ptr), &devptr, sizeof(void *));
}
#else
#define KR_STAMP(k) do { } while (0)
#define KR_STAMP_RT(k) do { } while (0)
#endif
// X_0 (the column tiles v of this workgroup's 16 columns) += C R^ for the pending chunk (file header)
template <bool PF>
__device__ __forceinline__ void kr_apply_pending(const KronArgs &a, int unit, int c0, d4 (&v)[KR_NC], double *lds)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, ci = lane & 15;
    const int site0 = a.pf_site0;
    const kr_gcdp img = (kr_gcdp)(a.pf_img + (long)unit * a.pf_img_su);
    const kr_gcdp G = (kr_gcdp)(a.X0 + (long)unit * a.x_su);
    double *limg = lds + KR_PF_IMG, *lx = lds + KR_PF_X, *lr = lds + KR_PF_R0, *ld = lds + KR_PF_D;
    // requests first: image (2 doubles per request) and x
    constexpr int NI = LU_IMG / 2 / 256;
    static_assert(NI * 512 == LU_IMG, "image staging");
    kr_d2 iv[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) iv[i] = reinterpret_cast<kr_gcd2p>(img)[tid + 256 * i];
    const double xin = img[LU_IMG + (tid & 63)];
    // image -> LDS, every tile as its matrix N row-major: N[ci][4 q + g] is then the A operand of N itself
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int p = 2 * (tid + 256 * i), tl = p >> 8, r = (p >> 6) & 3, ln = p & 63;
        double *d = limg + tl * KR_PF_TS + (4 * r + (ln >> 4)) * 17 + (ln & 15);
        d[0] = iv[i].x;
        d[1] = iv[i].y;
    }
    if (tid < 64) lx[tid] = xin;
    // R0[s][j] = G[site0 + s][j]: register site0 / 64 of the (y, x) tiles, s = ci + 16 g
    {
        const int rr = site0 >> 6;
#pragma unroll
        for (int t = 0; t < KR_NC; ++t) {
            const double r0 = rr == 0 ? v[t][0] : (rr == 1 ? v[t][1] : (rr == 2 ? v[t][2] : v[t][3]));
            lr[(KR_NC * w + t) * KR_PF_RLD + ci + 16 * g] = r0;
        }
    }
    __syncthreads();
    KR_STAMP(2);
    auto A = [&](int tl, int q) { return limg[tl * KR_PF_TS + ci * 17 + 4 * q + g]; };
    auto xr = [&](int J, int r) { return lx[16 * J + 4 * r + g]; };
    constexpr int TU = LU_OFF_U / LU_TILE, TL = LU_OFF_L / LU_TILE, TP = LU_OFF_PT / LU_TILE, TQ = LU_OFF_Q / LU_TILE;
    // D = C R^ (below) on this wave's rows 64 w .. 64 w + 63.  Its A operands, C[16 (4 w + mm) + ci][16 J + 4 q + g], come
    // one block J ahead of its 16 MFMAs, the first during the solves (the four row tiles of a request share one address;
    // all 64 in flight were 128 more VGPRs: one workgroup per CU)
    const kr_gcdp gc = G + 64 * w + ci + (long)KR_N * (site0 + g);
    double ca[2][4][4];  // [J & 1][mm][q]
    auto fetch = [&](int J, double (&c)[4][4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int mm = 0; mm < 4; ++mm) c[mm][q] = gc[16 * mm + (long)KR_N * (16 * J + 4 * q)];
    };
    fetch(0, ca[0]);
    // (the four waves solve the same 64 x 16 block: each needs all of R^ as B operands)
#ifdef KR_PROBE_PRODUCTS
    // TIMING PROBE, WRONG VALUES (diagnostic build with KR_STAMPS only): what the solves would cost as two
    // block-triangular products on prebuilt inverse blocks, with image tiles standing in for the blocks nothing builds yet.
    // Wave w forms block row w of each product (independent accumulators), the intermediate and R^ go through LDS.
    d4 rh[4];
    {
        double *lw = lr + KR_COLS * KR_PF_RLD, *lh = lr;  // behind R0 (free up to KR_LDS_PF); over R0, dead after the first product
        static_assert(KR_PF_R0 + 2 * KR_COLS * KR_PF_RLD <= KR_LDS_PF, "probe LDS");
        d4 pa[4];
#pragma unroll
        for (int J = 0; J < 4; ++J) {
            pa[J] = (d4){0.0, 0.0, 0.0, 0.0};
            if (J <= w)
#pragma unroll
                for (int q = 0; q < 4; ++q) pa[J] = FK_MFMA(A(TL + J, q), lr[ci * KR_PF_RLD + 16 * J + 4 * q + g], pa[J]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            lw[ci * KR_PF_RLD + 16 * w + 4 * r + g] = (pa[0][r] + pa[1][r] + pa[2][r] + pa[3][r]) * xr(w, r);
        __syncthreads();
#pragma unroll
        for (int J = 0; J < 4; ++J) {
            pa[J] = (d4){0.0, 0.0, 0.0, 0.0};
            if (J >= w)
#pragma unroll
                for (int q = 0; q < 4; ++q) pa[J] = FK_MFMA(A(TU + J, q), lw[ci * KR_PF_RLD + 16 * J + 4 * q + g], pa[J]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) lh[ci * KR_PF_RLD + 16 * w + 4 * r + g] = pa[0][r] + pa[1][r] + pa[2][r] + pa[3][r];
        __syncthreads();
#pragma unroll
        for (int J = 0; J < 4; ++J)
#pragma unroll
            for (int q = 0; q < 4; ++q) rh[J][q] = lh[ci * KR_PF_RLD + 16 * J + 4 * q + g];
    }
#else
    d4 xv[4], rh[4];
#pragma unroll
    for (int J = 0; J < 4; ++J) {
        d4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = lr[ci * KR_PF_RLD + 16 * J + 4 * r + g];
#pragma unroll
        for (int K = 0; K < J; ++K)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = FK_MFMA(A(TL + lu_pair(K, J), q), xv[K][q], acc);
        d4 z = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; ++q) z = FK_MFMA(A(TQ + J, q), acc[q], z);
#pragma unroll
        for (int r = 0; r < 4; ++r) xv[J][r] = z[r] * xr(J, r);
    }
#pragma unroll
    for (int J = 3; J >= 0; --J) {
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int K = J + 1; K < 4; ++K)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = FK_MFMA(A(TU + lu_pair(J, K), q), rh[K][q], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = xv[J][r] + xr(J, r) * acc[r];
        d4 o = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; ++q) o = FK_MFMA(A(TP + J, q), acc[q], o);
        rh[J] = o;
    }
#endif
    KR_STAMP(3);
    // tile mm of D holds D[16 (4 w + mm) + 4 r + g][j = ci]
    d4 dm[4];
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) dm[mm] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int J = 0; J < 4; ++J) {
        if (J < 3) fetch(J + 1, ca[(J + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int mm = 0; mm < 4; ++mm) {
                const int i = 16 * (4 * w + mm) + ci, s = 16 * J + 4 * q + g;
                const double c = ca[J & 1][mm][q] - (i == site0 + s ? 1.0 : 0.0);
                dm[mm] = FK_MFMA(c, rh[J][q], dm[mm]);
            }
        __builtin_amdgcn_sched_barrier(0);
    }
    KR_STAMP(4);
    __syncthreads();  // every wave is done with the image (the update goes over it)
#pragma unroll
    for (int mm = 0; mm < 4; ++mm)
#pragma unroll
        for (int r = 0; r < 4; ++r) ld[ci * KR_PF_DLD + 16 * (4 * w + mm) + 4 * r + g] = dm[mm][r];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < KR_NC; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[t][r] += ld[(KR_NC * w + t) * KR_PF_DLD + ci + 16 * (g + 4 * r)];
    // (the update region lies behind the transpose tiles: the first step's tile stores need no barrier; the staging image
    // at the end that overlaps it is behind the steps' barriers)
}

// One chain of a workgroup: columns c0 .. c0 + KR_COLS - 1 of X_0 (x0u, this unit's matrix) through the steps st[0 .. nsteps),
// result to ou.  PF: the pending chunk is applied to X_0 first.  WT: the result is stored write-through (the hand-off of
// kron_wrap_kernel).
template <bool PF, bool WT>
__device__ __forceinline__ void kr_chain(const KronArgs &a, const KronStep *steps, int nsteps, const double *x0u, double *ou,
                                         int unit, int c0, double *lds)
{
    const int wk = a.nb == 2 ? unit >> 1 : unit, blk = a.nb == 2 ? unit & 1 : 0;
    const bool bn = blk != 0;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, ci = lane & 15;
    const long conf_off = (long)wk * a.conf_stride;
    double *tile = lds + w * (KR_NC * 16 * KR_TLD);

    // X_0: column c0 + KR_NC w + t, parity (y, x): register r = entries ci + 16 (g + 4 r), 64 consecutive doubles
    d4 v[KR_NC];
    {
        const double *x0 = x0u + (long)KR_N * (c0 + KR_NC * w) + ci + 16 * g;
#pragma unroll
        for (int t = 0; t < KR_NC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[t][r] = x0[KR_N * t + 64 * r];
    }
    // entry index of register r of this lane at parity par (0: a = y, b = x; 1: a = x, b = y)
    auto idx = [&](int par, int r) { return par ? (g + 4 * r) + 16 * ci : ci + 16 * (g + 4 * r); };
    // Everything a step needs from memory besides its column tiles - A operands (lane: F[row ci][k = 4 q + g] of the
    // column-major 16 x 16 factor; fa sums over a, fb over b) and the HS-field bytes of its two scalings - is requested one
    // step ahead, behind the step before's MFMAs, and without a branch (a missing scaling reads X_0 and is not applied):
    // requested at the top of each step, each was a full trip to the L2 in front of the first product.
    struct Ops {
        double av[4], bv[4];
        int8_t cpre[4], cpost[4];
    };
    auto request = [&](int s, Ops &o) {
        const KronStep &st = steps[s];
        const int par = s & 1;
        const double *fx = st.ax + KR_N * blk, *fy = st.ay + KR_N * blk;
        const double *fa = par ? fx : fy, *fb = par ? fy : fx;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o.av[q] = fa[ci + 16 * (4 * q + g)];
            o.bv[q] = fb[ci + 16 * (4 * q + g)];
        }
        const int8_t *dummy = reinterpret_cast<const int8_t *>(x0u);
        const int8_t *pre = st.pre_conf ? st.pre_conf + conf_off : dummy, *post = st.post_conf ? st.post_conf + conf_off : dummy;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o.cpre[r] = pre[st.pre_conf ? idx(par, r) : 0];
            o.cpost[r] = post[st.post_conf ? idx(par ^ 1, r) : 0];
        }
    };
    Ops cur, nxt;
    request(0, cur);
    double cs[KR_NC];  // final column scale (read from X_0 and not applied when there is none)
    {
        const double *cd = a.col_d ? a.col_d + (long)unit * a.col_stride + c0 + KR_NC * w : x0u;
#pragma unroll
        for (int t = 0; t < KR_NC; ++t) cs[t] = cd[t];
    }
    if constexpr (PF) kr_apply_pending<PF>(a, unit, c0, v, lds);
    KR_STAMP(5);

    for (int s = 0; s < nsteps; ++s) {
        const KronStep &st = steps[s];
        if (st.pre_conf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double f = fk_conf(cur.cpre[r], st.pre_sign, bn, a.epl, a.eml);
#pragma unroll
                for (int t = 0; t < KR_NC; ++t) v[t][r] *= f;
            }
        }
        // P = Fa V  ->  tile[a][b]
#pragma unroll
        for (int t = 0; t < KR_NC; ++t) {
            d4 p = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) p = FK_MFMA(cur.av[q], v[t][q], p);
#pragma unroll
            for (int r = 0; r < 4; ++r) tile[t * 16 * KR_TLD + (g + 4 * r) * KR_TLD + ci] = p[r];
        }
        request(min(s + 1, nsteps - 1), nxt);
        __syncthreads();
        // Q = Fb P^T: B operand of k-block q is P[a = ci][b = 4 q + g]; the result has b in the registers, a on the lanes
#pragma unroll
        for (int t = 0; t < KR_NC; ++t) {
            d4 q4 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) q4 = FK_MFMA(cur.bv[q], tile[t * 16 * KR_TLD + ci * KR_TLD + 4 * q + g], q4);
            v[t] = q4;
        }
        __syncthreads();  // (the next step's tile writes, or the staging image, reuse the LDS)
        if (st.post_conf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double f = fk_conf(cur.cpost[r], st.post_sign, bn, a.epl, a.eml);
#pragma unroll
                for (int t = 0; t < KR_NC; ++t) v[t][r] *= f;
            }
        }
        cur = nxt;
    }
    KR_STAMP(6);
    // ---- staging image: transposed [entry][column] (row stride KR_SLD), else [column][entry] (the global image)
    const int par = nsteps & 1;
#pragma unroll
    for (int t = 0; t < KR_NC; ++t) {
        const int cl = KR_NC * w + t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = idx(par, r);
            lds[a.transpose_out ? i * KR_SLD + cl : cl * KR_N + i] = a.col_d ? v[t][r] * cs[t] : v[t][r];
        }
    }
    __syncthreads();
    double *o = ou;
    if constexpr (WT) {  // transposed, as below, each 16 bytes with one write-through store
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(o, 0, KR_N * KR_N * (int)sizeof(double), 0x00020000);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = 2 * (tid + 256 * k), i = e >> 4, cl = e & 15;
            __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const kr_u4 *>(lds + i * KR_SLD + cl), rs,
                                                   (c0 + KR_N * i + cl) * (int)sizeof(double), 0, 16 /* sc1 */);
        }
    } else {
        fk_store_image<KR_N, KR_COLS, KR_SLD, 0>(o, lds, a, c0, tid);
    }
}

// unit and first column of a workgroup.  XG: the 16 workgroups of a unit share an XCD (blockIdx.x % 8, as the flush kernels
// place units): each of them reads all of C and the image, which then come into one L2 once instead of into eight
template <bool XG>
__device__ __forceinline__ void kr_place(int &unit, int &c0)
{
    const unsigned bq = XG ? blockIdx.x >> 3 : blockIdx.x;
    unit = XG ? (bq / (KR_N / KR_COLS)) * 8 + (blockIdx.x & 7) : bq / (KR_N / KR_COLS);
    c0 = KR_COLS * (bq % (KR_N / KR_COLS));
}

template <bool PF>
__global__ __launch_bounds__(256) void kron_chain_kernel(KronArgs a)
{
    __shared__ __attribute__((aligned(16))) double lds[PF ? KR_LDS_PF : KR_LDS];
#ifndef KR_NO_XCD_GROUPS
    constexpr bool XG = PF;
#else
    constexpr bool XG = false;
#endif
    int unit, c0;
    kr_place<XG>(unit, c0);
    if (unit >= a.n_units) return;
    KR_STAMP(0);
    KR_STAMP_RT(1);
    kr_chain<PF, false>(a, a.st, a.nsteps, a.X0 + (long)unit * a.x_su, a.out + (long)unit * a.out_su, unit, c0, lds);
    KR_STAMP(7);
    KR_STAMP_RT(8);
}

// wrap_greens! in one launch (engine.cpp: wrap_greens_kron): both one-step chains, st[0] from X0 into out (= P', stored
// transposed) and st[1] from out into wrap_out (transposed again).  A unit's second step reads columns of out that all 16
// workgroups of the unit wrote, and nothing of any other unit, so the hand-off is per unit: write-through (sc1) stores of
// P', every wave drains them, then one lane per workgroup adds to the unit's arrival word (agent scope, relaxed), polls it
// until the unit's 16 workgroups of this launch are in (the words are never cleared: wrap_target counts all launches so
// far), and takes one agent-scope acquire for the workgroup's plain loads of P'.  The grid must be co-resident
// (launch_kron_wrap checks it); the poll is bounded all the same: a time-out sets bit 5 of the error word and runs through.
constexpr unsigned KR_SPIN = 1000000u;  // ~1 s of polling; the wait is a few microseconds
template <bool PF>
__global__ __launch_bounds__(256) void kron_wrap_kernel(KronArgs a)
{
    __shared__ __attribute__((aligned(16))) double lds[PF ? KR_LDS_PF : KR_LDS];
#ifndef KR_NO_XCD_GROUPS
    constexpr bool XG = true;
#else
    constexpr bool XG = false;
#endif
    int unit, c0;
    kr_place<XG>(unit, c0);
    if (unit >= a.n_units) return;
    KR_STAMP(0);
    KR_STAMP_RT(1);
    double *mid = a.out + (long)unit * a.out_su;
    kr_chain<PF, true>(a, a.st, 1, a.X0 + (long)unit * a.x_su, mid, unit, c0, lds);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave, before the arrival below
    KR_STAMP(7);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned *cnt = a.wrap_cnt + KR_CNT_STRIDE * unit;
        __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool in = false;
        for (unsigned s = 0; s < KR_SPIN && !in; ++s) {
            in = (int)(__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - a.wrap_target) >= 0;
            if (!in) __builtin_amdgcn_s_sleep(2);
        }
        if (!in) atomicOr(a.errflag, 32);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    KR_STAMP(9);
    kr_chain<false, false>(a, a.st + 1, 1, mid, a.wrap_out + (long)unit * a.out_su, unit, c0, lds);
    KR_STAMP(10);
    KR_STAMP_RT(8);
}

int kron_wrap_blocks_per_cu(bool pf)
{
    int nb = 0;
    const hipError_t e = pf ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kron_wrap_kernel<true>, 256, 0)
                            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kron_wrap_kernel<false>, 256, 0);
    return e == hipSuccess ? nb : 0;
}

hipError_t launch_kron_wrap(const KronArgs &a, hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    if (a.nsteps != 2 || a.nb < 1 || a.nb > 2 || !a.transpose_out || a.col_d || !a.wrap_out || !a.wrap_cnt || !a.errflag)
        return hipErrorInvalidValue;
    if (a.x_su < KR_N * KR_N || a.out_su < KR_N * KR_N) return hipErrorInvalidValue;
    if (a.pf_img && (a.pf_site0 < 0 || a.pf_site0 % 64 != 0 || a.pf_site0 + 64 > KR_N || a.pf_img_su < LU_STRIDE))
        return hipErrorInvalidValue;
    return fk_launch(a.pf_img ? kron_wrap_kernel<true> : kron_wrap_kernel<false>, dim3(kron_wrap_grid(a.n_units)), a, s, start, stop);
}

hipError_t launch_kron_chain(const KronArgs &a, hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    if (a.nsteps < 1 || a.nsteps > SLAB_MAX_STEPS || a.nb < 1 || a.nb > 2) return hipErrorInvalidValue;
    if (a.pf_img && (a.pf_site0 < 0 || a.pf_site0 % 64 != 0 || a.pf_site0 + 64 > KR_N || a.pf_img_su < LU_STRIDE))
        return hipErrorInvalidValue;
    // the pending-chunk form: whole groups of eight units (XCD placement)
    if (a.pf_img) return fk_launch(kron_chain_kernel<true>, dim3((a.n_units + 7) / 8 * 8 * (KR_N / KR_COLS)), a, s, start, stop);
    return fk_launch(kron_chain_kernel<false>, dim3(a.n_units * (KR_N / KR_COLS)), a, s, start, stop);
}

}  // namespace dqmc
