// bilayer.hip — slice-matrix chains and wraps with the hopping exponential of the two-layer square lattice applied in
// factored form (n = 512 = 16 x 16 x 2).
//
// On the periodic 16 x 16 x 2 BilayerSquareLattice (site i = x + 16 y + 256 z, z the layer) every hopping exponential is,
// up to rounding, a Kronecker product A = Ez (x) Ey (x) Ex with Ex, Ey 16 x 16 and Ez 2 x 2 (hopping_forms.h: kron_split
// checks it at handle creation).  A column v of 512 entries is two planes V_z[x][y] = v[x + 16 y + 256 z], and
//   (A v)_z = sum_z' Ez[z][z'] vec(Ex V_z' Ey^T):
// the two 16-contractions of kron.hip on each plane, 16 v_mfma_f64_16x16x4_f64 per column instead of the 256 of the dense
// product, and a 2 x 2 mix of the planes, two multiply-adds per entry on the vector ALU.
//
//   X_s = post_s (.) ( A_s * ( pre_s (.) X_{s-1} ) ),  s = 1 .. nsteps,    out = X_nsteps (.) col_d   (or its transpose)
//
// with the argument conventions of kron.hip (KronArgs); the factors of block b are column-major at
//   st.ax + 256 b: Ex          st.ay + BL_FB b: Ey, and Ez behind it (Ez[z + 2 z'] at 256 + z + 2 z')
//
// Layout.  A wave owns two consecutive columns (h = 0, 1), each plane as one MFMA accumulator tile of kron.hip's scheme:
// tile 2 h + z, register r of lane (g = lane >> 4, c = lane & 15) is V_z[a = g + 4 r][b = c], where (a, b) = (y, x) or
// (x, y) by step parity.  P = Fa V takes the tile's registers as its B operands, P^T goes through LDS once (a 16 x 17 tile
// per plane), Q = Fb P^T leaves the tile with its roles swapped: one transpose per step, the parity alternates, (y, x) at the
// start, where a load of one register is 64 consecutive doubles.  The two planes of a column sit in the same registers of
// the same lanes, so the layer factor needs no data movement; it commutes with the in-plane factors and is applied right
// behind the step's first scaling.  A workgroup (4 waves, 8 columns) owns its columns through all steps; the result is
// staged in LDS and stored as whole 64-byte runs, as is or transposed.
#include "factored_common.h"

namespace dqmc {

constexpr int BL_N = 512;
constexpr int BL_P = 256;                         // sites of a plane
constexpr int BL_WAVES = 4;
constexpr int BL_NT = 4;                          // tiles per wave: two columns x two planes
constexpr int BL_COLS = 2 * BL_WAVES;             // columns per workgroup
constexpr int BL_FB = BILAYER_FB;                 // doubles per block behind st.ay: Ey (256), Ez (4), padding
constexpr int BL_TLD = 17;                        // row stride of a transpose tile (doubles), as in kron.hip
constexpr int BL_LDS_T = BL_WAVES * BL_NT * 16 * BL_TLD;
// transposed staging image [entry][column]: entry e, column cl at e BL_SLD + (e >> 4) BL_SPAD + cl.  Even, so that the
// 16-byte reads stay aligned; the 16 lanes of a store group hold entries 1 apart at even parity and 16 apart at odd parity:
// 10 resp. 162 doubles between them, 20 k and 4 k mod 32 in store banks, two lanes per bank pair either way (a plain
// stride puts the odd parity's 16 lanes on one pair)
constexpr int BL_SLD = 10, BL_SPAD = 2;
constexpr int BL_LDS_S = BL_N * BL_SLD + (BL_N / 16) * BL_SPAD;
constexpr int BL_LDS = BL_LDS_T > BL_LDS_S ? BL_LDS_T : BL_LDS_S;  // 41 472 bytes: three workgroups per CU
static_assert(BL_LDS >= BL_COLS * BL_N, "the untransposed staging image [column][entry] reuses the LDS");

__global__ __launch_bounds__(256) void bilayer_chain_kernel(KronArgs a)
{
    __shared__ __attribute__((aligned(16))) double lds[BL_LDS];
    const int unit = blockIdx.x / (BL_N / BL_COLS), c0 = BL_COLS * (blockIdx.x % (BL_N / BL_COLS));
    if (unit >= a.n_units) return;
    const int wk = a.nb == 2 ? unit >> 1 : unit, blk = a.nb == 2 ? unit & 1 : 0;
    const bool bn = blk != 0;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, ci = lane & 15;
    const int cp = c0 + 2 * w;  // this wave's columns cp, cp + 1
    const long conf_off = (long)wk * a.conf_stride;
    double *tile = lds + w * (BL_NT * 16 * BL_TLD);
    const double *x0u = a.X0 + (long)unit * a.x_su;

    // X_0: tile t = 2 h + z is plane z of column cp + h, parity (y, x): register r = entries ci + 16 (g + 4 r) of the plane
    d4 v[BL_NT];
    {
        const double *x0 = x0u + (long)BL_N * cp + ci + 16 * g;
#pragma unroll
        for (int t = 0; t < BL_NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[t][r] = x0[BL_N * (t >> 1) + BL_P * (t & 1) + 64 * r];
    }
    // in-plane entry index of register r of this lane at parity par (0: a = y, b = x; 1: a = x, b = y)
    auto idx = [&](int par, int r) { return par ? (g + 4 * r) + 16 * ci : ci + 16 * (g + 4 * r); };
    // the operands and the HS-field bytes of a step, requested one step ahead (a missing scaling reads X_0 and is not
    // applied), as in kron.hip: A operands F[row ci][k = 4 q + g] of the column-major factors, fa sums over a, fb over b
    struct Ops {
        double av[4], bv[4], ez[4];
        int8_t cpre[2][4], cpost[2][4];
    };
    auto request = [&](int s, Ops &o) {
        const KronStep &st = a.st[s];
        const int par = s & 1;
        const double *fx = st.ax + BL_P * blk, *fy = st.ay + BL_FB * blk;
        const double *fa = par ? fx : fy, *fb = par ? fy : fx;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o.av[q] = fa[ci + 16 * (4 * q + g)];
            o.bv[q] = fb[ci + 16 * (4 * q + g)];
            o.ez[q] = fy[BL_P + q];
        }
        const int8_t *dummy = reinterpret_cast<const int8_t *>(x0u);
        const int8_t *pre = st.pre_conf ? st.pre_conf + conf_off : dummy, *post = st.post_conf ? st.post_conf + conf_off : dummy;
#pragma unroll
        for (int z = 0; z < 2; ++z)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o.cpre[z][r] = pre[st.pre_conf ? BL_P * z + idx(par, r) : 0];
                o.cpost[z][r] = post[st.post_conf ? BL_P * z + idx(par ^ 1, r) : 0];
            }
    };
    Ops cur, nxt;
    request(0, cur);
    double cs[2];  // final column scale (read from X_0 and not applied when there is none)
    {
        const double *cd = a.col_d ? a.col_d + (long)unit * a.col_stride + cp : x0u;
        cs[0] = cd[0];
        cs[1] = cd[1];
    }

    for (int s = 0; s < a.nsteps; ++s) {
        const KronStep &st = a.st[s];
        if (st.pre_conf) {
#pragma unroll
            for (int z = 0; z < 2; ++z)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double f = fk_conf(cur.cpre[z][r], st.pre_sign, bn, a.epl, a.eml);
                    v[z][r] *= f;
                    v[2 + z][r] *= f;
                }
        }
        // the layer factor: (V_0, V_1) <- (Ez00 V_0 + Ez01 V_1, Ez10 V_0 + Ez11 V_1), column by column
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const d4 p0 = v[2 * h], p1 = v[2 * h + 1];
            v[2 * h] = cur.ez[0] * p0 + cur.ez[2] * p1;
            v[2 * h + 1] = cur.ez[1] * p0 + cur.ez[3] * p1;
        }
        // P = Fa V  ->  tile[a][b]
#pragma unroll
        for (int t = 0; t < BL_NT; ++t) {
            d4 p = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) p = FK_MFMA(cur.av[q], v[t][q], p);
#pragma unroll
            for (int r = 0; r < 4; ++r) tile[t * 16 * BL_TLD + (g + 4 * r) * BL_TLD + ci] = p[r];
        }
        request(min(s + 1, a.nsteps - 1), nxt);
        __syncthreads();
        // Q = Fb P^T: B operand of k-block q is P[a = ci][b = 4 q + g]; the result has b in the registers, a on the lanes
#pragma unroll
        for (int t = 0; t < BL_NT; ++t) {
            d4 q4 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) q4 = FK_MFMA(cur.bv[q], tile[t * 16 * BL_TLD + ci * BL_TLD + 4 * q + g], q4);
            v[t] = q4;
        }
        __syncthreads();  // (the next step's tile writes, or the staging image, reuse the LDS)
        if (st.post_conf) {
#pragma unroll
            for (int z = 0; z < 2; ++z)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double f = fk_conf(cur.cpost[z][r], st.post_sign, bn, a.epl, a.eml);
                    v[z][r] *= f;
                    v[2 + z][r] *= f;
                }
        }
        cur = nxt;
    }
    // ---- staging image: transposed [entry][column] (see BL_SLD), else [column][entry] (the global image)
    const int par = a.nsteps & 1;
#pragma unroll
    for (int t = 0; t < BL_NT; ++t) {
        const int h = t >> 1, cl = 2 * w + h;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = BL_P * (t & 1) + idx(par, r);
            const double val = a.col_d ? v[t][r] * (h ? cs[1] : cs[0]) : v[t][r];
            lds[a.transpose_out ? e * BL_SLD + (e >> 4) * BL_SPAD + cl : cl * BL_N + e] = val;
        }
    }
    __syncthreads();
    fk_store_image<BL_N, BL_COLS, BL_SLD, BL_SPAD>(a.out + (long)unit * a.out_su, lds, a, c0, tid);
}

hipError_t launch_bilayer_chain(const KronArgs &a, hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    if (a.nsteps < 1 || a.nsteps > SLAB_MAX_STEPS || a.nb < 1 || a.nb > 2 || a.n_units < 1) return hipErrorInvalidValue;
    if (a.x_su < (long)BL_N * BL_N || a.out_su < (long)BL_N * BL_N || a.pf_img) return hipErrorInvalidValue;
    return fk_launch(bilayer_chain_kernel, dim3(a.n_units * (BL_N / BL_COLS)), a, s, start, stop);
}

}  // namespace dqmc
