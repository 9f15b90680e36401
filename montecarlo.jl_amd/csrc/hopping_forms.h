// hopping_forms.h — the factored forms of the hopping exponentials eT2 / eTinv2: one table, the gates that admit a matrix
// to a form, and the device image of its factors.  Plain C++17, no HIP: engine.cpp includes it, and
// tests/hopping_forms_check.cpp builds it alone under the host sanitizers.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace dqmc {

// A handle has at most one form.  The device image (dqmc_handle::kron_f) is [eT2, eTinv2, eT2', eTinv2'] x (operand set a:
// nb x fa doubles, operand set b: nb x fb doubles); a KronStep's ax / ay point at the two sets of one of the four matrices.
//   Square16   16 x 16 periodic square lattice, site x + 16 y: Ey (x) Ex (kron.hip instead of slab.hip).
//              a = Ex, b = Ey, 16 x 16 column-major.  The exponentials of the lattice measure 16-28 ulp off the product.
//   Rect32x8   32 x 8 rectangular lattice, site x + 32 y: Ey (x) Ex with unequal factors (rect.hip).  a = Ex (32 x 32),
//              b = Ey (8 x 8).  Up to 16 ulp; 8 x 32, 64 x 4 and any other hopping keep the dense slab path.
//   Cubic8     8 x 8 x 8 cubic lattice, site x + 8 y + 64 z: Ez (x) Ey (x) Ex (kron3.hip instead of the dense GEMMs).
//              a = the operand image of Exy = Ey (x) Ex (4096), b = that of I2 (x) Ez (256): kron3_images.  18-39 ulp.
//   Bilayer16  two-layer 16 x 16 x 2 lattice, site x + 16 y + 256 z: Ez (x) Ey (x) Ex (bilayer.hip).  a = Ex, b = Ey with
//              the 2 x 2 Ez behind it at + 256 and zero padding up to HOP_BILAYER_FB.  Up to 35 ulp.
//   Tri16      triangular 16 x 16 lattice: (Fy (x) Fx) Ed, factors from the host (tri.hip).  a = Fx, b = Fy, then Fd.
//   Ttp16      t-t' square 16 x 16 lattice: (Fy (x) Fx) Ed Ea, factors from the host (ttp.hip).  a = Fx, b = Fy, Fd, Fa.
// The gate forms are tried in the order of the enum at dqmc_create, the first accepted one is taken; any other hopping
// keeps the dense path.  pending_chunk: the form's kernel applies a sweep's pending last chunk in the first launch of a
// wrap; one_launch_wrap: it has the wrap in one launch with a hand-off per unit (both: kron.hip only).
enum class HopForm { None, Square16, Rect32x8, Cubic8, Bilayer16, Tri16, Ttp16 };
constexpr int HOP_BILAYER_FB = 264;
struct HopFormRow {
    int n, naxes, dims[3];  // sites, and the axis lengths of the Kronecker product, innermost (x) first
    int fa, fb;             // doubles per block of the two operand sets
    bool host_factors;      // the factors come from the host (and fb / 256 + 1 of them), not from kron_split
    bool pending_chunk, one_launch_wrap;
};
constexpr HopFormRow HOP_FORMS[] = {
    {0, 0, {1, 1, 1}, 0, 0, false, false, false},
    {256, 2, {16, 16, 1}, 256, 256, false, true, true},
    {256, 2, {32, 8, 1}, 1024, 64, false, false, false},
    {512, 3, {8, 8, 8}, 4096, 256, false, false, false},
    {512, 3, {16, 16, 2}, 256, HOP_BILAYER_FB, false, false, false},
    {256, 2, {16, 16, 1}, 256, 512, true, false, false},
    {256, 2, {16, 16, 1}, 256, 768, true, false, false},
};
constexpr const HopFormRow &hop_row(HopForm f) { return HOP_FORMS[(int)f]; }

// E (n x n, column-major, n = the product of dims) as a Kronecker product of naxes factors, axis 0 innermost: factor a is
// the block of E along axis a at the origin of the others, divided by E[0] for a > 0 (axis 0 is copied).  Accepted when
// max|E - (x) F| <= 256 eps max|E|, the product of an entry taken outermost axis first.
inline bool kron_split(const double *E, int n, const int *dims, int naxes, double *const *f)
{
    const double e00 = E[0];
    if (!(e00 > 0.0)) return false;
    int stride[3];
    for (int a = 0, s = 1; a < naxes; s *= dims[a++]) {
        stride[a] = s;
        for (int j = 0; j < dims[a]; ++j)
            for (int i = 0; i < dims[a]; ++i) {
                const double e = E[(size_t)s * i + (size_t)n * s * j];
                f[a][i + dims[a] * j] = a ? e / e00 : e;
            }
    }
    double emax = 0.0, rmax = 0.0;
    for (int c = 0; c < n; ++c)
        for (int r = 0; r < n; ++r) {
            const double e = E[r + (size_t)n * c];
            auto at = [&](int a) { return f[a][(r / stride[a]) % dims[a] + dims[a] * ((c / stride[a]) % dims[a])]; };
            double p = at(naxes - 1);
            for (int a = naxes - 2; a >= 0; --a) p = p * at(a);
            emax = std::max(emax, std::fabs(e));
            rmax = std::max(rmax, std::fabs(e - p));
        }
    return std::isfinite(emax) && rmax <= 256.0 * 2.220446049250313e-16 * emax;
}

// The operand images kron3.hip reads (see there) of A = Ez (x) Exy, Exy = Ey (x) Ex; tr: of A' = Ez' (x) Exy'
inline void kron3_images(const double *fx, const double *fy, const double *fz, bool tr, double *img_xy, double *img_z)
{
    auto exy = [&](int r, int c) {
        if (tr) std::swap(r, c);
        return fy[(r >> 3) + 8 * (c >> 3)] * fx[(r & 7) + 8 * (c & 7)];
    };
    auto ez = [&](int r, int c) { return tr ? fz[c + 8 * r] : fz[r + 8 * c]; };
    for (int mp = 0; mp < 4; ++mp)
        for (int m = 0; m < 4; ++m)
            for (int r = 0; r < 4; ++r)
                for (int lane = 0; lane < 64; ++lane)
                    img_xy[((mp * 4 + m) * 4 + r) * 64 + lane] = exy(16 * mp + (lane & 15), 16 * m + 4 * r + (lane >> 4));
    for (int q = 0; q < 4; ++q)
        for (int lane = 0; lane < 64; ++lane) {
            const int row = lane & 15, k = 4 * q + (lane >> 4);
            img_z[q * 64 + lane] = (row >> 3) == (k >> 3) ? ez(row & 7, k & 7) : 0.0;
        }
}

// eT2 / eTinv2 of the 16 x 16 periodic triangular lattice (n = 256, site x + 16 y; hopping along X = (1, 0), Y = (0, 1) and
// D = XY) as (Fy (x) Fx) Ed, where Ed applies Fd along the diagonals x - y = const:
//   (Ed v)(x, y) = sum_y' Fd[y, y'] v(x - y + y', y')
// The factors come from the host (dqmc_set_triangular_factors).  X, Y and D commute, so every order of the three products is
// E up to rounding; the gate bounds the claimed form and the two orders the kernel applies (tri.hip: Fx Ed Fy from a step
// that starts with y in the registers, Fy Ed Fx from one that starts with x), each by 256 eps max|E|.  Their transposes
// (the daggered products and the wraps' right products) have the same residuals.
inline bool tri_factor_ok(const double *E, const double *fx, const double *fy, const double *fd)
{
    const int n = 256;
    if (!(E[0] > 0.0)) return false;
    auto F = [](const double *f, int r, int c) { return f[(r & 15) + 16 * (c & 15)]; };
    double emax = 0.0, rmax = 0.0;
    for (int y2 = 0; y2 < 16; ++y2)
        for (int x2 = 0; x2 < 16; ++x2)
            for (int y = 0; y < 16; ++y)
                for (int x = 0; x < 16; ++x) {
                    const double e = E[(x + 16 * y) + (size_t)n * (x2 + 16 * y2)];
                    double claim = 0.0, xdy = 0.0, ydx = 0.0;
                    for (int k = 0; k < 16; ++k) {
                        claim += F(fy, y, k) * F(fx, x, x2 - y2 + k) * F(fd, k, y2);   // (Fy (x) Fx) Ed
                        xdy += F(fx, x, x2 + y - k) * F(fd, y, k) * F(fy, k, y2);      // Fx Ed Fy
                        ydx += F(fy, y, k) * F(fd, k, y2) * F(fx, x - k + y2, x2);     // Fy Ed Fx
                    }
                    emax = std::max(emax, std::fabs(e));
                    rmax = std::max(rmax, std::max(std::fabs(e - claim), std::max(std::fabs(e - xdy), std::fabs(e - ydx))));
                }
    return std::isfinite(emax) && std::isfinite(rmax) && rmax <= 256.0 * 2.220446049250313e-16 * emax;
}

// eT2 / eTinv2 of the 16 x 16 periodic square lattice with next-nearest-neighbour hopping (n = 256, site x + 16 y; hopping
// along X = (1, 0), Y = (0, 1), D = XY and A = X Y^-1) as (Fy (x) Fx) Ed Ea: Ed as above, and Ea applies Fa along the
// anti-diagonals x + y = const:
//   (Ea v)(x, y) = sum_y' Fa[y, y'] v(x + y - y', y')
// The factors come from the host (dqmc_set_square_tp_factors).  The four shifts commute, so every order of the four products
// is E up to rounding; the gate bounds the claimed form and the four orders the kernel applies (ttp.hip: Fx Ea Ed Fy from a
// step that starts with y in the registers, Fy Ea Ed Fx from one that starts with x, and, as the transposes of what the
// transposed factors give in the daggered products and the wraps' right products, Fy Ed Ea Fx and Fx Ed Ea Fy), each by
// 256 eps max|E|.  Every order is formed by applying its factors to the identity, 16 terms per entry and factor.
inline bool ttp_factor_ok(const double *E, const double *fx, const double *fy, const double *fd, const double *fa)
{
    const int n = 256;
    if (!(E[0] > 0.0)) return false;
    std::vector<double> M((size_t)n * n), T((size_t)n * n);
    // M <- Op(F) M, op 0: Fx on x, 1: Fy on y, 2: Ed, 3: Ea
    auto apply = [&](int op, const double *F) {
        for (int c = 0; c < n; ++c) {
            const double *m = M.data() + (size_t)n * c;
            double *t = T.data() + (size_t)n * c;
            for (int y = 0; y < 16; ++y)
                for (int x = 0; x < 16; ++x) {
                    double acc = 0.0;
                    for (int k = 0; k < 16; ++k) {
                        const double f = F[(op == 0 ? x : y) + 16 * k];
                        const int src = op == 0 ? k + 16 * y : op == 1 ? x + 16 * k : op == 2 ? ((x - y + k) & 15) + 16 * k
                                                                                               : ((x + y - k) & 15) + 16 * k;
                        acc += f * m[src];
                    }
                    t[x + 16 * y] = acc;
                }
        }
        M.swap(T);
    };
    const double *F[4] = {fx, fy, fd, fa};
    // (the operators are listed right to left: the first one is applied first)
    static const int orders[5][4] = {{3, 2, 0, 1}, {1, 2, 3, 0}, {0, 2, 3, 1}, {0, 3, 2, 1}, {1, 3, 2, 0}};
    double emax = 0.0, rmax = 0.0;
    for (size_t i = 0; i < (size_t)n * n; ++i) emax = std::max(emax, std::fabs(E[i]));
    for (const auto &ord : orders) {
        std::fill(M.begin(), M.end(), 0.0);
        for (int i = 0; i < n; ++i) M[i + (size_t)n * i] = 1.0;
        for (int k = 0; k < 4; ++k) apply(ord[k], F[ord[k]]);
        for (size_t i = 0; i < (size_t)n * n; ++i) {
            const double r = std::fabs(E[i] - M[i]);
            if (!(r <= rmax)) rmax = r;  // (a NaN is kept)
        }
    }
    return std::isfinite(emax) && std::isfinite(rmax) && rmax <= 256.0 * 2.220446049250313e-16 * emax;
}

// The gate of `form` on every block of eT2 and eTinv2 (nb blocks of n x n each), and the device image of the factors and
// their transposes (the transposed product has the same residual: no second check).  A gate form splits the matrices
// itself; a host form checks host_f, [block][eT2, eTinv2][factor][16 x 16].  False, with the first rejected block in
// *bad_block, when a gate rejects; img is then of no use.
inline bool build_hop_image(HopForm form, int nb, const double *eT2, const double *eTinv2, const double *host_f,
                            std::vector<double> &img, int *bad_block = nullptr)
{
    const HopFormRow &row = hop_row(form);
    const size_t nn = (size_t)row.n * row.n, per = (size_t)nb * (row.fa + row.fb);
    const int nf = row.host_factors ? 1 + row.fb / 256 : row.naxes;
    img.assign(4 * per, 0.0);
    std::vector<double> split(row.host_factors ? 0 : 1024 + 256 + 64);
    for (int b = 0; b < nb; ++b)
        for (int m = 0; m < 2; ++m) {
            const double *E = (m ? eTinv2 : eT2) + (size_t)b * nn;
            const double *hf = row.host_factors ? host_f + ((size_t)b * 2 + m) * nf * 256 : nullptr;
            double *f[3] = {split.data(), split.data() + 1024, split.data() + 1024 + 256};
            const bool ok = form == HopForm::Tri16   ? tri_factor_ok(E, hf, hf + 256, hf + 512)
                            : form == HopForm::Ttp16 ? ttp_factor_ok(E, hf, hf + 256, hf + 512, hf + 768)
                                                     : kron_split(E, row.n, row.dims, row.naxes, f);
            if (!ok) {
                if (bad_block) *bad_block = b;
                return false;
            }
            for (int t = 0; t < 2; ++t) {  // as is, transposed
                double *set = img.data() + (size_t)(m + 2 * t) * per;
                double *da = set + (size_t)b * row.fa, *db = set + (size_t)nb * row.fa + (size_t)b * row.fb;
                auto put = [t](double *dst, const double *src, int d) {
                    for (int j = 0; j < d; ++j)
                        for (int i = 0; i < d; ++i) dst[i + d * j] = t ? src[j + d * i] : src[i + d * j];
                };
                if (form == HopForm::Cubic8) {
                    kron3_images(f[0], f[1], f[2], t == 1, da, db);
                } else if (row.host_factors) {  // [factor][block]: factor k of all blocks behind factor k - 1 of all blocks
                    for (int k = 0; k < nf; ++k) put(set + ((size_t)k * nb + b) * 256, hf + 256 * k, 16);
                } else {
                    put(da, f[0], row.dims[0]);
                    put(db, f[1], row.dims[1]);
                    if (row.naxes == 3) put(db + row.dims[1] * row.dims[1], f[2], row.dims[2]);
                }
            }
        }
    return true;
}

}  // namespace dqmc
