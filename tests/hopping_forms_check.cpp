// The factored hopping forms' host code (csrc/hopping_forms.h) on its own: built by tests/test_hopping_forms_host.py with
// g++ -fsanitize=address,undefined and run as a child process on the CPU.  Inputs come from an integer LCG and plain
// multiplications and additions (no libm), so the bits, and with them the image hashes this prints, are the same everywhere.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "hopping_forms.h"

using namespace dqmc;

static int failures = 0;
static void expect(bool ok, const std::string &what)
{
    if (!ok) {
        std::printf("FAILED: %s\n", what.c_str());
        ++failures;
    }
}

struct Lcg {
    uint64_t s;
    double next()  // in [0.5, 1.5)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return 0.5 + (double)(s >> 11) * (1.0 / 9007199254740992.0);
    }
};

static uint64_t fnv1a64(const std::vector<double> &v)
{
    uint64_t h = 1469598103934665603ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(double); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

// n x n Kronecker product of positive non-symmetric random factors, axis 0 innermost
static std::vector<double> make_kron(const int *dims, int naxes, uint64_t seed)
{
    Lcg g{seed};
    std::vector<double> f[3];
    int n = 1;
    for (int a = 0; a < naxes; ++a) {
        f[a].resize((size_t)dims[a] * dims[a]);
        for (double &x : f[a]) x = g.next();
        n *= dims[a];
    }
    std::vector<double> E((size_t)n * n);
    for (int c = 0; c < n; ++c)
        for (int r = 0; r < n; ++r) {
            double p = 1.0;
            for (int a = naxes - 1, rr = r, cc = c, s = n; a >= 0; --a) {
                s /= dims[a];
                p *= f[a][rr / s + dims[a] * (cc / s)];
                rr %= s;
                cc %= s;
            }
            E[r + (size_t)n * c] = p;
        }
    return E;
}
// nb blocks, each its own product
static std::vector<double> make_blocks(const int *dims, int naxes, int nb, uint64_t seed)
{
    std::vector<double> all;
    for (int b = 0; b < nb; ++b) {
        const std::vector<double> E = make_kron(dims, naxes, seed + 1000 * b);
        all.insert(all.end(), E.begin(), E.end());
    }
    return all;
}

static const char *NAMES[] = {"None", "Square16", "Rect32x8", "Cubic8", "Bilayer16", "Tri16", "Ttp16"};
static bool gate(HopForm f, const std::vector<double> &E)  // one block, the same matrix as eT2 and eTinv2
{
    std::vector<double> img;
    return build_hop_image(f, 1, E.data(), E.data(), nullptr, img);
}

static void gate_forms()
{
    const HopForm forms[] = {HopForm::Square16, HopForm::Rect32x8, HopForm::Cubic8, HopForm::Bilayer16};
    for (HopForm f : forms) {
        const HopFormRow &row = hop_row(f);
        const std::string name = NAMES[(int)f];
        for (int nb = 1; nb <= 2; ++nb) {
            const std::vector<double> e2 = make_blocks(row.dims, row.naxes, nb, 11 * (int)f + nb);
            const std::vector<double> ei = make_blocks(row.dims, row.naxes, nb, 77 * (int)f + nb);
            std::vector<double> img;
            const bool ok = build_hop_image(f, nb, e2.data(), ei.data(), nullptr, img);
            expect(ok, name + ": a Kronecker product of its own shape is accepted");
            expect(img.size() == (size_t)4 * nb * (row.fa + row.fb), name + ": image size");
            std::printf("hash %s/nb%d %016llx\n", name.c_str(), nb, (unsigned long long)fnv1a64(img));
        }
        // one block, perturbed
        const std::vector<double> E = make_kron(row.dims, row.naxes, 5 + (int)f);
        const size_t n = row.n, off = (n - 1) + n * (n - 2);  // an entry outside every axis block
        auto with = [&](size_t at, double v) {
            std::vector<double> P = E;
            P[at] = v;
            return P;
        };
        expect(gate(f, E), name + ": the unperturbed block");
        expect(!gate(f, with(off, E[off] * (1.0 + 1e-12))), name + ": one entry scaled by 1 + 1e-12 is rejected");
        uint64_t bits;
        std::memcpy(&bits, &E[off], 8);
        ++bits;
        double ulp;
        std::memcpy(&ulp, &bits, 8);
        expect(ulp != E[off] && gate(f, with(off, ulp)), name + ": one entry moved by one ulp is accepted");
        expect(!gate(f, with(0, 0.0)), name + ": E[0] = 0 is rejected");
        expect(!gate(f, with(0, -E[0])), name + ": E[0] < 0 is rejected");
        expect(!gate(f, with(0, std::numeric_limits<double>::quiet_NaN())), name + ": E[0] = NaN is rejected");
        expect(!gate(f, with(off, std::numeric_limits<double>::infinity())), name + ": an Inf is rejected");
    }
    // products of another shape at the same n
    const int sq[2] = {16, 16}, r328[2] = {32, 8}, r832[2] = {8, 32};
    expect(!gate(HopForm::Square16, make_kron(r328, 2, 31)), "Square16 rejects a 32 x 8 product");
    expect(!gate(HopForm::Rect32x8, make_kron(sq, 2, 32)), "Rect32x8 rejects a 16 x 16 product");
    expect(!gate(HopForm::Rect32x8, make_kron(r832, 2, 33)), "Rect32x8 rejects an 8 x 32 product");
}

// Circulant factors F[r][c] = coef[(r - c) mod 16] with positive, asymmetric coefficients: polynomials in the shifts X, Y,
// D = XY (and A = X Y^-1), which commute, and E as the same polynomial product written out entry by entry
struct HostCase {
    int nf, nb;
    std::vector<double> hf, E[2];  // [block][eT2, eTinv2][factor][256]; eT2 and eTinv2, nb blocks each
};
static HostCase make_host_case(HopForm form)
{
    HostCase hc;
    const int nf = hc.nf = form == HopForm::Tri16 ? 3 : 4, nb = hc.nb = form == HopForm::Tri16 ? 2 : 1, n = 256;
    std::vector<double> &hf = hc.hf;
    hf.resize((size_t)nb * 2 * nf * 256);
    Lcg g{(uint64_t)(900 + nf)};
    for (int b = 0; b < nb; ++b)
        for (int m = 0; m < 2; ++m) {
            {
                double coef[4][16];
                for (int k = 0; k < 4; ++k)
                    for (int s = 0; s < 16; ++s) coef[k][s] = k < nf ? g.next() * (1.0 / 16.0) : (s == 0 ? 1.0 : 0.0);
                for (int k = 0; k < nf; ++k)
                    for (int c = 0; c < 16; ++c)
                        for (int r = 0; r < 16; ++r) hf[(((size_t)b * 2 + m) * nf + k) * 256 + r + 16 * c] = coef[k][(r - c) & 15];
                std::vector<double> M((size_t)n * n);
                const int na = nf == 4 ? 16 : 1;  // (three factors: the anti-diagonal polynomial is the identity)
                for (int y2 = 0; y2 < 16; ++y2)
                    for (int x2 = 0; x2 < 16; ++x2)
                        for (int y = 0; y < 16; ++y)
                            for (int x = 0; x < 16; ++x) {
                                double acc = 0.0;
                                for (int sd = 0; sd < 16; ++sd)
                                    for (int sa = 0; sa < na; ++sa)
                                        acc += coef[2][sd] * coef[3][sa] * coef[0][(x - x2 - sd + sa) & 15] * coef[1][(y - y2 - sd - sa) & 15];
                                M[(x + 16 * y) + (size_t)n * (x2 + 16 * y2)] = acc;
                            }
                hc.E[m].insert(hc.E[m].end(), M.begin(), M.end());
            }
        }
    return hc;
}
static void host_forms()
{
    for (HopForm form : {HopForm::Tri16, HopForm::Ttp16}) {
        const std::string name = NAMES[(int)form];
        const HostCase hc = make_host_case(form);
        const int nf = hc.nf, nb = hc.nb;
        const std::vector<double> &hf = hc.hf, *E = hc.E;
        std::vector<double> img;
        expect(build_hop_image(form, nb, E[0].data(), E[1].data(), hf.data(), img), name + ": commuting circulant factors are accepted");
        expect(img.size() == (size_t)4 * nb * nf * 256, name + ": image size");
        std::printf("hash %s/nb%d %016llx\n", name.c_str(), nb, (unsigned long long)fnv1a64(img));
        // Fd of block 0, eT2 swapped with its transpose
        std::vector<double> sw = hf;
        for (int c = 0; c < 16; ++c)
            for (int r = 0; r < 16; ++r) sw[512 + r + 16 * c] = hf[512 + c + 16 * r];
        int bad = -1;
        expect(!build_hop_image(form, nb, E[0].data(), E[1].data(), sw.data(), img, &bad) && bad == 0,
               name + ": a factor swapped with its transpose is rejected");
    }
}

int main()
{
    gate_forms();
    host_forms();
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("ok\n");
    return failures ? 1 : 0;
}
