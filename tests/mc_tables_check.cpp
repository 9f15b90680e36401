// The host tables of the classical MC flavor (csrc/mc_tables.h) on their own: built by tests/test_mc_tables_host.py with
// g++ -fsanitize=address,undefined and run as a child process on the CPU.  The program only prints: its inputs (lattices
// and colourings made here with integer arithmetic, sums from an integer LCG) and what the header makes of them.  The
// pytest side restates every item in numpy and compares; nothing is recorded from the code under test.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "mc_tables.h"

using namespace mc_tables;

static int failures = 0;
static void expect(bool ok, const std::string &what)
{
    if (!ok) {
        std::printf("FAILED: %s\n", what.c_str());
        ++failures;
    }
}

template <typename T>
static void line(const std::string &name, const char *key, const std::vector<T> &v)
{
    std::printf("case %s %s", name.c_str(), key);
    for (const T &x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

// a lattice as the ABI takes it: neighs [N][z] (z fastest) and bonds n_bonds x 2 column-major, both 1-based
struct Lattice {
    std::string name;
    int N, z;
    std::vector<int64_t> neighs, bonds;
};
static void add_bonds(Lattice &l)  // site i with its first z / 2 neighbours
{
    const int nb = l.N * (l.z / 2);
    l.bonds.assign((size_t)2 * nb, 0);
    for (int i = 0, b = 0; i < l.N; ++i)
        for (int k = 0; k < l.z / 2; ++k, ++b) {
            l.bonds[b] = i + 1;
            l.bonds[nb + b] = l.neighs[(size_t)i * l.z + k];
        }
}
static Lattice chain(int L)
{
    Lattice l{"chain" + std::to_string(L), L, 2, {}, {}};
    for (int i = 0; i < L; ++i) {
        l.neighs.push_back((i + 1) % L + 1);
        l.neighs.push_back((i + L - 1) % L + 1);
    }
    add_bonds(l);
    return l;
}
static Lattice grid(int L, bool triangular)  // periodic L x L, site x + L y; triangular: the (+1, +1) diagonal as well
{
    Lattice l{(triangular ? "triangular" : "square") + std::to_string(L), L * L, triangular ? 6 : 4, {}, {}};
    auto at = [L](int x, int y) { return (int64_t)((x + L) % L + L * ((y + L) % L) + 1); };
    for (int y = 0; y < L; ++y)
        for (int x = 0; x < L; ++x) {
            std::vector<int64_t> row = {at(x + 1, y), at(x, y + 1)};
            if (triangular) row.push_back(at(x + 1, y + 1));
            row.push_back(at(x - 1, y));
            row.push_back(at(x, y - 1));
            if (triangular) row.push_back(at(x - 1, y - 1));
            l.neighs.insert(l.neighs.end(), row.begin(), row.end());
        }
    add_bonds(l);
    return l;
}
// in site order, the smallest colour no neighbour j < i has
static std::vector<int32_t> greedy(const std::vector<int> &nbr, int N, int z)
{
    std::vector<int32_t> colour((size_t)N, -1);
    for (int i = 0; i < N; ++i) {
        int c = 0;
        for (bool clash = true; clash; c += clash) {
            clash = false;
            for (int k = 0; k < z; ++k) clash = clash || colour[nbr[(size_t)i * z + k]] == c;
        }
        colour[i] = c;
    }
    return colour;
}

static void colour_cases()
{
    const Lattice cases[] = {grid(4, false), grid(3, false), grid(4, true), chain(5), chain(300), chain(700)};
    for (const Lattice &l : cases) {
        std::vector<int> nbr, pairs;
        std::string err;
        const int nb = (int)l.bonds.size() / 2;
        expect(lattice_tables("f", l.N, l.z, nb, 0, l.neighs.data(), l.bonds.data(), nbr, pairs, &err), l.name + ": accepted");
        std::printf("case %s shape %d %d %d\n", l.name.c_str(), l.N, l.z, nb);
        line(l.name, "neighs", l.neighs);
        line(l.name, "bonds", l.bonds);
        line(l.name, "nbr", nbr);
        line(l.name, "pairs", pairs);
        line(l.name, "padded", padded_rows(nbr, l.N, l.z, l.N + 1));
        const std::vector<int32_t> colour = greedy(nbr, l.N, l.z);
        int nc = 0;
        for (int32_t c : colour) nc = std::max(nc, c + 1);
        line(l.name, "colour", colour);
        for (int n_off : {nc + 1, MAX_COLOURS + 1}) {  // the two engines' lengths of off
            Colouring t;
            expect(colour_tables("f", nbr, l.N, l.z, colour.data(), nc, n_off, 256, t, &err), l.name + ": colouring accepted");
            const std::string tag = "off" + std::to_string(n_off == nc + 1 ? 0 : 17) + ".";
            line(l.name, (tag + "site").c_str(), t.site);
            line(l.name, (tag + "rows").c_str(), t.rows);
            line(l.name, (tag + "off").c_str(), t.off);
            line(l.name, (tag + "largest_threads").c_str(), std::vector<int>{t.largest, t.threads});
        }
    }
}

static void refused(const char *name, bool ok, const std::string &err, const std::string &text)
{
    expect(!ok, std::string(name) + ": refused");
    expect(err.compare(0, 9, "dqmc_fn: ") == 0, std::string(name) + ": the message starts with the function's name");
    expect(err.find(text) != std::string::npos, std::string(name) + ": the message says '" + text + "', got '" + err + "'");
    std::printf("refused %s: %s\n", name, err.c_str());
}
static void refusals()
{
    const Lattice l = grid(4, false);
    std::vector<int> nbr, pairs;
    std::string err;
    const int nb = (int)l.bonds.size() / 2;
    expect(lattice_tables("dqmc_fn", l.N, l.z, nb, 0, l.neighs.data(), l.bonds.data(), nbr, pairs, &err), "square4");
    const std::vector<int32_t> good = greedy(nbr, l.N, l.z);
    Colouring t;
    auto with = [&](int site, int32_t c) {
        std::vector<int32_t> v = good;
        v[site] = c;
        return v;
    };
    refused("colour_high", colour_tables("dqmc_fn", nbr, l.N, l.z, with(5, 2).data(), 2, 3, 256, t, &err), err,
            "the colour of site 5 is out of range");
    refused("colour_negative", colour_tables("dqmc_fn", nbr, l.N, l.z, with(0, -1).data(), 2, 3, 256, t, &err), err,
            "the colour of site 0 is out of range");
    refused("n_colours_0", colour_tables("dqmc_fn", nbr, l.N, l.z, good.data(), 0, 1, 256, t, &err), err,
            "n_colours must be in 1..16");
    refused("n_colours_17", colour_tables("dqmc_fn", nbr, l.N, l.z, good.data(), 17, 18, 256, t, &err), err,
            "n_colours must be in 1..16");
    refused("shared", colour_tables("dqmc_fn", nbr, l.N, l.z, with(1, good[0]).data(), 2, 3, 256, t, &err), err,
            "the neighbours 0 and 1 (0-based sites) share colour 0");
    refused("null", colour_tables("dqmc_fn", nbr, l.N, l.z, nullptr, 2, 3, 256, t, &err), err, "null colouring");
    {
        const Lattice one = chain(1);  // its only site is its own neighbour
        std::vector<int> n1, p1;
        expect(lattice_tables("dqmc_fn", 1, 2, 1, 0, one.neighs.data(), one.bonds.data(), n1, p1, &err), "chain1");
        const int32_t c0 = 0;
        refused("self", colour_tables("dqmc_fn", n1, 1, 2, &c0, 1, 2, 256, t, &err), err, "site 0 lists itself as a neighbour");
    }
    std::vector<int64_t> bad = l.neighs;
    bad[7] = 0;
    refused("neighbour_0", lattice_tables("dqmc_fn", l.N, l.z, nb, 0, bad.data(), l.bonds.data(), nbr, pairs, &err), err,
            "neighbour index out of range 1..n_sites");
    bad[7] = l.N + 1;
    refused("neighbour_N1", lattice_tables("dqmc_fn", l.N, l.z, nb, 0, bad.data(), l.bonds.data(), nbr, pairs, &err), err,
            "neighbour index out of range 1..n_sites");
    bad = l.bonds;
    bad[3] = l.N + 1;
    refused("bond_N1", lattice_tables("dqmc_fn", l.N, l.z, nb, 0, l.neighs.data(), bad.data(), nbr, pairs, &err), err,
            "bond index out of range 1..n_sites");
    refused("no_bonds_table", lattice_tables("dqmc_fn", l.N, l.z, nb, 0, l.neighs.data(), nullptr, nbr, pairs, &err), err,
            "neighbour or bonds table missing");
    refused("series_negative", lattice_tables("dqmc_fn", l.N, l.z, nb, -1, l.neighs.data(), l.bonds.data(), nbr, pairs, &err),
            err, "n_bonds and series_capacity must be >= 0");
}

static void binner_counts()
{
    for (int64_t cap : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)100000, (int64_t)1 << 40}) {
        const int L = bin_levels(cap);
        std::printf("levels %" PRId64 " %d\n", cap, L);
        std::printf("lmax %" PRId64, cap);
        for (int64_t T = 0; T <= 70; ++T) std::printf(" %d", bin_lmax(T));
        std::printf("\nreliable %" PRId64, cap);
        for (int64_t T = 0; T <= 70; ++T) std::printf(" %d", bin_reliable(T, L));
        std::printf("\n");
    }
    for (int64_t therm : {0, 3})
        for (int64_t rate : {1, 2, 3})
            for (int64_t first = 1; first <= 6; ++first) {
                std::printf("measurements_in %" PRId64 " %" PRId64 " %" PRId64, therm, rate, first);
                for (int64_t last = first - 1; last <= 12; ++last) std::printf(" %" PRId64, measurements_in(first, last, therm, rate));
                std::printf("\n");
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
static void hex_line(const char *name, const char *key, const std::vector<double> &v)
{
    std::printf("finish %s %s", name, key);
    for (double x : v) std::printf(" %a", x);
    std::printf("\n");
}
// the sums are made up (the finish is plain arithmetic on them), level-0 sums larger than those of `level`
static void finish_case(const char *name, int ne, int np, bool from_first, int64_t T, int level, uint64_t seed)
{
    Lcg g{seed};
    std::vector<double> xs0(ne), x20(ne), xs(ne), x2(ne), xy(np);
    for (int k = 0; k < ne; ++k) {
        xs0[k] = 40.0 * g.next();
        x20[k] = 90.0 * g.next();
        xs[k] = 10.0 * g.next();
        x2[k] = 30.0 * g.next();
    }
    for (int p = 0; p < np; ++p) xy[p] = 20.0 * g.next();
    std::vector<double> mean(ne), varN(ne), varN0(ne), tau(ne), covN(np);
    bin_finish(ne, np, from_first, T, level, xs0.data(), x20.data(), xs.data(), x2.data(), xy.data(), mean.data(),
               varN.data(), varN0.data(), tau.data(), covN.data());
    std::printf("finish %s shape %d %d %d %" PRId64 " %d\n", name, ne, np, from_first ? 1 : 0, T, level);
    hex_line(name, "xs0", xs0);
    hex_line(name, "x20", x20);
    hex_line(name, "xs", xs);
    hex_line(name, "x2", x2);
    hex_line(name, "xy", xy);
    hex_line(name, "mean", mean);
    hex_line(name, "varN", varN);
    hex_line(name, "varN0", varN0);
    hex_line(name, "tau", tau);
    hex_line(name, "covN", covN);
    if ((T >> level) < 2)
        for (int k = 0; k < ne; ++k) expect(varN[k] != varN[k], std::string(name) + ": varN below two samples is NaN");
    if (T < 2)
        for (int k = 0; k < ne; ++k) expect(varN0[k] != varN0[k], std::string(name) + ": varN0 below two samples is NaN");
}

int main()
{
    colour_cases();
    refusals();
    binner_counts();
    finish_case("ising", 4, 2, false, 37, 2, 11);      // [E, E2, |M|, M2], pairs (E, E2), (|M|, M2)
    finish_case("fss3", 5, 4, true, 37, 2, 12);        // [M2, M4, S_0 .. S_2], pairs (M2, .)
    finish_case("fss0", 2, 1, true, 1000, 0, 13);      // n_k = 0, level 0
    finish_case("ising_short", 4, 2, false, 5, 2, 14); // one sample at the level: NaN there, numbers at level 0
    finish_case("fss_single", 3, 2, true, 1, 0, 15);   // one sample in all: NaN everywhere but the mean
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("ok\n");
    return failures ? 1 : 0;
}
