// mc_tables.h — what the two engines of the classical MC flavor (ising.hip, qstate.hip) work out on the host before
// anything reaches the device: the lattice tables of a create, the colour-sorted tables of a checkerboard sweep, the
// arithmetic of the logarithmic binner, the beta domain of the q-state sweep, and the q-state engine's replica exchange (the pair tables, the product rule, the
// cut of a sweep call into launches).  Plain C++17, no device runtime: mc_host.h includes it, and
// tests/mc_tables_check.cpp and tests/qs_exchange_check.cpp build it alone under the host sanitizers.  A refusal returns false with the message in *err,
// prefixed with the name of the ABI function the caller passes as fn.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace mc_tables {

constexpr int ROW = 8;           // a site's neighbour row on the device: z <= 8 entries padded with zeros to 8
constexpr int MAX_COLOURS = 16;
constexpr int WAVE = 64;

// The tables of dqmc_mc_params / dqmc_qs_params (1-based, neighs [N][z] with z fastest, bonds n_bonds x 2 column-major)
// as the engines keep them: nbr [N][z] and pairs [n_bonds][2], 0-based.  N and z are the caller's to check against its
// own limits first.
inline bool lattice_tables(const std::string &fn, int N, int z, int n_bonds, long series_capacity, const int64_t *neighs,
                           const int64_t *bonds, std::vector<int> &nbr, std::vector<int> &pairs, std::string *err)
{
    if (n_bonds < 0 || series_capacity < 0) return *err = fn + ": n_bonds and series_capacity must be >= 0", false;
    if (!neighs || (n_bonds > 0 && !bonds)) return *err = fn + ": neighbour or bonds table missing", false;
    for (long i = 0; i < (long)z * N; ++i)
        if (neighs[i] < 1 || neighs[i] > N) return *err = fn + ": neighbour index out of range 1..n_sites", false;
    for (long i = 0; i < 2L * n_bonds; ++i)
        if (bonds[i] < 1 || bonds[i] > N) return *err = fn + ": bond index out of range 1..n_sites", false;
    nbr.resize((size_t)N * z);
    for (size_t i = 0; i < nbr.size(); ++i) nbr[i] = (int)neighs[i] - 1;
    pairs.resize((size_t)2 * n_bonds);
    for (int b = 0; b < n_bonds; ++b) {
        pairs[2 * b] = (int)bonds[b] - 1;
        pairs[2 * b + 1] = (int)bonds[n_bonds + b] - 1;
    }
    return true;
}

// nbr [N][z] as n_rows >= N rows of ROW entries, zeros behind a row's z and in the rows past N
inline std::vector<int> padded_rows(const std::vector<int> &nbr, int N, int z, int n_rows)
{
    std::vector<int> rows((size_t)n_rows * ROW, 0);
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < z; ++k) rows[(size_t)i * ROW + k] = nbr[(size_t)i * z + k];
    return rows;
}

// A colouring (colour[i] in [0, n_colours), n_colours <= 16, no site sharing its colour with a neighbour) as the tables a
// checkerboard sweep reads: the sites sorted by colour, site order within a class; their padded neighbour rows in that
// order; the class offsets, n_off >= n_colours + 1 entries (the classes past n_colours are empty); the largest class, and
// the workgroup size that gives each of its sites a lane: whole waves, max_threads at most.
struct Colouring {
    std::vector<int> site, rows, off;  // [N], [N][ROW], [n_off]
    int largest = 0, threads = 0;
};
inline bool colour_tables(const std::string &fn, const std::vector<int> &nbr, int N, int z, const int32_t *colour,
                          int n_colours, int n_off, int max_threads, Colouring &out, std::string *err)
{
    if (!colour) return *err = fn + ": null colouring", false;
    if (n_colours < 1 || n_colours > MAX_COLOURS) return *err = fn + ": n_colours must be in 1..16", false;
    for (int i = 0; i < N; ++i)
        if (colour[i] < 0 || colour[i] >= n_colours)
            return *err = fn + ": the colour of site " + std::to_string(i) + " is out of range 0..n_colours-1", false;
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < z; ++k) {
            const int j = nbr[(size_t)i * z + k];
            if (j == i)
                return *err = fn + ": site " + std::to_string(i) + " lists itself as a neighbour (0-based): no colouring",
                       false;
            if (colour[j] == colour[i])
                return *err = fn + ": the neighbours " + std::to_string(i) + " and " + std::to_string(j) +
                              " (0-based sites) share colour " + std::to_string(colour[i]),
                       false;
        }
    out.off.assign((size_t)n_off, 0);
    out.site.assign((size_t)N, 0);
    out.rows.assign((size_t)N * ROW, 0);
    for (int i = 0; i < N; ++i) out.off[(size_t)colour[i] + 1] += 1;
    out.largest = 0;
    for (int c = 0; c + 1 < n_off; ++c) {
        out.largest = std::max(out.largest, out.off[(size_t)c + 1]);
        out.off[(size_t)c + 1] += out.off[c];
    }
    std::vector<int> fill(out.off.begin(), out.off.end() - 1);
    for (int i = 0; i < N; ++i) {
        const int e = fill[colour[i]]++;
        out.site[e] = i;
        for (int k = 0; k < z; ++k) out.rows[(size_t)e * ROW + k] = nbr[(size_t)i * z + k];
    }
    out.threads = std::min(max_threads, std::max(WAVE, (out.largest + WAVE - 1) / WAVE * WAVE));
    return true;
}

// measurements of run! (MC.jl:262-283) among the sweeps first..last: i > thermalization && i % rate == 0
inline int64_t measurements_in(int64_t first, int64_t last, int64_t thermalization, int64_t rate)
{
    const int64_t lo = std::max<int64_t>(first - 1, thermalization);  // (first >= 1)
    return last > lo ? last / rate - lo / rate : 0;
}

// ---- the logarithmic binner (include/dqmc_hip.h, "error bars of the MC flavor"): count[level] = T >> level after T pushes
inline int bin_levels(int64_t capacity)  // ceil(log2(capacity + 1)), one at least
{
    int L = 1;
    while (((int64_t)1 << L) < capacity + 1) ++L;
    return L;
}
inline int bin_lmax(int64_t T)  // the level that keeps push T + 1: the trailing 1-bits of T (>= the levels: no room left)
{
    int lmax = 0;
    while ((T >> lmax) & 1) ++lmax;
    return lmax;
}
inline int bin_reliable(int64_t T, int L)  // the last level with count >= 32, else 0
{
    int lv = 0;
    for (int l = 0; l < L; ++l)
        if ((T >> l) >= 32) lv = l;
    return lv;
}
// varN and covN of the header: (q/(n - 1) - a b/(n (n - 1)))/n, NaN below two samples (varN: a = b, q = x2_sum)
inline double bin_covN(double a, double b, double q, double n)
{
    if (n < 2.0) return std::nan("");
    return (q / (n - 1.0) - a * b / (n * (n - 1.0))) / n;
}
// mean, varN, varN0 and tau of n_elem elements and covN of n_pairs pairs from the sums of level 0 (xs0, x20) and of
// `level` (xs, x2, xy) after T pushes.  Pair p is the elements (2 p, 2 p + 1), or (0, 1 + p) with pairs_from_first.
inline void bin_finish(int n_elem, int n_pairs, bool pairs_from_first, int64_t T, int level, const double *xs0,
                       const double *x20, const double *xs, const double *x2, const double *xy, double *mean,
                       double *varN, double *varN0, double *tau, double *covN)
{
    const double n0 = (double)T, nl = (double)(T >> level);
    for (int k = 0; k < n_elem; ++k) {
        mean[k] = xs0[k] / n0;
        varN[k] = bin_covN(xs[k], xs[k], x2[k], nl);
        varN0[k] = bin_covN(xs0[k], xs0[k], x20[k], n0);
        tau[k] = 0.5 * (varN[k] / varN0[k] - 1.0);
    }
    for (int p = 0; p < n_pairs; ++p)
        covN[p] = pairs_from_first ? bin_covN(xs[0], xs[1 + p], xy[p], nl) : bin_covN(xs[2 * p], xs[2 * p + 1], xy[p], nl);
}

// ---- the finite domain of the q-state sweep's acceptance product (include/dqmc_hip.h, "Sweep" of the q-state section)
// Every partial product of p = fl(p w[a_k][b_k]), k < z, is the exponential of a sum of at most z exponents, each within
// beta range of zero, range = (max_d e_q30[d] - min_d e_q30[d]) 2^-30 (exact in fp64: the difference is below 2^34).
// With beta z range <= 700 all of them lie in [e^-700, e^700]: finite, non-zero and normal, with room for the rounding
// of 8 factors.  The comparison is fl(fl(beta z) range) <= 700.
constexpr double QS_BETA_DOMAIN = 700.0;
inline double qs_table_range(const int64_t *e_q30, int q)
{
    int64_t lo = e_q30[0], hi = e_q30[0];
    for (int d = 1; d < q; ++d) {
        lo = std::min(lo, e_q30[d]);
        hi = std::max(hi, e_q30[d]);
    }
    return (double)(hi - lo) * (1.0 / 1073741824.0);
}
inline bool qs_beta_in_domain(const std::string &fn, double beta, int z, const int64_t *e_q30, int q, std::string *err)
{
    const double range = qs_table_range(e_q30, q);
    if (beta * (double)z * range <= QS_BETA_DOMAIN) return true;
    char buf[256];
    std::snprintf(buf, sizeof buf,
                  ": beta = %.17g with z = %d and a table range of %.17g gives beta z range = %.17g, above the bound of "
                  "%g under which every partial acceptance product is finite and non-zero",
                  beta, z, range, beta * (double)z * range, QS_BETA_DOMAIN);
    return *err = fn + buf, false;
}

// ---- replica exchange of the q-state engine (include/dqmc_hip.h, "Replica exchange" of the q-state section)
// J, the entries of a pair's table: the smallest integer with 2^J > 2 n_bonds max_d |e_q30[d]| >= |E_a - E_b|
inline int qs_exchange_bits(int64_t n_bonds, const int64_t *e_q30, int q)
{
    unsigned __int128 bound = 0;
    for (int d = 0; d < q; ++d) {
        const unsigned __int128 a = (unsigned __int128)(e_q30[d] < 0 ? -e_q30[d] : e_q30[d]);
        bound = std::max(bound, a);
    }
    bound = bound * (unsigned __int128)(2 * n_bonds);
    int J = 0;
    while (J < 127 && ((unsigned __int128)1 << J) <= bound) ++J;
    return J;
}
// the pair's table for db = beta_a - beta_b: t[j] = exp(-(|db| 2^(j - 30))), the scaling exact, one libm call per entry
inline void qs_exchange_table(double db, int J, double *t)
{
    for (int j = 0; j < J; ++j) t[j] = std::exp(-std::ldexp(std::fabs(db), j - 30));
}
// p = 1.0, then p = p * t[j] for every set bit j of |d| in ascending order (|d| < 2^J)
inline double qs_exchange_product(const double *t, int J, uint64_t abs_d)
{
    double p = 1.0;
    for (int j = 0; j < J; ++j)
        if ((abs_d >> j) & 1) p = p * t[j];
    return p;
}
// does the pair swap?  d = E_a - E_b, sgn = the sign of db; u is looked at only where the product decides
inline bool qs_exchange_swaps(int sgn, int64_t d, const double *t, int J, double u)
{
    if (sgn == 0 || d == 0 || (d > 0) == (sgn > 0)) return true;
    return u < qs_exchange_product(t, J, d < 0 ? (uint64_t)0 - (uint64_t)d : (uint64_t)d);
}
// One dqmc_qs_sweep(n, first, thermalization, rate) call as launches of the sweep kernel.  A launch ends at every sweep
// with an exchange round (global index a multiple of k; k = 0: no rounds) and at the work bound of `chunk` sweeps,
// whichever comes first.  defer_last: the launch's last sweep has a round and is measured, so its measurement is the
// exchange kernel's.  T_at_start: the binner's push count when the launch starts, T0 at the first.
struct SweepLaunch {
    int n_sweeps;
    int64_t first;
    bool defer_last;
    int64_t T_at_start;
};
// (at_measured: a launch also ends at every measured sweep - the cut of qs_scaling_cut below)
inline std::vector<SweepLaunch> qs_cut_launches(int n, int64_t first, int64_t thermalization, int64_t rate, int64_t k,
                                                int chunk, int64_t T0, bool at_measured)
{
    std::vector<SweepLaunch> out;
    int64_t T = T0;
    for (int done = 0; done < n;) {
        const int64_t f = first + done;
        int64_t m = std::min<int64_t>(std::max(chunk, 1), n - done);
        if (k > 0) m = std::min<int64_t>(m, k - (f - 1) % k);
        if (at_measured) {  // the first measured sweep at or behind f: the smallest multiple of rate above thermalization
            const int64_t g0 = std::max<int64_t>(f, thermalization + 1);
            m = std::min<int64_t>(m, (g0 + rate - 1) / rate * rate - f + 1);
        }
        const int64_t last = f + m - 1;
        const bool round = k > 0 && last % k == 0;
        out.push_back(SweepLaunch{(int)m, f, round && last > thermalization && last % rate == 0, T});
        T += measurements_in(f, last, thermalization, rate);
        done += (int)m;
    }
    return out;
}
inline std::vector<SweepLaunch> qs_sweep_cut(int n, int64_t first, int64_t thermalization, int64_t rate, int64_t k,
                                             int chunk, int64_t T0)
{
    return qs_cut_launches(n, first, thermalization, rate, k, chunk, T0, false);
}
// The same call with the scaling measurement on (include/dqmc_hip.h, "Scaling" of the q-state section): a launch
// additionally ends at every measured sweep, so that the measured configuration lies in device memory when the
// measurement kernel runs behind the launch (and behind its round).  A launch then holds at most one measured sweep,
// its last.  Rounds, defer_last and T_at_start follow the rule above; the launches still add up to the n sweeps.
inline std::vector<SweepLaunch> qs_scaling_cut(int n, int64_t first, int64_t thermalization, int64_t rate, int64_t k,
                                               int chunk, int64_t T0)
{
    return qs_cut_launches(n, first, thermalization, rate, k, chunk, T0, true);
}

// The arguments of dqmc_qs_set_stiffness with n_dir > 0 (include/dqmc_hip.h, "Stiffness" of the q-state section), checked
// on the host before the device is touched: the counts, the range of every slot class (which slots are counted is the
// caller's definition), d1 exactly antisymmetric and d2 exactly symmetric with magnitudes <= 2^32, x finite.
inline bool qs_stiffness_check(const std::string &fn, int N, int z, int q, int n_dir, int n_classes, const int8_t *slot_class,
                               const int64_t *d1, const int64_t *d2, const double *x, std::string *err)
{
    if (n_dir < 1 || n_dir > 4) return *err = fn + ": n_dir must be in 0..4 (0 = off)", false;
    if (n_classes < 1 || n_classes > 8) return *err = fn + ": n_classes must be in 1..8", false;
    if (!slot_class || !d1 || !d2 || !x) return *err = fn + ": slot_class, d1_q30, d2_q30 or x missing", false;
    for (long i = 0; i < (long)z * N; ++i)
        if (slot_class[i] < -1 || slot_class[i] >= n_classes)
            return *err = fn + ": the class of slot " + std::to_string(i % z) + " of site " + std::to_string(i / z) +
                          " (0-based) is outside -1.." + std::to_string(n_classes - 1),
                   false;
    const int64_t top = (int64_t)1 << 32;
    for (int d = 0; d < q; ++d) {
        if (d1[d] > top || d1[d] < -top || d2[d] > top || d2[d] < -top)
            return *err = fn + ": d1_q30 / d2_q30 entry " + std::to_string(d) + " exceeds 2^32 in magnitude", false;
        if (d1[d] != -d1[(q - d) % q])
            return *err = fn + ": d1_q30[" + std::to_string(d) + "] != -d1_q30[" + std::to_string((q - d) % q) +
                          "]: the table is not antisymmetric",
                   false;
        if (d2[d] != d2[(q - d) % q])
            return *err = fn + ": d2_q30[" + std::to_string(d) + "] != d2_q30[" + std::to_string((q - d) % q) +
                          "]: the table is not symmetric",
                   false;
    }
    for (int i = 0; i < n_dir * n_classes; ++i)
        if (!std::isfinite(x[i])) return *err = fn + ": x[" + std::to_string(i) + "] is not finite", false;
    return true;
}

}  // namespace mc_tables
