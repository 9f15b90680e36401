// The host arithmetic of the q-state engine's replica exchange (csrc/mc_tables.h: J, a pair's table, the product rule,
// the cut of a dqmc_qs_sweep call into launches) and the beta domain of its sweep (qs_beta_in_domain) on their own: built by tests/test_qs_exchange_host.py with
// g++ -fsanitize=address,undefined and run as a child process on the CPU.  The program only prints its inputs and what
// the header makes of them (doubles as hex floats); the pytest side restates every line in numpy and compares.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mc_tables.h"

using namespace mc_tables;

int main()
{
    // J: n_bonds, then the table
    const std::vector<std::pair<int64_t, std::vector<int64_t>>> bits = {
        {18, {1073741824, 0, 0}},                                        // 3 x 3 Potts
        {32, {1073741824, 331802365, -868669089, -868669089, 331802365}},  // clock q = 5 (entries of any sign)
        {65536, {4294967296, -4294967296}},                              // the create-time limits
        {0, {1073741824, 0}},
        {7, {0, 0, 0}},
        {1, {1, 0}},
        {2147483647, {4294967296, 0}},                                   // beyond what a table can hold
        // |e_q30| = 2^32 on the bond counts of CubicLattice(4, 3) and BilayerSquareLattice(4): clock q = 7 with J = 4
        {324, {4294967296, 2677868308, -955720134, -3869631822, -3869631822, -955720134, 2677868308}},
        {80, {-4294967296, 0, 0}},                                       // Potts q = 3 with J = -4
    };
    for (const auto &c : bits) {
        std::printf("bits %" PRId64 " %d :", c.first, qs_exchange_bits(c.first, c.second.data(), (int)c.second.size()));
        for (int64_t e : c.second) std::printf(" %" PRId64, e);
        std::printf("\n");
    }
    // a pair's table and the product rule: db, J, then per |d| the product; then decisions (sgn, d, u) -> swap
    const double dbs[] = {0.05, -0.05, 0.3, 1.0e-9, 7.25, 0.0};
    const uint64_t ds[] = {0, 1, 2, 3, 1073741824ull, 1073741825ull, 741939459ull, (1ull << 34) - 1, 0x2AAAAAAAAAAAull,
                           (1ull << 50) - 1};
    for (double db : dbs) {
        const int J = 50;
        std::vector<double> t((size_t)J);
        qs_exchange_table(db, J, t.data());
        std::printf("table %a %d", db, J);
        for (double x : t) std::printf(" %a", x);
        std::printf("\n");
        for (uint64_t d : ds) std::printf("product %a %" PRIu64 " %a\n", db, d, qs_exchange_product(t.data(), J, d));
        const int sgn = db > 0.0 ? 1 : (db < 0.0 ? -1 : 0);
        for (int64_t d : {(int64_t)0, (int64_t)1073741824, (int64_t)-1073741824, (int64_t)5, (int64_t)-5})
            for (double u : {0.0, 0.5, 0.9499, 0.9999999})
                std::printf("swaps %a %" PRId64 " %a %d\n", db, d, u, qs_exchange_swaps(sgn, d, t.data(), J, u) ? 1 : 0);
    }
    // the finite domain of the sweep's acceptance product: z, the table, then (beta, verdict) for the doubles around
    // 700 / (z range), nine steps of one ulp, and the message of the first refusal
    const std::vector<std::pair<int, std::vector<int64_t>>> domains = {
        {4, {1073741824, 536870912, -536870912, -1073741824, -536870912, 536870912}},  // clock q = 6: range 2
        {8, {4294967296, -4294967296, -4294967296}},                                    // |J e| = 4 of both signs: range 8
        {8, {4294967296, 2677868308, -955720134, -3869631822, -3869631822, -955720134, 2677868308}},  // clock q = 7, J = 4
        {5, {-1073741824, 0, 0}},                                                       // Potts q = 3, J = -1, z = 5
    };
    for (const auto &c : domains) {
        const int q = (int)c.second.size();
        const double range = qs_table_range(c.second.data(), q);
        std::printf("domain %d %a :", c.first, range);
        for (int64_t e : c.second) std::printf(" %" PRId64, e);
        std::printf("\n");
        double beta = QS_BETA_DOMAIN / ((double)c.first * range);
        for (int i = 0; i < 4; ++i) beta = std::nextafter(beta, 0.0);
        std::string first;
        for (int i = 0; i < 9; ++i, beta = std::nextafter(beta, 1.0e300)) {
            std::string err;
            const bool ok = qs_beta_in_domain("fn", beta, c.first, c.second.data(), q, &err);
            if (!ok && first.empty()) first = err;
            std::printf("verdict %d %a %d\n", c.first, beta, ok ? 1 : 0);
        }
        std::printf("refusal %s\n", first.c_str());
        for (double b : {0.0, 1.0, 50.0, 1.0e300}) {
            std::string err;
            std::printf("verdict %d %a %d\n", c.first, b, qs_beta_in_domain("fn", b, c.first, c.second.data(), q, &err) ? 1 : 0);
        }
    }
    // the launch cut: n, first, thermalization, rate, k, chunk, T0
    const int64_t cuts[][7] = {
        {10, 1, 0, 1, 3, 100, 0},    // rounds behind 3, 6, 9; every sweep measured
        {10, 5, 3, 2, 4, 100, 7},    // first in the middle of a period
        {7, 1, 0, 1, 1, 100, 0},     // k = 1: a launch per sweep, every measurement deferred
        {5, 1, 0, 1, 9, 100, 0},     // k > n: one launch, no round
        {12, 1, 0, 5, 6, 4, 0},      // a work bound smaller than k
        {12, 3, 6, 3, 6, 4, 2},      // .. with a thermalization inside and first off the period
        {9, 1, 0, 2, 3, 100, 0},     // rounds on measured (6) and unmeasured (3, 9) sweeps
        {9, 1, 0, 1, 0, 4, 0},       // no rounds: the work bound alone
        {0, 1, 0, 1, 2, 4, 0},       // nothing to do
        {1100, 1, 0, 1, 0, 976, 0},  // the L = 4 .. 5 bound
    };
    for (const auto &c : cuts) {
        std::printf("cut %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " :", c[0], c[1],
                    c[2], c[3], c[4], c[5], c[6]);
        for (const SweepLaunch &l : qs_sweep_cut((int)c[0], c[1], c[2], c[3], c[4], (int)c[5], c[6]))
            std::printf(" %d,%" PRId64 ",%d,%" PRId64, l.n_sweeps, l.first, l.defer_last ? 1 : 0, l.T_at_start);
        std::printf("\n");
    }
    std::printf("ok\n");
    return 0;
}
