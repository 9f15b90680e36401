// The launch cut of a dqmc_qs_sweep call with the scaling measurement on (csrc/mc_tables.h: qs_scaling_cut) beside the
// cut without it (qs_sweep_cut): built by tests/test_qstate_scaling_host.py with g++ -fsanitize=address,undefined and run
// as a child process on the CPU.  The program only prints its inputs and the launches the header makes of them; the
// pytest side checks every line.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mc_tables.h"

using namespace mc_tables;

static void print(const char *tag, const std::vector<SweepLaunch> &v)
{
    std::printf("%s", tag);
    for (const SweepLaunch &l : v)
        std::printf(" %d,%" PRId64 ",%d,%" PRId64, l.n_sweeps, l.first, l.defer_last ? 1 : 0, l.T_at_start);
    std::printf("\n");
}

int main()
{
    const int64_t starts[][3] = {{23, 1, 0}, {17, 6, 5}, {0, 3, 2}, {1, 12, 0}};  // n, first, T0
    for (const auto &s : starts)
        for (int64_t rate : {1, 3})
            for (int64_t therm : {0, 4})
                for (int64_t k : {0, 1, 2, 5})
                    for (int chunk : {1, 7}) {
                        std::printf("case %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %" PRId64 "\n", s[0],
                                    s[1], therm, rate, k, chunk, s[2]);
                        print("plain", qs_sweep_cut((int)s[0], s[1], therm, rate, k, chunk, s[2]));
                        print("scaling", qs_scaling_cut((int)s[0], s[1], therm, rate, k, chunk, s[2]));
                    }
    std::printf("ok\n");
    return 0;
}
