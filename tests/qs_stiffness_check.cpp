// The host-side validation of dqmc_qs_set_stiffness (csrc/mc_tables.h, qs_stiffness_check) on its own, built by
// tests/test_qstate_stiffness_host.py under the host sanitizers: one accepted argument set, then every refusal, each
// from the accepted set with one thing wrong.  Prints "<name> <0|1> <message>" per case and "ok" at the end.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "mc_tables.h"

int main()
{
    const int N = 6, z = 4, q = 5, n_dir = 2, n_c = 3;
    std::vector<int8_t> cls((size_t)z * N);
    for (size_t i = 0; i < cls.size(); ++i) cls[i] = (int8_t)((int)(i % 4) - 1);  // -1 .. 2
    const int64_t top = (int64_t)1 << 32;
    std::vector<int64_t> d1 = {0, top, -7, 7, -top}, d2 = {top, 3, -top, -top, 3};
    std::vector<double> x = {1.0, 0.0, 0.5, 0.0, 1.0, -0.5};
    int bad = 0;
    auto run = [&](const char *name, bool want, int nd, int nc, const int8_t *c, const int64_t *a, const int64_t *b,
                   const double *xx) {
        std::string msg;
        const bool got = mc_tables::qs_stiffness_check("f", N, z, q, nd, nc, c, a, b, xx, &msg);
        std::printf("%s %d %s\n", name, (int)got, msg.c_str());
        if (got != want || (!got && msg.rfind("f: ", 0) != 0)) ++bad;
    };
    run("valid", true, n_dir, n_c, cls.data(), d1.data(), d2.data(), x.data());
    run("n_dir_low", false, -1, n_c, cls.data(), d1.data(), d2.data(), x.data());
    run("n_dir_high", false, 5, n_c, cls.data(), d1.data(), d2.data(), x.data());
    run("n_classes_low", false, n_dir, 0, cls.data(), d1.data(), d2.data(), x.data());
    run("n_classes_high", false, n_dir, 9, cls.data(), d1.data(), d2.data(), x.data());
    run("null_class", false, n_dir, n_c, nullptr, d1.data(), d2.data(), x.data());
    run("null_d1", false, n_dir, n_c, cls.data(), nullptr, d2.data(), x.data());
    run("null_d2", false, n_dir, n_c, cls.data(), d1.data(), nullptr, x.data());
    run("null_x", false, n_dir, n_c, cls.data(), d1.data(), d2.data(), nullptr);
    {
        auto c = cls;
        c.back() = 3;
        run("class_high", false, n_dir, n_c, c.data(), d1.data(), d2.data(), x.data());
        c.back() = -2;
        run("class_low", false, n_dir, n_c, c.data(), d1.data(), d2.data(), x.data());
    }
    {
        auto a = d1;
        a[2] = 7;  // a[2] == a[3]: not antisymmetric
        run("d1_symmetry", false, n_dir, n_c, cls.data(), a.data(), d2.data(), x.data());
        a = d1;
        a[0] = 1;  // d1[0] must be its own negative
        run("d1_zero", false, n_dir, n_c, cls.data(), a.data(), d2.data(), x.data());
        a = d1;
        a[1] = top + 1;
        a[4] = -top - 1;
        run("d1_magnitude", false, n_dir, n_c, cls.data(), a.data(), d2.data(), x.data());
    }
    {
        auto b = d2;
        b[1] = 4;
        run("d2_symmetry", false, n_dir, n_c, cls.data(), d1.data(), b.data(), x.data());
        b = d2;
        b[0] = top + 1;
        run("d2_magnitude", false, n_dir, n_c, cls.data(), d1.data(), b.data(), x.data());
    }
    {
        auto xx = x;
        xx[5] = std::numeric_limits<double>::infinity();
        run("x_inf", false, n_dir, n_c, cls.data(), d1.data(), d2.data(), xx.data());
        xx[5] = std::nan("");
        run("x_nan", false, n_dir, n_c, cls.data(), d1.data(), d2.data(), xx.data());
    }
    if (bad) {
        std::printf("%d cases wrong\n", bad);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
