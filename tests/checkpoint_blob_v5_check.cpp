// Stand-alone check of format versions 5 - 8 of the checkpoint blob (csrc/state_blob.cpp: the extension for the response
// binners), built with g++ -fsanitize=address,undefined by tests/test_response_host.py and run as a child process on the
// CPU.  With no response binner on, versions 1 - 4 are written byte for byte as before; versions 5 - 8 round-trip; every
// truncation, a trailing byte, every single flipped extension byte (a wrong checksum), every single configuration field
// that differs and another F table are refused with the reason named; a version 5 - 8 blob is refused by a handle
// without the binners and by validate_all / validate_any, a version 1 - 4 blob by a handle with them; layouts that would
// overflow size_t are refused.
#include "state_blob.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace dqmc_blob;

static int failures = 0;
#define EXPECT(cond, ...)                              \
    do {                                               \
        if (!(cond)) {                                 \
            std::printf("FAIL line %d: ", __LINE__);   \
            std::printf(__VA_ARGS__);                  \
            std::printf("\n");                         \
            ++failures;                                \
        }                                              \
    } while (0)

static bool starts(const std::string &s, const char *prefix) { return s.compare(0, std::strlen(prefix), prefix) == 0; }

static Shape shape()
{
    Shape s{};
    std::strncpy(s.source_hash, "0123456789ab", HASH_BYTES);
    s.n_sites = 9; s.model_kind = 1; s.slices = 10; s.safe_mult = 5; s.n_walkers = 3; s.nb = 2;
    s.delta_tau = 0.1; s.U = 4.0;
    s.sec_n[0] = 2 * 2 * 81 + 2 * 9 + 1; s.sec_n_red[0] = s.sec_n[0];
    s.sec_n[5] = 5;
    s.bin[0] = {1, 2 * 81 + 2 * 9, 3, 7, 5};
    s.gm_kind = 1;
    return s;
}

static std::vector<uint8_t> build(const Shape &s, const Momenta &m, const Thermo &t, const Response &r)
{
    Layout l;
    ExtLayout e;
    ThermoLayout tl;
    ResponseLayout rl;
    std::string why;
    EXPECT(layout(s, &l, &why) && ext_layout(s, m, &e, &why) && thermo_layout(s, m, t, &tl, &why) &&
               response_layout(s, m, t, r, &rl, &why), "layout: %s", why.c_str());
    std::vector<uint8_t> b(rl.total);
    for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)(i * 131 + 7);  // the payload: anything
    write_header(s, m, t, r, b.data());
    write_ext(m, e, b.data());
    seal_ext(e, b.data());
    write_thermo(t, tl, b.data());
    seal_thermo(tl, b.data());
    write_response(r, rl, b.data());
    seal_response(rl, b.data());
    return b;
}

int main()
{
    const Shape s = shape();
    const int n_q = 3, n_dirs = 9, K = 5, n_ch = 3, K_cc = 5;
    std::vector<double> ct(n_dirs * n_q), st(n_dirs * n_q), F(K * K * n_ch), F2;
    for (size_t i = 0; i < ct.size(); ++i) { ct[i] = 1.0 / (double)(i + 1); st[i] = -0.5 * (double)i; }
    for (size_t i = 0; i < F.size(); ++i) F[i] = 0.25 * (double)i - 3.0;
    Momenta m_off, m_on;
    m_on.n_q = n_q; m_on.n_dirs = n_dirs; m_on.cos_tab = ct.data(); m_on.sin_tab = st.data();
    m_on.bin[0] = {1, 4 * n_q, 3, 7, 5};
    Thermo t_off, t_on;
    t_on.n = 12; t_on.n_red = 12; t_on.bin = {1, 11, 3, 7, 5}; t_on.T_hash = 0x1234; t_on.U_s = 4.0;
    Response r_off, r_on;
    r_on.n_ch = n_ch; r_on.K = K; r_on.K_cc = K_cc; r_on.F = F.data();
    r_on.bin[0] = {1, 2 * n_ch * n_q, 3, 7, 5};
    r_on.bin[1] = {1, 2 * n_ch * n_q, 2, 3, 2};
    r_on.bin[2] = {1, 2 * K_cc * n_q + K_cc, 3, 7, 3};
    std::string why;
    Shape back;
    Momenta mb;
    Thermo tb;
    Response rb;

    int base = 0;
    for (const Momenta *m : {&m_off, &m_on})
        for (const Thermo *t : {&t_off, &t_on}) {
            const int old_version = (t->any() ? 3 : 1) + (m->any() ? 1 : 0), version = old_version + 4;
            ++base;
            // ---- the binners off: versions 1 - 4 byte for byte, through the new entry points too
            ThermoLayout tl;
            EXPECT(thermo_layout(s, *m, *t, &tl), "thermo_layout");
            std::vector<uint8_t> a(tl.total), b = build(s, *m, *t, r_off);
            {
                ExtLayout e;
                ext_layout(s, *m, &e);
                for (size_t i = 0; i < a.size(); ++i) a[i] = (uint8_t)(i * 131 + 7);
                write_header(s, *m, *t, a.data());
                write_ext(*m, e, a.data()); seal_ext(e, a.data());
                write_thermo(*t, tl, a.data()); seal_thermo(tl, a.data());
            }
            EXPECT(a == b && a[8] == old_version, "the binners off do not write the version-%d bytes", old_version);
            EXPECT(validate_full(b.data(), b.size(), s, *m, *t, r_off, &back, &mb, &tb, &rb, &why) == 0 && !rb.any(),
                   "version %d through validate_full: %s", old_version, why.c_str());
            EXPECT(validate_full(b.data(), b.size(), s, *m, *t, r_on, &back, &mb, &tb, &rb, &why) != 0 &&
                       starts(why, "binner response_pairing on"), "version %d into a handle with the binners: \"%s\"", old_version, why.c_str());
            // ---- versions 5 - 8
            std::vector<uint8_t> blob = build(s, *m, *t, r_on);
            ResponseLayout rl;
            EXPECT(response_layout(s, *m, *t, r_on, &rl) && rl.start == tl.total && rl.total == blob.size() && rl.checksum + 8 == rl.total &&
                       rl.F == rl.start + 16 + 3 * 32 && rl.bin_xs[0] == rl.F + 8 * F.size(), "the extension's layout (version %d)", version);
            EXPECT(blob[8] == version, "version field %d, expected %d", (int)blob[8], version);
            EXPECT(validate_full(blob.data(), blob.size(), s, *m, *t, r_on, &back, &mb, &tb, &rb, &why) == 0, "a valid version-%d blob was refused: %s",
                   version, why.c_str());
            EXPECT(rb.n_ch == n_ch && rb.K == K && rb.K_cc == K_cc && rb.F == nullptr && rb.bin[1].T == 2 && rb.bin[2].E == 2 * K_cc * n_q + K_cc &&
                       rb.bin[0].cap == 7 && mb.any() == m->any() && tb.any() == t->any(), "the extension does not read back (version %d)", version);
            EXPECT(validate_all(blob.data(), blob.size(), s, *m, *t, &back, &mb, &tb, &why) != 0 && starts(why, "version"),
                   "validate_all took version %d: \"%s\"", version, why.c_str());
            EXPECT(validate_any(blob.data(), blob.size(), s, *m, &back, &mb, &why) != 0 && starts(why, "version"),
                   "validate_any took version %d: \"%s\"", version, why.c_str());
            EXPECT(validate_full(blob.data(), blob.size(), s, *m, *t, r_off, &back, &mb, &tb, &rb, &why) != 0 && starts(why, "binner response_"),
                   "version %d into a handle without the binners: \"%s\"", version, why.c_str());
            // truncations and a trailing byte
            int refused = 0, total = 0;
            for (size_t n = 0; n < blob.size(); n += (n < rl.start ? 97 : 1), ++total)
                refused += validate_full(blob.data(), n, s, *m, *t, r_on, &back, &mb, &tb, &rb, &why) != 0;
            EXPECT(refused == total, "%d of %d truncations refused (version %d)", refused, total, version);
            {
                std::vector<uint8_t> longer = blob;
                longer.push_back(0);
                EXPECT(validate_full(longer.data(), longer.size(), s, *m, *t, r_on, &back, &mb, &tb, &rb, &why) != 0 && starts(why, "n_bytes"),
                       "a trailing byte: \"%s\"", why.c_str());
            }
            // every single flipped byte of the extension
            refused = total = 0;
            for (size_t i = rl.start; i < rl.total; ++i, ++total) {
                std::vector<uint8_t> bad = blob;
                bad[i] ^= 0x40;
                refused += validate_full(bad.data(), bad.size(), s, *m, *t, r_on, &back, &mb, &tb, &rb, &why) != 0;
            }
            EXPECT(refused == total, "%d of %d flipped extension bytes refused (version %d)", refused, total, version);
            // every single configuration field that differs, the reason named
            F2 = F;
            F2[7] += 1.0;
            struct Case { const char *prefix; Response r; } cases[9] = {
                {"response n_ch", r_on}, {"response K:", r_on}, {"response K_cc", r_on}, {"binner response_pairing E", r_on},
                {"binner response_pairing_susceptibility L", r_on}, {"binner response_current cap", r_on},
                {"binner response_current on", r_on}, {"response F: entry 7", r_on}, {"binner response_pairing_susceptibility on", r_on}};
            cases[0].r.n_ch = 2; cases[1].r.K = 4; cases[2].r.K_cc = 4; cases[3].r.bin[0].E += 1; cases[4].r.bin[1].L += 1;
            cases[5].r.bin[2].cap += 1; cases[6].r.bin[2].on = 0; cases[7].r.F = F2.data(); cases[8].r.bin[1].on = 0;
            for (const Case &c : cases) {
                EXPECT(validate_full(blob.data(), blob.size(), s, *m, *t, c.r, &back, &mb, &tb, &rb, &why) != 0 && starts(why, c.prefix),
                       "expected \"%s ...\", got \"%s\" (version %d)", c.prefix, why.c_str(), version);
            }
            {   // a push count beyond the capacity (state, checked as a range) with the checksum made right again
                Response r = r_on;
                r.bin[0].T = 8;
                std::vector<uint8_t> bad = build(s, *m, *t, r);
                EXPECT(validate_full(bad.data(), bad.size(), s, *m, *t, r_on, &back, &mb, &tb, &rb, &why) != 0 &&
                           starts(why, "binner response_pairing T"), "T beyond the capacity: \"%s\"", why.c_str());
            }
            {   // the current binner alone: no channels, no F
                Response r;
                r.K_cc = K_cc;
                r.bin[2] = {1, 2 * K_cc * n_q + K_cc, 3, 7, 3};
                std::vector<uint8_t> cur = build(s, *m, *t, r);
                EXPECT(validate_full(cur.data(), cur.size(), s, *m, *t, r, &back, &mb, &tb, &rb, &why) == 0 && rb.n_ch == 0 && rb.bin[2].T == 3,
                       "the current binner alone: %s", why.c_str());
            }
        }
    EXPECT(base == 4, "four base versions");
    {   // layouts that would overflow
        Response r = r_on;
        r.bin[0].E = 0x7fffffff; r.bin[0].L = 41;
        Shape big = s;
        big.n_walkers = 0x7fffffff;
        ResponseLayout rl;
        Shape huge = big;
        huge.bin[0].E = 0x7fffffff; huge.bin[0].L = 41;
        for (int k = 1; k < N_BIN; ++k) huge.bin[k] = huge.bin[0];
        (void)response_layout(huge, m_off, t_off, r, &rl, &why);  // (must not trip the sanitizers either way)
        r.K = 0x7fffffff; r.n_ch = 8;
        (void)response_layout(s, m_off, t_off, r, &rl, &why);
        r.n_ch = 9;
        EXPECT(!response_layout(s, m_off, t_off, r, &rl, &why) && starts(why, "response n_ch"), "n_ch = 9: \"%s\"", why.c_str());
        r = r_on;
        r.bin[1].L = 42;
        EXPECT(!response_layout(s, m_off, t_off, r, &rl, &why) && starts(why, "response binner"), "L = 42: \"%s\"", why.c_str());
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
