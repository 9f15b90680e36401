// Stand-alone check of format versions 3 and 4 of the checkpoint blob (csrc/state_blob.cpp: the extension for the
// thermodynamics section), built with -fsanitize=address,undefined by tests/test_thermo_reference.py and run as a child
// process on the CPU.  With the section off the version-1 / version-2 bytes are written unchanged; a version-3 and a
// version-4 blob round-trip; every truncation, a trailing byte, flipped extension bytes (a wrong checksum), another
// hopping matrix, another U_s and a binner shape that differs are refused with the reason named, and so are a version
// 3 / 4 blob by a handle without the section and a version 1 / 2 blob by a handle with it.  validate_all takes const
// buffers and writes nothing but its outputs.  Exit status 0 and "ok" on the last line when all of that holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "state_blob.h"

using namespace dqmc_blob;

static int failures = 0;
#define EXPECT(cond, ...)                \
    do {                                 \
        if (!(cond)) {                   \
            ++failures;                  \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");           \
        }                                \
    } while (0)

static Shape small_shape()
{
    Shape s{};
    std::strncpy(s.source_hash, "0123456789ab", HASH_BYTES);
    s.n_sites = 9; s.model_kind = 1; s.slices = 10; s.safe_mult = 5; s.n_walkers = 3; s.nb = 2;
    s.delta_tau = 0.1; s.U = 4.0;
    s.sec_n[0] = 2 * 2 * 81 + 2 * 9 + 1; s.sec_n_red[0] = s.sec_n[0];
    s.sec_n[5] = 5;
    s.bin[0] = {1, 2 * 81 + 18, 2, 3, 2};
    s.gm_rate = 2; s.gm_kind = 1; s.gm_updates = 60;
    return s;
}

static uint64_t lcg(uint64_t *x) { return *x = *x * 6364136223846793005ull + 1442695040888963407ull; }
static bool starts(const std::string &s, const char *prefix) { return s.compare(0, std::strlen(prefix), prefix) == 0; }

static std::vector<uint8_t> make_blob(const Shape &s, const Momenta &m, const Thermo &t, ExtLayout *e, ThermoLayout *tl)
{
    std::string why;
    EXPECT(ext_layout(s, m, e, &why) && thermo_layout(s, m, t, tl, &why), "layouts: %s", why.c_str());
    std::vector<uint8_t> blob(tl->total, 0);
    uint64_t rng = 20260101;
    for (size_t i = header_bytes(); i < blob.size(); ++i) blob[i] = (uint8_t)(lcg(&rng) >> 40);  // payload and arrays: anything
    write_header(s, m, t, blob.data());
    write_ext(m, *e, blob.data());
    seal_ext(*e, blob.data());
    write_thermo(t, *tl, blob.data());
    seal_thermo(*tl, blob.data());
    return blob;
}

int main()
{
    const Shape s = small_shape();
    const int n_dirs = 9, n_q = 4;
    std::vector<double> ct((size_t)n_dirs * n_q), st(ct.size());
    for (size_t i = 0; i < ct.size(); ++i) { ct[i] = 1.0 / (double)(i + 1); st[i] = -0.5 * (double)i; }
    Momenta m_on, m_off;
    m_on.n_q = n_q; m_on.n_dirs = n_dirs; m_on.cos_tab = ct.data(); m_on.sin_tab = st.data();
    m_on.bin[0] = {1, 4 * n_q, 3, 7, 5};
    const double hop[4] = {0.0, -1.0, -1.0, -0.4};
    Thermo t_on, t_off;
    t_on.n = 12; t_on.n_red = 12; t_on.bin = {1, 11, 3, 7, 5};
    t_on.T_hash = fnv1a64(hop, sizeof(hop)); t_on.U_s = 4.0;
    EXPECT(fnv1a64(hop, sizeof(hop)) != fnv1a64(hop, sizeof(hop) - 8) && fnv1a64(hop, 0) == 0xcbf29ce484222325ull, "fnv1a64");
    std::string why;

    // ---- the section off: versions 1 and 2 byte for byte, through the new entry points too
    for (const Momenta *m : {&m_off, &m_on}) {
        ExtLayout e, e2;
        ThermoLayout tl;
        EXPECT(ext_layout(s, *m, &e, &why), "ext_layout: %s", why.c_str());
        std::vector<uint8_t> a(e.total, 0);
        write_header(s, *m, a.data());
        write_ext(*m, e, a.data());
        seal_ext(e, a.data());
        EXPECT(thermo_layout(s, *m, t_off, &tl, &why) && tl.start == e.total && tl.total == e.total, "no extension with the section off");
        std::vector<uint8_t> b(tl.total, 0);
        EXPECT(ext_layout(s, *m, &e2, &why), "ext_layout");
        write_header(s, *m, t_off, b.data());
        write_ext(*m, e2, b.data());
        seal_ext(e2, b.data());
        write_thermo(t_off, tl, b.data());
        seal_thermo(tl, b.data());
        EXPECT(a == b, "the section off does not write the version-%d bytes", m->any() ? 2 : 1);
        EXPECT(a[8] == (m->any() ? 2 : 1), "version field %d", (int)a[8]);
        Shape back{};
        Momenta mb;
        Thermo tb;
        EXPECT(validate_all(b.data(), b.size(), s, *m, t_off, &back, &mb, &tb, &why) == 0 && !tb.any() && mb.any() == m->any(),
               "version 1 / 2 through validate_all: %s", why.c_str());
        EXPECT(validate_any(b.data(), b.size(), s, *m, &back, &mb, &why) == 0, "version 1 / 2 through validate_any: %s", why.c_str());
        why.clear();
        EXPECT(validate_all(b.data(), b.size(), s, *m, t_on, &back, &mb, &tb, &why) != 0 && starts(why, "section thermodynamics n"),
               "version 1 / 2 into a handle with the section: \"%s\"", why.c_str());
    }

    // ---- versions 3 (no momentum binner) and 4 (with one)
    for (const Momenta *m : {&m_off, &m_on}) {
        const int version = m->any() ? 4 : 3;
        ExtLayout e;
        ThermoLayout tl;
        const std::vector<uint8_t> blob = make_blob(s, *m, t_on, &e, &tl);
        const size_t W = 3;
        EXPECT(blob[8] == version, "version field %d, expected %d", (int)blob[8], version);
        EXPECT(tl.start == e.total && tl.sec == tl.start + 64 && tl.bin_xs == tl.sec + 12 * 8 && tl.bin_x2 == tl.bin_xs + 3 * W * 11 * 8 &&
                   tl.bin_c == tl.bin_x2 + 3 * W * 11 * 8 && tl.checksum == tl.bin_c + 2 * W * 11 * 8 && tl.total == tl.checksum + 8,
               "the extension's layout (version %d)", version);
        {   // the version-1 / 2 part is the old blob but for the version field and the header checksum
            std::vector<uint8_t> old(e.total, 0);
            std::memcpy(old.data(), blob.data(), e.total);
            write_header(s, *m, old.data());
            Shape back{};
            Momenta mb;
            EXPECT(validate_any(old.data(), old.size(), s, *m, &back, &mb, &why) == 0, "the front part is no version-%d blob: %s",
                   version - 2, why.c_str());
        }
        Shape back{};
        Momenta mb;
        Thermo tb;
        EXPECT(validate_all(blob.data(), blob.size(), s, *m, t_on, &back, &mb, &tb, &why) == 0, "a valid version-%d blob was refused: %s",
               version, why.c_str());
        EXPECT(back.n_walkers == 3 && back.bin[0].T == 2 && mb.any() == m->any() && tb.n == 12 && tb.n_red == 12 && tb.bin.on == 1 &&
                   tb.bin.E == 11 && tb.bin.L == 3 && tb.bin.cap == 7 && tb.bin.T == 5 && tb.T_hash == t_on.T_hash && tb.U_s == 4.0,
               "the extension does not read back (version %d)", version);
        // the older reader does not take it
        why.clear();
        EXPECT(validate_any(blob.data(), blob.size(), s, *m, &back, &mb, &why) != 0 && starts(why, "version"), "validate_any took version %d: \"%s\"",
               version, why.c_str());
        // a handle without the section refuses it and names the field
        why.clear();
        EXPECT(validate_all(blob.data(), blob.size(), s, *m, t_off, &back, &mb, &tb, &why) != 0 && starts(why, "section thermodynamics n"),
               "version %d into a handle without the section: \"%s\"", version, why.c_str());
        // every truncation and a trailing byte; the outputs stay untouched
        int refused = 0, total = 0;
        for (size_t cut = 0; cut < blob.size(); cut += (cut < tl.start ? 97 : 1)) {
            std::vector<uint8_t> part(blob.begin(), blob.begin() + cut);  // (its own allocation: a read past `cut` is an ASan report)
            Thermo keep;
            keep.n = 77;
            ++total;
            if (validate_all(part.data(), part.size(), s, *m, t_on, &back, &mb, &keep, &why) != 0 && keep.n == 77) ++refused;
        }
        EXPECT(refused == total, "%d of %d truncations refused (version %d)", refused, total, version);
        {
            std::vector<uint8_t> longer(blob);
            longer.push_back(0);
            why.clear();
            EXPECT(validate_all(longer.data(), longer.size(), s, *m, t_on, &back, &mb, &tb, &why) != 0 && starts(why, "n_bytes"),
                   "a trailing byte: \"%s\"", why.c_str());
        }
        // a wrong checksum: any flipped byte of the extension, its arrays included
        refused = total = 0;
        uint64_t rng = 7;
        for (int k = 0; k < 200; ++k) {
            std::vector<uint8_t> bad(blob);
            const size_t at = tl.start + (size_t)(lcg(&rng) >> 33) % (tl.total - tl.start);
            bad[at] ^= (uint8_t)(1u << ((lcg(&rng) >> 40) & 7));
            ++total;
            if (validate_all(bad.data(), bad.size(), s, *m, t_on, &back, &mb, &tb, &why) != 0) ++refused;
        }
        EXPECT(refused == total, "%d of %d flipped extension bytes refused (version %d)", refused, total, version);
        {
            std::vector<uint8_t> bad(blob);
            bad[tl.sec + 3] ^= 0x10;  // (inside the section's sums: only the checksum can notice)
            why.clear();
            EXPECT(validate_all(bad.data(), bad.size(), s, *m, t_on, &back, &mb, &tb, &why) != 0 && starts(why, "thermodynamics extension checksum"),
                   "a damaged sum: \"%s\"", why.c_str());
        }
        // configuration that differs, each named
        struct Case { const char *prefix; Thermo t; } cases[5] = {{"thermodynamics hopping matrix", t_on}, {"thermodynamics U_s", t_on},
                                                                 {"binner thermodynamics E", t_on}, {"binner thermodynamics cap", t_on},
                                                                 {"binner thermodynamics on", t_on}};
        cases[0].t.T_hash ^= 1;
        cases[1].t.U_s = -4.0;
        cases[2].t.bin.E = 10;
        cases[3].t.bin.cap = 8;
        cases[4].t.bin = Shape::Bin{};
        for (const Case &c : cases) {
            why.clear();
            EXPECT(validate_all(blob.data(), blob.size(), s, *m, c.t, &back, &mb, &tb, &why) != 0 && starts(why, c.prefix),
                   "expected \"%s ...\", got \"%s\" (version %d)", c.prefix, why.c_str(), version);
        }
        {   // the state field's range
            Thermo over = t_on;
            over.bin.T = 8;
            ExtLayout e2;
            ThermoLayout tl2;
            const std::vector<uint8_t> bad = make_blob(s, *m, over, &e2, &tl2);
            why.clear();
            EXPECT(validate_all(bad.data(), bad.size(), s, *m, t_on, &back, &mb, &tb, &why) != 0 && starts(why, "binner thermodynamics T"),
                   "T above the capacity: \"%s\"", why.c_str());
        }
        {   // the binner off: the section alone
            Thermo nobin = t_on;
            nobin.bin = Shape::Bin{};
            ExtLayout e2;
            ThermoLayout tl2;
            const std::vector<uint8_t> b2 = make_blob(s, *m, nobin, &e2, &tl2);
            EXPECT(tl2.total == tl2.start + 64 + 12 * 8 + 8, "layout without the binner");
            EXPECT(validate_all(b2.data(), b2.size(), s, *m, nobin, &back, &mb, &tb, &why) == 0 && tb.bin.on == 0, "without the binner: %s", why.c_str());
        }
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
