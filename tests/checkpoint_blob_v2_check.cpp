// Stand-alone check of format version 2 of the checkpoint blob (csrc/state_blob.cpp: the extension for the momentum
// binners), built with -fsanitize=address,undefined by tests/test_momentum_host.py and run as a child process on the CPU.
// A shape without momentum binners writes exactly the version-1 bytes; a version-2 blob round-trips; every truncation, a
// trailing byte, flipped extension bytes, another n_q, a table entry that differs and a binner shape that differs are
// refused with the reason named.  validate_any takes const buffers and writes nothing but its outputs, so "refused
// before any write" is a property of its signature; the outputs are checked to stay untouched on a refusal.
// Exit status 0 and "ok" on the last line when all of that holds.
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
    s.sec_n[1] = 4 * 9 + 3 * 9 + 1; s.sec_n_red[1] = s.sec_n[1];
    s.sec_n[5] = 5;
    s.bin[1] = {1, 4 * 9 + 27, 3, 7, 5};
    s.td_every = 5; s.td_what = 3; s.td_R = 3;
    s.gm_rate = 2; s.gm_kind = 1; s.gm_updates = 60;
    return s;
}

static uint64_t lcg(uint64_t *x) { return *x = *x * 6364136223846793005ull + 1442695040888963407ull; }
static bool starts(const std::string &s, const char *prefix) { return s.compare(0, std::strlen(prefix), prefix) == 0; }

int main()
{
    const Shape s = small_shape();
    const int n_dirs = 9, n_q = 4;
    std::vector<double> ct((size_t)n_dirs * n_q), st(ct.size());
    for (size_t i = 0; i < ct.size(); ++i) { ct[i] = 1.0 / (double)(i + 1); st[i] = -0.5 * (double)i; }
    Momenta m;
    m.n_q = n_q; m.n_dirs = n_dirs; m.cos_tab = ct.data(); m.sin_tab = st.data();
    m.bin[0] = {1, 4 * n_q, 3, 7, 5};
    m.bin[2] = {1, (4 * 2 + 4) * 3 * n_q, 1, 1, 1};  // one level: no compressor
    std::string why;

    // ---- no momentum binner: the version-1 bytes, momenta set or not
    {
        Momenta off = m;
        off.bin[0] = off.bin[2] = Shape::Bin{};
        Layout l;
        ExtLayout e;
        EXPECT(layout(s, &l, &why) && ext_layout(s, off, &e, &why), "layouts: %s", why.c_str());
        EXPECT(e.total == l.total && e.start == l.total, "no extension without a momentum binner");
        std::vector<uint8_t> a(l.total, 0), b(e.total, 0);
        write_header(s, a.data());
        write_header(s, off, b.data());
        write_ext(off, e, b.data());
        seal_ext(e, b.data());
        EXPECT(a == b, "a shape without momentum binners does not write the version-1 bytes");
        Shape back{};
        Momenta mb;
        EXPECT(validate_any(b.data(), b.size(), s, off, &back, &mb, &why) == 0 && !mb.any(), "version 1 through validate_any: %s", why.c_str());
        EXPECT(validate(b.data(), b.size(), s, &back, &why) == 0, "version 1 through validate: %s", why.c_str());
        // a handle with a momentum binner on refuses the version-1 blob and names the binner
        why.clear();
        EXPECT(validate_any(b.data(), b.size(), s, m, &back, &mb, &why) != 0 && starts(why, "binner momentum_correlations on"),
               "version 1 into a handle with momentum binners: \"%s\"", why.c_str());
    }

    // ---- version 2
    Layout l;
    ExtLayout e;
    EXPECT(layout(s, &l, &why) && ext_layout(s, m, &e, &why), "layouts: %s", why.c_str());
    const size_t W = 3, tab = (size_t)n_dirs * n_q * 8;
    EXPECT(e.start == l.total && e.cos_tab == e.start + 8 + 3 * 32 && e.sin_tab == e.cos_tab + tab &&
               e.bin_xs[0] == e.sin_tab + tab, "the extension's fixed part");
    EXPECT(e.bin_x2[0] == e.bin_xs[0] + 3 * W * 16 * 8 && e.bin_c[0] == e.bin_x2[0] + 3 * W * 16 * 8 &&
               e.bin_xs[2] == e.bin_c[0] + 2 * W * 16 * 8, "the first momentum binner's arrays");
    EXPECT(e.checksum == e.bin_x2[2] + W * 144 * 8 && e.total == e.checksum + 8, "the last binner has no compressor; the checksum ends the blob");
    std::vector<uint8_t> blob(e.total, 0);
    uint64_t rng = 20250101;
    for (size_t i = header_bytes(); i < blob.size(); ++i) blob[i] = (uint8_t)(lcg(&rng) >> 40);  // payload and binner arrays: anything
    write_header(s, m, blob.data());
    write_ext(m, e, blob.data());
    seal_ext(e, blob.data());
    Shape back{};
    Momenta mb;
    EXPECT(validate_any(blob.data(), blob.size(), s, m, &back, &mb, &why) == 0, "a valid version-2 blob was refused: %s", why.c_str());
    EXPECT(back.n_walkers == 3 && back.bin[1].T == 5 && mb.n_q == n_q && mb.n_dirs == n_dirs && mb.bin[0].on == 1 && mb.bin[0].E == 16 &&
               mb.bin[0].T == 5 && mb.bin[1].on == 0 && mb.bin[2].E == 144 && mb.bin[2].T == 1 && mb.bin[2].cap == 1,
           "the extension does not read back");
    {   // the tables come back bit for bit
        bool same = true;
        for (size_t i = 0; i < ct.size(); ++i) {
            double c, sn;
            std::memcpy(&c, blob.data() + e.cos_tab + 8 * i, 8);
            std::memcpy(&sn, blob.data() + e.sin_tab + 8 * i, 8);
            same = same && c == ct[i] && sn == st[i];
        }
        EXPECT(same, "the tables do not round-trip");
    }
    // the version-1 reader refuses it by its version
    why.clear();
    EXPECT(validate(blob.data(), blob.size(), s, &back, &why) != 0 && starts(why, "version"), "validate on version 2: \"%s\"", why.c_str());
    // T is state: it may differ from the handle's
    {
        Momenta other = m;
        other.bin[0].T = 0;
        EXPECT(validate_any(blob.data(), blob.size(), s, other, &back, &mb, &why) == 0 && mb.bin[0].T == 5, "T must not be compared: %s", why.c_str());
    }

    // outputs stay untouched on a refusal
    Shape untouched_s{};
    untouched_s.n_sites = -77;
    Momenta untouched_m;
    untouched_m.n_q = -77;
#define REFUSED(buf, n, hm, prefix, what)                                                                             \
    do {                                                                                                              \
        why.clear();                                                                                                  \
        const int rc_ = validate_any((buf), (n), s, (hm), &untouched_s, &untouched_m, &why);                          \
        EXPECT(rc_ != 0 && starts(why, prefix), "%s: rc %d, \"%s\"", what, rc_, why.c_str());                         \
        EXPECT(untouched_s.n_sites == -77 && untouched_m.n_q == -77, "%s: an output was written", what);              \
    } while (0)

    // every truncation, each in a buffer of exactly that size, and a trailing byte
    for (size_t n = 0; n < e.total; ++n) {
        std::vector<uint8_t> cut(blob.begin(), blob.begin() + n);
        char what[64];
        std::snprintf(what, sizeof(what), "truncation to %zu bytes", n);
        REFUSED(cut.empty() ? (const uint8_t *)"" : cut.data(), n, m, "n_bytes", what);
    }
    {
        std::vector<uint8_t> longer(blob);
        longer.push_back(0);
        REFUSED(longer.data(), longer.size(), m, "n_bytes", "a trailing byte");
    }
    // flipped extension bytes, fixed seed: anywhere in the extension, binner arrays and checksum included
    for (int i = 0; i < 400; ++i) {
        std::vector<uint8_t> bad(blob);
        const size_t at = e.start + (size_t)(lcg(&rng) >> 33) % (e.total - e.start);
        bad[at] ^= (uint8_t)(1 + (lcg(&rng) >> 33) % 255);
        why.clear();
        const int rc = validate_any(bad.data(), bad.size(), s, m, &untouched_s, &untouched_m, &why);
        EXPECT(rc != 0 && !why.empty(), "a flipped extension byte %zu was accepted", at);
        EXPECT(untouched_s.n_sites == -77 && untouched_m.n_q == -77, "flipped byte %zu: an output was written", at);
    }
    {   // one in a table, named by the checksum
        std::vector<uint8_t> bad(blob);
        bad[e.cos_tab + 3] ^= 0x10;
        REFUSED(bad.data(), bad.size(), m, "extension checksum", "a flipped table byte");
    }
    // the handle has another n_q (with tables to match)
    {
        std::vector<double> c2((size_t)n_dirs * 5, 0.25), s2(c2.size(), 0.5);
        Momenta other = m;
        other.n_q = 5; other.cos_tab = c2.data(); other.sin_tab = s2.data();
        other.bin[0].E = 4 * 5; other.bin[2].E = 12 * 3 * 5;
        REFUSED(blob.data(), blob.size(), other, "momenta n_q", "another n_q");
    }
    // a table entry of the handle differs in its last bit
    {
        std::vector<double> c2(ct), s2(st);
        uint64_t u;
        std::memcpy(&u, &c2[7], 8);
        u ^= 1;
        std::memcpy(&c2[7], &u, 8);
        Momenta other = m;
        other.cos_tab = c2.data();
        REFUSED(blob.data(), blob.size(), other, "momenta cos_tab", "a cosine entry that differs");
        std::memcpy(&u, &s2[35], 8);
        u ^= 1ull << 63;
        std::memcpy(&s2[35], &u, 8);
        other = m;
        other.sin_tab = s2.data();
        REFUSED(blob.data(), blob.size(), other, "momenta sin_tab", "a sine entry that differs");
    }
    // binner shapes that differ
    {
        Momenta other = m;
        other.bin[0].E = 17;  // (sign weighting on the importing side)
        REFUSED(blob.data(), blob.size(), other, "binner momentum_correlations E", "another E");
        other = m;
        other.bin[0].cap = 8; other.bin[0].L = 4;
        REFUSED(blob.data(), blob.size(), other, "binner momentum_correlations L", "another L");
        other = m;
        other.bin[1] = {1, 16, 3, 7, 0};
        REFUSED(blob.data(), blob.size(), other, "binner momentum_susceptibilities on", "a binner the blob does not have");
        other = m;
        other.bin[2] = Shape::Bin{};
        REFUSED(blob.data(), blob.size(), other, "binner momentum_time_displaced on", "a binner the handle does not have");
    }
    // the version-1 part is still checked first
    {
        Shape hs = s;
        hs.n_walkers = 4;
        why.clear();
        EXPECT(validate_any(blob.data(), blob.size(), hs, m, &untouched_s, &untouched_m, &why) != 0 && starts(why, "n_walkers"),
               "another n_walkers: \"%s\"", why.c_str());
    }
    // shapes no handle can have
    {
        Momenta z = m;
        z.n_q = 10;
        EXPECT(!ext_layout(s, z, &e, &why), "n_q > n_dirs");
        z = m;
        z.bin[0].L = 64;
        EXPECT(!ext_layout(s, z, &e, &why), "64 levels");
        z = m;
        z.n_q = z.n_dirs = 0x7fffffff; z.bin[0].E = 0x7fffffff; z.bin[0].L = 41;
        (void)ext_layout(s, z, &e, &why);  // must not overflow, whatever it answers
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
