// Stand-alone check of csrc/state_blob.cpp, built with -fsanitize=address,undefined by tests/test_checkpoint_blob.py and run
// as a child process on the CPU: a valid blob of a small shape validates; every truncation of it, a buffer one byte too
// long and a few hundred single-byte corruptions of its header from a fixed seed are refused with a message; the field
// packing round-trips.  Exit status 0 and "ok" on the last line when all of that holds.
#include <cstdio>
#include <cstdlib>
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
    s.n_sites = 6; s.model_kind = 1; s.slices = 10; s.safe_mult = 5; s.n_walkers = 3; s.nb = 2;
    s.delta_tau = 0.1; s.U = 4.0;
    s.sec_n[0] = 2 * 2 * 36 + 2 * 6 + 1; s.sec_n_red[0] = s.sec_n[0];
    s.sec_n[1] = 4 * 5 + 3 * 6 + 1; s.sec_n_red[1] = s.sec_n[1];
    s.sec_n[4] = 41; s.sec_n_red[4] = 40;
    s.sec_n[5] = 5; s.sec_n_red[5] = 5;
    s.bin[0] = {1, 2 * 36 + 12, 3, 7, 5};
    s.bin[4] = {1, 2, 1, 1, 1};   // one level: no compressor
    s.bin[6] = {1, 1, 3, 7, 5};
    s.td_every = 5; s.td_what = 3; s.td_R = 3;
    s.sign_on = 1; s.gm_rate = 2; s.gm_kind = 1; s.gm_updates = 60;
    return s;
}

static uint64_t lcg(uint64_t *x) { return *x = *x * 6364136223846793005ull + 1442695040888963407ull; }

int main()
{
    const Shape s = small_shape();
    Layout l;
    std::string why;
    EXPECT(layout(s, &l, &why), "layout refused the small shape: %s", why.c_str());
    EXPECT(l.conf == header_bytes(), "the payload starts behind the header");
    EXPECT(l.total > header_bytes() && l.total < (1u << 20), "blob size %zu", l.total);
    // offsets ascend and the last part ends at total
    EXPECT(l.conf < l.rng && l.rng < l.stats && l.stats < l.gm && l.gm < l.sign_fail && l.sign_fail < l.sec[0], "fixed parts ascend");
    EXPECT(l.bin_c[6] + (size_t)(3 - 1) * 3 * 1 * 8 == l.total, "the last binner's compressor ends the blob");

    // exactly-sized heap buffers, so that a read behind the end is the sanitizer's to report
    std::vector<uint8_t> blob(l.total, 0);
    write_header(s, blob.data());
    Shape back{};
    EXPECT(validate(blob.data(), blob.size(), s, &back, &why) == 0, "a valid blob was refused: %s", why.c_str());
    EXPECT(back.n_walkers == 3 && back.bin[0].T == 5 && back.gm_updates == 60 && back.U == 4.0 && back.sec_n[4] == 41 &&
               std::memcmp(back.source_hash, s.source_hash, HASH_BYTES) == 0,
           "the header does not read back");

    // state fields may differ from the handle's, the source hash too
    Shape other = s;
    other.bin[0].T = 0; other.gm_updates = 0; other.source_hash[0] = 'x';
    EXPECT(validate(blob.data(), blob.size(), other, &back, &why) == 0, "state fields must not be compared: %s", why.c_str());

    // every truncation, each in a buffer of exactly that size
    for (size_t n = 0; n < l.total; ++n) {
        std::vector<uint8_t> cut(blob.begin(), blob.begin() + n);
        why.clear();
        const int rc = validate(cut.empty() ? (const uint8_t *)"" : cut.data(), n, s, &back, &why);
        EXPECT(rc != 0 && why.compare(0, 7, "n_bytes") == 0, "truncation to %zu bytes: rc %d, \"%s\"", n, rc, why.c_str());
    }
    {   // one trailing byte
        std::vector<uint8_t> longer(blob);
        longer.push_back(0);
        why.clear();
        EXPECT(validate(longer.data(), longer.size(), s, &back, &why) != 0 && why.compare(0, 7, "n_bytes") == 0,
               "a trailing byte: \"%s\"", why.c_str());
    }
    // single-byte corruptions of the header, fixed seed: every one is refused (the checksum covers what no field check does)
    uint64_t rng = 20240229;
    int refused = 0;
    const int n_corrupt = 400;
    for (int i = 0; i < n_corrupt; ++i) {
        std::vector<uint8_t> bad(blob);
        const size_t at = (size_t)(lcg(&rng) >> 33) % header_bytes();
        const uint8_t flip = (uint8_t)(1 + (lcg(&rng) >> 33) % 255);
        bad[at] ^= flip;
        why.clear();
        const int rc = validate(bad.data(), bad.size(), s, &back, &why);
        EXPECT(rc != 0 && !why.empty(), "corruption of byte %zu (xor %u) was accepted", at, (unsigned)flip);
        refused += rc != 0;
    }
    // corruptions with the checksum made good again: the field checks alone must stay in bounds, accept or refuse
    for (int i = 0; i < n_corrupt; ++i) {
        std::vector<uint8_t> bad(blob);
        const size_t at = 16 + (size_t)(lcg(&rng) >> 33) % (header_bytes() - 24);
        bad[at] ^= (uint8_t)(1 + (lcg(&rng) >> 33) % 255);
        // (FNV-1a 64 as in state_blob.cpp)
        uint64_t h = 0xcbf29ce484222325ull;
        for (size_t k = 0; k + 8 < header_bytes(); ++k) h = (h ^ bad[k]) * 0x100000001b3ull;
        for (int k = 0; k < 8; ++k) bad[header_bytes() - 8 + k] = (uint8_t)(h >> (8 * k));
        why.clear();
        const int rc = validate(bad.data(), bad.size(), s, &back, &why);
        EXPECT(rc == 0 || !why.empty(), "a refusal without a message at byte %zu", at);
        // a changed configuration field must be refused; the hash, a binner's T and the update count are free
        const bool free_field = (at >= 16 && at < 32) || at >= header_bytes() - 16;
        bool in_T = false;
        for (int k = 0; k < N_BIN; ++k) {
            const size_t b0 = 16 + HASH_BYTES + 24 + 16 + 2 * N_SEC * 8 + (size_t)k * 32;
            in_T = in_T || (at >= b0 + 24 && at < b0 + 32) || (at >= b0 + 12 && at < b0 + 16);
        }
        if (!free_field && !in_T) EXPECT(rc != 0, "a changed configuration byte %zu was accepted", at);
    }
    // shapes no handle can have
    {
        Shape z = s;
        z.n_walkers = 0;
        EXPECT(!layout(z, &l, &why), "n_walkers = 0");
        z = s;
        z.sec_n[0] = ~0ull;
        EXPECT(!layout(z, &l, &why), "a section of 2^64 - 1 doubles");
        z = s;
        z.bin[0].L = 64;
        EXPECT(!layout(z, &l, &why), "64 binner levels");
        z = s;
        z.bin[0].E = 0x7fffffff; z.bin[0].L = 41; z.n_walkers = 0x7fffffff; z.n_sites = 0x7fffffff; z.slices = 0x7fffffff;
        (void)layout(z, &l, &why);  // must not overflow, whatever it answers
    }
    // the field packing: bit i % 64 of chunk i / 64, padding bits zero
    for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)160}) {
        std::vector<int8_t> conf(n), out(n);
        for (size_t i = 0; i < n; ++i) conf[i] = (lcg(&rng) >> 40) & 1 ? 1 : -1;
        std::vector<uint8_t> chunks((n + 63) / 64 * 8, 0xff);
        pack_conf(conf.data(), n, chunks.data());
        unpack_conf(chunks.data(), n, out.data());
        EXPECT(conf == out, "pack / unpack of %zu sites", n);
        for (size_t i = n; i < chunks.size() * 8; ++i) EXPECT(!((chunks[i >> 3] >> (i & 7)) & 1), "padding bit %zu set", i);
        for (size_t i = 0; i < n; ++i) EXPECT((((chunks[i >> 3] >> (i & 7)) & 1) != 0) == (conf[i] == 1), "bit %zu", i);
    }
    std::printf("%d corruptions refused of %d\n", refused, n_corrupt);
    std::printf(failures ? "FAILED (%d)\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
