// Stand-alone check of the classical MC flavor's checkpoint blob (csrc/mc_blob.cpp), built with
// g++ -fsanitize=address,undefined by tests/test_mc_blob.py and run as a child process on the CPU.  An Ising and a q-state
// shape, each with every section on and with every section off: layout, write and validate round trips; every refusal of
// validate's list, in its order; a buffer cut at every record boundary and one byte short; every single flipped header
// byte, flipped payload bytes and every flipped checksum byte; each configuration field changed in turn with the field
// named; a q-state byte >= q, a non-zero padding byte or bit, T above the capacity, n_series above the capacity, replica
// labels that are no permutation; configurations no handle can have.
#include "mc_blob.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace mc_blob;

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

static bool has(const std::string &s, const char *part) { return s.find(part) != std::string::npos; }
static bool starts(const std::string &s, const char *prefix) { return s.compare(0, std::strlen(prefix), prefix) == 0; }

static void put_le(uint8_t *p, uint64_t v, int bytes)
{
    for (int i = 0; i < bytes; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

static Config ising(bool on)
{
    Config c{};
    std::strncpy(c.source_hash, "0123456789ab", HASH_BYTES);
    c.kind = KIND_ISING;
    c.n_sites = on ? 37 : 36;  // 37: five bits of the second word used, 27 padding bits
    c.z = 4;
    c.n_walkers = on ? 6 : 5;
    c.series_capacity = on ? 5 : 0;
    c.n_bonds = 2 * c.n_sites;
    c.n_k = -1;
    c.hash_neighs = 11, c.hash_bonds = 12, c.hash_betas = 13;
    if (on) {
        c.update_kind = 1, c.n_colours = 3, c.hash_colouring = 14;
        c.cluster_rate = 3;
        c.exchange_R = 3, c.exchange_rate = 2;
        c.n_k = 2, c.hash_phases = 15;
        c.bin[SEC_MAIN] = {1, 7, 4, 2, 4, 64};
        c.bin[SEC_SCALING] = {1, 7, 4, 3, 6, 64};
    }
    return c;
}

static Config qstate(bool on)
{
    Config c{};
    std::strncpy(c.source_hash, "ba9876543210", HASH_BYTES);
    c.kind = KIND_QSTATE;
    c.n_sites = 15;  // one padding byte per walker
    c.z = 4;
    c.q = on ? 6 : 3;
    c.n_walkers = on ? 6 : 2;
    c.series_capacity = on ? 4 : 0;
    c.n_bonds = 30;
    c.update_kind = 1, c.n_colours = 4;
    c.hash_neighs = 21, c.hash_bonds = 22, c.hash_energy = 23, c.hash_order = 24, c.hash_colouring = 25, c.hash_betas = 26;
    if (on) {
        c.cluster_rate = 2;
        c.exchange_R = 3, c.exchange_rate = 2;
        c.n_k = 2, c.hash_phases = 27;
        c.n_dir = 2, c.n_classes = 2, c.hash_twist = 28, c.hash_stiffness = 29;
        c.bin[SEC_MAIN] = {1, 7, 6, 3, 6, 64};
        c.bin[SEC_SCALING] = {1, 7, 3, 2, 4, 64};
        c.bin[SEC_STIFFNESS] = {1, 7, 4, 2, 4, 64};
    }
    return c;
}

// a whole blob of configuration c whose state is in range: anything in the free arrays, T = 7 in every section that is on
static std::vector<uint8_t> build(const Config &c, Layout *l)
{
    std::string why;
    EXPECT(layout(c, l, &why), "layout: %s", why.c_str());
    std::vector<uint8_t> b(l->total, 0);
    for (const Record &r : l->rec)
        for (uint64_t i = 0; i < r.count * r.elem_bytes; ++i) b[r.offset + i] = (uint8_t)((r.offset + i) * 131 + 7);
    const Record *conf = l->find(TAG_CONF), *ns = l->find(TAG_N_SERIES), *rep = l->find(TAG_X_REPLICA), *host = l->find(TAG_HOST);
    const size_t W = (size_t)c.n_walkers;
    if (c.kind == KIND_QSTATE) {
        const size_t row = (size_t)4 * ((c.n_sites + 3) / 4);
        for (size_t w = 0; w < W; ++w)
            for (size_t i = 0; i < row; ++i) b[conf->offset + w * row + i] = i < (size_t)c.n_sites ? (uint8_t)((i + w) % c.q) : 0;
    } else if (c.n_sites % 32) {
        const size_t nw = (size_t)(c.n_sites + 31) / 32;
        for (size_t w = 0; w < W; ++w) put_le(&b[conf->offset + 4 * ((nw - 1) * W + w)], (0x15u ^ (uint32_t)w) & ((1u << (c.n_sites % 32)) - 1), 4);
    }
    for (size_t w = 0; w < W; ++w) put_le(&b[ns->offset + 8 * w], (uint64_t)(c.series_capacity ? (w % (c.series_capacity + 1)) : 0), 8);
    if (rep)
        for (size_t w = 0; w < W; ++w) put_le(&b[rep->offset + 4 * w], (uint64_t)((w + w / c.exchange_R) % c.exchange_R), 4);
    for (int s = 0; s < N_SEC; ++s) put_le(&b[host->offset + 8 * s], c.bin[s].on ? 7 : 0, 8);
    put_le(&b[host->offset + 8 * N_SEC], 5, 8);
    write_header(c, *l, b.data());
    seal(*l, b.data());
    return b;
}

static void refused(const std::vector<uint8_t> &b, size_t n, const Config &handle, const char *expect, int line)
{
    std::string why;
    Layout l;
    const int rc = validate(b.data(), n, handle, &l, &why);
    if (rc != -1 || !has(why, expect)) {
        std::printf("FAIL line %d: rc %d, why \"%s\", expected \"%s\"\n", line, rc, why.c_str(), expect);
        ++failures;
    }
}
#define REFUSED(b, n, handle, expect) refused(b, n, handle, expect, __LINE__)

// a copy of `good` with `bytes` little-endian bytes of v at `at`, sealed again
static std::vector<uint8_t> patched(const std::vector<uint8_t> &good, const Layout &l, size_t at, uint64_t v, int bytes)
{
    std::vector<uint8_t> b = good;
    put_le(&b[at], v, bytes);
    seal(l, b.data());
    return b;
}

static void check_shape(const Config &c, const char *name)
{
    Layout l;
    const std::vector<uint8_t> good = build(c, &l);
    std::string why;
    Layout back;
    EXPECT(validate(good.data(), good.size(), c, &back, &why) == 0, "%s: a valid blob is refused: %s", name, why.c_str());
    EXPECT(back.total == l.total && back.header == l.header && back.rec.size() == l.rec.size(), "%s: layout came back changed", name);
    for (size_t i = 0; i < l.rec.size() && i < back.rec.size(); ++i)
        EXPECT(std::memcmp(&l.rec[i], &back.rec[i], sizeof(Record)) == 0, "%s: record %zu came back changed", name, i);
    // records: in the order of the table, 8-byte aligned, inside the blob, no overlap, no tag twice
    size_t at = l.header;
    for (size_t i = 0; i < l.rec.size(); ++i) {
        const Record &r = l.rec[i];
        EXPECT(r.offset % 8 == 0 && r.offset >= at && r.offset + r.count * r.elem_bytes <= l.checksum, "%s: record %zu misplaced", name, i);
        at = r.offset + r.count * r.elem_bytes;
        for (size_t j = 0; j < i; ++j) EXPECT(l.rec[j].tag != r.tag, "%s: tag %u twice", name, r.tag);
    }
    EXPECT(l.total == l.checksum + 8 && l.rec.back().tag == TAG_HOST, "%s: the end of the blob", name);
    // the same configuration lays out the same way twice (export and import share the function)
    Layout again;
    EXPECT(layout(c, &again) && again.total == l.total, "%s: layout is not a function of the configuration", name);

    // 1 - 4: no header, magic, version, size
    REFUSED(good, 0, c, "does not hold a header");
    REFUSED(good, 100, c, "does not hold a header");
    {
        std::vector<uint8_t> b = good;
        b[0] ^= 1;
        REFUSED(b, b.size(), c, "wrong magic");
        b = good;
        b[8] = 2;
        REFUSED(b, b.size(), c, "format version 2");
    }
    REFUSED(good, good.size() - 1, c, "the header implies");
    {
        std::vector<uint8_t> longer = good;
        longer.push_back(0);
        REFUSED(longer, longer.size(), c, "the header implies");
    }
    // cut at every record boundary, and one byte short of it
    for (const Record &r : l.rec) {
        REFUSED(good, (size_t)r.offset, c, "the header implies");
        REFUSED(good, (size_t)r.offset - 1, c, "the header implies");
    }
    REFUSED(good, l.checksum, c, "the header implies");
    // 5: one flipped byte anywhere in the header, in the payload, in the checksum
    int n_refused = 0, n_tried = 0;
    for (size_t i = 0; i < l.header; ++i, ++n_tried) {
        std::vector<uint8_t> b = good;
        b[i] ^= 0x20;
        if (validate(b.data(), b.size(), c, nullptr, &why) == -1) ++n_refused;
    }
    for (size_t i = l.header; i < l.checksum; i += 13, ++n_tried) {
        std::vector<uint8_t> b = good;
        b[i] ^= 0x01;
        REFUSED(b, b.size(), c, "checksum mismatch");
        ++n_refused;
    }
    for (size_t i = l.checksum; i < l.total; ++i, ++n_tried) {
        std::vector<uint8_t> b = good;
        b[i] ^= 0x80;
        REFUSED(b, b.size(), c, "checksum mismatch");
        ++n_refused;
    }
    EXPECT(n_refused == n_tried, "%s: %d of %d flipped bytes refused", name, n_refused, n_tried);
    {  // a flipped byte of the carried source hash is a damaged blob too; another source hash in the handle is no reason
        std::vector<uint8_t> b = good;
        b[16] ^= 1;
        REFUSED(b, b.size(), c, "checksum mismatch");
        Config other = c;
        std::strncpy(other.source_hash, "ffffffffffff", HASH_BYTES);
        EXPECT(validate(good.data(), good.size(), other, nullptr, &why) == 0, "%s: the source hash is checked: %s", name, why.c_str());
    }
    // a record table that is not the configuration's (sealed again: the checksum is right)
    {
        const size_t table = l.header - 24 * l.rec.size();
        REFUSED(patched(good, l, table + 16, l.rec[0].offset + 8, 8), good.size(), c, "record table");
        REFUSED(patched(good, l, table + 8, l.rec[0].count + 1, 8), good.size(), c, "record table");
        REFUSED(patched(good, l, table, 99, 4), good.size(), c, "record table");
    }
    // 6: each configuration field of the handle changed in turn
    size_t nf = 0;
    const Field *f = fields(&nf);
    EXPECT(nf >= 30, "%zu fields", nf);
    for (size_t i = 0; i < nf; ++i) {
        Config other = c;
        char *p = (char *)&other + f[i].offset;
        p[0] ^= 1;
        if (validate(good.data(), good.size(), other, nullptr, &why) != -1 || !starts(why, f[i].name)) {
            std::printf("FAIL %s: field \"%s\" changed, why \"%s\"\n", name, f[i].name, why.c_str());
            ++failures;
        }
        // two fields differ: the first of the header's order is named
        if (i + 1 < nf) {
            char *q = (char *)&other + f[i + 1].offset;
            q[0] ^= 1;
            EXPECT(validate(good.data(), good.size(), other, nullptr, &why) == -1 && starts(why, f[i].name), "%s: not the first field: %s", name,
                   why.c_str());
        }
    }
    // 7: the ranges of the state
    const Record *host = l.find(TAG_HOST), *ns = l.find(TAG_N_SERIES), *conf = l.find(TAG_CONF), *rep = l.find(TAG_X_REPLICA);
    for (int s = 0; s < N_SEC; ++s) {
        if (c.bin[s].on) {
            EXPECT(validate(patched(good, l, host->offset + 8 * s, (uint64_t)c.bin[s].cap, 8).data(), good.size(), c, nullptr, &why) == 0,
                   "%s: T == capacity refused", name);
            REFUSED(patched(good, l, host->offset + 8 * s, (uint64_t)c.bin[s].cap + 1, 8), good.size(), c, "outside 0..capacity");
            REFUSED(patched(good, l, host->offset + 8 * s, ~(uint64_t)0, 8), good.size(), c, "outside 0..capacity");
        } else
            REFUSED(patched(good, l, host->offset + 8 * s, 1, 8), good.size(), c, "outside 0..capacity");
    }
    REFUSED(patched(good, l, ns->offset + 8 * (c.n_walkers - 1), (uint64_t)c.series_capacity + 1, 8), good.size(), c, "n_series of walker");
    REFUSED(patched(good, l, ns->offset, ~(uint64_t)0, 8), good.size(), c, "n_series of walker");
    if (c.kind == KIND_QSTATE) {
        const size_t row = (size_t)4 * ((c.n_sites + 3) / 4);
        REFUSED(patched(good, l, conf->offset + row + 3, (uint64_t)c.q, 1), good.size(), c, "site 3 of walker 1 is not below q");
        REFUSED(patched(good, l, conf->offset + 14, 255, 1), good.size(), c, "is not below q");
        REFUSED(patched(good, l, conf->offset + row * c.n_walkers - 1, 1, 1), good.size(), c, "padding byte");
        EXPECT(validate(patched(good, l, conf->offset + 14, (uint64_t)c.q - 1, 1).data(), good.size(), c, nullptr, &why) == 0, "%s: q - 1 refused", name);
    } else if (c.n_sites % 32) {
        const size_t nw = (size_t)(c.n_sites + 31) / 32, last = conf->offset + 4 * ((nw - 1) * c.n_walkers + 2);
        REFUSED(patched(good, l, last, 0x15u | (1u << (c.n_sites % 32)), 4), good.size(), c, "padding bit behind the spins of walker 2");
        REFUSED(patched(good, l, last, 0x80000000u, 4), good.size(), c, "padding bit");
        EXPECT(validate(patched(good, l, last, (1u << (c.n_sites % 32)) - 1, 4).data(), good.size(), c, nullptr, &why) == 0, "%s: all spins up refused", name);
    }
    if (rep) {
        REFUSED(patched(good, l, rep->offset, (uint64_t)c.exchange_R, 4), good.size(), c, "no permutation");
        REFUSED(patched(good, l, rep->offset + 4 * c.exchange_R, 2, 4), good.size(), c, "ladder at walker 3 are no permutation");  // 2 twice
        REFUSED(patched(good, l, rep->offset + 4, 0xffffffffu, 4), good.size(), c, "no permutation");
    }
    std::printf("%s: %zu records, %zu bytes, %d flipped bytes refused of %d, %zu fields named\n", name, l.rec.size(), l.total, n_refused, n_tried, nf);
}

int main()
{
    check_shape(ising(true), "ising all on");
    check_shape(ising(false), "ising all off");
    check_shape(qstate(true), "qstate all on");
    check_shape(qstate(false), "qstate all off");

    // which records a configuration has
    Layout on, off;
    EXPECT(layout(ising(true), &on) && layout(ising(false), &off), "layout");
    EXPECT(on.find(TAG_X_REPLICA) && on.find(TAG_K_SUM_M4) && on.find(TAG_BIN) && on.find(TAG_BIN + 7) && on.find(TAG_CURSOR_CB) &&
               !on.find(TAG_BIN + 8) && !on.find(TAG_ST_SUM_T) && !on.find(TAG_MX) && !on.find(TAG_CURSOR_CONF),
           "ising all on: records");
    EXPECT(!off.find(TAG_X_REPLICA) && !off.find(TAG_K_SUM_M4) && !off.find(TAG_K_SUM_S) && !off.find(TAG_BIN) && off.find(TAG_CURSOR_CB),
           "ising all off: records");
    EXPECT(off.find(TAG_SERIES_A)->count == 0 && on.find(TAG_SERIES_A)->count == 30 && on.find(TAG_CONF)->count == 12, "ising counts");
    EXPECT(on.find(TAG_BIN + 3)->count == 6u * 4 * 6 && on.find(TAG_BIN + 6)->count == 7u * 3 * 6, "ising binner counts");
    EXPECT(layout(qstate(true), &on) && layout(qstate(false), &off), "layout");
    EXPECT(on.find(TAG_ST_LAST_K) && on.find(TAG_BIN + 11) && on.find(TAG_K_SUM_S) && !on.find(TAG_K_SUM_M4) && on.find(TAG_CURSOR_CONF) &&
               on.find(TAG_MY) && !on.find(TAG_M) && !on.find(TAG_CURSOR_CB) && !on.find(TAG_SERIES_B),
           "qstate all on: records");
    EXPECT(!off.find(TAG_ST_SUM_T) && !off.find(TAG_BIN) && !off.find(TAG_K_SUM_S) && !off.find(TAG_X_PROP), "qstate all off: records");
    EXPECT(on.find(TAG_CONF)->count == 16u * 6 && on.find(TAG_CONF)->elem_bytes == 1 && on.find(TAG_SERIES_A)->count == 3u * 4 * 6, "qstate counts");
    // the other engine: a q-state handle refuses an Ising blob by its first field
    {
        Layout l;
        const std::vector<uint8_t> b = build(ising(true), &l);
        REFUSED(b, b.size(), qstate(true), "engine kind: the blob has 0, the handle 1");
    }
    // a configuration no handle can have: refused by layout, and by validate when a header carries it
    struct Bad {
        const char *what;
        void (*change)(Config &);
    } bad[] = {
        {"engine kind", [](Config &c) { c.kind = 2; }},
        {"n_sites", [](Config &c) { c.n_sites = 0; }},
        {"n_sites", [](Config &c) { c.n_sites = 16385; }},
        {"z", [](Config &c) { c.z = 9; }},
        {"q", [](Config &c) { c.q = 65; }},
        {"n_walkers", [](Config &c) { c.n_walkers = 0; }},
        {"n_walkers", [](Config &c) { c.n_walkers = -3; }},
        {"series_capacity", [](Config &c) { c.series_capacity = -1; }},
        {"n_colours", [](Config &c) { c.n_colours = 17; }},
        {"exchange n_replicas", [](Config &c) { c.exchange_R = 4; }},  // 6 walkers
        {"exchange n_replicas", [](Config &c) { c.exchange_R = 1; }},
        {"n_k", [](Config &c) { c.n_k = 9; }},
        {"n_k", [](Config &c) { c.n_k = -1; }},  // (the q-state engine: 0 = off)
        {"stiffness", [](Config &c) { c.n_dir = 5; }},
        {"binner L", [](Config &c) { c.bin[0].L = 0; }},
        {"binner L", [](Config &c) { c.bin[1].cap = 0; }},
        {"binner n_elem", [](Config &c) { c.bin[2].n_elem = 65; }},
        {"binner on", [](Config &c) { c.bin[2].on = 2; }},
    };
    for (const Bad &t : bad) {
        Config c = qstate(true);
        t.change(c);
        Layout l;
        std::string why;
        EXPECT(!layout(c, &l, &why) && has(why, t.what), "layout accepts a bad %s (%s)", t.what, why.c_str());
        // the header of a good blob rewritten with the bad configuration (its table kept), sealed again
        Layout gl;
        const Config g = qstate(true);
        std::vector<uint8_t> b = build(g, &gl);
        write_header(c, gl, b.data());
        seal(gl, b.data());
        REFUSED(b, b.size(), g, "the header describes no handle");
    }
    {
        Config c = ising(true);
        c.n_dir = 1;
        Layout l;
        std::string why;
        EXPECT(!layout(c, &l, &why) && has(why, "stiffness on the Ising engine"), "layout: %s", why.c_str());
        c = ising(true);
        c.q = 3;
        EXPECT(!layout(c, &l, &why) && has(why, "q"), "layout: %s", why.c_str());
    }
    EXPECT(hash_pair(1, 2) != hash_pair(2, 1) && hash_pair(1, 2) == hash_pair(1, 2), "hash_pair");
    {
        const uint8_t w[16] = {1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0};
        EXPECT(hash_pair(1, 2) == dqmc_blob::fnv1a64(w, 16), "hash_pair is FNV-1a 64 of the two little-endian words");
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
