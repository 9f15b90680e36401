// mc_blob.cpp — see mc_blob.h.  No HIP here.
#include "mc_blob.h"

#include <cstring>

namespace mc_blob {

namespace {

void put32(uint8_t *p, uint32_t v)
{
    for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
void put64(uint8_t *p, uint64_t v)
{
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
uint32_t get32(const uint8_t *p)
{
    uint32_t v = 0;
    for (int i = 0; i < 4; ++i) v |= (uint32_t)p[i] << (8 * i);
    return v;
}
uint64_t get64(const uint8_t *p)
{
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

#define MC_F4(name, member) {name, offsetof(Config, member), 4}
#define MC_F8(name, member) {name, offsetof(Config, member), 8}
#define MC_BIN(sec, label)                                                                                     \
    MC_F4("binner " label " on", bin[sec].on), MC_F8("binner " label " capacity", bin[sec].cap),               \
        MC_F4("binner " label " L", bin[sec].L), MC_F4("binner " label " n_elem", bin[sec].n_elem),             \
        MC_F4("binner " label " n_pairs", bin[sec].n_pairs), MC_F4("binner " label " n_comp", bin[sec].n_comp)
const Field FIELDS[] = {
    MC_F4("engine kind", kind),
    MC_F4("n_sites", n_sites),
    MC_F4("z", z),
    MC_F4("q", q),
    MC_F4("n_walkers", n_walkers),
    MC_F4("series_capacity", series_capacity),
    MC_F4("n_bonds", n_bonds),
    MC_F4("update kind", update_kind),
    MC_F4("n_colours", n_colours),
    MC_F4("cluster rate", cluster_rate),
    MC_F4("exchange n_replicas", exchange_R),
    MC_F4("exchange rate", exchange_rate),
    MC_F4("n_k", n_k),
    MC_F4("stiffness n_dir", n_dir),
    MC_F4("stiffness n_classes", n_classes),
    MC_BIN(SEC_MAIN, "main"),
    MC_BIN(SEC_SCALING, "scaling"),
    MC_BIN(SEC_STIFFNESS, "stiffness"),
    MC_F8("neighbour table", hash_neighs),
    MC_F8("bonds table", hash_bonds),
    MC_F8("pair-energy table", hash_energy),
    MC_F8("order-parameter tables", hash_order),
    MC_F8("twist tables", hash_twist),
    MC_F8("colouring", hash_colouring),
    MC_F8("betas", hash_betas),
    MC_F8("k-vector phase tables", hash_phases),
    MC_F8("stiffness classes and projections", hash_stiffness),
};
#undef MC_BIN
#undef MC_F8
#undef MC_F4
const size_t N_FIELDS = sizeof(FIELDS) / sizeof(FIELDS[0]);

size_t fields_bytes()
{
    size_t n = 0;
    for (size_t i = 0; i < N_FIELDS; ++i) n += (size_t)FIELDS[i].bytes;
    return n;
}

uint64_t field_get(const Config &c, const Field &f)
{
    const char *p = (const char *)&c + f.offset;
    if (f.bytes == 4) {
        uint32_t v;
        std::memcpy(&v, p, 4);
        return v;
    }
    uint64_t v;
    std::memcpy(&v, p, 8);
    return v;
}

void field_set(Config &c, const Field &f, uint64_t v)
{
    char *p = (char *)&c + f.offset;
    if (f.bytes == 4) {
        const uint32_t w = (uint32_t)v;
        std::memcpy(p, &w, 4);
    } else
        std::memcpy(p, &v, 8);
}

const size_t OFF_MAGIC = 0, OFF_VERSION = 8, OFF_HEADER_BYTES = 12, OFF_HASH = 16, OFF_FIELDS = OFF_HASH + HASH_BYTES;
const size_t RECORD_BYTES = 24;
size_t fixed_bytes() { return OFF_FIELDS + fields_bytes() + 8; }  // .. u32 records, u32 0

size_t align8(size_t n) { return (n + 7) & ~(size_t)7; }

}  // namespace

const Field *fields(size_t *n)
{
    *n = N_FIELDS;
    return FIELDS;
}

uint64_t hash_pair(uint64_t a, uint64_t b)
{
    uint8_t w[16];
    put64(w, a);
    put64(w + 8, b);
    return dqmc_blob::fnv1a64(w, 16);
}

bool layout(const Config &c, Layout *out, std::string *why)
{
    auto bad = [&](const char *what) {
        if (why) *why = std::string("the header describes no handle: ") + what;
        return false;
    };
    const bool ising = c.kind == KIND_ISING;
    if (c.kind != KIND_ISING && c.kind != KIND_QSTATE) return bad("engine kind");
    if (c.n_sites < 1 || c.n_sites > 16384) return bad("n_sites");
    if (c.z < 1 || c.z > 8) return bad("z");
    if (ising ? c.q != 0 : (c.q < 2 || c.q > 64)) return bad("q");
    if (c.n_walkers < 1 || c.n_walkers > (1 << 24)) return bad("n_walkers");
    if (c.series_capacity < 0) return bad("series_capacity");
    if (c.n_bonds < 0) return bad("n_bonds");
    if (c.n_colours < 0 || c.n_colours > 16) return bad("n_colours");
    if (c.cluster_rate < 0 || c.exchange_rate < 0) return bad("a rate");
    if (c.exchange_R < 0 || c.exchange_R == 1 || (c.exchange_R && c.n_walkers % c.exchange_R != 0)) return bad("exchange n_replicas");
    if (c.n_k < (ising ? -1 : 0) || c.n_k > MAX_K) return bad("n_k");
    if (c.n_dir < 0 || c.n_dir > ST_DIRS || c.n_classes < 0 || c.n_classes > ST_CLASSES) return bad("stiffness n_dir, n_classes");
    if (ising && (c.n_dir || c.n_classes || c.bin[SEC_STIFFNESS].on)) return bad("stiffness on the Ising engine");
    for (int s = 0; s < N_SEC; ++s) {
        const Config::Bin &b = c.bin[s];
        if (b.on != 0 && b.on != 1) return bad("binner on");
        if (!b.on) continue;
        if (b.L < 1 || b.L > 64 || b.cap < 1 || b.cap > ((int64_t)1 << 40)) return bad("binner L, capacity");
        if (b.n_elem < 1 || b.n_elem > 64 || b.n_pairs < 0 || b.n_pairs > 64 || b.n_comp < 0 || b.n_comp > 64)
            return bad("binner n_elem, n_pairs, n_comp");
    }
    Layout l;
    const uint64_t W = (uint64_t)c.n_walkers, cap = (uint64_t)c.series_capacity;
    auto add = [&](uint32_t tag, uint32_t bytes, uint64_t count) { l.rec.push_back(Record{tag, bytes, count, 0}); };
    if (ising) add(TAG_CONF, 4, (uint64_t)((c.n_sites + 31) / 32) * W);
    else add(TAG_CONF, 1, (uint64_t)4 * ((c.n_sites + 3) / 4) * W);
    add(TAG_KEY, 8, W);
    add(TAG_CURSOR_SWEEP, 8, W);
    if (!ising) add(TAG_CURSOR_CONF, 8, W);
    add(TAG_CURSOR_CLUSTER, 8, W);
    if (ising) add(TAG_CURSOR_CB, 8, W);
    if (ising) {
        add(TAG_E, 4, W);
        add(TAG_M, 4, W);
    } else {
        add(TAG_E, 8, W);
        add(TAG_MX, 8, W);
        add(TAG_MY, 8, W);
    }
    for (uint32_t t : {TAG_SUM_E, TAG_SUM_E2, TAG_SUM_M, TAG_SUM_M2}) add(t, 8, W);
    if (!ising) add(TAG_SUM_M4, 8, W);
    for (uint32_t t : {TAG_N_MEAS, TAG_PROP, TAG_ACC, TAG_N_SERIES}) add(t, 8, W);
    if (ising) {
        add(TAG_SERIES_A, 4, cap * W);
        add(TAG_SERIES_B, 4, cap * W);
    } else
        add(TAG_SERIES_A, 8, 3 * cap * W);
    for (uint32_t t : {TAG_G_PROP, TAG_G_ACC, TAG_G_SUM}) add(t, 8, W);
    if (c.exchange_R >= 2) {
        add(TAG_X_REPLICA, 4, W);
        add(TAG_X_PROP, 8, W);
        add(TAG_X_ACC, 8, W);
    }
    if (ising ? c.n_k >= 0 : c.n_k > 0) {
        if (ising) add(TAG_K_SUM_M4, 8, W);
        add(TAG_K_SUM_S, 8, (uint64_t)MAX_K * W);
        add(TAG_K_N_MEAS, 8, W);
    }
    if (c.n_dir > 0) {
        for (uint32_t t : {TAG_ST_SUM_T, TAG_ST_SUM_J, TAG_ST_SUM_J2}) add(t, 8, (uint64_t)ST_DIRS * W);
        add(TAG_ST_N_MEAS, 8, W);
        add(TAG_ST_LAST_I, 8, (uint64_t)ST_CLASSES * W);
        add(TAG_ST_LAST_K, 8, (uint64_t)ST_CLASSES * W);
    }
    for (int s = 0; s < N_SEC; ++s) {
        const Config::Bin &b = c.bin[s];
        if (!b.on) continue;
        const uint64_t L = (uint64_t)b.L;
        add(TAG_BIN + 4 * s + 0, 8, L * (uint64_t)b.n_elem * W);
        add(TAG_BIN + 4 * s + 1, 8, L * (uint64_t)b.n_elem * W);
        add(TAG_BIN + 4 * s + 2, 8, L * (uint64_t)b.n_pairs * W);
        add(TAG_BIN + 4 * s + 3, 8, (L - 1) * (uint64_t)b.n_comp * W);
    }
    add(TAG_HOST, 8, HOST_WORDS);
    l.header = fixed_bytes() + RECORD_BYTES * l.rec.size();
    // (every count is below 2^6 2^6 2^24 or 3 2^31 2^24: the sums stay far below 2^64)
    uint64_t at = align8(l.header);
    for (Record &r : l.rec) {
        r.offset = at;
        at = (at + r.count * r.elem_bytes + 7) & ~(uint64_t)7;
    }
    if (at + 8 > (uint64_t)SIZE_MAX) return bad("sizes beyond size_t");
    l.checksum = (size_t)at;
    l.total = (size_t)at + 8;
    *out = l;
    return true;
}

void write_header(const Config &c, const Layout &l, uint8_t *out)
{
    std::memset(out, 0, l.header);
    put64(out + OFF_MAGIC, MAGIC);
    put32(out + OFF_VERSION, VERSION);
    put32(out + OFF_HEADER_BYTES, (uint32_t)l.header);
    std::memcpy(out + OFF_HASH, c.source_hash, HASH_BYTES);
    uint8_t *p = out + OFF_FIELDS;
    for (size_t i = 0; i < N_FIELDS; ++i) {
        const uint64_t v = field_get(c, FIELDS[i]);
        if (FIELDS[i].bytes == 4) put32(p, (uint32_t)v);
        else put64(p, v);
        p += FIELDS[i].bytes;
    }
    put32(p, (uint32_t)l.rec.size());
    put32(p + 4, 0);
    p += 8;
    for (const Record &r : l.rec) {
        put32(p, r.tag);
        put32(p + 4, r.elem_bytes);
        put64(p + 8, r.count);
        put64(p + 16, r.offset);
        p += RECORD_BYTES;
    }
}

void seal(const Layout &l, uint8_t *blob) { put64(blob + l.checksum, dqmc_blob::fnv1a64(blob, l.checksum)); }

namespace {

const char *sec_name(int s) { return s == SEC_MAIN ? "main" : (s == SEC_SCALING ? "scaling" : "stiffness"); }

// the ranges of the state (step 7 of validate)
int check_state(const uint8_t *buf, const Config &c, const Layout &l, std::string *why)
{
    auto bad = [&](const std::string &what) {
        *why = what;
        return -1;
    };
    const size_t W = (size_t)c.n_walkers;
    const Record *host = l.find(TAG_HOST);
    for (int s = 0; s < N_SEC; ++s) {
        const int64_t T = (int64_t)get64(buf + host->offset + 8 * s);
        if (c.bin[s].on ? (T < 0 || T > c.bin[s].cap) : T != 0)
            return bad(std::string("T of the binner's ") + sec_name(s) + " section is outside 0..capacity");
    }
    const Record *ns = l.find(TAG_N_SERIES);
    for (size_t w = 0; w < W; ++w) {
        const int64_t n = (int64_t)get64(buf + ns->offset + 8 * w);
        if (n < 0 || n > c.series_capacity) return bad("n_series of walker " + std::to_string(w) + " is outside 0..series_capacity");
    }
    const Record *conf = l.find(TAG_CONF);
    const uint8_t *cb = buf + conf->offset;
    if (c.kind == KIND_QSTATE) {
        const size_t row = (size_t)4 * ((c.n_sites + 3) / 4);
        for (size_t w = 0; w < W; ++w)
            for (size_t i = 0; i < row; ++i) {
                const uint8_t v = cb[w * row + i];
                if (i < (size_t)c.n_sites ? v >= c.q : v != 0)
                    return bad(i < (size_t)c.n_sites
                                   ? "the state of site " + std::to_string(i) + " of walker " + std::to_string(w) + " is not below q"
                                   : "a padding byte behind the sites of walker " + std::to_string(w) + " is not zero");
            }
    } else if (c.n_sites % 32) {
        const size_t nw = (size_t)(c.n_sites + 31) / 32;
        const uint32_t pad = ~(uint32_t)0 << (c.n_sites % 32);
        for (size_t w = 0; w < W; ++w)
            if (get32(cb + 4 * ((nw - 1) * W + w)) & pad)
                return bad("a padding bit behind the spins of walker " + std::to_string(w) + " is not zero");
    }
    if (const Record *rep = l.find(TAG_X_REPLICA)) {
        const size_t R = (size_t)c.exchange_R;
        for (size_t w0 = 0; w0 < W; w0 += R) {
            std::vector<bool> mark(R, false);
            for (size_t i = 0; i < R; ++i) {
                const uint32_t v = get32(buf + rep->offset + 4 * (w0 + i));
                if (v >= R || mark[v])
                    return bad("the replica labels of the ladder at walker " + std::to_string(w0) + " are no permutation");
                mark[v] = true;
            }
        }
    }
    return 0;
}

}  // namespace

int validate(const uint8_t *buf, size_t n_bytes, const Config &handle, Layout *l, std::string *why)
{
    std::string sink;
    if (!why) why = &sink;
    auto bad = [&](const std::string &what) {
        *why = what;
        return -1;
    };
    if (!buf) return bad("null buffer");
    if (n_bytes < fixed_bytes())
        return bad("the buffer (" + std::to_string(n_bytes) + " bytes) does not hold a header (" + std::to_string(fixed_bytes()) + " bytes)");
    if (get64(buf + OFF_MAGIC) != MAGIC) return bad("not a classical MC state blob: wrong magic");
    if (get32(buf + OFF_VERSION) != VERSION)
        return bad("format version " + std::to_string(get32(buf + OFF_VERSION)) + ", this library reads version " + std::to_string(VERSION));
    Config c{};
    std::memcpy(c.source_hash, buf + OFF_HASH, HASH_BYTES);
    const uint8_t *p = buf + OFF_FIELDS;
    for (size_t i = 0; i < N_FIELDS; ++i) {
        field_set(c, FIELDS[i], FIELDS[i].bytes == 4 ? (uint64_t)get32(p) : get64(p));
        p += FIELDS[i].bytes;
    }
    Layout bl;
    std::string lw;
    if (!layout(c, &bl, &lw)) return bad(lw);
    if (bl.total != n_bytes)
        return bad("the header implies " + std::to_string(bl.total) + " bytes, the buffer has " + std::to_string(n_bytes));
    {  // the record table is the one layout() gives (n_bytes >= bl.total > bl.header: in range)
        std::vector<uint8_t> head(bl.header);
        write_header(c, bl, head.data());
        if (std::memcmp(head.data() + OFF_HEADER_BYTES, buf + OFF_HEADER_BYTES, 4) != 0 ||
            std::memcmp(head.data() + fixed_bytes() - 8, buf + fixed_bytes() - 8, bl.header - (fixed_bytes() - 8)) != 0)
            return bad("the record table is not the one of the header's configuration");
    }
    if (get64(buf + bl.checksum) != dqmc_blob::fnv1a64(buf, bl.checksum)) return bad("checksum mismatch: the blob is damaged");
    for (size_t i = 0; i < N_FIELDS; ++i) {
        const uint64_t a = field_get(c, FIELDS[i]), b = field_get(handle, FIELDS[i]);
        if (a != b) {
            const bool hash = FIELDS[i].bytes == 8 && std::strncmp(FIELDS[i].name, "binner", 6) != 0;
            if (hash) return bad(std::string(FIELDS[i].name) + ": the blob's differs from the handle's");
            const long long sa = FIELDS[i].bytes == 4 ? (long long)(int32_t)a : (long long)a;
            const long long sb = FIELDS[i].bytes == 4 ? (long long)(int32_t)b : (long long)b;
            return bad(std::string(FIELDS[i].name) + ": the blob has " + std::to_string(sa) + ", the handle " + std::to_string(sb));
        }
    }
    if (int rc = check_state(buf, c, bl, why)) return rc;
    if (l) *l = bl;
    return 0;
}

}  // namespace mc_blob
