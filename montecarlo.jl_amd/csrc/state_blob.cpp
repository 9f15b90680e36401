// state_blob.cpp — see state_blob.h.  No HIP, no engine types: bytes in, bytes out.
#include "state_blob.h"

#include <cstring>

namespace dqmc_blob {
namespace {

// bin_name(k): the section names the error messages use
const char *const SEC_NAME[N_SEC] = {"greens", "correlations", "pairing", "susceptibilities", "time_displaced", "sign"};
const char *const BIN_NAME[N_BIN] = {"greens", "correlations", "pairing", "susceptibilities", "user", "time_displaced",
                                     "sign:greens", "sign:correlations", "sign:pairing", "sign:susceptibilities",
                                     "sign:time_displaced"};
const char *const MOM_NAME[N_MOM] = {"momentum_correlations", "momentum_susceptibilities", "momentum_time_displaced"};
const char *const RESP_NAME[N_RESP] = {"response_pairing", "response_pairing_susceptibility", "response_current"};

void put(uint8_t *&p, uint64_t v, int bytes)
{
    for (int i = 0; i < bytes; ++i) *p++ = (uint8_t)(v >> (8 * i));
}
uint64_t get(const uint8_t *&p, int bytes)
{
    uint64_t v = 0;
    for (int i = 0; i < bytes; ++i) v |= (uint64_t)*p++ << (8 * i);
    return v;
}
uint64_t bits_of(double d)
{
    uint64_t u;
    std::memcpy(&u, &d, sizeof(u));
    return u;
}
double double_of(uint64_t u)
{
    double d;
    std::memcpy(&d, &u, sizeof(d));
    return d;
}
uint64_t fnv1a(const uint8_t *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

enum { HEADER_BYTES = 8 + 4 + 4 + HASH_BYTES + 6 * 4 + 2 * 8 + 2 * N_SEC * 8 + N_BIN * 32 + 6 * 4 + 8 + 8 };
enum { EXT_FIXED_BYTES = 2 * 4 + N_MOM * 32 };
enum { THERMO_FIXED_BYTES = 2 * 8 + 32 + 8 + 8 };
enum { RESPONSE_FIXED_BYTES = 4 * 4 + N_RESP * 32 };

bool mul(size_t a, size_t b, size_t *out) { return !__builtin_mul_overflow(a, b, out); }
bool add(size_t a, size_t b, size_t *out) { return !__builtin_add_overflow(a, b, out); }
// *off += count * bytes, the old *off into *at
bool take(size_t *off, size_t *at, size_t count, size_t bytes)
{
    size_t sz;
    *at = *off;
    return mul(count, bytes, &sz) && add(*off, sz, off);
}
int refuse(std::string *why, const std::string &msg)
{
    if (why) *why = msg;
    return -1;
}

}  // namespace

size_t header_bytes() { return HEADER_BYTES; }

uint64_t fnv1a64(const void *bytes, size_t n) { return fnv1a((const uint8_t *)bytes, n); }

size_t conf_chunks(int32_t n_sites, int32_t slices) { return ((size_t)n_sites * (size_t)slices + 63) / 64; }

bool layout(const Shape &s, Layout *out, std::string *why)
{
    auto bad = [&](const char *what) {
        if (why) *why = what;
        return false;
    };
    if (s.n_sites < 1 || s.slices < 1 || s.n_walkers < 1 || s.nb < 1 || s.nb > 2) return bad("n_sites, slices, n_walkers, nb");
    const size_t W = (size_t)s.n_walkers;
    Layout l{};
    size_t off = HEADER_BYTES;
    bool ok = take(&off, &l.conf, W * conf_chunks(s.n_sites, s.slices), 8);
    ok = ok && take(&off, &l.rng, W, RNG_BYTES);
    ok = ok && take(&off, &l.stats, W, STATS_BYTES);
    ok = ok && take(&off, &l.gm, W, GM_BYTES);
    ok = ok && take(&off, &l.sign_fail, W, 8);
    for (int i = 0; i < N_SEC && ok; ++i) {
        if (s.sec_n[i] > (uint64_t)SIZE_MAX / 8) return bad("section size");
        ok = take(&off, &l.sec[i], (size_t)s.sec_n[i], 8);
    }
    for (int k = 0; k < N_BIN && ok; ++k) {
        const Shape::Bin &b = s.bin[k];
        l.bin_xs[k] = l.bin_x2[k] = l.bin_c[k] = off;
        if (!b.on) continue;
        if (b.E < 1 || b.L < 1 || b.L > 41) return bad("binner elements / levels");
        size_t we;
        ok = mul(W, (size_t)b.E, &we) && mul(we, 8, &we);
        ok = ok && take(&off, &l.bin_xs[k], (size_t)b.L, we);
        ok = ok && take(&off, &l.bin_x2[k], (size_t)b.L, we);
        ok = ok && take(&off, &l.bin_c[k], (size_t)b.L - 1, we);
    }
    if (!ok) return bad("blob size overflows");
    l.total = off;
    if (out) *out = l;
    return true;
}

static void write_header_version(const Shape &s, uint32_t version, uint8_t *out)
{
    uint8_t *p = out;
    put(p, MAGIC, 8);
    put(p, version, 4);
    put(p, HEADER_BYTES, 4);
    std::memcpy(p, s.source_hash, HASH_BYTES);
    p += HASH_BYTES;
    for (int32_t v : {s.n_sites, s.model_kind, s.slices, s.safe_mult, s.n_walkers, s.nb}) put(p, (uint32_t)v, 4);
    put(p, bits_of(s.delta_tau), 8);
    put(p, bits_of(s.U), 8);
    for (int i = 0; i < N_SEC; ++i) put(p, s.sec_n[i], 8);
    for (int i = 0; i < N_SEC; ++i) put(p, s.sec_n_red[i], 8);
    for (int k = 0; k < N_BIN; ++k) {
        const Shape::Bin &b = s.bin[k];
        put(p, (uint32_t)b.on, 4);
        put(p, (uint32_t)b.E, 4);
        put(p, (uint32_t)b.L, 4);
        put(p, 0, 4);
        put(p, (uint64_t)b.cap, 8);
        put(p, (uint64_t)b.T, 8);
    }
    for (int32_t v : {s.td_every, s.td_what, s.td_R, s.sign_on, s.gm_rate, s.gm_kind}) put(p, (uint32_t)v, 4);
    put(p, (uint64_t)s.gm_updates, 8);
    put(p, fnv1a(out, (size_t)(p - out)), 8);
}
void write_header(const Shape &s, uint8_t *out) { write_header_version(s, VERSION, out); }
void write_header(const Shape &s, const Momenta &m, uint8_t *out) { write_header_version(s, m.any() ? VERSION_MOMENTA : VERSION, out); }

// validate without its last step, the comparison of n_bytes with the size the header implies (*total).  newest: the
// highest format version the caller reads
static int validate_head(const uint8_t *buf, size_t n_bytes, const Shape &h, uint32_t newest, Shape *blob, uint32_t *version_out,
                         size_t *total, std::string *why)
{
    if (!buf) return refuse(why, "buffer: NULL");
    if (n_bytes < HEADER_BYTES)
        return refuse(why, "n_bytes: " + std::to_string(n_bytes) + " bytes do not hold the " + std::to_string((int)HEADER_BYTES) +
                               "-byte header");
    const uint8_t *p = buf;
    if (get(p, 8) != MAGIC) return refuse(why, "magic: not a dqmc_state_export blob");
    const uint32_t version = (uint32_t)get(p, 4);
    if (version < VERSION || version > newest)
        return refuse(why, "version: format version " + std::to_string(version) + ", this library reads version " +
                               std::to_string(VERSION) + (newest > VERSION ? " and " + std::to_string(newest) : std::string()));
    if (get(p, 4) != HEADER_BYTES) return refuse(why, "header_bytes: not the header size of format version 1");
    const uint8_t *sum_at = buf + HEADER_BYTES - 8;
    if (get(sum_at, 8) != fnv1a(buf, HEADER_BYTES - 8))
        return refuse(why, "checksum: the header is damaged (it claims format version " + std::to_string(version) + ")");

    Shape s{};
    std::memcpy(s.source_hash, p, HASH_BYTES);
    p += HASH_BYTES;
    for (int32_t *v : {&s.n_sites, &s.model_kind, &s.slices, &s.safe_mult, &s.n_walkers, &s.nb}) *v = (int32_t)(uint32_t)get(p, 4);
    s.delta_tau = double_of(get(p, 8));
    s.U = double_of(get(p, 8));
    for (int i = 0; i < N_SEC; ++i) s.sec_n[i] = get(p, 8);
    for (int i = 0; i < N_SEC; ++i) s.sec_n_red[i] = get(p, 8);
    for (int k = 0; k < N_BIN; ++k) {
        Shape::Bin &b = s.bin[k];
        b.on = (int32_t)(uint32_t)get(p, 4);
        b.E = (int32_t)(uint32_t)get(p, 4);
        b.L = (int32_t)(uint32_t)get(p, 4);
        (void)get(p, 4);
        b.cap = (int64_t)get(p, 8);
        b.T = (int64_t)get(p, 8);
    }
    for (int32_t *v : {&s.td_every, &s.td_what, &s.td_R, &s.sign_on, &s.gm_rate, &s.gm_kind}) *v = (int32_t)(uint32_t)get(p, 4);
    s.gm_updates = (int64_t)get(p, 8);

    // configuration: the first field that differs from the importing handle
#define SAME(field, name)                                                                                             \
    if (!(s.field == h.field))                                                                                        \
        return refuse(why, std::string(name) + ": the blob has " + std::to_string(s.field) + ", the handle " +        \
                               std::to_string(h.field))
    SAME(n_sites, "n_sites");
    SAME(model_kind, "model_kind");
    SAME(slices, "slices");
    SAME(safe_mult, "safe_mult");
    SAME(n_walkers, "n_walkers");
    SAME(nb, "nb");
    if (bits_of(s.delta_tau) != bits_of(h.delta_tau)) return refuse(why, "delta_tau: differs from the handle's");
    if (bits_of(s.U) != bits_of(h.U)) return refuse(why, "U: differs from the handle's");
    SAME(sign_on, "sign_on");
    for (int i = 0; i < N_SEC; ++i) {
        SAME(sec_n[i], std::string("section ") + SEC_NAME[i] + " n");
        SAME(sec_n_red[i], std::string("section ") + SEC_NAME[i] + " n_red");
    }
    SAME(td_every, "time_displaced every");
    SAME(td_what, "time_displaced what");
    SAME(td_R, "time_displaced R");
    for (int k = 0; k < N_BIN; ++k) {
        SAME(bin[k].on, std::string("binner ") + BIN_NAME[k] + " on");
        SAME(bin[k].E, std::string("binner ") + BIN_NAME[k] + " E");
        SAME(bin[k].L, std::string("binner ") + BIN_NAME[k] + " L");
        SAME(bin[k].cap, std::string("binner ") + BIN_NAME[k] + " cap");
    }
    SAME(gm_rate, "gm_rate");
    SAME(gm_kind, "gm_kind");
#undef SAME
    // state: ranges only
    for (int k = 0; k < N_BIN; ++k) {
        const Shape::Bin &b = s.bin[k];
        if (b.T < 0 || b.T > (b.on ? b.cap : 0))
            return refuse(why, std::string("binner ") + BIN_NAME[k] + " T: " + std::to_string(b.T) + " pushes outside 0 .. capacity");
    }
    if (s.gm_updates < 0) return refuse(why, "gm_updates: negative");
    Layout l;
    std::string lw;
    if (!layout(s, &l, &lw)) return refuse(why, lw + ": not a shape a handle can have");
    if (blob) *blob = s;
    *version_out = version;
    *total = l.total;
    return 0;
}
static int refuse_size(std::string *why, size_t n_bytes, size_t want)
{
    return refuse(why, "n_bytes: the buffer has " + std::to_string(n_bytes) + " bytes, the header describes " + std::to_string(want));
}
int validate(const uint8_t *buf, size_t n_bytes, const Shape &h, Shape *blob, std::string *why)
{
    Shape s{};
    uint32_t version = 0;
    size_t total = 0;
    if (validate_head(buf, n_bytes, h, VERSION, &s, &version, &total, why) != 0) return -1;
    if (n_bytes != total) return refuse_size(why, n_bytes, total);
    if (blob) *blob = s;
    return 0;
}

bool ext_layout(const Shape &s, const Momenta &m, ExtLayout *out, std::string *why)
{
    auto bad = [&](const char *what) {
        if (why) *why = what;
        return false;
    };
    Layout l;
    if (!layout(s, &l, why)) return false;
    ExtLayout e{};
    e.start = e.total = l.total;
    if (!m.any()) {
        if (out) *out = e;
        return true;
    }
    if (m.n_dirs < 1 || m.n_q < 1 || m.n_q > m.n_dirs) return bad("momenta n_q, n_dirs");
    const size_t W = (size_t)s.n_walkers;
    size_t off = e.start, skip, tab;
    bool ok = take(&off, &skip, EXT_FIXED_BYTES, 1) && mul((size_t)m.n_dirs, (size_t)m.n_q, &tab);
    ok = ok && take(&off, &e.cos_tab, tab, 8) && take(&off, &e.sin_tab, tab, 8);
    for (int k = 0; k < N_MOM && ok; ++k) {
        const Shape::Bin &b = m.bin[k];
        e.bin_xs[k] = e.bin_x2[k] = e.bin_c[k] = off;
        if (!b.on) continue;
        if (b.E < 1 || b.L < 1 || b.L > 41) return bad("momentum binner elements / levels");
        size_t we;
        ok = mul(W, (size_t)b.E, &we) && mul(we, 8, &we);
        ok = ok && take(&off, &e.bin_xs[k], (size_t)b.L, we);
        ok = ok && take(&off, &e.bin_x2[k], (size_t)b.L, we);
        ok = ok && take(&off, &e.bin_c[k], (size_t)b.L - 1, we);
    }
    ok = ok && take(&off, &e.checksum, 1, 8);
    if (!ok) return bad("blob size overflows");
    e.total = off;
    if (out) *out = e;
    return true;
}

void write_ext(const Momenta &m, const ExtLayout &e, uint8_t *blob)
{
    if (!m.any()) return;
    uint8_t *p = blob + e.start;
    put(p, (uint32_t)m.n_q, 4);
    put(p, (uint32_t)m.n_dirs, 4);
    for (int k = 0; k < N_MOM; ++k) {
        const Shape::Bin &b = m.bin[k];
        put(p, (uint32_t)b.on, 4);
        put(p, (uint32_t)b.E, 4);
        put(p, (uint32_t)b.L, 4);
        put(p, 0, 4);
        put(p, (uint64_t)b.cap, 8);
        put(p, (uint64_t)b.T, 8);
    }
    const size_t tab = (size_t)m.n_dirs * (size_t)m.n_q;
    for (size_t i = 0; i < tab; ++i) put(p, bits_of(m.cos_tab[i]), 8);
    for (size_t i = 0; i < tab; ++i) put(p, bits_of(m.sin_tab[i]), 8);
}

void seal_ext(const ExtLayout &e, uint8_t *blob)
{
    if (e.total == e.start) return;
    uint8_t *p = blob + e.checksum;
    put(p, fnv1a(blob + e.start, e.checksum - e.start), 8);
}

// validate_any for the blob's version-1 / 2 part.  newest: the highest format version the caller reads; with a version
// above 2 more bytes may follow that part, whose size goes to *end
static int validate_core(const uint8_t *buf, size_t n_bytes, const Shape &h, const Momenta &hm, uint32_t newest, Shape *blob,
                         Momenta *mblob, uint32_t *version_out, size_t *end, std::string *why)
{
    Shape s{};
    uint32_t version = 0;
    size_t total = 0;
    if (validate_head(buf, n_bytes, h, newest, &s, &version, &total, why) != 0) return -1;
    // (a version above 4 is the version below it by 4 with the response extension behind everything else)
    const bool more = version > VERSION_THERMO_MOMENTA;
    const uint32_t base = more ? version - VERSION_RESPONSE_STEP : version;
    const bool tail = base >= VERSION_THERMO || more;
    const std::string fmt = std::to_string(version);
    Momenta m{};
    *version_out = version;
    *end = total;
    if (base == VERSION || base == VERSION_THERMO) {
        if (tail ? n_bytes < total : n_bytes != total) return refuse_size(why, n_bytes, total);
        for (int k = 0; k < N_MOM; ++k)
            if (hm.bin[k].on)
                return refuse(why, std::string("binner ") + MOM_NAME[k] + " on: the blob (format version " + fmt + ") has 0, the handle 1");
    } else {
        if (n_bytes < total || n_bytes - total < EXT_FIXED_BYTES) return refuse_size(why, n_bytes, total + EXT_FIXED_BYTES);
        const uint8_t *p = buf + total;
        m.n_q = (int32_t)(uint32_t)get(p, 4);
        m.n_dirs = (int32_t)(uint32_t)get(p, 4);
        for (int k = 0; k < N_MOM; ++k) {
            Shape::Bin &b = m.bin[k];
            b.on = (int32_t)(uint32_t)get(p, 4);
            b.E = (int32_t)(uint32_t)get(p, 4);
            b.L = (int32_t)(uint32_t)get(p, 4);
            (void)get(p, 4);
            b.cap = (int64_t)get(p, 8);
            b.T = (int64_t)get(p, 8);
            if (b.on != 0 && b.on != 1) return refuse(why, std::string("binner ") + MOM_NAME[k] + " on: neither 0 nor 1");
        }
        if (!m.any()) return refuse(why, "extension: a format version " + std::to_string(version) + " blob with no momentum binner in it");
        ExtLayout e;
        std::string lw;
        if (!ext_layout(s, m, &e, &lw)) return refuse(why, lw + ": not a shape a handle can have");
        if (tail ? n_bytes < e.total : n_bytes != e.total) return refuse_size(why, n_bytes, e.total);
        *end = e.total;
        const uint8_t *sum_at = buf + e.checksum;
        if (get(sum_at, 8) != fnv1a(buf + e.start, e.checksum - e.start))
            return refuse(why, "extension checksum: the extension is damaged");
#define SAME_M(field, name)                                                                                           \
    if (!(m.field == hm.field))                                                                                       \
        return refuse(why, std::string(name) + ": the blob has " + std::to_string(m.field) + ", the handle " +        \
                               std::to_string(hm.field))
        SAME_M(n_q, "momenta n_q");
        SAME_M(n_dirs, "momenta n_dirs");
        for (int k = 0; k < N_MOM; ++k) {
            SAME_M(bin[k].on, std::string("binner ") + MOM_NAME[k] + " on");
            SAME_M(bin[k].E, std::string("binner ") + MOM_NAME[k] + " E");
            SAME_M(bin[k].L, std::string("binner ") + MOM_NAME[k] + " L");
            SAME_M(bin[k].cap, std::string("binner ") + MOM_NAME[k] + " cap");
        }
#undef SAME_M
        if (!hm.cos_tab || !hm.sin_tab) return refuse(why, "momenta tables: the handle has none");
        const size_t tab = (size_t)m.n_dirs * (size_t)m.n_q;
        const uint8_t *c = buf + e.cos_tab, *sn = buf + e.sin_tab;
        for (size_t i = 0; i < tab; ++i)
            if (get(c, 8) != bits_of(hm.cos_tab[i]))
                return refuse(why, "momenta cos_tab: entry " + std::to_string(i) + " differs from the handle's");
        for (size_t i = 0; i < tab; ++i)
            if (get(sn, 8) != bits_of(hm.sin_tab[i]))
                return refuse(why, "momenta sin_tab: entry " + std::to_string(i) + " differs from the handle's");
        for (int k = 0; k < N_MOM; ++k) {
            const Shape::Bin &b = m.bin[k];
            if (b.T < 0 || b.T > (b.on ? b.cap : 0))
                return refuse(why, std::string("binner ") + MOM_NAME[k] + " T: " + std::to_string(b.T) + " pushes outside 0 .. capacity");
        }
    }
    if (blob) *blob = s;
    if (mblob) *mblob = m;
    return 0;
}
int validate_any(const uint8_t *buf, size_t n_bytes, const Shape &h, const Momenta &hm, Shape *blob, Momenta *mblob,
                 std::string *why)
{
    uint32_t version = 0;
    size_t end = 0;
    return validate_core(buf, n_bytes, h, hm, VERSION_MOMENTA, blob, mblob, &version, &end, why);
}

bool thermo_layout(const Shape &s, const Momenta &m, const Thermo &t, ThermoLayout *out, std::string *why)
{
    auto bad = [&](const char *what) {
        if (why) *why = what;
        return false;
    };
    ExtLayout e;
    if (!ext_layout(s, m, &e, why)) return false;
    ThermoLayout l{};
    l.start = l.total = e.total;
    if (!t.any()) {
        if (out) *out = l;
        return true;
    }
    if (t.n > (uint64_t)SIZE_MAX / 8) return bad("section thermodynamics size");
    const size_t W = (size_t)s.n_walkers;
    size_t off = l.start, skip;
    bool ok = take(&off, &skip, THERMO_FIXED_BYTES, 1) && take(&off, &l.sec, (size_t)t.n, 8);
    l.bin_xs = l.bin_x2 = l.bin_c = off;
    if (ok && t.bin.on) {
        if (t.bin.E < 1 || t.bin.L < 1 || t.bin.L > 41) return bad("thermodynamics binner elements / levels");
        size_t we;
        ok = mul(W, (size_t)t.bin.E, &we) && mul(we, 8, &we);
        ok = ok && take(&off, &l.bin_xs, (size_t)t.bin.L, we);
        ok = ok && take(&off, &l.bin_x2, (size_t)t.bin.L, we);
        ok = ok && take(&off, &l.bin_c, (size_t)t.bin.L - 1, we);
    }
    ok = ok && take(&off, &l.checksum, 1, 8);
    if (!ok) return bad("blob size overflows");
    l.total = off;
    if (out) *out = l;
    return true;
}

void write_header(const Shape &s, const Momenta &m, const Thermo &t, uint8_t *out)
{
    if (!t.any()) write_header(s, m, out);
    else write_header_version(s, m.any() ? VERSION_THERMO_MOMENTA : VERSION_THERMO, out);
}

void write_thermo(const Thermo &t, const ThermoLayout &l, uint8_t *blob)
{
    if (!t.any()) return;
    uint8_t *p = blob + l.start;
    put(p, t.n, 8);
    put(p, t.n_red, 8);
    put(p, (uint32_t)t.bin.on, 4);
    put(p, (uint32_t)t.bin.E, 4);
    put(p, (uint32_t)t.bin.L, 4);
    put(p, 0, 4);
    put(p, (uint64_t)t.bin.cap, 8);
    put(p, (uint64_t)t.bin.T, 8);
    put(p, t.T_hash, 8);
    put(p, bits_of(t.U_s), 8);
}

void seal_thermo(const ThermoLayout &l, uint8_t *blob)
{
    if (l.total == l.start) return;
    uint8_t *p = blob + l.checksum;
    put(p, fnv1a(blob + l.start, l.checksum - l.start), 8);
}

// validate_all for the blob's version 1 - 4 part.  newest: the highest format version the caller reads; with a version
// above 4 more bytes may follow that part, whose size goes to *end
static int validate_front(const uint8_t *buf, size_t n_bytes, const Shape &h, const Momenta &hm, const Thermo &ht, uint32_t newest,
                          Shape *blob, Momenta *mblob, Thermo *tblob, uint32_t *version_out, size_t *end_out, std::string *why)
{
    Shape s{};
    Momenta m{};
    Thermo t{};
    uint32_t version = 0;
    size_t end = 0;
    if (validate_core(buf, n_bytes, h, hm, newest, &s, &m, &version, &end, why) != 0) return -1;
    const bool more = version > VERSION_THERMO_MOMENTA;
    const uint32_t base = more ? version - VERSION_RESPONSE_STEP : version;
    *version_out = version;
    *end_out = end;
    if (base < VERSION_THERMO) {
        if (ht.any())
            return refuse(why, "section thermodynamics n: the blob (format version " + std::to_string(version) + ") has 0, the handle " +
                                   std::to_string(ht.n));
    } else {
        if (n_bytes - end < THERMO_FIXED_BYTES) return refuse_size(why, n_bytes, end + THERMO_FIXED_BYTES);
        const uint8_t *p = buf + end;
        t.n = get(p, 8);
        t.n_red = get(p, 8);
        t.bin.on = (int32_t)(uint32_t)get(p, 4);
        t.bin.E = (int32_t)(uint32_t)get(p, 4);
        t.bin.L = (int32_t)(uint32_t)get(p, 4);
        (void)get(p, 4);
        t.bin.cap = (int64_t)get(p, 8);
        t.bin.T = (int64_t)get(p, 8);
        t.T_hash = get(p, 8);
        t.U_s = double_of(get(p, 8));
        if (t.bin.on != 0 && t.bin.on != 1) return refuse(why, "binner thermodynamics on: neither 0 nor 1");
        if (!t.any()) return refuse(why, "extension: a format version " + std::to_string(version) + " blob with no thermodynamics section in it");
        ThermoLayout l;
        std::string lw;
        if (!thermo_layout(s, m, t, &l, &lw)) return refuse(why, lw + ": not a shape a handle can have");
        if (more ? n_bytes < l.total : n_bytes != l.total) return refuse_size(why, n_bytes, l.total);
        *end_out = l.total;
        const uint8_t *sum_at = buf + l.checksum;
        if (get(sum_at, 8) != fnv1a(buf + l.start, l.checksum - l.start))
            return refuse(why, "thermodynamics extension checksum: the extension is damaged");
#define SAME_T(field, name)                                                                                           \
    if (!(t.field == ht.field))                                                                                       \
        return refuse(why, std::string(name) + ": the blob has " + std::to_string(t.field) + ", the handle " +        \
                               std::to_string(ht.field))
        SAME_T(n, "section thermodynamics n");
        SAME_T(n_red, "section thermodynamics n_red");
        SAME_T(bin.on, "binner thermodynamics on");
        SAME_T(bin.E, "binner thermodynamics E");
        SAME_T(bin.L, "binner thermodynamics L");
        SAME_T(bin.cap, "binner thermodynamics cap");
#undef SAME_T
        if (t.T_hash != ht.T_hash) return refuse(why, "thermodynamics hopping matrix: differs from the handle's");
        if (bits_of(t.U_s) != bits_of(ht.U_s)) return refuse(why, "thermodynamics U_s: differs from the handle's");
        if (t.bin.T < 0 || t.bin.T > (t.bin.on ? t.bin.cap : 0))
            return refuse(why, "binner thermodynamics T: " + std::to_string(t.bin.T) + " pushes outside 0 .. capacity");
    }
    if (blob) *blob = s;
    if (mblob) *mblob = m;
    if (tblob) *tblob = t;
    return 0;
}
int validate_all(const uint8_t *buf, size_t n_bytes, const Shape &h, const Momenta &hm, const Thermo &ht, Shape *blob,
                 Momenta *mblob, Thermo *tblob, std::string *why)
{
    uint32_t version = 0;
    size_t end = 0;
    return validate_front(buf, n_bytes, h, hm, ht, VERSION_THERMO_MOMENTA, blob, mblob, tblob, &version, &end, why);
}

bool response_layout(const Shape &s, const Momenta &m, const Thermo &t, const Response &r, ResponseLayout *out, std::string *why)
{
    auto bad = [&](const char *what) {
        if (why) *why = what;
        return false;
    };
    ThermoLayout tl;
    if (!thermo_layout(s, m, t, &tl, why)) return false;
    ResponseLayout l{};
    l.start = l.total = tl.total;
    if (!r.any()) {
        if (out) *out = l;
        return true;
    }
    if (r.n_ch < 0 || r.n_ch > 8 || r.K < 0 || r.K_cc < 0 || (r.n_ch > 0 && r.K < 1)) return bad("response n_ch, K, K_cc");
    const size_t W = (size_t)s.n_walkers;
    size_t off = l.start, skip, tab;
    bool ok = take(&off, &skip, RESPONSE_FIXED_BYTES, 1) && mul((size_t)r.K, (size_t)r.K, &tab) && mul(tab, (size_t)r.n_ch, &tab);
    ok = ok && take(&off, &l.F, tab, 8);
    for (int k = 0; k < N_RESP && ok; ++k) {
        const Shape::Bin &b = r.bin[k];
        l.bin_xs[k] = l.bin_x2[k] = l.bin_c[k] = off;
        if (!b.on) continue;
        if (b.E < 1 || b.L < 1 || b.L > 41) return bad("response binner elements / levels");
        size_t we;
        ok = mul(W, (size_t)b.E, &we) && mul(we, 8, &we);
        ok = ok && take(&off, &l.bin_xs[k], (size_t)b.L, we);
        ok = ok && take(&off, &l.bin_x2[k], (size_t)b.L, we);
        ok = ok && take(&off, &l.bin_c[k], (size_t)b.L - 1, we);
    }
    ok = ok && take(&off, &l.checksum, 1, 8);
    if (!ok) return bad("blob size overflows");
    l.total = off;
    if (out) *out = l;
    return true;
}

void write_header(const Shape &s, const Momenta &m, const Thermo &t, const Response &r, uint8_t *out)
{
    if (!r.any()) write_header(s, m, t, out);
    else write_header_version(s, (t.any() ? (m.any() ? VERSION_THERMO_MOMENTA : VERSION_THERMO) : (m.any() ? VERSION_MOMENTA : VERSION)) +
                                     VERSION_RESPONSE_STEP, out);
}

void write_response(const Response &r, const ResponseLayout &l, uint8_t *blob)
{
    if (!r.any()) return;
    uint8_t *p = blob + l.start;
    put(p, (uint32_t)r.n_ch, 4);
    put(p, (uint32_t)r.K, 4);
    put(p, (uint32_t)r.K_cc, 4);
    put(p, 0, 4);
    for (int k = 0; k < N_RESP; ++k) {
        const Shape::Bin &b = r.bin[k];
        put(p, (uint32_t)b.on, 4);
        put(p, (uint32_t)b.E, 4);
        put(p, (uint32_t)b.L, 4);
        put(p, 0, 4);
        put(p, (uint64_t)b.cap, 8);
        put(p, (uint64_t)b.T, 8);
    }
    const size_t tab = (size_t)r.K * (size_t)r.K * (size_t)r.n_ch;
    for (size_t i = 0; i < tab; ++i) put(p, bits_of(r.F[i]), 8);
}

void seal_response(const ResponseLayout &l, uint8_t *blob)
{
    if (l.total == l.start) return;
    uint8_t *p = blob + l.checksum;
    put(p, fnv1a(blob + l.start, l.checksum - l.start), 8);
}

int validate_full(const uint8_t *buf, size_t n_bytes, const Shape &h, const Momenta &hm, const Thermo &ht, const Response &hr,
                  Shape *blob, Momenta *mblob, Thermo *tblob, Response *rblob, std::string *why)
{
    Shape s{};
    Momenta m{};
    Thermo t{};
    Response r{};
    uint32_t version = 0;
    size_t end = 0;
    if (validate_front(buf, n_bytes, h, hm, ht, VERSION_THERMO_MOMENTA + VERSION_RESPONSE_STEP, &s, &m, &t, &version, &end, why) != 0)
        return -1;
    if (version <= VERSION_THERMO_MOMENTA) {
        for (int k = 0; k < N_RESP; ++k)
            if (hr.bin[k].on)
                return refuse(why, std::string("binner ") + RESP_NAME[k] + " on: the blob (format version " + std::to_string(version) +
                                       ") has 0, the handle 1");
    } else {
        if (n_bytes < end || n_bytes - end < RESPONSE_FIXED_BYTES) return refuse_size(why, n_bytes, end + RESPONSE_FIXED_BYTES);
        const uint8_t *p = buf + end;
        r.n_ch = (int32_t)(uint32_t)get(p, 4);
        r.K = (int32_t)(uint32_t)get(p, 4);
        r.K_cc = (int32_t)(uint32_t)get(p, 4);
        (void)get(p, 4);
        for (int k = 0; k < N_RESP; ++k) {
            Shape::Bin &b = r.bin[k];
            b.on = (int32_t)(uint32_t)get(p, 4);
            b.E = (int32_t)(uint32_t)get(p, 4);
            b.L = (int32_t)(uint32_t)get(p, 4);
            (void)get(p, 4);
            b.cap = (int64_t)get(p, 8);
            b.T = (int64_t)get(p, 8);
            if (b.on != 0 && b.on != 1) return refuse(why, std::string("binner ") + RESP_NAME[k] + " on: neither 0 nor 1");
        }
        if (!r.any()) return refuse(why, "extension: a format version " + std::to_string(version) + " blob with no response binner in it");
        ResponseLayout l;
        std::string lw;
        if (!response_layout(s, m, t, r, &l, &lw)) return refuse(why, lw + ": not a shape a handle can have");
        if (n_bytes != l.total) return refuse_size(why, n_bytes, l.total);
        const uint8_t *sum_at = buf + l.checksum;
        if (get(sum_at, 8) != fnv1a(buf + l.start, l.checksum - l.start))
            return refuse(why, "response extension checksum: the extension is damaged");
#define SAME_R(field, name)                                                                                           \
    if (!(r.field == hr.field))                                                                                       \
        return refuse(why, std::string(name) + ": the blob has " + std::to_string(r.field) + ", the handle " +        \
                               std::to_string(hr.field))
        for (int k = 0; k < N_RESP; ++k) SAME_R(bin[k].on, std::string("binner ") + RESP_NAME[k] + " on");  // (which binners, first)
        SAME_R(n_ch, "response n_ch");
        SAME_R(K, "response K");
        SAME_R(K_cc, "response K_cc");
        for (int k = 0; k < N_RESP; ++k) {
            SAME_R(bin[k].on, std::string("binner ") + RESP_NAME[k] + " on");
            SAME_R(bin[k].E, std::string("binner ") + RESP_NAME[k] + " E");
            SAME_R(bin[k].L, std::string("binner ") + RESP_NAME[k] + " L");
            SAME_R(bin[k].cap, std::string("binner ") + RESP_NAME[k] + " cap");
        }
#undef SAME_R
        const size_t tab = (size_t)r.K * (size_t)r.K * (size_t)r.n_ch;
        if (tab && !hr.F) return refuse(why, "response F: the handle has none");
        const uint8_t *f = buf + l.F;
        for (size_t i = 0; i < tab; ++i)
            if (get(f, 8) != bits_of(hr.F[i])) return refuse(why, "response F: entry " + std::to_string(i) + " differs from the handle's");
        for (int k = 0; k < N_RESP; ++k) {
            const Shape::Bin &b = r.bin[k];
            if (b.T < 0 || b.T > (b.on ? b.cap : 0))
                return refuse(why, std::string("binner ") + RESP_NAME[k] + " T: " + std::to_string(b.T) + " pushes outside 0 .. capacity");
        }
    }
    if (blob) *blob = s;
    if (mblob) *mblob = m;
    if (tblob) *tblob = t;
    if (rblob) *rblob = r;
    return 0;
}

void pack_conf(const int8_t *conf, size_t n, uint8_t *chunks_le)
{
    const size_t bytes = (n + 63) / 64 * 8;
    std::memset(chunks_le, 0, bytes);
    for (size_t i = 0; i < n; ++i)
        if (conf[i] == 1) chunks_le[i >> 3] |= (uint8_t)(1u << (i & 7));
}
void unpack_conf(const uint8_t *chunks_le, size_t n, int8_t *conf)
{
    for (size_t i = 0; i < n; ++i) conf[i] = (chunks_le[i >> 3] >> (i & 7)) & 1 ? 1 : -1;
}

}  // namespace dqmc_blob
