// state_blob.h — the checkpoint blob of dqmc_state_export / dqmc_state_import (include/dqmc_hip.h "checkpoint and
// resume"): its header, the validation of a header against the handle that is to take it, and the offsets of the payload.
// Plain C++ with no HIP in it: engine.cpp fills a Shape from the handle and does the copies; the code here sees bytes only,
// so that it can be built and run under the host sanitizers on its own (tests/test_checkpoint_blob.py).
//
// Every field is little-endian and of fixed width; doubles travel as their IEEE bit pattern.
#ifndef DQMC_STATE_BLOB_H
#define DQMC_STATE_BLOB_H
#include <cstddef>
#include <cstdint>
#include <string>

namespace dqmc_blob {

enum { N_SEC = 6,    // DQMC_RED_GREENS .. DQMC_RED_SIGN
       N_BIN = 11 }; // DQMC_BIN_GREENS .. DQMC_BIN_TIME_DISPLACED, then DQMC_BIN_SIGN + k for the five measurement sections
static const uint64_t MAGIC = 0x31415453434d5144ull;  // the bytes "DQMCSTA1", read as one little-endian word
static const uint32_t VERSION = 1;
enum { HASH_BYTES = 16 };

// What the payload depends on, as the header carries it.  `T` of a binner and `gm_updates` are state (restored by the
// import); every other field is configuration and must agree with the importing handle.
struct Shape {
    char source_hash[HASH_BYTES];  // dqmc_build_source_hash of the exporting library, zero-padded; never checked
    int32_t n_sites, model_kind, slices, safe_mult, n_walkers, nb;
    double delta_tau, U;
    uint64_t sec_n[N_SEC], sec_n_red[N_SEC];  // doubles of a section's accumulator / of its part in the reduction (0: not configured)
    struct Bin {
        int32_t on, E, L;
        int64_t cap, T;
    } bin[N_BIN];
    int32_t td_every, td_what, td_R;
    int32_t sign_on;
    int32_t gm_rate, gm_kind;
    int64_t gm_updates;
};

// bytes per walker of the fixed-size records of the payload
enum { RNG_BYTES = 16,     // seed, draw
       STATS_BYTES = 80,   // prop_local, acc_local, 2 x {max, min, sum, count}
       GM_BYTES = 56 };    // moves_drawn, prop_global, acc_global, dS, last_p, active, site, last_accepted, pad

// byte offsets of the payload from the start of the blob, in blob order
struct Layout {
    size_t conf;       // n_walkers x conf_chunks(n_sites, slices) x uint64: dqmc_get_conf_bits per walker
    size_t rng;        // n_walkers x RNG_BYTES
    size_t stats;      // n_walkers x STATS_BYTES
    size_t gm;         // n_walkers x GM_BYTES
    size_t sign_fail;  // n_walkers x int64
    size_t sec[N_SEC];                                // sec_n doubles each (configured sections only)
    size_t bin_xs[N_BIN], bin_x2[N_BIN], bin_c[N_BIN];  // L W E, L W E, (L - 1) W E doubles (enabled binners only)
    size_t total;      // size of the whole blob
};

size_t header_bytes();
size_t conf_chunks(int32_t n_sites, int32_t slices);
// false if the shape is not one a handle can have (a count below its minimum) or the sizes overflow size_t
bool layout(const Shape &s, Layout *out, std::string *why = nullptr);
// header_bytes() bytes into `out`
void write_header(const Shape &s, uint8_t *out);
// Everything dqmc_state_import checks before its first write, in this order: the buffer holds a header; magic; format
// version; the header's checksum; every configuration field against `handle` (the first one that differs is named); the
// state fields' ranges; n_bytes against the size the header implies.  0 and *blob filled, or -1 and *why set.
int validate(const uint8_t *buf, size_t n_bytes, const Shape &handle, Shape *blob, std::string *why);

// ---- format version 2: the version-1 header (version field 2) and payload, then an extension for the momentum binners,
// which the 560-byte header has no room for.  A handle with no momentum binner enabled writes version 1 unchanged.
//   i32 n_q, n_dirs   N_MOM x (i32 on, E, L, pad, i64 cap, T)   cos_tab, sin_tab [n_dirs n_q doubles each]
//   xs, x2, c of every enabled momentum binner   u64 FNV-1a 64 of every extension byte in front of it
enum { N_MOM = 3 };  // DQMC_BIN_MOMENTUM_CORRELATIONS, _SUSCEPTIBILITIES, _TIME_DISPLACED
static const uint32_t VERSION_MOMENTA = 2;
struct Momenta {
    int32_t n_q = 0, n_dirs = 0;
    const double *cos_tab = nullptr, *sin_tab = nullptr;  // n_dirs n_q doubles each, borrowed (nullptr in what validate_any hands back)
    Shape::Bin bin[N_MOM] = {};
    bool any() const { return bin[0].on || bin[1].on || bin[2].on; }  // false: the blob is version 1
};
// byte offsets from the start of the blob; with !m.any() only `start` and `total` are set, both to the version-1 size
struct ExtLayout {
    size_t start, cos_tab, sin_tab;
    size_t bin_xs[N_MOM], bin_x2[N_MOM], bin_c[N_MOM];
    size_t checksum, total;
};
bool ext_layout(const Shape &s, const Momenta &m, ExtLayout *out, std::string *why = nullptr);
// write_header with the version the pair (s, m) calls for
void write_header(const Shape &s, const Momenta &m, uint8_t *out);
// the extension's fixed fields and tables into blob + e.start (nothing when !m.any())
void write_ext(const Momenta &m, const ExtLayout &e, uint8_t *blob);
// the checksum over blob[e.start, e.checksum), once the binner arrays are in place
void seal_ext(const ExtLayout &e, uint8_t *blob);
// validate for both versions.  Version 1: as validate, and refused when the handle has a momentum binner enabled.
// Version 2: the header and payload as above, then the extension: n_bytes holds its fixed fields; its own shape is one a
// handle can have; n_bytes against the size it implies; its checksum; n_q, n_dirs and every binner's on / E / L / cap
// against `hm` (the first that differs is named); both tables byte for byte against hm's; the ranges of T.  0 and *blob /
// *mblob filled (mblob's T are the state to restore), or -1 and *why set.
int validate_any(const uint8_t *buf, size_t n_bytes, const Shape &handle, const Momenta &hm, Shape *blob, Momenta *mblob,
                 std::string *why);

// ---- format versions 3 and 4: the version-1 (3) or version-2 (4) blob, its version field apart, then an extension for the
// thermodynamics section (DQMC_RED_THERMODYNAMICS, DQMC_BIN_THERMODYNAMICS), which the header's tables have no room for.  A
// handle without the section writes version 1 / 2 unchanged.
//   u64 n, n_red   i32 on, E, L, pad, i64 cap, T (the binner)   u64 T_hash   f64 U_s
//   the section's n doubles   xs, x2, c of the binner if enabled   u64 FNV-1a 64 of every extension byte in front of it
static const uint32_t VERSION_THERMO = 3, VERSION_THERMO_MOMENTA = 4;
struct Thermo {
    uint64_t n = 0, n_red = 0;  // doubles of the section / of its part in the reduction; n == 0: off, the blob is version 1 / 2
    Shape::Bin bin = {};
    uint64_t T_hash = 0;        // fnv1a64 of the hopping matrix the section was configured with
    double U_s = 0.0;
    bool any() const { return n != 0; }
};
// byte offsets from the start of the blob; with !t.any() only `start` and `total` are set, both to the size of the version-1 / 2 blob
struct ThermoLayout {
    size_t start, sec, bin_xs, bin_x2, bin_c, checksum, total;
};
uint64_t fnv1a64(const void *bytes, size_t n);
bool thermo_layout(const Shape &s, const Momenta &m, const Thermo &t, ThermoLayout *out, std::string *why = nullptr);
// write_header with the version the triple calls for (t.any(): 3 or 4, else as write_header(s, m, out))
void write_header(const Shape &s, const Momenta &m, const Thermo &t, uint8_t *out);
// the extension's fixed fields into blob + l.start (nothing when !t.any()); seal_thermo once the section and the binner
// arrays are in place
void write_thermo(const Thermo &t, const ThermoLayout &l, uint8_t *blob);
void seal_thermo(const ThermoLayout &l, uint8_t *blob);
// validate_any for all four versions.  Versions 1 and 2: as validate_any, and refused when the handle has the section.
// Versions 3 and 4: the version-1 / 2 part as there, then this extension: n_bytes holds its fixed fields; its shape is one a
// handle can have; n_bytes against the size it implies; its checksum; n, n_red, the binner's on / E / L / cap, T_hash and
// U_s against `ht` (the first that differs is named); the range of T.  0 and *blob / *mblob / *tblob filled, or -1 and *why.
int validate_all(const uint8_t *buf, size_t n_bytes, const Shape &handle, const Momenta &hm, const Thermo &ht, Shape *blob,
                 Momenta *mblob, Thermo *tblob, std::string *why);

// ---- format versions 5 - 8: the version 1 - 4 blob, its version field raised by 4, then an extension for the response
// binners (DQMC_BIN_RESPONSE_*).  A handle with none of them enabled writes versions 1 - 4 unchanged.
//   i32 n_ch, K, K_cc, pad   N_RESP x (i32 on, E, L, pad, i64 cap, T)   F [K K n_ch doubles]
//   xs, x2, c of every enabled response binner   u64 FNV-1a 64 of every extension byte in front of it
enum { N_RESP = 3 };  // DQMC_BIN_RESPONSE_PAIRING, _PAIRING_SUSCEPTIBILITY, _CURRENT
static const uint32_t VERSION_RESPONSE_STEP = 4;  // version = the version without the binners + 4
struct Response {
    int32_t n_ch = 0, K = 0, K_cc = 0;
    const double *F = nullptr;  // K K n_ch doubles, borrowed (nullptr in what validate_full hands back)
    Shape::Bin bin[N_RESP] = {};
    bool any() const { return bin[0].on || bin[1].on || bin[2].on; }  // false: the blob is version 1 - 4
};
// byte offsets from the start of the blob; with !r.any() only `start` and `total` are set, both to the version 1 - 4 size
struct ResponseLayout {
    size_t start, F;
    size_t bin_xs[N_RESP], bin_x2[N_RESP], bin_c[N_RESP];
    size_t checksum, total;
};
bool response_layout(const Shape &s, const Momenta &m, const Thermo &t, const Response &r, ResponseLayout *out,
                     std::string *why = nullptr);
// write_header with the version the four call for (r.any(): 5 - 8, else as write_header(s, m, t, out))
void write_header(const Shape &s, const Momenta &m, const Thermo &t, const Response &r, uint8_t *out);
// the extension's fixed fields and F into blob + l.start (nothing when !r.any()); seal_response once the binner arrays are in place
void write_response(const Response &r, const ResponseLayout &l, uint8_t *blob);
void seal_response(const ResponseLayout &l, uint8_t *blob);
// validate_all for all eight versions.  Versions 1 - 4: as validate_all, and refused when the handle has a response binner
// enabled.  Versions 5 - 8: the version 1 - 4 part as there, then this extension: n_bytes holds its fixed fields; its shape
// is one a handle can have; n_bytes against the size it implies; its checksum; n_ch, K, K_cc and every binner's on / E / L /
// cap against `hr` (the first that differs is named); F byte for byte against hr's; the ranges of T.  0 and *blob / *mblob
// / *tblob / *rblob filled, or -1 and *why.
int validate_full(const uint8_t *buf, size_t n_bytes, const Shape &handle, const Momenta &hm, const Thermo &ht,
                  const Response &hr, Shape *blob, Momenta *mblob, Thermo *tblob, Response *rblob, std::string *why);

// compress / decompress of one walker's field (HubbardModel.jl:56-59): element i of conf (+1 / -1) in bit i % 64 of chunk i / 64
void pack_conf(const int8_t *conf, size_t n, uint8_t *chunks_le);
void unpack_conf(const uint8_t *chunks_le, size_t n, int8_t *conf);

}  // namespace dqmc_blob
#endif
