// mc_blob.h — the checkpoint blob of dqmc_mc_state_* and dqmc_qs_state_* (include/dqmc_hip.h "checkpoint and resume of
// the classical MC flavor"): its header, the record table that places every array of the payload, and the validation of a
// blob against the handle that is to take it.  Plain C++ with no HIP in it, in the manner of state_blob.h: the engines
// (ising.hip, qstate.hip through mc_state.inl) fill a Config from the handle and do the copies; the code here sees bytes
// only, so that it can be built and run under the host sanitizers on its own (tests/test_mc_blob.py).
//
// Every field is little-endian and of fixed width; doubles travel as their IEEE bit pattern.
//   header   u64 magic "DQMCMCS1"   u32 format version (1)   u32 header bytes (fixed part + record table)
//            char[16] dqmc_build_source_hash of the exporting library, zero padded (carried, never checked)
//            the configuration fields of fields(), in that order, each 4 or 8 bytes
//            u32 records   u32 0
//            per record: u32 tag, u32 element bytes, u64 elements, u64 byte offset from the start of the blob
//   payload  the records' arrays in the order of the table, each 8-byte aligned
//   u64      FNV-1a 64 (dqmc_blob::fnv1a64) of every byte in front of it
// layout() is the one place that decides which records a configuration has and where they lie: export writes the table it
// returns, and validate() refuses a blob whose table is not the one layout() gives for the blob's own configuration.
#ifndef DQMC_MC_BLOB_H
#define DQMC_MC_BLOB_H
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "state_blob.h"

namespace mc_blob {

static const uint64_t MAGIC = 0x3153434d434d5144ull;  // the bytes "DQMCMCS1", read as one little-endian word
static const uint32_t VERSION = 1;
enum { HASH_BYTES = 16 };
enum Kind { KIND_ISING = 0, KIND_QSTATE = 1 };
enum { N_SEC = 3,  // the binner sections: main, FSS (Ising) / scaling (q-state), stiffness (q-state)
       SEC_MAIN = 0, SEC_SCALING = 1, SEC_STIFFNESS = 2 };
enum { MAX_K = 8, ST_DIRS = 4, ST_CLASSES = 8 };  // rows of the [8][W] S(k) sums and of the [4][W], [8][W] stiffness arrays

// How the handle is configured.  Every field must agree between the blob and the importing handle.
struct Config {
    char source_hash[HASH_BYTES];  // carried, never checked
    int32_t kind, n_sites, z, q, n_walkers, series_capacity, n_bonds;  // q: 0 for the Ising engine
    int32_t update_kind, n_colours;       // Ising: DQMC_MC_UPDATE_*, colours 0 while sequential; q-state: 1, C
    int32_t cluster_rate;                 // Ising: the global rate; q-state: the cluster rate; 0 = off
    int32_t exchange_R, exchange_rate;
    int32_t n_k;                          // wave vectors of FSS (Ising, -1 = off) / scaling (q-state, 0 = off)
    int32_t n_dir, n_classes;             // stiffness (q-state), 0 = off
    struct Bin {
        int32_t on, L, n_elem, n_pairs, n_comp;
        int64_t cap;
    } bin[N_SEC];
    // FNV-1a 64 of the tables the chains depend on (0: the handle has no such table)
    uint64_t hash_neighs, hash_bonds, hash_energy, hash_order, hash_twist, hash_colouring, hash_betas, hash_phases,
        hash_stiffness;
};

// one configuration field as the header carries it and as validate() names it
struct Field {
    const char *name;
    size_t offset;  // in Config
    int bytes;      // 4 (int32) or 8 (int64 / uint64)
};
const Field *fields(size_t *n);

enum Tag : uint32_t {
    TAG_CONF = 1,        // Ising: u32 [nw][W] bit-packed words; q-state: u8 [W][4 Nw] byte states
    TAG_KEY,             // u64 [W]: the Philox key of every walker
    TAG_CURSOR_SWEEP,    // u64 [W]: Ising: the draw cursor of the sequential sweep; q-state: sweeps drawn
    TAG_CURSOR_CONF,     // u64 [W]: q-state: configurations drawn (host)
    TAG_CURSOR_CLUSTER,  // u64 [W]: Wolff / cluster moves drawn
    TAG_CURSOR_CB,       // u64 [W]: Ising: checkerboard sweeps drawn
    TAG_E,               // Ising: i32 [W]; q-state: i64 [W] E_int
    TAG_M,               // Ising: i32 [W]
    TAG_MX,              // q-state: i64 [W]
    TAG_MY,
    TAG_SUM_E,           // f64 [W] each
    TAG_SUM_E2,
    TAG_SUM_M,
    TAG_SUM_M2,
    TAG_SUM_M4,          // q-state
    TAG_N_MEAS,          // i64 [W] each
    TAG_PROP,
    TAG_ACC,
    TAG_N_SERIES,
    TAG_SERIES_A,        // Ising: i32 [cap][W] E; q-state: i64 [W][cap][3]
    TAG_SERIES_B,        // Ising: i32 [cap][W] |M|
    TAG_G_PROP,          // i64 [W] each: cluster moves, moves with |C| > 1, sum of |C|
    TAG_G_ACC,
    TAG_G_SUM,
    TAG_X_REPLICA,       // i32 [W] (exchange_R >= 2 only, as the next two)
    TAG_X_PROP,          // i64 [W]
    TAG_X_ACC,
    TAG_K_SUM_M4,        // f64 [W]: Ising FSS
    TAG_K_SUM_S,         // f64 [8][W]
    TAG_K_N_MEAS,        // i64 [W]
    TAG_ST_SUM_T,        // f64 [4][W] each
    TAG_ST_SUM_J,
    TAG_ST_SUM_J2,
    TAG_ST_N_MEAS,       // i64 [W]
    TAG_ST_LAST_I,       // i64 [8][W] each
    TAG_ST_LAST_K,
    TAG_HOST,            // u64 [N_SEC + 1]: T of every binner section, the exchange cursor
    TAG_BIN = 64         // TAG_BIN + 4 section + {0: xs, 1: x2, 2: xy, 3: c}: f64 arrays of an enabled section
};
enum { HOST_WORDS = N_SEC + 1 };

struct Record {
    uint32_t tag, elem_bytes;
    uint64_t count, offset;
};

struct Layout {
    std::vector<Record> rec;
    size_t header, checksum, total;  // bytes of the header with its table; offset of the checksum; size of the blob
    const Record *find(uint32_t tag) const
    {
        for (const Record &r : rec)
            if (r.tag == tag) return &r;
        return nullptr;
    }
};

// false if the configuration is not one a handle can have (a count outside its range)
bool layout(const Config &c, Layout *out, std::string *why = nullptr);
// l.header bytes into `out`
void write_header(const Config &c, const Layout &l, uint8_t *out);
// the checksum into blob + l.checksum, once the payload is in place
void seal(const Layout &l, uint8_t *blob);
// Everything an import checks before its first write, in this order: the buffer holds a header; magic; format version;
// the size the header implies (and its record table) against n_bytes; the checksum; every configuration field against
// `handle` (the first that differs is named); the ranges of the state: every T <= capacity, n_series <= capacity, q-state
// bytes < q with zero padding behind site N, Ising padding bits zero, replica labels a permutation within each ladder.
// 0 and *l filled with the blob's layout, or -1 and *why set.
int validate(const uint8_t *buf, size_t n_bytes, const Config &handle, Layout *l, std::string *why);

// FNV-1a 64 of two hashes in order: how the hash of a pair of tables is formed
uint64_t hash_pair(uint64_t a, uint64_t b);

}  // namespace mc_blob
#endif
