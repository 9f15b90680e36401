// mc_host.h — the host layer under the two engines of the classical MC flavor (ising.hip: dqmc_mc_*, qstate.hip:
// dqmc_qs_*): what a handle is made of, how it reports errors, owns device memory and moves single values, and the
// binner sections.  Each engine keeps its kernels, its DevState, its launches and its create / sweep bodies.
// Everything here is static: a translation unit that includes it gets its own copy, and with it its own string for
// errors without a handle, so a failed dqmc_qs_create never shows under dqmc_mc_last_error(NULL).
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/dqmc_hip.h"
#include "mc_bin_device.h"
#include "mc_blob.h"
#include "mc_tables.h"

struct mc_handle_base {
    int W = 0, device = 0;  // walkers; the per-walker arrays are [row][W]
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;
    std::string err;
};

// FNV-1a 64 of a table, as the checkpoint blob's header carries it (mc_blob.h)
template <typename T>
static uint64_t mc_hash(const T *p, size_t count)
{
    return dqmc_blob::fnv1a64(p, count * sizeof(T));
}
template <typename T>
static uint64_t mc_hash(const std::vector<T> &v)
{
    return mc_hash(v.data(), v.size());
}

static thread_local std::string g_mc_null_error;  // what *_last_error(NULL) answers: create errors, null handles

static int mc_fail(mc_handle_base *h, int code, const std::string &msg)
{
    if (h) h->err = msg;
    else g_mc_null_error = msg;
    return code;
}

static const char *mc_last_error(const mc_handle_base *h) { return h ? h->err.c_str() : g_mc_null_error.c_str(); }

// (in a function whose handle is `h`)
#define MCHK(expr)                                                                          \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return mc_fail(h, DQMC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// zeroed device memory that the handle owns
template <typename T>
static int mc_alloc(mc_handle_base *h, T **p, size_t count)
{
    void *q = nullptr;
    MCHK(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
    h->allocs.push_back(q);
    MCHK(hipMemsetAsync(q, 0, (count ? count : 1) * sizeof(T), h->stream));
    *p = (T *)q;
    return 0;
}

template <typename T>
static void mc_release(mc_handle_base *h, T *&p)  // hipFree of one of the handle's allocations
{
    if (!p) return;
    for (size_t i = 0; i < h->allocs.size(); ++i)
        if (h->allocs[i] == (void *)p) {
            h->allocs.erase(h->allocs.begin() + i);
            break;
        }
    (void)hipFree(p);
    p = nullptr;
}

static int mc_walker(mc_handle_base *h, int32_t w, const char *fn)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, std::string(fn) + ": null handle");
    if (w < 0 || w >= h->W) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": walker out of range");
    return 0;
}

// one element of a [row][W] device array
template <typename T>
static int mc_put(mc_handle_base *h, T *base, int row, int w, T v)
{
    MCHK(hipMemcpyAsync(base + (size_t)row * h->W + w, &v, sizeof(T), hipMemcpyHostToDevice, h->stream));
    MCHK(hipStreamSynchronize(h->stream));
    return 0;
}

template <typename T>
static int mc_get(mc_handle_base *h, const T *base, int row, int w, T *v)
{
    MCHK(hipMemcpyAsync(v, base + (size_t)row * h->W + w, sizeof(T), hipMemcpyDeviceToHost, h->stream));
    MCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- create and destroy
static int mc_check_device(const std::string &fn, int device_id)  // before there is a handle
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return mc_fail(nullptr, DQMC_ERR_NO_DEVICE, fn + ": no HIP device visible");
    if (device_id < 0 || device_id >= ndev) return mc_fail(nullptr, DQMC_ERR_INVALID, fn + ": device_id out of range");
    return 0;
}

static int mc_open(mc_handle_base *h, const std::string &fn)  // the handle's device and a stream of its own
{
    if (hipSetDevice(h->device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
        return mc_fail(h, DQMC_ERR_HIP, fn + ": cannot open the device");
    return 0;
}

template <typename H>
static int mc_destroy(H *h)
{
    if (!h) return DQMC_OK;
    if (h->stream) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
    }
    for (void *p : h->allocs) (void)hipFree(p);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return DQMC_OK;
}

// a create gives up: the handle's message moves to where *_last_error(NULL) finds it
template <typename H>
static int mc_bail(H *h, int rc)
{
    g_mc_null_error = h->err;
    mc_destroy(h);
    return rc;
}

// ---- a section of the logarithmic binner: per level n_elem sums x_sum and x2_sum, n_pairs cross sums xy_sum and (below
// the last level) n_comp compressor values, each [W]: [L][n_elem][W] twice, [L][n_pairs][W], [L - 1][n_comp][W].
// count[level] = T >> level for every walker, so no count lives on the device.
struct mc_bin_section {
    int n_elem = 0, n_pairs = 0, n_comp = 0, L = 0;
    int64_t T = 0;  // pushes
    double *xs = nullptr, *x2 = nullptr, *xy = nullptr, *c = nullptr;  // xs == nullptr: the section is not there

    void free(mc_handle_base *h)
    {
        for (double **p : {&xs, &x2, &xy, &c}) mc_release(h, *p);
        *this = mc_bin_section{};
    }
    int alloc(mc_handle_base *h, int elems, int pairs, int comps, int levels)  // empty, or freed with the error kept
    {
        free(h);
        n_elem = elems, n_pairs = pairs, n_comp = comps, L = levels;
        const size_t W = h->W;
        int rc = 0;
        if ((rc = mc_alloc(h, &xs, (size_t)L * n_elem * W)) || (rc = mc_alloc(h, &x2, (size_t)L * n_elem * W)) ||
            (rc = mc_alloc(h, &xy, (size_t)L * n_pairs * W)) || (rc = mc_alloc(h, &c, (size_t)(L - 1) * n_comp * W)))
            free(h);
        return rc;
    }
    int clear(mc_handle_base *h)
    {
        T = 0;
        if (!xs) return 0;
        const size_t W = h->W;
        MCHK(hipMemsetAsync(xs, 0, (size_t)L * n_elem * W * 8, h->stream));
        MCHK(hipMemsetAsync(x2, 0, (size_t)L * n_elem * W * 8, h->stream));
        MCHK(hipMemsetAsync(xy, 0, (size_t)L * n_pairs * W * 8, h->stream));
        if (L > 1) MCHK(hipMemsetAsync(c, 0, (size_t)(L - 1) * n_comp * W * 8, h->stream));
        return 0;
    }
    // x_sum, x2_sum (n_elem each) and xy_sum (n_pairs) of one level of one walker; a null pointer is skipped
    int get_level(mc_handle_base *h, int walker, int level, double *oxs, double *ox2, double *oxy) const
    {
        const size_t W = h->W, pitch = W * sizeof(double);
        MCHK(hipSetDevice(h->device));
        if (oxs)
            MCHK(hipMemcpy2DAsync(oxs, 8, xs + (size_t)level * n_elem * W + walker, pitch, 8, n_elem, hipMemcpyDeviceToHost,
                                  h->stream));
        if (ox2)
            MCHK(hipMemcpy2DAsync(ox2, 8, x2 + (size_t)level * n_elem * W + walker, pitch, 8, n_elem, hipMemcpyDeviceToHost,
                                  h->stream));
        if (oxy)
            MCHK(hipMemcpy2DAsync(oxy, 8, xy + (size_t)level * n_pairs * W + walker, pitch, 8, n_pairs, hipMemcpyDeviceToHost,
                                  h->stream));
        MCHK(hipStreamSynchronize(h->stream));
        return 0;
    }
    int next_lmax(mc_handle_base *h, const char *fn, int *lmax) const  // the level the next push stops at
    {
        *lmax = mc_tables::bin_lmax(T);
        if (*lmax >= L) return mc_fail(h, DQMC_ERR_STATE, std::string(fn) + ": binner capacity exhausted");
        return 0;
    }
    // the section as the kernel of the next push sees it (out->xs == nullptr: the section is not there), and that push done
    int push_arg(mc_handle_base *h, const char *fn, mc_bin_arg *out) const
    {
        *out = mc_bin_arg{};
        if (!xs) return 0;
        int lmax = 0;
        if (int rc = next_lmax(h, fn, &lmax)) return rc;
        *out = mc_bin_arg{xs, x2, xy, c, lmax, L - 1};
        return 0;
    }
    void pushed()
    {
        if (xs) T += 1;
    }
    // the bodies of the *_binner_get_level and *_binner_finish calls (level < 0 in finish: the reliable level)
    int level_sums(mc_handle_base *h, const char *fn, int walker, int level, double *oxs, double *ox2, double *oxy,
                   int64_t *count) const
    {
        if (level < 0 || level >= L) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": level out of range");
        if (int rc = get_level(h, walker, level, oxs, ox2, oxy)) return rc;
        if (count) *count = T >> level;
        return 0;
    }
    int finish(mc_handle_base *h, const char *fn, int walker, int level, bool pairs_from_first, double *mean, double *varN,
               double *varN0, double *tau, double *covN, int64_t *count, int32_t *level_used) const
    {
        if (level >= L) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": level out of range");
        if (level < 0) level = mc_tables::bin_reliable(T, L);
        std::vector<double> s((size_t)4 * n_elem + n_pairs);
        double *xs0 = s.data(), *x20 = xs0 + n_elem, *xsl = x20 + n_elem, *x2l = xsl + n_elem, *xyl = x2l + n_elem;
        if (int rc = get_level(h, walker, 0, xs0, x20, nullptr)) return rc;
        if (int rc = get_level(h, walker, level, xsl, x2l, xyl)) return rc;
        mc_tables::bin_finish(n_elem, n_pairs, pairs_from_first, T, level, xs0, x20, xsl, x2l, xyl, mean, varN, varN0, tau,
                              covN);
        *count = T >> level;
        *level_used = level;
        return 0;
    }
};

// ---- the binner of a handle H: h->bin is the main section with `on` and `cap` (the capacity, shared by all sections),
// and h->sections() lists every section once, in the order of the checkpoint blob's SEC_* (mc_blob.h).  A new section is
// added to that list and to the engine's *_bin_alloc; everything below, and the checkpoint (mc_state.inl), follows.
static const int64_t MC_BIN_DEFAULT_CAPACITY = 100000;  // BinningAnalysis' _default_capacity

// (in a function whose handle is `h`)
#define MC_BIN_OK(h, fn)                                                                     \
    if (!(h)) return mc_fail(nullptr, DQMC_ERR_INVALID, std::string(fn) + ": null handle"); \
    if (!(h)->bin.on) return mc_fail((h), DQMC_ERR_STATE, std::string(fn) + ": the binner is not enabled")

template <typename H>
static void mc_bin_free(H *h)  // every section; the binner is off afterwards
{
    for (mc_bin_section *s : h->sections()) s->free(h);
    h->bin.on = false;
    h->bin.cap = 0;
}

template <typename H>
static int mc_bin_clear(H *h)
{
    for (mc_bin_section *s : h->sections())
        if (int rc = s->clear(h)) return rc;
    return 0;
}

// the head of *_binner_enable: the capacity as it will be used (0 selects the default)
template <typename H>
static int mc_binner_capacity(H *h, const char *fn, int64_t *capacity)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, std::string(fn) + ": null handle");
    if (*capacity < 0) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": capacity must be positive (0 selects 100000)");
    if (*capacity == 0) *capacity = MC_BIN_DEFAULT_CAPACITY;
    if (*capacity > ((int64_t)1 << 40)) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": capacity above 2^40");
    return 0;
}

template <typename H>
static int mc_binner_size(H *h, const char *fn, int32_t *n_levels, int64_t *n_pushed)
{
    MC_BIN_OK(h, fn);
    if (n_levels) *n_levels = h->bin.L;
    if (n_pushed) *n_pushed = h->bin.T;
    return DQMC_OK;
}

template <typename H>
static int mc_binner_reliable_level(H *h, const char *fn, int32_t *level)
{
    MC_BIN_OK(h, fn);
    if (!level) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": null level");
    *level = mc_tables::bin_reliable(h->bin.T, h->bin.L);
    return DQMC_OK;
}

// section `sec` of an enabled binner for a call about `walker`; off: what follows "fn" when the section is not there
// (nullptr for the main section, which is there whenever the binner is)
template <typename H>
static int mc_binner_section(H *h, const char *fn, int sec, const char *off, int32_t walker, const mc_bin_section **s)
{
    MC_BIN_OK(h, fn);
    *s = h->sections()[sec];
    if (off && !(*s)->xs) return mc_fail(h, DQMC_ERR_STATE, std::string(fn) + off);
    return mc_walker(h, walker, fn);
}

template <typename H>
static int mc_binner_get_level(H *h, const char *fn, int sec, const char *off, int32_t walker, int32_t level, double *x_sum,
                               double *x2_sum, double *xy_sum, int64_t *count)
{
    const mc_bin_section *s = nullptr;
    if (int rc = mc_binner_section(h, fn, sec, off, walker, &s)) return rc;
    return s->level_sums(h, fn, walker, level, x_sum, x2_sum, xy_sum, count);
}

// Out: one of the dqmc_*_binned structs.  pairs_from_first: pair k = (element 0, element 1 + k), else (2 k, 2 k + 1)
template <typename H, typename Out>
static int mc_binner_finish(H *h, const char *fn, int sec, const char *off, bool pairs_from_first, int32_t walker,
                            int32_t level, Out *out)
{
    const mc_bin_section *s = nullptr;
    if (int rc = mc_binner_section(h, fn, sec, off, walker, &s)) return rc;
    if (!out) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": null out");
    Out r{};  // (entries past the section's elements stay 0)
    if (int rc = s->finish(h, fn, walker, level, pairs_from_first, r.mean, r.varN, r.varN0, r.tau, r.covN, &r.count, &r.level))
        return rc;
    *out = r;
    return DQMC_OK;
}

// ---- replica exchange: what has one shape in both engines (h->xch: R, rate, cursor, sgn, replica, prop, acc; the pair
// tables and the kernels are the engine's)
template <typename H>
static int mc_exchange_ladders(H *h, const char *fn, int32_t n_replicas, int32_t rate, int *R)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, std::string(fn) + ": null handle");
    if (n_replicas < 0 || rate < 0)
        return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": n_replicas and rate must be >= 0 (0 = off)");
    *R = n_replicas >= 2 ? n_replicas : 0;
    if (*R && h->W % *R != 0)
        return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": n_walkers must be a multiple of n_replicas");
    return 0;
}

template <typename H, typename Out>
static int mc_get_exchange_stats(H *h, const char *fn, int32_t walker, Out *out)
{
    if (int rc = mc_walker(h, walker, fn)) return rc;
    if (!out) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": null out");
    MCHK(hipSetDevice(h->device));
    const auto &t = h->xch;
    long long prop = 0, acc = 0;
    int label = 0;
    int rc = 0;
    if (t.sgn && ((rc = mc_get(h, t.prop, 0, walker, &prop)) || (rc = mc_get(h, t.acc, 0, walker, &acc)) ||
                  (rc = mc_get(h, t.replica, 0, walker, &label))))
        return rc;
    out->prop_exchange = prop;
    out->acc_exchange = acc;
    out->replica = label;
    out->rounds = t.cursor;
    return DQMC_OK;
}
