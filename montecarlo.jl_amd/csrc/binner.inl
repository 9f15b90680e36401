// binner.inl — host side of the logarithmic binners (binner.hip; ABI in include/dqmc_hip.h "error bars"), included by
// engine.cpp.  A binner keeps T, the number of pushes so far: count[level] = T >> level for every (walker, element), so
// no count lives on the device; the cascade length of a push (trailing 1-bits of T) is a kernel argument.

static const int64_t BIN_DEFAULT_CAPACITY = 100000;  // BinningAnalysis' _default_capacity

#define BIN_OK(h, which)                                                                        \
    if ((which) < DQMC_BIN_GREENS || (which) >= DQMC_BIN_RESPONSE_END)                           \
        return fail((h), DQMC_ERR_INVALID, "binner section out of range");                      \
    if (!(h)->bin[(which)].on) return fail((h), DQMC_ERR_STATE, "this section's binner is not enabled")

// DQMC_BIN_* numbers the measurement sections as DQMC_RED_* does (dqmc_handle::sec), except that DQMC_BIN_USER = 4, which
// has no accumulator, sits in front of DQMC_BIN_TIME_DISPLACED = 5 (DQMC_RED_TIME_DISPLACED = 4)
static const dqmc_handle::Section &binner_section(dqmc_handle *h, int which)
{
    return h->sec[which == DQMC_BIN_TIME_DISPLACED ? DQMC_RED_TIME_DISPLACED : which];
}
// elements of a section as its measurement is configured now (0: not configured)
static long binner_section_elements(dqmc_handle *h, int which)
{
    // (the user binner, the sign binners and the momentum binners have no accumulator section, and the thermodynamics
    // binner's length follows sign weighting: a change of what they depend on frees or re-creates them where it is made)
    return which == DQMC_BIN_USER || which >= DQMC_BIN_SIGN ? h->bin[which].E : binner_section(h, which).bin_E;
}
// the binner of the signs that go with a measurement section's pushes: DQMC_BIN_SIGN + the section's DQMC_RED_* index
static int binner_sign_of(int which) { return DQMC_BIN_SIGN + (which == DQMC_BIN_TIME_DISPLACED ? DQMC_RED_TIME_DISPLACED : which); }
static int binner_levels(int64_t capacity)  // ceil(log2(capacity + 1))
{
    int L = 1;
    while (((int64_t)1 << L) < capacity + 1) ++L;
    return L;
}
static void binner_free(dqmc_handle *h, dqmc_handle::Binner &b)
{
    for (double **p : {&b.xs, &b.x2, &b.c, &b.out}) dfree(h, p);
    b = dqmc_handle::Binner{};
}
static int binner_alloc(dqmc_handle *h, int which, long E, int64_t capacity)
{
    if (capacity < 0) return fail(h, DQMC_ERR_INVALID, "binner capacity must be positive (0 selects 100000)");
    if (capacity == 0) capacity = BIN_DEFAULT_CAPACITY;
    if (capacity > ((int64_t)1 << 40)) return fail(h, DQMC_ERR_INVALID, "binner capacity above 2^40");
    if (E < 1 || E > 0x7fffffffL) return fail(h, DQMC_ERR_INVALID, "binner element count out of range");
    dqmc_handle::Binner &b = h->bin[which];
    HIPCHK(hipStreamSynchronize(h->stream));
    binner_free(h, b);
    const int L = binner_levels(capacity);
    const size_t we = (size_t)h->W * (size_t)E;
    int rc = dalloc(h, &b.xs, (size_t)L * we);
    if (!rc) rc = dalloc(h, &b.x2, (size_t)L * we);
    if (!rc) rc = dalloc(h, &b.c, (size_t)(L - 1) * we);
    if (!rc) rc = dalloc(h, &b.out, 8 * (size_t)E + 1);
    if (rc) {
        binner_free(h, b);
        return rc;
    }
    b.on = true;
    b.E = (int)E;
    b.L = L;
    b.cap = capacity;
    b.T = 0;
    return DQMC_OK;
}
static int binner_room(dqmc_handle *h, int which)
{
    const dqmc_handle::Binner &b = h->bin[which];
    if (!b.on) return 0;
    if (b.E != binner_section_elements(h, which))
        return fail(h, DQMC_ERR_STATE, "the section's layout has changed since dqmc_binner_enable: enable it again");
    if (b.T >= b.cap) return fail(h, DQMC_ERR_STATE, "binner capacity exhausted");  // the reference: OverflowError
    return 0;
}
static int binner_push(dqmc_handle *h, int which, const BinPush &p)
{
    dqmc_handle::Binner &b = h->bin[which];
    int lmax = 0;
    while ((b.T >> lmax) & 1) ++lmax;
    if (lmax >= b.L) return fail(h, DQMC_ERR_STATE, "binner capacity exhausted");
    Timed t(h, DQMC_K_MISC);
    HIPCHK(launch_binner_push(p, h->W, b.E, b.L, lmax, b.xs, b.x2, b.c, h->stream));
    b.T += 1;
    return 0;
}
static int binner_push_section(dqmc_handle *h, int which)
{
    BinPush p;
    p.G = h->tmp2;  // the true G of every unit, as the measurement kernels have just read it
    p.stride_unit = h->nn;
    p.n = h->n;
    p.nb = h->nb;
    p.model = h->p.model_kind;
    p.n_dirs = h->n_dirs;
    p.mode = binner_section(h, which).bin_mode;
    p.src = binner_section(h, which).per_walker;
    // finish!: * delta_tau as sus_reduce_kernel (the time-displaced rows go as tdm.hip stored them)
    if (which == DQMC_BIN_SUSCEPTIBILITIES) p.scale = h->p.delta_tau;
    if (!h->sign_on) return binner_push(h, which, p);
    // sign weighting: s_w x for the sources that read G (the per_walker ones are signed already), and s_w itself into
    // the section's sign binner, which has the section's capacity and push count
    p.sw = h->sign_sw;
    CHK(binner_push(h, which, p));
    BinPush q;
    q.src = h->sign_sw;
    return binner_push(h, binner_sign_of(which), q);
}
static int binner_reset(dqmc_handle *h)
{
    for (auto &b : h->bin) {
        if (!b.on) continue;
        const size_t we = (size_t)h->W * (size_t)b.E * sizeof(double);
        HIPCHK(hipMemsetAsync(b.xs, 0, b.L * we, h->stream));
        HIPCHK(hipMemsetAsync(b.x2, 0, b.L * we, h->stream));
        if (b.L > 1) HIPCHK(hipMemsetAsync(b.c, 0, (b.L - 1) * we, h->stream));
        b.T = 0;
    }
    return 0;
}
static int binner_reliable(const dqmc_handle::Binner &b)  // the last level with count >= 32, else 0
{
    int lv = 0;
    for (int l = 0; l < b.L; ++l)
        if ((b.T >> l) >= 32) lv = l;
    return lv;
}
// runs binner_finish_kernel into b.out; level < 0 selects the reliable level
static int binner_finish_device(dqmc_handle *h, int which, int32_t level)
{
    dqmc_handle::Binner &b = h->bin[which];
    if (level >= b.L) return fail(h, DQMC_ERR_INVALID, "binner level out of range");
    if (level < 0) level = binner_reliable(b);
    Timed t(h, DQMC_K_MISC);
    HIPCHK(launch_binner_finish(h->W, b.E, (long)b.T, level, b.xs, b.x2, b.out, h->stream));
    return 0;
}

static int mom_enable(dqmc_handle *h, int which, int64_t capacity);  // momentum.inl
static int thermo_enable(dqmc_handle *h, int64_t capacity);          // thermo.inl
static int resp_enable(dqmc_handle *h, int which, int64_t capacity); // response.inl
int dqmc_binner_enable(dqmc_handle *h, int32_t which, int64_t capacity)
{
    ENTER(h);
    if (which >= DQMC_BIN_MOMENTUM_CORRELATIONS && which < DQMC_BIN_MOMENTUM_END) return mom_enable(h, which, capacity);
    if (which == DQMC_BIN_THERMODYNAMICS) return thermo_enable(h, capacity);
    if (which >= DQMC_BIN_RESPONSE_PAIRING && which < DQMC_BIN_RESPONSE_END) return resp_enable(h, which, capacity);
    if (which < DQMC_BIN_GREENS || which == DQMC_BIN_USER || which > DQMC_BIN_TIME_DISPLACED)
        return fail(h, DQMC_ERR_INVALID, "dqmc_binner_enable takes a measurement section (dqmc_binner_user_create makes the user "
                                         "binner, the sign binners come with their sections)");
    if (which == DQMC_BIN_TIME_DISPLACED) {
        NEED_PREPARED(h);
        if (!h->td.every) return fail(h, DQMC_ERR_STATE, "call dqmc_set_time_displaced first");
    }
    if (which == DQMC_BIN_SUSCEPTIBILITIES) {  // its layout needs the unequal-time stack
        NEED_UT(h);
        if (!h->n_dirs) return fail(h, DQMC_ERR_STATE, "call dqmc_set_pair_directions first");
        CHK(ut_sus_layout(h));
    }
    const long E = binner_section_elements(h, which);
    if (!E) return fail(h, DQMC_ERR_STATE, "configure the section's measurement (pair directions / local targets) first");
    CHK(binner_alloc(h, which, E, capacity));
    if (h->sign_on) CHK(binner_alloc(h, binner_sign_of(which), 1, h->bin[which].cap));
    return DQMC_OK;
}
int dqmc_binner_user_create(dqmc_handle *h, int64_t n_elements, int64_t capacity)
{
    ENTER(h);
    if (n_elements < 1) return fail(h, DQMC_ERR_INVALID, "n_elements must be positive");
    return binner_alloc(h, DQMC_BIN_USER, (long)n_elements, capacity);
}
int dqmc_binner_user_push(dqmc_handle *h, const double *device_samples)
{
    ENTER(h);
    BIN_OK(h, DQMC_BIN_USER);
    if (!device_samples) return fail(h, DQMC_ERR_INVALID, "device_samples is NULL");
    CHK(binner_room(h, DQMC_BIN_USER));
    BinPush p;
    p.src = device_samples;
    CHK(binner_push(h, DQMC_BIN_USER, p));
    HIPCHK(hipStreamSynchronize(h->stream));  // the caller's buffer is free again on return
    return DQMC_OK;
}
int dqmc_binner_size(dqmc_handle *h, int32_t which, size_t *n_elements, int32_t *n_levels, int64_t *n_pushed)
{
    if (!h) return DQMC_ERR_INVALID;
    BIN_OK(h, which);
    const dqmc_handle::Binner &b = h->bin[which];
    if (n_elements) *n_elements = (size_t)b.E;
    if (n_levels) *n_levels = b.L;
    if (n_pushed) *n_pushed = b.T;
    return DQMC_OK;
}
int dqmc_binner_reliable_level(dqmc_handle *h, int32_t which, int32_t *level)
{
    if (!h || !level) return DQMC_ERR_INVALID;
    BIN_OK(h, which);
    *level = binner_reliable(h->bin[which]);
    return DQMC_OK;
}
int dqmc_binner_get_level(dqmc_handle *h, int32_t which, int32_t walker, int32_t level, double *x_sum, double *x2_sum,
                          int64_t *count)
{
    ENTER(h);
    BIN_OK(h, which);
    WALKER_OK(h, walker);
    const dqmc_handle::Binner &b = h->bin[which];
    if (level < 0 || level >= b.L) return fail(h, DQMC_ERR_INVALID, "binner level out of range");
    const size_t off = ((size_t)level * h->W + walker) * (size_t)b.E;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (x_sum) HIPCHK(hipMemcpy(x_sum, b.xs + off, b.E * sizeof(double), hipMemcpyDeviceToHost));
    if (x2_sum) HIPCHK(hipMemcpy(x2_sum, b.x2 + off, b.E * sizeof(double), hipMemcpyDeviceToHost));
    if (count) *count = b.T >> level;
    return DQMC_OK;
}
int dqmc_binner_finish(dqmc_handle *h, int32_t which, int32_t level, double *mean, double *std_error,
                       double *std_error_walkers, double *tau)
{
    ENTER(h);
    BIN_OK(h, which);
    CHK(binner_finish_device(h, which, level));
    const dqmc_handle::Binner &b = h->bin[which];
    HIPCHK(hipStreamSynchronize(h->stream));
    double *dst[4] = {mean, std_error, std_error_walkers, tau};
    for (int q = 0; q < 4; ++q)
        if (dst[q]) HIPCHK(hipMemcpy(dst[q], b.out + (size_t)q * b.E, b.E * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
int dqmc_binner_export_moments(dqmc_handle *h, int32_t which, int32_t level, void *device_out)
{
    ENTER(h);
    BIN_OK(h, which);
    if (!device_out) return fail(h, DQMC_ERR_INVALID, "device_out is NULL");
    CHK(binner_finish_device(h, which, level));
    const dqmc_handle::Binner &b = h->bin[which];
    HIPCHK(hipMemcpyAsync(device_out, b.out + 4 * (size_t)b.E, (4 * (size_t)b.E + 1) * sizeof(double),
                          hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}
