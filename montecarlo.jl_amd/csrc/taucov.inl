// taucov.inl — host side of the tau-tau' covariance accumulators (taucov.hip; ABI in include/dqmc_hip.h "tau-tau'
// covariance"), included by engine.cpp behind momentum.inl.  An accumulator (dqmc_handle::TauCov) keeps, per walker and
// series, the open bin's sum, the shift and the shifted first and second moments of the closed bins' means.  The host
// counts the samples: every walker's bin closes with the same push, so whether a push closes a bin, and whether that bin
// is the first, are launch arguments and nothing is decided on the device.  h->tcov takes the momentum time-displaced
// sample right behind mom_push, h->ucov the caller's samples.

static size_t tcov_doubles(const dqmc_handle *h, const dqmc_handle::TauCov &t)  // W S (R^2 + 3 R)
{
    return (size_t)h->W * (size_t)t.S * ((size_t)t.R * t.R + 3 * (size_t)t.R);
}
// the stream must be idle
static void tcov_free(dqmc_handle *h, dqmc_handle::TauCov &t)
{
    for (double **p : {&t.a, &t.c, &t.s1, &t.s2, &t.sample}) dfree(h, p);
    t = dqmc_handle::TauCov{};
}
static void tcov_off(dqmc_handle *h) { tcov_free(h, h->tcov); }
// (re)creates an accumulator over S series of R values, empty; on a failed allocation it is left off
static int tcov_alloc(dqmc_handle *h, dqmc_handle::TauCov &t, long S, int R, int bin_size)
{
    if (R > TAUCOV_MAX_R) return fail(h, DQMC_ERR_INVALID, "a series of the tau-tau' covariance holds at most 2048 values");
    HIPCHK(hipStreamSynchronize(h->stream));
    tcov_free(h, t);
    const size_t sr = (size_t)h->W * (size_t)S * (size_t)R;
    int rc = dalloc(h, &t.a, sr);
    if (!rc) rc = dalloc(h, &t.c, sr);
    if (!rc) rc = dalloc(h, &t.s1, sr);
    if (!rc) rc = dalloc(h, &t.s2, sr * (size_t)R);
    if (rc) {
        tcov_free(h, t);
        return rc;
    }
    t.bin_size = bin_size; t.S = S; t.R = R;
    return DQMC_OK;
}
static int tcov_clear(dqmc_handle *h, dqmc_handle::TauCov &t)
{
    if (!t.bin_size) return 0;
    const size_t sr = (size_t)h->W * (size_t)t.S * (size_t)t.R * sizeof(double);
    for (double *p : {t.a, t.c, t.s1}) HIPCHK(hipMemsetAsync(p, 0, sr, h->stream));
    HIPCHK(hipMemsetAsync(t.s2, 0, sr * (size_t)t.R, h->stream));
    t.open = t.nb = 0;
    return 0;
}
static int tcov_reset(dqmc_handle *h)
{
    CHK(tcov_clear(h, h->tcov));
    return tcov_clear(h, h->ucov);
}
// the launch arguments every segment of one push shares, and the host's count of it
static TauCovPush tcov_args(dqmc_handle::TauCov &t, const double *X, long x_walker)
{
    TauCovPush p;
    p.X = X; p.x_walker = x_walker;
    p.R = t.R; p.S = t.S;
    p.close = t.open + 1 == t.bin_size;
    p.first = t.nb == 0;
    p.bin_size = (double)t.bin_size;
    p.a = t.a; p.c = t.c; p.s1 = t.s1; p.s2 = t.s2;
    return p;
}
static void tcov_count(dqmc_handle::TauCov &t)
{
    if (++t.open == t.bin_size) {
        t.open = 0;
        t.nb += 1;
    }
}
// one pass's momentum time-displaced sample into h->tcov, on the handle's stream.  The sample is the momentum binner's
// while that is on, else the accumulator's own copy, filled by the same transform.  Its series: (block, q) of the
// [Gl0 C] rows at the front of the sample, then (channel, q) of [CDC][SDCx][SDCy][SDCz] behind the four Green's groups.
static int tcov_push(dqmc_handle *h)
{
    dqmc_handle::TauCov &t = h->tcov;
    const dqmc_handle::Binner &b = h->bin[DQMC_BIN_MOMENTUM_TIME_DISPLACED];
    const long nq = h->mom.n_q, R = t.R;
    const double *X = h->mom.sample[mom_index(DQMC_BIN_MOMENTUM_TIME_DISPLACED)];
    long E = b.E;
    if (!b.on) {
        CHK(mom_fill(h, DQMC_BIN_MOMENTUM_TIME_DISPLACED, t.sample, t.sample_E));
        X = t.sample;
        E = t.sample_E;
    }
    TauCovPush p = tcov_args(t, X, E);
    p.n_q = (int)nq;
    p.j_stride = R * nq;
    p.r_stride = nq;
    Timed tm(h, DQMC_K_MISC);
    if (t.what & DQMC_TD_GREENS) {
        p.x_off = 0; p.series0 = 0; p.n_series = (long)h->nb * nq;
        HIPCHK(launch_taucov_push(p, h->W, h->stream));
    }
    if (t.what & DQMC_TD_DENSITY) {
        p.x_off = (h->td.what & DQMC_TD_GREENS) ? 4L * h->nb * R * nq : 0;
        p.series0 = (t.what & DQMC_TD_GREENS) ? (long)h->nb * nq : 0;
        p.n_series = 4 * nq;
        HIPCHK(launch_taucov_push(p, h->W, h->stream));
    }
    tcov_count(t);
    return DQMC_OK;
}
static int tcov_get(dqmc_handle *h, const dqmc_handle::TauCov &t, int64_t *nb, double *shift, double *S1, double *S2)
{
    if (!t.bin_size) return fail(h, DQMC_ERR_STATE, "the tau-tau' covariance is not enabled");
    const size_t sr = (size_t)h->W * (size_t)t.S * (size_t)t.R * sizeof(double);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (nb)
        for (int w = 0; w < h->W; ++w) nb[w] = t.nb;
    if (shift) HIPCHK(hipMemcpy(shift, t.c, sr, hipMemcpyDeviceToHost));
    if (S1) HIPCHK(hipMemcpy(S1, t.s1, sr, hipMemcpyDeviceToHost));
    if (S2) HIPCHK(hipMemcpy(S2, t.s2, sr * (size_t)t.R, hipMemcpyDeviceToHost));
    return DQMC_OK;
}
static void tcov_plan(const dqmc_handle *h, const dqmc_handle::TauCov &t, int64_t out[5])
{
    for (int i = 0; i < 5; ++i) out[i] = 0;
    if (!t.bin_size) return;
    out[0] = t.bin_size; out[1] = t.S; out[2] = t.R;
    out[3] = (int64_t)((tcov_doubles(h, t) + (size_t)h->W * (size_t)t.sample_E * (t.sample ? 1 : 0)) * sizeof(double));
    out[4] = t.nb;
}

int dqmc_set_tau_covariance(dqmc_handle *h, int32_t bin_size, int32_t what)
{
    ENTER(h);
    if (bin_size == 0) {  // off: as a handle that never enabled it
        HIPCHK(hipStreamSynchronize(h->stream));
        tcov_off(h);
        return DQMC_OK;
    }
    if (bin_size < 0) return fail(h, DQMC_ERR_INVALID, "bin_size must be 0 or positive");
    if (what < 1 || what > (DQMC_TD_GREENS | DQMC_TD_DENSITY))
        return fail(h, DQMC_ERR_INVALID, "what must be a non-empty mask of DQMC_TD_GREENS | DQMC_TD_DENSITY");
    if (!h->mom.n_q) return fail(h, DQMC_ERR_STATE, "call dqmc_set_momenta first");
    if (!h->td.every) return fail(h, DQMC_ERR_STATE, "call dqmc_set_time_displaced first");
    if (what & ~h->td.what) return fail(h, DQMC_ERR_STATE, "dqmc_set_time_displaced does not record these rows");
    if (h->sign_on)
        return fail(h, DQMC_ERR_STATE, "the tau-tau' covariance is not available with sign weighting on");
    dqmc_handle::TauCov &t = h->tcov;
    const long S = (((what & DQMC_TD_GREENS) ? (long)h->nb : 0) + ((what & DQMC_TD_DENSITY) ? 4L : 0)) * h->mom.n_q;
    CHK(tcov_alloc(h, t, S, h->td.R, bin_size));
    t.what = what;
    t.sample_E = mom_elements(h, DQMC_BIN_MOMENTUM_TIME_DISPLACED);
    const int rc = dalloc(h, &t.sample, (size_t)h->W * (size_t)t.sample_E);  // (read while the momentum binner is off)
    if (rc) {
        tcov_off(h);
        return rc;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}
int dqmc_tau_covariance_plan(dqmc_handle *h, int64_t out[5])
{
    if (!h || !out) return DQMC_ERR_INVALID;
    tcov_plan(h, h->tcov, out);
    return DQMC_OK;
}
int dqmc_tau_covariance_get(dqmc_handle *h, int64_t *n_bins, double *shift, double *S1, double *S2)
{
    ENTER(h);
    return tcov_get(h, h->tcov, n_bins, shift, S1, S2);
}
int dqmc_user_covariance(dqmc_handle *h, int64_t n_series, int32_t R, int32_t bin_size)
{
    ENTER(h);
    if (bin_size == 0) {
        HIPCHK(hipStreamSynchronize(h->stream));
        tcov_free(h, h->ucov);
        return DQMC_OK;
    }
    if (bin_size < 0) return fail(h, DQMC_ERR_INVALID, "bin_size must be 0 or positive");
    if (n_series < 1 || n_series > 0x7fffffffL || R < 1)
        return fail(h, DQMC_ERR_INVALID, "n_series and R must be positive");
    CHK(tcov_alloc(h, h->ucov, (long)n_series, R, bin_size));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}
int dqmc_user_covariance_push(dqmc_handle *h, const double *device_samples)
{
    ENTER(h);
    dqmc_handle::TauCov &t = h->ucov;
    if (!t.bin_size) return fail(h, DQMC_ERR_STATE, "call dqmc_user_covariance first");
    if (!device_samples) return fail(h, DQMC_ERR_INVALID, "device_samples is NULL");
    TauCovPush p = tcov_args(t, device_samples, t.S * t.R);  // [W][n_series][R]: series j at j R, r fastest
    p.n_q = 1;
    p.j_stride = t.R;
    p.r_stride = 1;
    p.n_series = t.S;
    {
        Timed tm(h, DQMC_K_MISC);
        HIPCHK(launch_taucov_push(p, h->W, h->stream));
    }
    tcov_count(t);
    HIPCHK(hipStreamSynchronize(h->stream));  // the caller's buffer is free again on return
    return DQMC_OK;
}
int dqmc_user_covariance_plan(dqmc_handle *h, int64_t out[5])
{
    if (!h || !out) return DQMC_ERR_INVALID;
    tcov_plan(h, h->ucov, out);
    return DQMC_OK;
}
int dqmc_user_covariance_get(dqmc_handle *h, int64_t *n_bins, double *shift, double *S1, double *S2)
{
    ENTER(h);
    return tcov_get(h, h->ucov, n_bins, shift, S1, S2);
}
