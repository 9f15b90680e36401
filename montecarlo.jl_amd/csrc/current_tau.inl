// current_tau.inl — host side of the imaginary-time-resolved current-current recording (current_tau.hip; ABI in
// include/dqmc_hip.h "current response in imaginary time"), included by engine.cpp behind entangle.inl.  The reference
// has no such measurement.  Its state is dqmc_handle::CurrentTau, outside dqmc_handle::sec[] like the entanglement
// sums: no DQMC_RED_* section, no binner, nothing in the packed reduction or the state blob.  every == 0: off, nothing
// allocated; dqmc_accumulate_susceptibilities (unequal_time.inl) then takes the path it always took.

// the stream must be idle
static void ctd_off(dqmc_handle *h)
{
    dqmc_handle::CurrentTau &c = h->ctd;
    dfree(h, &c.tab);
    dfree(h, &c.x);
    dfree(h, &c.kb);
    dfree(h, &c.sums);
    c = dqmc_handle::CurrentTau{};
}
// dqmc_reset_accumulators, dqmc_set_sign_weighting: the sums and the three counters
static int ctd_reset(dqmc_handle *h)
{
    const dqmc_handle::CurrentTau &c = h->ctd;
    if (!c.every) return 0;
    HIPCHK(hipMemsetAsync(c.sums, 0, (size_t)h->W * c.P * sizeof(double), h->stream));
    return 0;
}
// row `row` of every walker from the packed tuple (G00 of the pass, G0l, Gl0, Gll): the slice's own ccs sums into the
// zeroed scratch, their transform into the row and, with add_to, their hand-over to the susceptibility sample (Timed by
// the caller)
static int ctd_row(dqmc_handle *h, int row, double cc_fac, const double *g0l, const double *gl0, const double *gll,
                   double *add_to, long add_stride, long add_off)
{
    const dqmc_handle::CurrentTau &c = h->ctd;
    const long rows = (long)c.R * c.K * c.n_q;
    HIPCHK(hipMemsetAsync(c.x, 0, sizeof(double) * h->W * h->n_dirs * c.K, h->stream));
    HIPCHK(launch_cc_slice(h->cc, h->n, h->nb, h->W, cc_fac, cc_fac, g0l, gl0, gll, h->nn, h->dir_ptr, h->pair_src,
                           h->pair_trg, h->n_dirs, c.x, (long)h->n_dirs * c.K, 0, h->stream));
    HIPCHK(launch_current_tau_row(h->n_dirs, c.n_q, c.K, h->W, c.x, c.tab, h->sign_on ? h->sign_sw : nullptr, c.sums,
                                  (long)c.P, (long)row * c.K * c.n_q, rows + (long)row * c.K * c.n_q, add_to, add_stride,
                                  add_off, h->stream));
    return 0;
}
// the end of a recorded pass: kbond of the pass's G00 as DQMC_BIN_RESPONSE_CURRENT takes it, and the counters
static int ctd_finish(dqmc_handle *h, double cc_fac)
{
    const dqmc_handle::CurrentTau &c = h->ctd;
    const double *sw = h->sign_on ? h->sign_sw : nullptr;
    HIPCHK(launch_bond_kinetic(h->n, h->nb, c.K, h->W, cc_fac, h->ut->g00, h->nn, h->cc.trg, h->cc.tts, sw, c.kb, c.K, 0,
                               h->stream));
    HIPCHK(launch_current_tau_finish(c.K, h->W, c.kb, sw, c.sums, (long)c.P, 2L * c.R * c.K * c.n_q, h->stream));
    return 0;
}

int dqmc_set_current_time_displaced(dqmc_handle *h, int32_t every)
{
    ENTER(h);
    if (every == 0) {  // off: as a handle that never recorded
        HIPCHK(hipStreamSynchronize(h->stream));
        ctd_off(h);
        return DQMC_OK;
    }
    if (!h->n_dirs) return fail(h, DQMC_ERR_STATE, "call dqmc_set_pair_directions first");
    if (!h->K_cc) return fail(h, DQMC_ERR_STATE, "call dqmc_set_current_targets first");
    if (!h->mom.n_q) return fail(h, DQMC_ERR_STATE, "call dqmc_set_momenta first");
    NEED_PREPARED(h);
    if (every < 1 || h->M % every != 0) return fail(h, DQMC_ERR_INVALID, "every must be 0 or a positive divisor of slices");
    // ---- nothing has been written up to here ----
    HIPCHK(hipStreamSynchronize(h->stream));
    ctd_off(h);
    dqmc_handle::CurrentTau &c = h->ctd;
    const int nd = h->n_dirs, nq = h->mom.n_q, K = h->K_cc, R = 1 + h->M / every;
    std::vector<double> tab(2 * (size_t)nd * nq);
    for (int d = 0; d < nd; ++d)
        for (int q = 0; q < nq; ++q) {
            tab[2 * ((size_t)d * nq + q)] = h->mom.cos_h[d + (size_t)nd * q];
            tab[2 * ((size_t)d * nq + q) + 1] = h->mom.sin_h[d + (size_t)nd * q];
        }
    const size_t P = 2 * (size_t)R * K * nq + K + 3;
    int rc = dalloc(h, &c.tab, tab.size(), false);
    if (!rc) rc = dalloc(h, &c.x, (size_t)h->W * nd * K);
    if (!rc) rc = dalloc(h, &c.kb, (size_t)h->W * K);
    if (!rc) rc = dalloc(h, &c.sums, (size_t)h->W * P);
    if (rc) {
        ctd_off(h);
        return rc;
    }
    HIPCHK(hipMemcpy(c.tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    c.every = every; c.R = R; c.K = K; c.n_q = nq; c.P = P;
    HIPCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}
int dqmc_current_time_displaced_plan(dqmc_handle *h, int32_t out[4])
{
    if (!h || !out) return DQMC_ERR_INVALID;
    const dqmc_handle::CurrentTau &c = h->ctd;
    out[0] = c.R; out[1] = c.every; out[2] = c.K; out[3] = c.n_q;
    return DQMC_OK;
}
int dqmc_current_time_displaced_size(dqmc_handle *h, size_t *n)
{
    if (!h || !n) return DQMC_ERR_INVALID;
    *n = h->ctd.every ? (size_t)h->W * h->ctd.P : 0;
    return DQMC_OK;
}
int dqmc_get_current_time_displaced(dqmc_handle *h, double *host_out)
{
    ENTER(h);
    const dqmc_handle::CurrentTau &c = h->ctd;
    if (!c.every) return fail(h, DQMC_ERR_STATE, "call dqmc_set_current_time_displaced first");
    if (!host_out) return fail(h, DQMC_ERR_INVALID, "host_out is NULL");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(host_out, c.sums, (size_t)h->W * c.P * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
int dqmc_set_current_time_displaced_sums(dqmc_handle *h, const double *host_in)
{
    ENTER(h);
    const dqmc_handle::CurrentTau &c = h->ctd;
    if (!c.every) return fail(h, DQMC_ERR_STATE, "call dqmc_set_current_time_displaced first");
    if (!host_in) return fail(h, DQMC_ERR_INVALID, "host_in is NULL");
    for (int w = 0; w < h->W; ++w)  // the two counts of every walker
        for (int i = 1; i <= 2; ++i) {
            const double v = host_in[(size_t)w * c.P + c.P - i];
            if (!(v >= 0.0) || !(v < 9e15) || v != std::floor(v))
                return fail(h, DQMC_ERR_INVALID, "dqmc_set_current_time_displaced_sums: the sample counts must be non-negative integers");
        }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(c.sums, host_in, (size_t)h->W * c.P * sizeof(double), hipMemcpyHostToDevice));
    return DQMC_OK;
}
