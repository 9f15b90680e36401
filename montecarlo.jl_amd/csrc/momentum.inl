// momentum.inl — host side of the momentum-space binners (momentum.hip; ABI in include/dqmc_hip.h "momentum-space
// observables"), included by engine.cpp behind binner.inl.  The phase tables of dqmc_set_momenta live on the device; a
// momentum binner is an ordinary Binner over a per-walker sample of its own, h->mom.sample[k], which mom_push fills
// with the transform of the source section's per-walker buffer right before the push.  The sources are read as their own
// binners read them: the correlation pair sums and the time-displaced rows as stored, the susceptibility rows times
// delta_tau; with sign weighting all three have been rewritten in place as s_w x by the signed reduce kernels
// (sign.hip: corr_reduce_signed_kernel, reduce_signed_kernel), so the transform never multiplies by s_w itself.

static int mom_index(int which) { return which - DQMC_BIN_MOMENTUM_CORRELATIONS; }
// elements of a momentum sample as the handle is configured now, without the trailing s_w (0: its source is not configured)
static long mom_elements(const dqmc_handle *h, int which)
{
    const long nq = h->mom.n_q;
    if (!nq) return 0;
    if (which != DQMC_BIN_MOMENTUM_TIME_DISPLACED) return 4 * nq;
    const dqmc_handle::TimeDisplaced &t = h->td;
    if (!t.every) return 0;
    return ((t.what & DQMC_TD_GREENS) ? 4L * h->nb : 0) * t.R * nq + ((t.what & DQMC_TD_DENSITY) ? 4L : 0) * t.R * nq;
}
// the stream must be idle
static void mom_disable(dqmc_handle *h, int which)
{
    if (h->bin[which].on) binner_free(h, h->bin[which]);
    dfree(h, &h->mom.sample[mom_index(which)]);
}
static void mom_off(dqmc_handle *h)
{
    for (int which = DQMC_BIN_MOMENTUM_CORRELATIONS; which < DQMC_BIN_MOMENTUM_END; ++which) mom_disable(h, which);
    for (int which = DQMC_BIN_RESPONSE_PAIRING; which < DQMC_BIN_RESPONSE_END; ++which) resp_disable(h, which);  // they use the tables
    ctd_off(h);  // (and so does the imaginary-time current recording)
    tcov_off(h);  // (and the tau-tau' covariance of the momentum sample)
    dfree(h, &h->mom.cos_d);
    dfree(h, &h->mom.sin_d);
    h->mom.cos_h.clear();
    h->mom.sin_h.clear();
    h->mom.n_q = 0;
}
static int mom_enable(dqmc_handle *h, int which, int64_t capacity)
{
    if (!h->mom.n_q) return fail(h, DQMC_ERR_STATE, "call dqmc_set_momenta first");
    if (which == DQMC_BIN_MOMENTUM_TIME_DISPLACED && !h->td.every)
        return fail(h, DQMC_ERR_STATE, "call dqmc_set_time_displaced first");
    if (which == DQMC_BIN_MOMENTUM_SUSCEPTIBILITIES) {  // its source's layout needs the unequal-time stack
        NEED_UT(h);
        CHK(ut_sus_layout(h));
    }
    const long E = mom_elements(h, which) + (h->sign_on ? 1 : 0);
    CHK(binner_alloc(h, which, E, capacity));  // (waits for the stream)
    double **smp = &h->mom.sample[mom_index(which)];
    dfree(h, smp);
    const int rc = dalloc(h, smp, (size_t)h->W * (size_t)E);
    if (rc) {
        binner_free(h, h->bin[which]);
        return rc;
    }
    return DQMC_OK;
}
// the transform of every walker's source sample into Y [W][y_stride] (y_stride: the sample's elements, with the trailing
// s_w while sign weighting is on): on the handle's stream, behind the source section's kernels
static int mom_fill(dqmc_handle *h, int which, double *Y, long y_stride)
{
    const dqmc_handle::Momenta &m = h->mom;
    const int nd = h->n_dirs, nq = m.n_q;
    MomentumArgs a;
    a.Y = Y;
    a.y_stride = y_stride;
    a.n_dirs = nd;
    a.n_q = nq;
    if (h->sign_on) {  // the first launch also stores s_w behind the sample
        a.sw = h->sign_sw;
        a.sign_at = y_stride - 1;
    }
    {
        Timed t(h, DQMC_K_MISC);
        // one launch per run of source rows that share a table
        auto seg = [&](const double *tab, long x_off, int rows, long y_off) {
            a.tab = tab; a.x_off = x_off; a.rows = rows; a.y_off = y_off;
            const hipError_t e = launch_momentum(a, h->W, h->stream);
            a.sw = nullptr;
            return e;
        };
        if (which == DQMC_BIN_MOMENTUM_CORRELATIONS) {  // [cdc][sdc_x][sdc_y][sdc_z]: four rows
            a.X = h->sec[DQMC_RED_CORRELATIONS].per_walker;
            a.x_stride = 4L * nd;
            HIPCHK(seg(m.cos_d, 0, 4, 0));
        } else if (which == DQMC_BIN_MOMENTUM_SUSCEPTIBILITIES) {  // [cds][sds_x][sds_y][sds_z] in front of ps / ccs
            const dqmc_handle::Section &sus = h->sec[DQMC_RED_SUSCEPTIBILITIES];
            a.X = sus.per_walker;
            a.x_stride = sus.bin_E;
            a.scale = h->p.delta_tau;  // finish!: * delta_tau, as the source's binner takes it
            HIPCHK(seg(m.cos_d, 0, 4, 0));
        } else {
            const dqmc_handle::Section &td = h->sec[DQMC_RED_TIME_DISPLACED];
            const dqmc_handle::TimeDisplaced &t = h->td;
            a.X = td.per_walker;
            a.x_stride = td.bin_E;
            long x_off = 0, y_off = 0;
            if (t.what & DQMC_TD_GREENS) {  // Gl0 then G0l, n_blocks R rows each -> [Gl0 C][Gl0 S][G0l C][G0l S]
                const int rows = h->nb * t.R;
                for (int g = 0; g < 2; ++g) {
                    HIPCHK(seg(m.cos_d, x_off, rows, y_off));
                    HIPCHK(seg(m.sin_d, x_off, rows, y_off + (long)rows * nq));
                    x_off += (long)rows * nd;
                    y_off += 2L * rows * nq;
                }
            }
            if (t.what & DQMC_TD_DENSITY) HIPCHK(seg(m.cos_d, x_off, 4 * t.R, y_off));  // [CDC][SDCx][SDCy][SDCz], R rows each
        }
    }
    return DQMC_OK;
}
// the transform into h->mom.sample, then the push
static int mom_push(dqmc_handle *h, int which)
{
    double *Y = h->mom.sample[mom_index(which)];
    CHK(mom_fill(h, which, Y, h->bin[which].E));
    BinPush p;
    p.src = Y;
    return binner_push(h, which, p);
}

int dqmc_set_momenta(dqmc_handle *h, int32_t n_q, const double *cos_tab, const double *sin_tab)
{
    ENTER(h);
    if (n_q == 0) {  // off: as a handle that never set them
        HIPCHK(hipStreamSynchronize(h->stream));
        mom_off(h);
        return DQMC_OK;
    }
    if (!h->n_dirs) return fail(h, DQMC_ERR_STATE, "call dqmc_set_pair_directions first");
    if (n_q < 0 || n_q > h->n_dirs) return fail(h, DQMC_ERR_INVALID, "n_q must be 0 or 1 .. n_dirs");
    if (!cos_tab || !sin_tab) return fail(h, DQMC_ERR_INVALID, "cos_tab / sin_tab is NULL");
    const size_t cnt = (size_t)h->n_dirs * (size_t)n_q;
    std::vector<double> ch(cos_tab, cos_tab + cnt), sh(sin_tab, sin_tab + cnt);  // (the arguments may be the handle's own copies)
    HIPCHK(hipStreamSynchronize(h->stream));
    mom_off(h);
    CHK(dalloc(h, &h->mom.cos_d, cnt, false));
    CHK(dalloc(h, &h->mom.sin_d, cnt, false));
    HIPCHK(hipMemcpy(h->mom.cos_d, ch.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->mom.sin_d, sh.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
    h->mom.cos_h.swap(ch);
    h->mom.sin_h.swap(sh);
    h->mom.n_q = n_q;
    return DQMC_OK;
}
int dqmc_momenta_plan(dqmc_handle *h, int32_t out[4])
{
    if (!h || !out) return DQMC_ERR_INVALID;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!h->mom.n_q) return DQMC_OK;
    out[0] = h->mom.n_q; out[1] = h->n_dirs; out[2] = 64; out[3] = 64;  // momentum.hip: MT x MT tiles of the sample
    return DQMC_OK;
}
