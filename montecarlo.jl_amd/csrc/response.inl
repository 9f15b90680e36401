// response.inl — host side of the response binners (response.hip, momentum.hip; ABI in include/dqmc_hip.h "pair structure
// factors and superfluid stiffness"), included by engine.cpp behind thermo.inl.  Like a momentum binner, a response binner
// is an ordinary Binner over a per-walker sample of its own, h->rsp.sample[k], which resp_push fills right before the
// push: the pairing sample (equal-time, or the ps part of the susceptibility sample) contracted with the channel table
// into h->rsp.Z and transformed with both phase tables; the ccs rows of the susceptibility sample transformed with both
// tables, followed by the bond kinetic energy of the pass's G00.  With sign weighting the sources are s_w x already.

static int resp_index(int which) { return which - DQMC_BIN_RESPONSE_PAIRING; }
// elements of a response sample as the handle is configured now, without the trailing s_w (0: a source is not configured)
static long resp_elements(const dqmc_handle *h, int which)
{
    const long nq = h->mom.n_q;
    if (!nq) return 0;
    if (which == DQMC_BIN_RESPONSE_CURRENT) return h->K_cc ? 2L * h->K_cc * nq + h->K_cc : 0;
    return h->rsp.n_ch && h->K_loc ? 2L * h->rsp.n_ch * nq : 0;
}
// the stream must be idle
static void resp_disable(dqmc_handle *h, int which)
{
    if (h->bin[which].on) binner_free(h, h->bin[which]);
    dfree(h, &h->rsp.sample[resp_index(which)]);
    if (!h->bin[DQMC_BIN_RESPONSE_PAIRING].on && !h->bin[DQMC_BIN_RESPONSE_PAIRING_SUSCEPTIBILITY].on) dfree(h, &h->rsp.Z);
}
static void resp_channels_off(dqmc_handle *h)
{
    resp_disable(h, DQMC_BIN_RESPONSE_PAIRING);
    resp_disable(h, DQMC_BIN_RESPONSE_PAIRING_SUSCEPTIBILITY);
    dfree(h, &h->rsp.F_d);
    h->rsp.F_h.clear();
    h->rsp.n_ch = 0;
}
static int resp_enable(dqmc_handle *h, int which, int64_t capacity)
{
    const bool current = which == DQMC_BIN_RESPONSE_CURRENT;
    if (!h->mom.n_q) return fail(h, DQMC_ERR_STATE, "call dqmc_set_momenta first");
    if (current && !h->K_cc) return fail(h, DQMC_ERR_STATE, "call dqmc_set_current_targets first");
    if (!current && !h->rsp.n_ch) return fail(h, DQMC_ERR_STATE, "call dqmc_set_pair_channels first");
    if (which != DQMC_BIN_RESPONSE_PAIRING) {  // its source's layout needs the unequal-time stack
        NEED_UT(h);
        CHK(ut_sus_layout(h));
    }
    const long E = resp_elements(h, which) + (h->sign_on ? 1 : 0);
    CHK(binner_alloc(h, which, E, capacity));  // (waits for the stream)
    double **smp = &h->rsp.sample[resp_index(which)];
    dfree(h, smp);
    int rc = dalloc(h, smp, (size_t)h->W * (size_t)E);
    if (!rc && !current && !h->rsp.Z) rc = dalloc(h, &h->rsp.Z, (size_t)h->W * h->rsp.n_ch * h->n_dirs);
    if (rc) {
        resp_disable(h, which);
        return rc;
    }
    return DQMC_OK;
}
// on the handle's stream, behind the source section's kernels
static int resp_push(dqmc_handle *h, int which)
{
    const dqmc_handle::Binner &b = h->bin[which];
    const dqmc_handle::Momenta &m = h->mom;
    const dqmc_handle::Response &r = h->rsp;
    const int nd = h->n_dirs, nq = m.n_q;
    if (b.E != resp_elements(h, which) + (h->sign_on ? 1 : 0))
        return fail(h, DQMC_ERR_STATE, "the section's layout has changed since dqmc_binner_enable: enable it again");
    MomentumArgs a;
    a.Y = r.sample[resp_index(which)];
    a.y_stride = b.E;
    a.n_dirs = nd;
    a.n_q = nq;
    if (h->sign_on) {  // the first launch also stores s_w behind the sample
        a.sw = h->sign_sw;
        a.sign_at = b.E - 1;
    }
    {
        Timed t(h, DQMC_K_MISC);
        int rows = 0;
        if (which == DQMC_BIN_RESPONSE_CURRENT) {  // the K_cc rows of ccs, read in place
            const dqmc_handle::Section &sus = h->sec[DQMC_RED_SUSCEPTIBILITIES];
            rows = h->K_cc;
            a.X = sus.per_walker;
            a.x_stride = sus.bin_E;
            a.x_off = ut_cc_offset(h);
            a.scale = h->p.delta_tau;  // finish!: * delta_tau, as the source's binner takes it
        } else {  // the channel contraction into Z, whose n_ch rows are transformed
            const bool eq = which == DQMC_BIN_RESPONSE_PAIRING;
            const dqmc_handle::Section &src = h->sec[eq ? DQMC_RED_PAIRING : DQMC_RED_SUSCEPTIBILITIES];
            rows = r.n_ch;
            HIPCHK(launch_pair_channels(nd, h->K_loc * h->K_loc, r.n_ch, h->W, src.per_walker, src.bin_E, eq ? 0 : 4L * nd,
                                        r.F_d, r.Z, (long)r.n_ch * nd, h->stream));
            a.X = r.Z;
            a.x_stride = (long)r.n_ch * nd;
            if (!eq) a.scale = h->p.delta_tau;
        }
        a.rows = rows;
        a.tab = m.cos_d; a.y_off = 0;
        HIPCHK(launch_momentum(a, h->W, h->stream));
        a.sw = nullptr;
        a.tab = m.sin_d; a.y_off = (long)rows * nq;
        HIPCHK(launch_momentum(a, h->W, h->stream));
        if (which == DQMC_BIN_RESPONSE_CURRENT)  // the bond kinetic energy of the same sample, from the pass's G00
            HIPCHK(launch_bond_kinetic(h->n, h->nb, h->K_cc, h->W, h->p.model_kind == DQMC_ATTRACTIVE ? 2.0 : 1.0, h->ut->g00,
                                       h->nn, h->cc.trg, h->cc.tts, h->sign_on ? h->sign_sw : nullptr, a.Y, b.E,
                                       2L * rows * nq, h->stream));
    }
    BinPush p;
    p.src = a.Y;
    return binner_push(h, which, p);
}

int dqmc_set_pair_channels(dqmc_handle *h, int32_t n_ch, const double *F)
{
    ENTER(h);
    static_assert(DQMC_BIN_RESPONSE_PAIRING == DQMC_BIN_THERMODYNAMICS + 1, "the response binners follow the thermodynamics one");
    if (n_ch == 0) {  // off: as a handle that never set them
        HIPCHK(hipStreamSynchronize(h->stream));
        resp_channels_off(h);
        return DQMC_OK;
    }
    if (!h->K_loc) return fail(h, DQMC_ERR_STATE, "call dqmc_set_local_targets first");
    if (n_ch < 0 || n_ch > 8) return fail(h, DQMC_ERR_INVALID, "n_ch must be 0 or 1 .. 8");
    if (!F) return fail(h, DQMC_ERR_INVALID, "F is NULL");
    const size_t cnt = (size_t)h->K_loc * h->K_loc * (size_t)n_ch;
    std::vector<double> fh(F, F + cnt);  // (the argument may be the handle's own copy)
    HIPCHK(hipStreamSynchronize(h->stream));
    resp_channels_off(h);
    CHK(dalloc(h, &h->rsp.F_d, cnt, false));
    HIPCHK(hipMemcpy(h->rsp.F_d, fh.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
    h->rsp.F_h.swap(fh);
    h->rsp.n_ch = n_ch;
    return DQMC_OK;
}
int dqmc_response_plan(dqmc_handle *h, int32_t out[4])
{
    if (!h || !out) return DQMC_ERR_INVALID;
    out[0] = h->rsp.n_ch; out[1] = h->K_loc; out[2] = h->K_cc; out[3] = h->mom.n_q;
    return DQMC_OK;
}
