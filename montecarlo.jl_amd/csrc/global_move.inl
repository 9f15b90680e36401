// global_move.inl — global moves of the DQMC flavor (include/dqmc_hip.h "global moves"; part of engine.cpp).
//
// The reference reserves the hook (DQMC.jl:526-532) and the parameters (DQMC.jl:53-54, 72-73) but has no move.  Here a
// move flips the whole HS field or one site's time line and is accepted with the ratio of the fermion determinants,
// which needs log|det(I + B_M ... B_1)| and its sign per unit: logdet_from_scratch.  Everything a move decides stays on
// the device (csrc/logdet.hip); the host only queues launches.

// logabsdet / sign of every unit for the current field into lad / sg (device, `units` entries): the from-scratch chain
// of calculate_greens(mc, 0) with the matrix handed to its second UDT copied aside (bufA), then logdet_kernel on that
// copy and on the D the UDT left in Dr.  Overwrites Ul .. Tr, tmp1 / tmp2, bufA / bufB and greens_temp.
static int logdet_from_scratch(dqmc_handle *h, double *lad, int *sg)
{
    CHK(calculate_greens_from_scratch(h, 0, h->greens_temp, h->bufA));
    Timed t(h, DQMC_K_MISC);
    HIPCHK(launch_logdet(h->n, h->units, h->bufA, h->nn, h->Dr, h->n, lad, sg, h->stream));
    return 0;
}
// the cache of the current field's values (invalid once conf_version has moved on)
static int logdet_current(dqmc_handle *h)
{
    if (h->gm_cache_version == h->conf_version) return 0;
    CHK(logdet_from_scratch(h, h->gm_lad[0], h->gm_sg[0]));
    h->gm_cache_version = h->conf_version;
    return 0;
}
// ---- sign reweighting (include/dqmc_hip.h "sign reweighting"; kernels in sign.hip) ---------------------------------
// s_w = prod_b sign_b is a property of the field (the determinant does not change under a cyclic rotation of the slices),
// so it comes from the cache above at any current_slice, and the accumulate calls of one measurement point share one
// chain.  The attractive model's weight is a square: +1 by construction, no chain.
static int sign_begin(dqmc_handle *h, int sec_a, int sec_b)
{
    if (!h->sign_on) return 0;
    const int *sg = nullptr;
    if (h->p.model_kind == DQMC_REPULSIVE) {
        CHK(logdet_current(h));
        sg = h->gm_sg[0];
    }
    double *sums = h->sec[DQMC_RED_SIGN].acc;
    Timed t(h, DQMC_K_MISC);
    HIPCHK(launch_sign_prepare(h->nb, h->W, sg, h->sign_sw, h->sign_fail, sums + sec_a, sec_b >= 0 ? sums + sec_b : nullptr,
                               h->stream));
    return 0;
}
// one move of `walker` (< 0: every walker); leaves the handle as dqmc_prepare would for the resulting fields
static int global_move(dqmc_handle *h, int kind, int walker)
{
    CHK(logdet_current(h));
    {
        Timed t(h, DQMC_K_MISC);
        HIPCHK(launch_gm_propose(h->N, h->M, h->W, kind, walker, h->conf, h->rng, h->gm, h->stream));
    }
    h->conf_version++;
    CHK(logdet_from_scratch(h, h->gm_lad[1], h->gm_sg[1]));
    {
        Timed t(h, DQMC_K_MISC);
        HIPCHK(launch_gm_decide(h->N, h->M, h->nb, h->W, kind, h->lambda, h->p.check_sign_problem, h->conf, h->rng, h->gm,
                                h->stats, h->gm_lad[0], h->gm_sg[0], h->gm_lad[1], h->gm_sg[1], h->stream));
    }
    // the field is the old or the new one per walker, and the cache holds the values of whichever it is
    h->conf_version++;
    h->gm_cache_version = h->conf_version;
    discard_pending_flush(h);
    CHK(init_stack(h));
    CHK(build_stack(h));
    CHK(propagate(h));
    return 0;
}
// update(mc, i) (DQMC.jl:523-538) with the reference's hook filled in: i = 1 + (updates since dqmc_prepare) / (2 slices)
static int update_hooked(dqmc_handle *h)
{
    CHK(propagate(h));
    if (h->gm_rate > 0) {
        const long long i = 1 + h->gm_updates / (2LL * h->M);
        if (h->current_slice == h->M && h->direction == -1 && i % h->gm_rate == 0) CHK(global_move(h, h->gm_kind, -1));
    }
    h->gm_updates++;
    return sweep_spatial(h);
}

int dqmc_logdet(dqmc_handle *h, double *logabsdet, int32_t *sign)
{
    ENTER(h);
    if (!logabsdet || !sign) return fail(h, DQMC_ERR_INVALID, "dqmc_logdet: null output");
    h->gm_cache_version = -1;  // from scratch, as documented
    CHK(logdet_current(h));
    CHK(dqmc_synchronize(h));
    HIPCHK(hipMemcpy(logabsdet, h->gm_lad[0], sizeof(double) * h->units, hipMemcpyDeviceToHost));
    static_assert(sizeof(int) == sizeof(int32_t), "sign buffer");
    HIPCHK(hipMemcpy(sign, h->gm_sg[0], sizeof(int) * h->units, hipMemcpyDeviceToHost));
    return DQMC_OK;
}
int dqmc_get_sign(dqmc_handle *h, int32_t *sign)
{
    ENTER(h);
    if (!sign) return fail(h, DQMC_ERR_INVALID, "dqmc_get_sign: null output");
    if (h->p.model_kind != DQMC_REPULSIVE) {  // a square: nothing to launch
        for (int w = 0; w < h->W; ++w) sign[w] = 1;
        return DQMC_OK;
    }
    CHK(logdet_current(h));
    CHK(dqmc_synchronize(h));
    std::vector<int> sg(h->units);
    HIPCHK(hipMemcpy(sg.data(), h->gm_sg[0], sizeof(int) * h->units, hipMemcpyDeviceToHost));
    for (int w = 0; w < h->W; ++w) {
        int s = 1;
        for (int b = 0; b < h->nb; ++b) s *= sg[(size_t)w * h->nb + b];
        sign[w] = s;
    }
    return DQMC_OK;
}
// Diagnostic: the per-unit signs of the cache replaced by the caller's.  The chain runs first, so that gm_lad[0] holds the
// true values and the cache counts as current; everything is checked before the first write.
int dqmc_impose_unit_signs(dqmc_handle *h, const int32_t *sign)
{
    ENTER(h);
    if (!sign) return fail(h, DQMC_ERR_INVALID, "dqmc_impose_unit_signs: null input");
    if (!h->prepared) return fail(h, DQMC_ERR_STATE, "dqmc_impose_unit_signs: call dqmc_prepare first");
    if (h->p.model_kind != DQMC_REPULSIVE)
        return fail(h, DQMC_ERR_STATE, "dqmc_impose_unit_signs: the attractive model's sign is +1 by construction, there is no array");
    for (int u = 0; u < h->units; ++u)
        if (sign[u] < -1 || sign[u] > 1) return fail(h, DQMC_ERR_INVALID, "dqmc_impose_unit_signs: a sign must be -1, 0 or +1");
    CHK(logdet_current(h));
    CHK(dqmc_synchronize(h));  // (the chain's own signs are written before the caller's)
    static_assert(sizeof(int) == sizeof(int32_t), "sign buffer");
    HIPCHK(hipMemcpy(h->gm_sg[0], sign, sizeof(int) * h->units, hipMemcpyHostToDevice));
    return DQMC_OK;
}
int dqmc_set_sign_weighting(dqmc_handle *h, int32_t on)
{
    ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i <= DQMC_RED_THERMODYNAMICS; ++i) {  // signed and unsigned sums never mix
        const dqmc_handle::Section &sc = h->sec[i];
        if (!sc.n || i == DQMC_RED_SIGN) continue;
        double cnt = 0.0;
        HIPCHK(hipMemcpy(&cnt, sc.acc + sc.n - 1, sizeof(double), hipMemcpyDeviceToHost));
        if (cnt != 0.0)
            return fail(h, DQMC_ERR_STATE, "dqmc_set_sign_weighting: a section has samples: call dqmc_reset_accumulators first");
    }
    for (int which = DQMC_BIN_GREENS; which <= DQMC_BIN_TIME_DISPLACED; ++which)
        if (which != DQMC_BIN_USER && h->bin[which].on && h->bin[which].T)
            return fail(h, DQMC_ERR_STATE, "dqmc_set_sign_weighting: a binner has samples: call dqmc_reset_accumulators first");
    for (int which = DQMC_BIN_MOMENTUM_CORRELATIONS; which < DQMC_BIN_RESPONSE_END; ++which)
        if (h->bin[which].on && h->bin[which].T)
            return fail(h, DQMC_ERR_STATE, "dqmc_set_sign_weighting: a binner has samples: call dqmc_reset_accumulators first");
    h->sign_on = on != 0;
    if (h->sign_on) tcov_off(h);  // (the covariance of s x is not that of x: dqmc_set_tau_covariance refuses it)
    h->red_valid = false;  // (re)sized: the last reduction is void
    dqmc_handle::Section &sg = h->sec[DQMC_RED_SIGN];
    sg.n_red = h->sign_on ? sg.n : 0;
    HIPCHK(hipMemsetAsync(sg.acc, 0, sg.n * sizeof(double), h->stream));
    CHK(ctd_reset(h));  // (the imaginary-time current sums: their passes feed the susceptibilities, empty by now)
    for (int which = DQMC_BIN_GREENS; which <= DQMC_BIN_TIME_DISPLACED; ++which) {
        if (which == DQMC_BIN_USER) continue;
        dqmc_handle::Binner &sb = h->bin[binner_sign_of(which)];
        if (h->sign_on && h->bin[which].on) CHK(binner_alloc(h, binner_sign_of(which), 1, h->bin[which].cap));
        else if (sb.on) binner_free(h, sb);
    }
    // a momentum sample ends with s_w while weighting is on: its binners are made again, empty, with their capacities
    for (int which = DQMC_BIN_MOMENTUM_CORRELATIONS; which < DQMC_BIN_MOMENTUM_END; ++which)
        if (h->bin[which].on) CHK(mom_enable(h, which, h->bin[which].cap));
    if (h->bin[DQMC_BIN_THERMODYNAMICS].on) CHK(thermo_enable(h, h->bin[DQMC_BIN_THERMODYNAMICS].cap));  // and so does this one
    for (int which = DQMC_BIN_RESPONSE_PAIRING; which < DQMC_BIN_RESPONSE_END; ++which)  // and the response samples
        if (h->bin[which].on) CHK(resp_enable(h, which, h->bin[which].cap));
    return dqmc_synchronize(h);
}
int dqmc_get_sign_weighting(dqmc_handle *h, int32_t *on)
{
    if (!h || !on) return DQMC_ERR_INVALID;
    *on = h->sign_on ? 1 : 0;
    return DQMC_OK;
}
int dqmc_get_sign_failures(dqmc_handle *h, int64_t *count)
{
    ENTER(h);
    if (!count) return fail(h, DQMC_ERR_INVALID, "dqmc_get_sign_failures: null output");
    static_assert(sizeof(long long) == sizeof(int64_t), "counter buffer");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(count, h->sign_fail, sizeof(int64_t) * h->W, hipMemcpyDeviceToHost));
    return DQMC_OK;
}
int dqmc_sign_sums_size(dqmc_handle *h, size_t *n) { return sec_size(h, DQMC_RED_SIGN, n); }
int dqmc_get_sign_sums(dqmc_handle *h, double *host_out)
{
    ENTER(h);
    if (!host_out) return fail(h, DQMC_ERR_INVALID, "host_out is NULL");
    return sec_get(h, DQMC_RED_SIGN, host_out);
}
int dqmc_export_sign_sums(dqmc_handle *h, void *device_out)
{
    ENTER(h);
    if (!device_out) return fail(h, DQMC_ERR_INVALID, "device_out is NULL");
    return sec_export(h, DQMC_RED_SIGN, device_out);
}
int dqmc_global_move(dqmc_handle *h, int32_t kind, int32_t walker)
{
    ENTER(h);
    if (!h->prepared) return fail(h, DQMC_ERR_STATE, "dqmc_global_move: call dqmc_prepare first");
    if (kind != DQMC_GLOBAL_FLIP_ALL && kind != DQMC_GLOBAL_FLIP_SITE)
        return fail(h, DQMC_ERR_INVALID, "dqmc_global_move: unknown kind (DQMC_GLOBAL_FLIP_ALL or DQMC_GLOBAL_FLIP_SITE)");
    if (walker >= h->W) return fail(h, DQMC_ERR_INVALID, "walker index out of range");
    CHK(global_move(h, kind, walker < 0 ? -1 : walker));
    return dqmc_synchronize(h);
}
int dqmc_set_global_rate(dqmc_handle *h, int32_t rate, int32_t kind)
{
    ENTER(h);
    if (rate < 0) return fail(h, DQMC_ERR_INVALID, "dqmc_set_global_rate: rate must be >= 0");
    if (kind != DQMC_GLOBAL_FLIP_ALL && kind != DQMC_GLOBAL_FLIP_SITE)
        return fail(h, DQMC_ERR_INVALID, "dqmc_set_global_rate: unknown kind (DQMC_GLOBAL_FLIP_ALL or DQMC_GLOBAL_FLIP_SITE)");
    h->gm_rate = rate;
    h->gm_kind = kind;
    return DQMC_OK;
}
int dqmc_get_global_stats(dqmc_handle *h, int32_t w, dqmc_global_stats *out)
{
    ENTER(h); WALKER_OK(h, w);
    if (!out) return fail(h, DQMC_ERR_INVALID, "dqmc_get_global_stats: null output");
    HIPCHK(hipStreamSynchronize(h->stream));
    GlobalMoveState g;
    HIPCHK(hipMemcpy(&g, h->gm + w, sizeof(g), hipMemcpyDeviceToHost));
    out->prop_global = g.prop_global;
    out->acc_global = g.acc_global;
    out->moves_drawn = g.moves_drawn;
    return DQMC_OK;
}
int dqmc_get_global_last(dqmc_handle *h, int32_t w, double *p, int32_t *accepted, int32_t *site)
{
    ENTER(h); WALKER_OK(h, w);
    if (!p || !accepted || !site) return fail(h, DQMC_ERR_INVALID, "dqmc_get_global_last: null output");
    HIPCHK(hipStreamSynchronize(h->stream));
    GlobalMoveState g;
    HIPCHK(hipMemcpy(&g, h->gm + w, sizeof(g), hipMemcpyDeviceToHost));
    *p = g.last_p;
    *accepted = g.last_accepted;
    *site = g.site;
    return DQMC_OK;
}
