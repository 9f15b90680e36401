// checkpoint.inl — dqmc_state_size / dqmc_state_export / dqmc_state_import (include/dqmc_hip.h "checkpoint and resume";
// part of engine.cpp).  The blob's header, its validation and the payload offsets are state_blob.{h,cpp}, plain C++; here
// the handle is described to that code and the copies between the device and the caller's buffer are made.
//
// What is saved is what cannot be recomputed: the HS field, the RNG cursors, the counters and every measurement sum.  The
// UDT stack, mc.s.greens, Ul .. Tr, the logdet cache and the unequal-time stack follow from the field, and the import
// rebuilds them as resume! does through run! (DQMC.jl:412-414: init!, build_stack, propagate).

static_assert(sizeof(DevStats) == dqmc_blob::STATS_BYTES, "DevStats is stored as it lies in memory");
static_assert(sizeof(GlobalMoveState) == dqmc_blob::GM_BYTES, "GlobalMoveState is stored as it lies in memory");
static_assert(DQMC_RED_SIGN + 1 == dqmc_blob::N_SEC && DQMC_BIN_SIGN + DQMC_RED_SIGN == dqmc_blob::N_BIN, "section tables");
static_assert(DQMC_BIN_MOMENTUM_CORRELATIONS == dqmc_blob::N_BIN && DQMC_BIN_MOMENTUM_END - DQMC_BIN_MOMENTUM_CORRELATIONS == dqmc_blob::N_MOM,
              "the momentum binners follow the header's binners: the extension of format version 2");

static void state_shape(const dqmc_handle *h, dqmc_blob::Shape *s)
{
    *s = dqmc_blob::Shape{};
    std::strncpy(s->source_hash, dqmc_build_source_hash(), dqmc_blob::HASH_BYTES);
    s->n_sites = h->n; s->model_kind = h->p.model_kind; s->slices = h->M; s->safe_mult = h->s;
    s->n_walkers = h->W; s->nb = h->nb;
    s->delta_tau = h->p.delta_tau; s->U = h->p.U;
    for (int i = 0; i <= DQMC_RED_SIGN; ++i) { s->sec_n[i] = h->sec[i].n; s->sec_n_red[i] = h->sec[i].n_red; }
    for (int k = 0; k < dqmc_blob::N_BIN; ++k) {
        const dqmc_handle::Binner &b = h->bin[k];
        if (b.on) s->bin[k] = {1, b.E, b.L, b.cap, b.T};
    }
    s->td_every = h->td.every; s->td_what = h->td.what; s->td_R = h->td.R;
    s->sign_on = h->sign_on ? 1 : 0;
    s->gm_rate = h->gm_rate; s->gm_kind = h->gm_kind; s->gm_updates = h->gm_updates;
}

// the momentum binners and the tables they were made for: what the extension of a version-2 blob carries.  With no
// momentum binner enabled it is empty (m->any() false) and the blob is version 1, momenta set or not.
static void state_momenta(const dqmc_handle *h, dqmc_blob::Momenta *m)
{
    *m = dqmc_blob::Momenta{};
    for (int k = 0; k < dqmc_blob::N_MOM; ++k) {
        const dqmc_handle::Binner &b = h->bin[DQMC_BIN_MOMENTUM_CORRELATIONS + k];
        if (b.on) m->bin[k] = {1, b.E, b.L, b.cap, b.T};
    }
    if (!m->any()) return;
    m->n_q = h->mom.n_q; m->n_dirs = h->n_dirs;
    m->cos_tab = h->mom.cos_h.data(); m->sin_tab = h->mom.sin_h.data();
}

// the thermodynamics section and its binner: what the extension of a version-3 / 4 blob carries.  With the section off it
// is empty (t->any() false) and the blob is version 1 / 2.
static void state_thermo(const dqmc_handle *h, dqmc_blob::Thermo *t)
{
    *t = dqmc_blob::Thermo{};
    if (!h->th.on) return;
    t->n = h->sec[DQMC_RED_THERMODYNAMICS].n; t->n_red = h->sec[DQMC_RED_THERMODYNAMICS].n_red;
    const dqmc_handle::Binner &b = h->bin[DQMC_BIN_THERMODYNAMICS];
    if (b.on) t->bin = {1, b.E, b.L, b.cap, b.T};
    t->T_hash = h->th.T_hash; t->U_s = h->th.U_s;
}

// the response binners and what they were made for: what the extension of a version 5 - 8 blob carries.  With none of them
// enabled it is empty (r->any() false) and the blob is version 1 - 4, channels set or not.
static_assert(DQMC_BIN_RESPONSE_END - DQMC_BIN_RESPONSE_PAIRING == dqmc_blob::N_RESP, "the response binners: the extension of format versions 5 - 8");
static void state_response(const dqmc_handle *h, dqmc_blob::Response *r)
{
    *r = dqmc_blob::Response{};
    for (int k = 0; k < dqmc_blob::N_RESP; ++k) {
        const dqmc_handle::Binner &b = h->bin[DQMC_BIN_RESPONSE_PAIRING + k];
        if (b.on) r->bin[k] = {1, b.E, b.L, b.cap, b.T};
    }
    if (!r->any()) return;
    r->n_ch = h->rsp.n_ch; r->K = h->rsp.n_ch ? h->K_loc : 0; r->K_cc = h->K_cc;
    r->F = h->rsp.F_h.data();
}

// The state dqmc_update_until_measure returns in (and dqmc_sweep when it started there), rebuilt from the HS field alone: dqmc_prepare's init_stack,
// build_stack and propagate, then the propagates of a down pass with no sweep_spatial in between, which leave the stack
// slots and mc.s.greens as a down pass that accepted nothing leaves them, at current_slice == 1, direction == +1.
static int rebuild_at_measurement_point(dqmc_handle *h)
{
    discard_pending_flush(h);
    CHK(init_stack(h));
    CHK(build_stack(h));
    do {
        CHK(propagate(h));
    } while (!(h->current_slice == 1 && h->direction == 1));
    h->prepared = true;
    return 0;
}

int dqmc_state_size(dqmc_handle *h, size_t *n_bytes)
{
    if (!h || !n_bytes) return DQMC_ERR_INVALID;
    dqmc_blob::Shape s;
    dqmc_blob::Momenta m;
    dqmc_blob::Thermo th;
    dqmc_blob::Response rs;
    dqmc_blob::ResponseLayout rl;
    state_shape(h, &s);
    state_momenta(h, &m);
    state_thermo(h, &th);
    state_response(h, &rs);
    if (!dqmc_blob::response_layout(s, m, th, rs, &rl)) return fail(h, DQMC_ERR_INVALID, "dqmc_state_size: the state does not fit a size_t");
    *n_bytes = rl.total;
    return DQMC_OK;
}

int dqmc_state_export(dqmc_handle *h, void *host_out, size_t n_bytes)
{
    ENTER(h);
    if (!host_out) return fail(h, DQMC_ERR_INVALID, "dqmc_state_export: host_out is NULL");
    if (!h->prepared || h->current_slice != 1 || h->direction != 1)
        return fail(h, DQMC_ERR_STATE, "dqmc_state_export: only at the measurement point (current_slice == 1, direction == +1), where "
                                       "dqmc_update_until_measure returns");
    if (h->pf.G) return fail(h, DQMC_ERR_STATE, "dqmc_state_export: a sweep update is pending on greens");
    dqmc_blob::Shape s;
    dqmc_blob::Layout l;
    dqmc_blob::Momenta m;
    dqmc_blob::ExtLayout e;
    dqmc_blob::Thermo th;
    dqmc_blob::ThermoLayout tl;
    dqmc_blob::Response rs;
    dqmc_blob::ResponseLayout rl;
    state_shape(h, &s);
    state_momenta(h, &m);
    state_thermo(h, &th);
    state_response(h, &rs);
    if (!dqmc_blob::layout(s, &l) || !dqmc_blob::ext_layout(s, m, &e) || !dqmc_blob::thermo_layout(s, m, th, &tl) ||
        !dqmc_blob::response_layout(s, m, th, rs, &rl))
        return fail(h, DQMC_ERR_INVALID, "dqmc_state_export: the state does not fit a size_t");
    if (n_bytes != rl.total)
        return fail(h, DQMC_ERR_INVALID, "dqmc_state_export: n_bytes is " + std::to_string(n_bytes) + ", dqmc_state_size reports " +
                                             std::to_string(rl.total));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<WalkerRng> rg(h->W);
    HIPCHK(hipMemcpy(rg.data(), h->rng, sizeof(WalkerRng) * h->W, hipMemcpyDeviceToHost));
    for (int w = 0; w < h->W; ++w)
        if (rg[w].uniforms)
            return fail(h, DQMC_ERR_STATE, "dqmc_state_export: walker " + std::to_string(w) + " runs on a host-supplied uniform "
                                           "stream (dqmc_set_uniforms), which the blob does not carry");
    uint8_t *out = (uint8_t *)host_out;
    dqmc_blob::write_header(s, m, th, rs, out);
    {   // only copies from here on: nothing is launched, no buffer of the handle is written
        const size_t sz = (size_t)h->N * h->M, chunk_bytes = dqmc_blob::conf_chunks(h->N, h->M) * 8;
        std::vector<int8_t> conf((size_t)h->W * sz);
        HIPCHK(hipMemcpy(conf.data(), h->conf, conf.size(), hipMemcpyDeviceToHost));
        for (int w = 0; w < h->W; ++w) dqmc_blob::pack_conf(conf.data() + (size_t)w * sz, sz, out + l.conf + (size_t)w * chunk_bytes);
    }
    for (int w = 0; w < h->W; ++w) {
        const uint64_t sd[2] = {rg[w].seed, rg[w].draw};
        std::memcpy(out + l.rng + (size_t)w * dqmc_blob::RNG_BYTES, sd, sizeof(sd));
    }
    HIPCHK(hipMemcpy(out + l.stats, h->stats, sizeof(DevStats) * h->W, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out + l.gm, h->gm, sizeof(GlobalMoveState) * h->W, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out + l.sign_fail, h->sign_fail, sizeof(long long) * h->W, hipMemcpyDeviceToHost));
    for (int i = 0; i <= DQMC_RED_SIGN; ++i)
        if (h->sec[i].n) HIPCHK(hipMemcpy(out + l.sec[i], h->sec[i].acc, h->sec[i].n * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < dqmc_blob::N_BIN; ++k) {
        const dqmc_handle::Binner &b = h->bin[k];
        if (!b.on) continue;
        const size_t we = (size_t)h->W * (size_t)b.E * sizeof(double);
        HIPCHK(hipMemcpy(out + l.bin_xs[k], b.xs, b.L * we, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out + l.bin_x2[k], b.x2, b.L * we, hipMemcpyDeviceToHost));
        if (b.L > 1) HIPCHK(hipMemcpy(out + l.bin_c[k], b.c, (b.L - 1) * we, hipMemcpyDeviceToHost));
    }
    if (m.any()) {  // format version 2: the extension
        dqmc_blob::write_ext(m, e, out);
        for (int k = 0; k < dqmc_blob::N_MOM; ++k) {
            const dqmc_handle::Binner &b = h->bin[DQMC_BIN_MOMENTUM_CORRELATIONS + k];
            if (!b.on) continue;
            const size_t we = (size_t)h->W * (size_t)b.E * sizeof(double);
            HIPCHK(hipMemcpy(out + e.bin_xs[k], b.xs, b.L * we, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(out + e.bin_x2[k], b.x2, b.L * we, hipMemcpyDeviceToHost));
            if (b.L > 1) HIPCHK(hipMemcpy(out + e.bin_c[k], b.c, (b.L - 1) * we, hipMemcpyDeviceToHost));
        }
        dqmc_blob::seal_ext(e, out);
    }
    if (th.any()) {  // format versions 3 / 4: the thermodynamics extension
        dqmc_blob::write_thermo(th, tl, out);
        const dqmc_handle::Section &sc = h->sec[DQMC_RED_THERMODYNAMICS];
        HIPCHK(hipMemcpy(out + tl.sec, sc.acc, sc.n * sizeof(double), hipMemcpyDeviceToHost));
        const dqmc_handle::Binner &b = h->bin[DQMC_BIN_THERMODYNAMICS];
        if (b.on) {
            const size_t we = (size_t)h->W * (size_t)b.E * sizeof(double);
            HIPCHK(hipMemcpy(out + tl.bin_xs, b.xs, b.L * we, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(out + tl.bin_x2, b.x2, b.L * we, hipMemcpyDeviceToHost));
            if (b.L > 1) HIPCHK(hipMemcpy(out + tl.bin_c, b.c, (b.L - 1) * we, hipMemcpyDeviceToHost));
        }
        dqmc_blob::seal_thermo(tl, out);
    }
    if (rs.any()) {  // format versions 5 - 8: the response extension
        dqmc_blob::write_response(rs, rl, out);
        for (int k = 0; k < dqmc_blob::N_RESP; ++k) {
            const dqmc_handle::Binner &b = h->bin[DQMC_BIN_RESPONSE_PAIRING + k];
            if (!b.on) continue;
            const size_t we = (size_t)h->W * (size_t)b.E * sizeof(double);
            HIPCHK(hipMemcpy(out + rl.bin_xs[k], b.xs, b.L * we, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(out + rl.bin_x2[k], b.x2, b.L * we, hipMemcpyDeviceToHost));
            if (b.L > 1) HIPCHK(hipMemcpy(out + rl.bin_c[k], b.c, (b.L - 1) * we, hipMemcpyDeviceToHost));
        }
        dqmc_blob::seal_response(rl, out);
    }
    return DQMC_OK;
}

int dqmc_state_import(dqmc_handle *h, const void *host_in, size_t n_bytes)
{
    ENTER(h);
    dqmc_blob::Shape mine, s;
    dqmc_blob::Momenta mine_m, m;
    dqmc_blob::Layout l;
    dqmc_blob::ExtLayout e;
    dqmc_blob::Thermo mine_t, th;
    dqmc_blob::ThermoLayout tl;
    dqmc_blob::Response mine_r, rs;
    dqmc_blob::ResponseLayout rl;
    std::string why;
    state_shape(h, &mine);
    state_momenta(h, &mine_m);
    state_thermo(h, &mine_t);
    state_response(h, &mine_r);
    if (dqmc_blob::validate_full((const uint8_t *)host_in, n_bytes, mine, mine_m, mine_t, mine_r, &s, &m, &th, &rs, &why) != 0 ||
        !dqmc_blob::layout(s, &l, &why) || !dqmc_blob::ext_layout(s, m, &e, &why) || !dqmc_blob::thermo_layout(s, m, th, &tl, &why) ||
        !dqmc_blob::response_layout(s, m, th, rs, &rl, &why))
        return fail(h, DQMC_ERR_INVALID, "dqmc_state_import: " + why);
    const uint8_t *in = (const uint8_t *)host_in;
    // the one index the payload carries: the site of a walker's latest global move (the next proposal overwrites it before
    // anything reads it; checked all the same, an index being what it is)
    for (int w = 0; w < h->W; ++w) {
        GlobalMoveState g;
        std::memcpy(&g, in + l.gm + (size_t)w * sizeof(g), sizeof(g));
        if (g.site < 0 || g.site >= h->N)
            return fail(h, DQMC_ERR_INVALID, "dqmc_state_import: payload: global-move site of walker " + std::to_string(w) +
                                                 " outside 0 .. n_sites - 1");
    }
    // ---- nothing has been written up to here ----
    HIPCHK(hipStreamSynchronize(h->stream));
    {
        const size_t sz = (size_t)h->N * h->M, chunk_bytes = dqmc_blob::conf_chunks(h->N, h->M) * 8;
        std::vector<int8_t> conf((size_t)h->W * sz);
        for (int w = 0; w < h->W; ++w) dqmc_blob::unpack_conf(in + l.conf + (size_t)w * chunk_bytes, sz, conf.data() + (size_t)w * sz);
        HIPCHK(hipMemcpy(h->conf, conf.data(), conf.size(), hipMemcpyHostToDevice));
    }
    h->conf_version++;          // the unequal-time stack is rebuilt lazily, as after any change of the field
    h->gm_cache_version = -1;   // and so are the logabsdet / sign of the current field
    h->red_valid = false;
    CHK(rebuild_at_measurement_point(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    // the counters behind the rebuild (its propagation checks have pushed to propagation_error)
    std::vector<WalkerRng> rg(h->W);
    for (int w = 0; w < h->W; ++w) {
        uint64_t sd[2];
        std::memcpy(sd, in + l.rng + (size_t)w * dqmc_blob::RNG_BYTES, sizeof(sd));
        rg[w] = {(unsigned long long)sd[0], (unsigned long long)sd[1], nullptr, 0ull, 0};
    }
    HIPCHK(hipMemcpy(h->rng, rg.data(), sizeof(WalkerRng) * h->W, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->stats, in + l.stats, sizeof(DevStats) * h->W, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->gm, in + l.gm, sizeof(GlobalMoveState) * h->W, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->sign_fail, in + l.sign_fail, sizeof(long long) * h->W, hipMemcpyHostToDevice));
    for (int i = 0; i <= DQMC_RED_SIGN; ++i)
        if (h->sec[i].n) HIPCHK(hipMemcpy(h->sec[i].acc, in + l.sec[i], h->sec[i].n * sizeof(double), hipMemcpyHostToDevice));
    for (int k = 0; k < dqmc_blob::N_BIN; ++k) {
        dqmc_handle::Binner &b = h->bin[k];
        if (!b.on) continue;
        const size_t we = (size_t)h->W * (size_t)b.E * sizeof(double);
        HIPCHK(hipMemcpy(b.xs, in + l.bin_xs[k], b.L * we, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b.x2, in + l.bin_x2[k], b.L * we, hipMemcpyHostToDevice));
        if (b.L > 1) HIPCHK(hipMemcpy(b.c, in + l.bin_c[k], (b.L - 1) * we, hipMemcpyHostToDevice));
        b.T = s.bin[k].T;
    }
    for (int k = 0; k < dqmc_blob::N_MOM; ++k) {  // (format version 2; a version-1 blob has none and the handle neither)
        dqmc_handle::Binner &b = h->bin[DQMC_BIN_MOMENTUM_CORRELATIONS + k];
        if (!b.on) continue;
        const size_t we = (size_t)h->W * (size_t)b.E * sizeof(double);
        HIPCHK(hipMemcpy(b.xs, in + e.bin_xs[k], b.L * we, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b.x2, in + e.bin_x2[k], b.L * we, hipMemcpyHostToDevice));
        if (b.L > 1) HIPCHK(hipMemcpy(b.c, in + e.bin_c[k], (b.L - 1) * we, hipMemcpyHostToDevice));
        b.T = m.bin[k].T;
    }
    if (th.any()) {  // (format versions 3 / 4; validate_all has made sure the handle has the section, shaped the same)
        const dqmc_handle::Section &sc = h->sec[DQMC_RED_THERMODYNAMICS];
        HIPCHK(hipMemcpy(sc.acc, in + tl.sec, sc.n * sizeof(double), hipMemcpyHostToDevice));
        dqmc_handle::Binner &b = h->bin[DQMC_BIN_THERMODYNAMICS];
        if (b.on) {
            const size_t we = (size_t)h->W * (size_t)b.E * sizeof(double);
            HIPCHK(hipMemcpy(b.xs, in + tl.bin_xs, b.L * we, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(b.x2, in + tl.bin_x2, b.L * we, hipMemcpyHostToDevice));
            if (b.L > 1) HIPCHK(hipMemcpy(b.c, in + tl.bin_c, (b.L - 1) * we, hipMemcpyHostToDevice));
            b.T = th.bin.T;
        }
    }
    for (int k = 0; k < dqmc_blob::N_RESP; ++k) {  // (format versions 5 - 8; validate_full has made sure both sides have the same ones)
        dqmc_handle::Binner &b = h->bin[DQMC_BIN_RESPONSE_PAIRING + k];
        if (!b.on) continue;
        const size_t we = (size_t)h->W * (size_t)b.E * sizeof(double);
        HIPCHK(hipMemcpy(b.xs, in + rl.bin_xs[k], b.L * we, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b.x2, in + rl.bin_x2[k], b.L * we, hipMemcpyHostToDevice));
        if (b.L > 1) HIPCHK(hipMemcpy(b.c, in + rl.bin_c[k], (b.L - 1) * we, hipMemcpyHostToDevice));
        b.T = rs.bin[k].T;
    }
    h->gm_updates = s.gm_updates;
    return dqmc_synchronize(h);
}
