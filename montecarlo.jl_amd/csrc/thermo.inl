// thermo.inl — host side of the scalar thermodynamics (thermo.hip; ABI in include/dqmc_hip.h "thermodynamics"), included
// by engine.cpp behind momentum.inl.  The reference has no such measurement.  The section is DQMC_RED_THERMODYNAMICS,
// acc = [10 sums][sum of s][count]; its binner DQMC_BIN_THERMODYNAMICS is an ordinary Binner over the section's
// per_walker buffer, E = 10 without and 11 with sign weighting (the sample then ends with s_w, as a momentum sample does),
// so it is made again wherever that setting changes (dqmc_set_sign_weighting).

static const int THERMO_MAX_ROW = 64;  // off-diagonal non-zeros of one row of the hopping matrix

static long thermo_elements(const dqmc_handle *h) { return DQMC_THERMO_ELEMENTS + (h->sign_on ? 1 : 0); }
// the stream must be idle
static void thermo_off(dqmc_handle *h)
{
    if (h->bin[DQMC_BIN_THERMODYNAMICS].on) binner_free(h, h->bin[DQMC_BIN_THERMODYNAMICS]);
    dfree(h, &h->th.row_ptr);
    dfree(h, &h->th.col);
    dfree(h, &h->th.val);
    dfree(h, &h->th.diag);
    h->th = dqmc_handle::Thermo{};
}
static int thermo_enable(dqmc_handle *h, int64_t capacity)
{
    if (!h->th.on) return fail(h, DQMC_ERR_STATE, "call dqmc_set_thermodynamics first");
    return binner_alloc(h, DQMC_BIN_THERMODYNAMICS, thermo_elements(h), capacity);
}

int dqmc_set_thermodynamics(dqmc_handle *h, const double *T)
{
    ENTER(h);
    static_assert(DQMC_THERMO_ELEMENTS == dqmc::DQMC_THERMO_ELEMENTS_K, "the kernel's sample is the header's");
    static_assert(DQMC_BIN_THERMODYNAMICS == DQMC_BIN_MOMENTUM_END, "the thermodynamics binner follows the momentum binners");
    if (!T) {  // off: as a handle that never configured the section
        HIPCHK(hipStreamSynchronize(h->stream));
        h->red_valid = false;
        thermo_off(h);
        return sec_layout(h, DQMC_RED_THERMODYNAMICS, 0, 0, 0, 0);
    }
    const int n = h->n, nb = h->nb;
    std::vector<int> ptr((size_t)nb * n + 1, 0), col;
    std::vector<double> val, diag((size_t)nb * n);
    for (int b = 0; b < nb; ++b)
        for (int i = 0; i < n; ++i) {
            const double *Tb = T + (size_t)b * h->nn;
            int cnt = 0;
            for (int j = 0; j < n; ++j) {
                const double v = Tb[i + (size_t)n * j];
                if (!std::isfinite(v)) return fail(h, DQMC_ERR_INVALID, "dqmc_set_thermodynamics: the hopping matrix has a non-finite entry");
                if (j == i) { diag[(size_t)b * n + i] = v; continue; }
                if (v == 0.0) continue;
                if (++cnt > THERMO_MAX_ROW)
                    return fail(h, DQMC_ERR_INVALID, "dqmc_set_thermodynamics: row " + std::to_string(i) + " of block " + std::to_string(b) +
                                                         " has more than 64 off-diagonal non-zeros");
                col.push_back(j);
                val.push_back(v);
            }
            ptr[(size_t)b * n + i + 1] = (int)col.size();
        }
    // ---- nothing has been written up to here ----
    HIPCHK(hipStreamSynchronize(h->stream));
    h->red_valid = false;  // (re)sized: the last reduction is void
    thermo_off(h);
    CHK(dalloc(h, &h->th.row_ptr, ptr.size(), false));
    CHK(dalloc(h, &h->th.col, col.size()));
    CHK(dalloc(h, &h->th.val, val.size()));
    CHK(dalloc(h, &h->th.diag, diag.size(), false));
    HIPCHK(hipMemcpy(h->th.row_ptr, ptr.data(), ptr.size() * sizeof(int), hipMemcpyHostToDevice));
    if (!col.empty()) {
        HIPCHK(hipMemcpy(h->th.col, col.data(), col.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->th.val, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(h->th.diag, diag.data(), diag.size() * sizeof(double), hipMemcpyHostToDevice));
    h->th.U_s = h->p.model_kind == DQMC_REPULSIVE ? h->p.U : -h->p.U;
    h->th.T_hash = dqmc_blob::fnv1a64(T, (size_t)nb * h->nn * sizeof(double));
    h->th.on = true;
    const size_t tn = DQMC_THERMO_ELEMENTS + 2;
    CHK(sec_layout(h, DQMC_RED_THERMODYNAMICS, tn, tn, DQMC_THERMO_ELEMENTS, DQMC_THERMO_ELEMENTS + 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}
int dqmc_accumulate_thermodynamics(dqmc_handle *h)
{
    ENTER(h); NEED_PREPARED(h);
    if (!h->th.on) return fail(h, DQMC_ERR_STATE, "call dqmc_set_thermodynamics first");
    const dqmc_handle::Section &sc = h->sec[DQMC_RED_THERMODYNAMICS];
    const dqmc_handle::Binner &b = h->bin[DQMC_BIN_THERMODYNAMICS];
    if (b.on && b.E != thermo_elements(h))
        return fail(h, DQMC_ERR_STATE, "the section's layout has changed since dqmc_binner_enable: enable it again");
    CHK(binner_room(h, DQMC_BIN_THERMODYNAMICS));
    const double *sw = nullptr;
    if (h->sign_on) {  // sign_begin with the section's own sum of signs as the destination (in front of true_greens)
        const int *sg = nullptr;
        if (h->p.model_kind == DQMC_REPULSIVE) {
            CHK(logdet_current(h));
            sg = h->gm_sg[0];
        }
        Timed t(h, DQMC_K_MISC);
        HIPCHK(launch_sign_prepare(h->nb, h->W, sg, h->sign_sw, h->sign_fail, sc.acc + DQMC_THERMO_ELEMENTS, nullptr, h->stream));
        sw = h->sign_sw;
    }
    CHK(true_greens(h, h->greens));
    {
        Timed t(h, DQMC_K_MISC);
        HIPCHK(launch_thermodynamics(h->n, h->nb, h->W, h->tmp2, h->nn, h->th.row_ptr, h->th.col, h->th.val, h->th.diag,
                                     h->th.U_s, sc.per_walker, thermo_elements(h), sw, sc.acc, h->stream));
    }
    if (b.on) {
        BinPush p;
        p.src = sc.per_walker;
        CHK(binner_push(h, DQMC_BIN_THERMODYNAMICS, p));
    }
    return DQMC_OK;
}
int dqmc_thermodynamics_size(dqmc_handle *h, size_t *n) { return sec_size(h, DQMC_RED_THERMODYNAMICS, n); }
int dqmc_get_thermodynamics(dqmc_handle *h, double *host_out)
{
    ENTER(h);
    if (!host_out) return fail(h, DQMC_ERR_INVALID, "host_out is NULL");
    return sec_get(h, DQMC_RED_THERMODYNAMICS, host_out);
}
int dqmc_export_thermodynamics(dqmc_handle *h, void *device_out)
{
    ENTER(h);
    if (!device_out) return fail(h, DQMC_ERR_INVALID, "device_out is NULL");
    return sec_export(h, DQMC_RED_THERMODYNAMICS, device_out);
}
