// entangle.inl — host side of the Renyi-2 entanglement measurement (entangle.hip; ABI in include/dqmc_hip.h
// "entanglement"), included by engine.cpp behind response.inl.  The reference has no such measurement.  Its state is
// dqmc_handle::Entangle, outside dqmc_handle::sec[]: no DQMC_RED_* section, no binner, nothing in the packed reduction or
// the state blob.  n_sub == 0: off, nothing allocated.

// the stream must be idle
static void ent_off(dqmc_handle *h)
{
    dqmc_handle::Entangle &e = h->ent;
    dfree(h, &e.sub_ptr);
    dfree(h, &e.sites);
    dfree(h, &e.img_off);
    dfree(h, &e.img);
    dfree(h, &e.lad);
    dfree(h, &e.sg);
    dfree(h, &e.sample);
    dfree(h, &e.sums);
    dfree(h, &e.fail);
    e = dqmc_handle::Entangle{};
}
static size_t ent_elements(const dqmc_handle *h) { return (size_t)h->ent.n_sub * h->W * h->W; }
// dqmc_reset_accumulators: the sums, the count and the failures
static int ent_reset(dqmc_handle *h)
{
    dqmc_handle::Entangle &e = h->ent;
    if (!e.n_sub) return 0;
    HIPCHK(hipMemsetAsync(e.sums, 0, ent_elements(h) * sizeof(double), h->stream));
    HIPCHK(hipMemsetAsync(e.fail, 0, sizeof(unsigned long long), h->stream));
    e.count = 0;
    return 0;
}

int dqmc_set_entanglement(dqmc_handle *h, int32_t n_sub, const int32_t *sub_ptr, const int32_t *sites)
{
    ENTER(h);
    static_assert(DQMC_ENT_MAX_SITES == dqmc::DQMC_ENT_MAX_SITES_K, "the kernel's limit is the header's");
    if (n_sub == 0) {  // off: as a handle that never configured the measurement
        HIPCHK(hipStreamSynchronize(h->stream));
        ent_off(h);
        return DQMC_OK;
    }
    if (h->W < 2) return fail(h, DQMC_ERR_STATE, "dqmc_set_entanglement: the estimator pairs walkers, the handle has fewer than two");
    if (n_sub < 0 || n_sub > DQMC_ENT_MAX_SUBSYSTEMS)
        return fail(h, DQMC_ERR_INVALID, "dqmc_set_entanglement: n_sub outside 0 .. " + std::to_string(DQMC_ENT_MAX_SUBSYSTEMS));
    if (!sub_ptr || !sites) return fail(h, DQMC_ERR_INVALID, "dqmc_set_entanglement: sub_ptr or sites is NULL");
    if (sub_ptr[0] != 0) return fail(h, DQMC_ERR_INVALID, "dqmc_set_entanglement: sub_ptr[0] is not 0");
    std::vector<long> off((size_t)n_sub);
    std::vector<char> seen((size_t)h->n);
    long total = 0;
    int na_max = 0;
    for (int s = 0; s < n_sub; ++s) {
        const long na = (long)sub_ptr[s + 1] - sub_ptr[s];
        const std::string which = "dqmc_set_entanglement: subsystem " + std::to_string(s);
        if (na < 1) return fail(h, DQMC_ERR_INVALID, which + " is empty");
        if (na > DQMC_ENT_MAX_SITES)
            return fail(h, DQMC_ERR_INVALID, which + " has " + std::to_string(na) + " sites, the limit is " + std::to_string(DQMC_ENT_MAX_SITES));
        std::fill(seen.begin(), seen.end(), 0);
        for (int i = sub_ptr[s]; i < sub_ptr[s + 1]; ++i) {
            const int a = sites[i];
            if (a < 0 || a >= h->n) return fail(h, DQMC_ERR_INVALID, which + " names site " + std::to_string(a) + " outside [0, n_sites)");
            if (seen[a]) return fail(h, DQMC_ERR_INVALID, which + " names site " + std::to_string(a) + " twice");
            seen[a] = 1;
        }
        off[s] = total;
        total += (long)h->units * 2 * na * na;
        na_max = std::max(na_max, (int)na);
    }
    // ---- nothing has been written up to here ----
    HIPCHK(hipStreamSynchronize(h->stream));
    ent_off(h);
    dqmc_handle::Entangle &e = h->ent;
    const size_t n_sites = (size_t)sub_ptr[n_sub], n_pairs = (size_t)h->W * (h->W - 1) / 2;
    e.sub_ptr_h.assign(sub_ptr, sub_ptr + n_sub + 1);
    e.sites_h.assign(sites, sites + n_sites);
    CHK(dalloc(h, &e.sub_ptr, (size_t)n_sub + 1, false));
    CHK(dalloc(h, &e.sites, n_sites, false));
    CHK(dalloc(h, &e.img_off, (size_t)n_sub, false));
    CHK(dalloc(h, &e.img, (size_t)total, false));
    CHK(dalloc(h, &e.lad, (size_t)n_sub * n_pairs * h->nb));
    CHK(dalloc(h, &e.sg, (size_t)n_sub * n_pairs * h->nb));
    CHK(dalloc(h, &e.sample, (size_t)n_sub * h->W * h->W));
    CHK(dalloc(h, &e.sums, (size_t)n_sub * h->W * h->W));
    CHK(dalloc(h, &e.fail, (size_t)1));
    HIPCHK(hipMemcpy(e.sub_ptr, e.sub_ptr_h.data(), e.sub_ptr_h.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e.sites, e.sites_h.data(), e.sites_h.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e.img_off, off.data(), off.size() * sizeof(long), hipMemcpyHostToDevice));
    HIPCHK(dqmc::entanglement_prepare(na_max));  // (once per handle: the limit is the largest subsystem's)
    e.off_h = off;
    e.n_sub = n_sub;
    HIPCHK(hipStreamSynchronize(h->stream));
    return DQMC_OK;
}
int dqmc_entanglement_size(dqmc_handle *h, size_t *n)
{
    if (!h || !n) return DQMC_ERR_INVALID;
    *n = h->ent.n_sub ? ent_elements(h) + 2 : 0;
    return DQMC_OK;
}
int dqmc_accumulate_entanglement(dqmc_handle *h)
{
    ENTER(h); NEED_PREPARED(h);
    dqmc_handle::Entangle &e = h->ent;
    if (!e.n_sub) return fail(h, DQMC_ERR_STATE, "call dqmc_set_entanglement first");
    if (h->sign_on) return fail(h, DQMC_ERR_STATE, "dqmc_accumulate_entanglement: the signed estimator is not implemented (sign weighting is on)");
    CHK(true_greens(h, h->greens));
    {
        Timed t(h, DQMC_K_MISC);
        HIPCHK(launch_entanglement_gather(h->n, h->units, e.n_sub, h->tmp2, h->nn, e.sub_ptr, e.sites, e.img_off, e.img, h->stream));
        const size_t n_pairs = (size_t)h->W * (h->W - 1) / 2, ww = (size_t)h->W * h->W;
        for (int s = 0; s < e.n_sub; ++s)
            HIPCHK(launch_entanglement_pairs(e.sub_ptr_h[s + 1] - e.sub_ptr_h[s], h->nb, h->W, e.img + e.off_h[s],
                                             e.lad + s * n_pairs * h->nb, e.sg + s * n_pairs * h->nb, e.sample + s * ww,
                                             e.sums + s * ww, e.fail, h->stream));
    }
    e.count += 1;
    return DQMC_OK;
}
int dqmc_get_entanglement(dqmc_handle *h, double *out, size_t n)
{
    ENTER(h);
    const dqmc_handle::Entangle &e = h->ent;
    if (!e.n_sub) return fail(h, DQMC_ERR_STATE, "call dqmc_set_entanglement first");
    if (!out || n != ent_elements(h) + 2) return fail(h, DQMC_ERR_INVALID, "dqmc_get_entanglement: host_out is NULL or n is not dqmc_entanglement_size");
    unsigned long long f = 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, e.sums, (n - 2) * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&f, e.fail, sizeof(f), hipMemcpyDeviceToHost));
    out[n - 2] = (double)e.count;
    out[n - 1] = (double)f;
    return DQMC_OK;
}
int dqmc_get_entanglement_sample(dqmc_handle *h, double *out, size_t n)
{
    ENTER(h);
    const dqmc_handle::Entangle &e = h->ent;
    if (!e.n_sub) return fail(h, DQMC_ERR_STATE, "call dqmc_set_entanglement first");
    if (!out || n != ent_elements(h)) return fail(h, DQMC_ERR_INVALID, "dqmc_get_entanglement_sample: host_out is NULL or n is not n_sub W W");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, e.sample, n * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
int dqmc_set_entanglement_sums(dqmc_handle *h, const double *in, size_t n)
{
    ENTER(h);
    dqmc_handle::Entangle &e = h->ent;
    if (!e.n_sub) return fail(h, DQMC_ERR_STATE, "call dqmc_set_entanglement first");
    if (!in || n != ent_elements(h) + 2) return fail(h, DQMC_ERR_INVALID, "dqmc_set_entanglement_sums: host_in is NULL or n is not dqmc_entanglement_size");
    const double c = in[n - 2], f = in[n - 1];
    if (!(c >= 0.0) || !(f >= 0.0) || !(c < 9e15) || !(f < 9e15) || c != std::floor(c) || f != std::floor(f))
        return fail(h, DQMC_ERR_INVALID, "dqmc_set_entanglement_sums: the count and the failures must be non-negative integers");
    const unsigned long long fi = (unsigned long long)f;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(e.sums, in, (n - 2) * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e.fail, &fi, sizeof(fi), hipMemcpyHostToDevice));
    e.count = (long long)c;
    return DQMC_OK;
}
