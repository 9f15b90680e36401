// mc_state.inl — the bodies of dqmc_mc_state_* and dqmc_qs_state_* (include/dqmc_hip.h, "checkpoint and resume of the
// classical MC flavor"), shared by the two engines.  Included by ising_state.inl and qs_state.inl, which say for their
// handle H what the blob code cannot know:
//   void mc_state_config(H *, mc_blob::Config *)                how the handle is configured, but for its binner
//   mc_state_slot mc_state_slot_of(H *, uint32_t tag)           where the array of a record below TAG_BIN lives (device
//                                                               or host)
// The binner is the same for both: h->sections() (mc_host.h) lists the sections in the blob's SEC_* order, and this file
// takes their shapes, their arrays and their push counts from that list, so a new section is in the checkpoint as soon
// as it is in the list (N_SEC of mc_blob.h bounds it).
// Every array of the state already lies in global memory as the blob holds it, so plain copies are the whole device side:
// there is no kernel here.  mc_blob::layout() places the records for export and import alike.

struct mc_state_slot {
    void *dev = nullptr, *host = nullptr;
};

// the record `tag`: an array of a binner section (TAG_BIN + 4 section + {xs, x2, xy, c}), else the engine's
template <typename H>
static mc_state_slot mc_state_find(H *h, uint32_t tag)
{
    if (tag < mc_blob::TAG_BIN) return mc_state_slot_of(h, tag);
    const auto secs = h->sections();
    const size_t i = tag - mc_blob::TAG_BIN;
    mc_state_slot s;
    if (i / 4 < secs.size()) {
        const mc_bin_section &b = *secs[i / 4];
        double *const a[4] = {b.xs, b.x2, b.xy, b.c};
        s.dev = a[i & 3];
    }
    return s;
}

// the host words: T of every section at its SEC_* index (0 where the engine has none), then the exchange cursor
template <typename H>
static void mc_state_host_get(H *h, uint64_t v[mc_blob::HOST_WORDS])
{
    const auto secs = h->sections();
    for (size_t i = 0; i < mc_blob::N_SEC; ++i) v[i] = i < secs.size() ? (uint64_t)secs[i]->T : 0;
    v[mc_blob::N_SEC] = h->xch.cursor;
}

template <typename H>
static void mc_state_host_set(H *h, const uint64_t v[mc_blob::HOST_WORDS])
{
    const auto secs = h->sections();
    for (size_t i = 0; i < secs.size(); ++i) secs[i]->T = (int64_t)v[i];
    h->xch.cursor = v[mc_blob::N_SEC];
}

template <typename H>
static int mc_state_layout(H *h, const char *fn, mc_blob::Config *c, mc_blob::Layout *l)
{
    *c = mc_blob::Config{};
    mc_state_config(h, c);
    const auto secs = h->sections();
    static_assert(secs.size() <= (size_t)mc_blob::N_SEC, "the blob has a place for every section");
    for (size_t i = 0; i < secs.size(); ++i)
        if (secs[i]->xs) c->bin[i] = {1, secs[i]->L, secs[i]->n_elem, secs[i]->n_pairs, secs[i]->n_comp, h->bin.cap};
    std::strncpy(c->source_hash, dqmc_build_source_hash(), mc_blob::HASH_BYTES);
    std::string why;
    if (!mc_blob::layout(*c, l, &why)) return mc_fail(h, DQMC_ERR_STATE, std::string(fn) + ": " + why);
    return 0;
}

template <typename H>
static int mc_state_size(H *h, const char *fn, size_t *n_bytes)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, std::string(fn) + ": null handle");
    if (!n_bytes) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": null n_bytes");
    mc_blob::Config c;
    mc_blob::Layout l;
    if (int rc = mc_state_layout(h, fn, &c, &l)) return rc;
    *n_bytes = l.total;
    return DQMC_OK;
}

template <typename H>
static int mc_state_export(H *h, const char *fn, void *buf, size_t n_bytes)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, std::string(fn) + ": null handle");
    if (!buf) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": null buffer");
    mc_blob::Config c;
    mc_blob::Layout l;
    if (int rc = mc_state_layout(h, fn, &c, &l)) return rc;
    if (n_bytes != l.total)
        return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": the buffer has " + std::to_string(n_bytes) + " bytes, the state " +
                                                std::to_string(l.total) + " (dqmc_*_state_size)");
    MCHK(hipSetDevice(h->device));
    MCHK(hipStreamSynchronize(h->stream));
    uint8_t *out = (uint8_t *)buf;
    std::memset(out, 0, l.total);  // (the alignment gaps between records)
    mc_blob::write_header(c, l, out);
    uint64_t host[mc_blob::HOST_WORDS];
    mc_state_host_get(h, host);
    for (const mc_blob::Record &r : l.rec) {
        const size_t bytes = (size_t)r.count * r.elem_bytes;
        if (!bytes) continue;
        if (r.tag == mc_blob::TAG_HOST) {
            std::memcpy(out + r.offset, host, bytes);
            continue;
        }
        const mc_state_slot s = mc_state_find(h, r.tag);
        if (s.host) std::memcpy(out + r.offset, s.host, bytes);
        else if (s.dev) MCHK(hipMemcpyAsync(out + r.offset, s.dev, bytes, hipMemcpyDeviceToHost, h->stream));
        else return mc_fail(h, DQMC_ERR_STATE, std::string(fn) + ": record " + std::to_string(r.tag) + " has no array in this handle");
    }
    MCHK(hipStreamSynchronize(h->stream));
    mc_blob::seal(l, out);
    return DQMC_OK;
}

template <typename H>
static int mc_state_import(H *h, const char *fn, const void *buf, size_t n_bytes)
{
    if (!h) return mc_fail(nullptr, DQMC_ERR_INVALID, std::string(fn) + ": null handle");
    if (!buf) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": null buffer");
    mc_blob::Config c;
    mc_blob::Layout mine, l;
    if (int rc = mc_state_layout(h, fn, &c, &mine)) return rc;
    const uint8_t *in = (const uint8_t *)buf;
    std::string why;
    if (mc_blob::validate(in, n_bytes, c, &l, &why) != 0) return mc_fail(h, DQMC_ERR_INVALID, std::string(fn) + ": " + why);
    for (const mc_blob::Record &r : l.rec)  // every record has its place before the first write
        if (r.tag != mc_blob::TAG_HOST && r.count) {
            const mc_state_slot s = mc_state_find(h, r.tag);
            if (!s.host && !s.dev)
                return mc_fail(h, DQMC_ERR_STATE, std::string(fn) + ": record " + std::to_string(r.tag) + " has no array in this handle");
        }
    MCHK(hipSetDevice(h->device));
    MCHK(hipStreamSynchronize(h->stream));
    for (const mc_blob::Record &r : l.rec) {
        const size_t bytes = (size_t)r.count * r.elem_bytes;
        if (!bytes) continue;
        if (r.tag == mc_blob::TAG_HOST) {
            uint64_t host[mc_blob::HOST_WORDS];
            std::memcpy(host, in + r.offset, bytes);
            mc_state_host_set(h, host);
            continue;
        }
        const mc_state_slot s = mc_state_find(h, r.tag);
        if (s.host) std::memcpy(s.host, in + r.offset, bytes);
        else MCHK(hipMemcpyAsync(s.dev, in + r.offset, bytes, hipMemcpyHostToDevice, h->stream));
    }
    MCHK(hipStreamSynchronize(h->stream));  // (the buffer is the caller's: copied before this returns)
    return DQMC_OK;
}
