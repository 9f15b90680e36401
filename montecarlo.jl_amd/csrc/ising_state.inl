// ising_state.inl — dqmc_mc_state_size / _export / _import (include/dqmc_hip.h, "checkpoint and resume of the classical MC
// flavor"): what mc_state.inl needs to know about a dqmc_mc_handle.  Included by ising.hip behind the handle.  No kernel.
#include "mc_state.inl"

static void mc_state_config(dqmc_mc_handle *h, mc_blob::Config *c)
{
    const bool cb = h->upd.kind == DQMC_MC_UPDATE_CHECKERBOARD;
    c->kind = mc_blob::KIND_ISING;
    c->n_sites = h->N;
    c->z = h->z;
    c->q = 0;
    c->n_walkers = h->W;
    c->series_capacity = h->cap;
    c->n_bonds = h->n_bonds;
    c->update_kind = h->upd.kind;
    c->n_colours = cb ? h->upd.C : 0;
    c->cluster_rate = h->global_rate;
    c->exchange_R = h->xch.R;
    c->exchange_rate = h->xch.rate;
    c->n_k = h->fss.n_k;
    c->hash_neighs = mc_hash(h->nbr_h);
    c->hash_bonds = mc_hash(h->bonds_h);
    c->hash_colouring = cb ? h->upd.hash : 0;
    c->hash_betas = mc_hash(h->beta_h);
    c->hash_phases = h->fss.n_k >= 0 ? h->fss.hash : 0;
}

static mc_state_slot mc_state_slot_of(dqmc_mc_handle *h, uint32_t tag)
{
    const DevState &d = h->d;
    void *p = nullptr;
    switch (tag) {
    case mc_blob::TAG_CONF: p = d.conf; break;
    case mc_blob::TAG_KEY: p = d.key; break;
    case mc_blob::TAG_CURSOR_SWEEP: p = d.draw; break;
    case mc_blob::TAG_CURSOR_CLUSTER: p = d.moves; break;
    case mc_blob::TAG_CURSOR_CB: p = h->upd.cursor; break;
    case mc_blob::TAG_E: p = d.E; break;
    case mc_blob::TAG_M: p = d.M; break;
    case mc_blob::TAG_SUM_E: p = d.sE; break;
    case mc_blob::TAG_SUM_E2: p = d.sE2; break;
    case mc_blob::TAG_SUM_M: p = d.sM; break;
    case mc_blob::TAG_SUM_M2: p = d.sM2; break;
    case mc_blob::TAG_N_MEAS: p = d.n_meas; break;
    case mc_blob::TAG_PROP: p = d.prop; break;
    case mc_blob::TAG_ACC: p = d.acc; break;
    case mc_blob::TAG_N_SERIES: p = d.n_series; break;
    case mc_blob::TAG_SERIES_A: p = d.serE; break;
    case mc_blob::TAG_SERIES_B: p = d.serM; break;
    case mc_blob::TAG_G_PROP: p = d.gprop; break;
    case mc_blob::TAG_G_ACC: p = d.gacc; break;
    case mc_blob::TAG_G_SUM: p = d.gsum; break;
    case mc_blob::TAG_X_REPLICA: p = h->xch.replica; break;
    case mc_blob::TAG_X_PROP: p = h->xch.prop; break;
    case mc_blob::TAG_X_ACC: p = h->xch.acc; break;
    case mc_blob::TAG_K_SUM_M4: p = h->fss.sM4; break;
    case mc_blob::TAG_K_SUM_S: p = h->fss.sS; break;
    case mc_blob::TAG_K_N_MEAS: p = h->fss.n_meas; break;
    }
    mc_state_slot s;
    s.dev = p;
    return s;
}

extern "C" {

int dqmc_mc_state_size(dqmc_mc_handle *h, size_t *n_bytes) { return mc_state_size(h, "dqmc_mc_state_size", n_bytes); }

int dqmc_mc_state_export(dqmc_mc_handle *h, void *buf, size_t n_bytes)
{
    return mc_state_export(h, "dqmc_mc_state_export", buf, n_bytes);
}

int dqmc_mc_state_import(dqmc_mc_handle *h, const void *buf, size_t n_bytes)
{
    return mc_state_import(h, "dqmc_mc_state_import", buf, n_bytes);
}

}  // extern "C"
