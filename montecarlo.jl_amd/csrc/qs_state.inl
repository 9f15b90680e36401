// qs_state.inl — dqmc_qs_state_size / _export / _import (include/dqmc_hip.h, "checkpoint and resume of the classical MC
// flavor"): what mc_state.inl needs to know about a dqmc_qs_handle.  Included by qstate.hip behind the handle.  No kernel.
#include "mc_state.inl"

static void mc_state_config(dqmc_qs_handle *h, mc_blob::Config *c)
{
    c->kind = mc_blob::KIND_QSTATE;
    c->n_sites = h->N;
    c->z = h->z;
    c->q = h->q;
    c->n_walkers = h->W;
    c->series_capacity = h->cap;
    c->n_bonds = h->n_bonds;
    c->update_kind = DQMC_MC_UPDATE_CHECKERBOARD;
    c->n_colours = h->C;
    c->cluster_rate = h->ca.rate;
    c->exchange_R = h->xch.R;
    c->exchange_rate = h->xch.rate;
    c->n_k = h->sc.n_k;
    c->n_dir = h->st.n_dir;
    c->n_classes = h->st.n_c;
    c->hash_neighs = mc_hash(h->nbr_h);
    c->hash_bonds = h->hash_bonds;
    c->hash_energy = mc_hash(h->e_h);
    c->hash_order = h->hash_order;
    c->hash_twist = h->st.n_dir > 0 ? h->st.hash_twist : 0;
    c->hash_colouring = h->hash_colour;
    c->hash_betas = mc_hash(h->beta_h);
    c->hash_phases = h->sc.n_k > 0 ? h->sc.hash : 0;
    c->hash_stiffness = h->st.n_dir > 0 ? h->st.hash : 0;
}

static mc_state_slot mc_state_slot_of(dqmc_qs_handle *h, uint32_t tag)
{
    const DevState &d = h->d;
    mc_state_slot s;
    void *p = nullptr;
    switch (tag) {
    case mc_blob::TAG_CONF: p = d.conf; break;
    case mc_blob::TAG_KEY: p = d.key; break;
    case mc_blob::TAG_CURSOR_SWEEP: p = d.cursor; break;
    case mc_blob::TAG_CURSOR_CONF: s.host = h->confs_h.data(); break;
    case mc_blob::TAG_CURSOR_CLUSTER: p = h->ca.cursor; break;
    case mc_blob::TAG_E: p = d.E; break;
    case mc_blob::TAG_MX: p = d.Mx; break;
    case mc_blob::TAG_MY: p = d.My; break;
    case mc_blob::TAG_SUM_E: p = d.sE; break;
    case mc_blob::TAG_SUM_E2: p = d.sE2; break;
    case mc_blob::TAG_SUM_M: p = d.sM; break;
    case mc_blob::TAG_SUM_M2: p = d.sM2; break;
    case mc_blob::TAG_SUM_M4: p = d.sM4; break;
    case mc_blob::TAG_N_MEAS: p = d.n_meas; break;
    case mc_blob::TAG_PROP: p = d.prop; break;
    case mc_blob::TAG_ACC: p = d.acc; break;
    case mc_blob::TAG_N_SERIES: p = d.n_series; break;
    case mc_blob::TAG_SERIES_A: p = d.ser; break;
    case mc_blob::TAG_G_PROP: p = h->ca.prop; break;
    case mc_blob::TAG_G_ACC: p = h->ca.acc; break;
    case mc_blob::TAG_G_SUM: p = h->ca.sum_size; break;
    case mc_blob::TAG_X_REPLICA: p = h->xch.replica; break;
    case mc_blob::TAG_X_PROP: p = h->xch.prop; break;
    case mc_blob::TAG_X_ACC: p = h->xch.acc; break;
    case mc_blob::TAG_K_SUM_S: p = h->sc.sS; break;
    case mc_blob::TAG_K_N_MEAS: p = h->sc.n_meas; break;
    case mc_blob::TAG_ST_SUM_T: p = h->st.sT; break;
    case mc_blob::TAG_ST_SUM_J: p = h->st.sJ; break;
    case mc_blob::TAG_ST_SUM_J2: p = h->st.sJ2; break;
    case mc_blob::TAG_ST_N_MEAS: p = h->st.n_meas; break;
    case mc_blob::TAG_ST_LAST_I: p = h->st.sI; break;
    case mc_blob::TAG_ST_LAST_K: p = h->st.sK; break;
    }
    s.dev = p;
    return s;
}

extern "C" {

int dqmc_qs_state_size(dqmc_qs_handle *h, size_t *n_bytes) { return mc_state_size(h, "dqmc_qs_state_size", n_bytes); }

int dqmc_qs_state_export(dqmc_qs_handle *h, void *buf, size_t n_bytes)
{
    return mc_state_export(h, "dqmc_qs_state_export", buf, n_bytes);
}

int dqmc_qs_state_import(dqmc_qs_handle *h, const void *buf, size_t n_bytes)
{
    return mc_state_import(h, "dqmc_qs_state_import", buf, n_bytes);
}

}  // extern "C"
