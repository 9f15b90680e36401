"""numpy restatements for the imaginary-time current recording (include/dqmc_hip.h "current response in imaginary
time"; test helper, numpy only): a row from four packed matrices, the trapezoid Matsubara transform and the
delete-one-walker jackknife of a ratio, each written the plain way, independent of montecarlo_jl_amd/dqmc.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measurement_ref as MR  # noqa: E402


def row(T, g00, g0l, gl0, gll, dir_of, nd, trg_cc, Ct, St):
    """one row of one walker from the packed tuple (lists of per-block matrices), Ct / St [nd, n_q] the phase tables:
    -> (C [K, n_q], S [K, n_q], abs sums of both, x [nd, K]); x = MR.cc_step, the per-slice ccs sums / N without
    delta_tau"""
    x, xa = MR.cc_step(T, g00, g0l, gl0, gll, dir_of, nd, trg_cc)
    return x.T @ Ct, x.T @ St, xa.T @ np.abs(Ct), xa.T @ np.abs(St), x


def row0_tuple(g00):
    """(G00, G0l, Gl0, Gll) of row 0: tau -> 0+, G0l = G00 - I"""
    return g00, [g - np.eye(g.shape[0]) for g in g00], g00, g00


def terms(dir_of, nd, trg_cc):
    """[K]: the number of quad products summed into an element of row k, plus the nd terms of the contraction"""
    ok = (trg_cc >= 0).astype(float)
    K = trg_cc.shape[1]
    per = [np.bincount(np.asarray(dir_of).ravel(), weights=np.outer(ok[:, k], ok[:, k]).ravel(), minlength=nd).sum() for k in range(K)]
    return np.array(per) + nd


def matsubara(lam, h, beta, n_max):
    """lam [R, ...] on tau_r = r h, (R - 1) h = beta: -> (omega [n_max + 1], sum_r h w_r cos(omega_m tau_r) lam[r]), a loop"""
    R = lam.shape[0]
    omega = np.array([2.0 * np.pi * m / beta for m in range(n_max + 1)])
    out = np.zeros((n_max + 1,) + lam.shape[1:], dtype=lam.dtype)
    for m in range(n_max + 1):
        for r in range(R):
            w = 0.5 if r in (0, R - 1) else 1.0
            out[m] += h * w * np.cos(omega[m] * r * h) * lam[r]
    return omega, out


def jackknife(sx, s, f=lambda v: v):
    """brute force: f of the ratio with every walker deleted in turn, by re-summing the others
    -> (f(ratio), sqrt((W - 1) / W sum (f_w - mean f_w)^2))"""
    W = len(s)
    full = f(sx.sum(axis=0) / s.sum())
    loo = []
    for w in range(W):
        keep = [v for v in range(W) if v != w]
        loo.append(f(sx[keep].sum(axis=0) / s[keep].sum()))
    loo = np.array(loo)
    return full, np.sqrt((W - 1) / W * ((loo - loo.mean(axis=0)) ** 2).sum(axis=0))


def jackknife_closed(sx, s):
    """the closed delete-one formula for the plain ratio: r_w = (X - x_w) / (S - s_w)"""
    X, S = sx.sum(axis=0), s.sum()
    r = (X[None, :] - sx) / (S - s)[:, None]
    W = len(s)
    return X / S, np.sqrt((W - 1) / W * ((r - r.mean(axis=0)) ** 2).sum(axis=0))


def pack(C, S, kbond, ssum, kept, left):
    """one walker's sums in the engine's layout from C, S [R, K, n_q]"""
    return np.concatenate([C.ravel(), S.ravel(), kbond, [ssum, kept, left]])
