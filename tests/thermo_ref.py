"""The ten thermodynamic scalars of include/dqmc_hip.h "thermodynamics" restated in numpy from the Green's blocks of one
sample and the hopping blocks, term by term as the table defines them (no trace identities), plus the same ten taken
directly from an exact-diagonalisation state.  Test infrastructure: the product never imports this."""
import numpy as np

FIELDS = ("n_up", "n_dn", "n", "D", "m2", "E_kin", "E_int", "E", "N2", "Mz2")


def thermo_ref(G_blocks, T_blocks, U_s):
    """G_blocks: [G] (attractive: G_up = G_dn = G) or [G_up, G_dn], G_ij = <c_i c+_j>; T_blocks likewise; -> array of 10"""
    G = [np.asarray(g, dtype=np.float64) for g in G_blocks]
    T = [np.asarray(t, dtype=np.float64) for t in T_blocks]
    if len(G) == 1:
        G, T = [G[0], G[0]], [T[0], T[0]]
    N = G[0].shape[0]
    I = np.eye(N)
    nu, nd = 1.0 - np.diag(G[0]), 1.0 - np.diag(G[1])
    n_up, n_dn = nu.sum() / N, nd.sum() / N
    n = n_up + n_dn
    D = (nu * nd).sum() / N
    off = 1.0 - I
    e_kin = sum((t * off * (-g.T)).sum() for t, g in zip(T, G)) / N          # sum_{i != j} T_ij (-G_ji)
    e_int = U_s * (D - n / 2 + 0.25)
    e = sum((t * (I - g.T)).sum() for t, g in zip(T, G)) / N + e_int         # sum_ij T_ij (delta_ij - G_ji)
    wick = sum(((I - g.T) * g).sum() for g in G)                            # sum_ij (delta_ij - G_ji) G_ij
    n2 = ((nu.sum() + nd.sum()) ** 2 + wick) / N
    mz2 = ((nu - nd).sum() ** 2 + wick) / N
    return np.array([n_up, n_dn, n, D, n - 2 * D, e_kin, e_int, e, n2, mz2])


def derived(m, beta, N):
    """kappa = beta (<N2> - N <n>^2), chi_s = beta <Mz2> / 4"""
    return beta * (m[8] - N * m[2] ** 2), beta * m[9] / 4.0


def ed_thermo(rho, c, cd, neighs, N, U_s, t, mu):
    """the same ten expectation values straight from the density matrix of oracle.ref_test_oracle.ed_hubbard_greens
    (modes N s + i), for H = -t sum c+_trg c_src + U_s sum (n_up - 1/2)(n_dn - 1/2) - mu sum n"""
    Id = np.eye(rho.shape[0])
    ex = lambda A: float(np.trace(rho @ A))
    nu = [cd[i] @ c[i] for i in range(N)]
    nd = [cd[N + i] @ c[N + i] for i in range(N)]
    Hk = np.zeros_like(rho)
    for s in range(2):
        for src in range(N):
            for trg in neighs[:, src] - 1:
                Hk -= t * cd[N * s + trg] @ c[N * s + src]
    Hi = sum(U_s * (a - 0.5 * Id) @ (b - 0.5 * Id) for a, b in zip(nu, nd))
    Nt, Mz = sum(nu) + sum(nd), sum(nu) - sum(nd)
    n_up, n_dn = ex(sum(nu)) / N, ex(sum(nd)) / N
    D = ex(sum(a @ b for a, b in zip(nu, nd))) / N
    return np.array([n_up, n_dn, n_up + n_dn, D, ex(sum((a - b) @ (a - b) for a, b in zip(nu, nd))) / N, ex(Hk) / N,
                     ex(Hi) / N, ex(Hk + Hi - mu * Nt) / N, ex(Nt @ Nt) / N, ex(Mz @ Mz) / N])


def ed_greens_blocks(rho, c, cd, N):
    """[G_up, G_dn] of the state"""
    G = np.array([[np.trace(rho @ c[a] @ cd[b]) for b in range(2 * N)] for a in range(2 * N)])
    return [G[:N, :N], G[N:, N:]]


def hopping_from_neighs(neighs, N, t, mu):
    T = np.diag(np.full(N, -float(mu)))
    for src in range(N):
        for trg in neighs[:, src] - 1:
            T[trg, src] -= t
    return T
