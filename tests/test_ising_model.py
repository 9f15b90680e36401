"""The classical MC flavor on the host side, no GPU: IsingModel's lattice choice, energy and propose_local against the
reference's fixtures (test/modeltests_IsingModel.jl:4-38), the refusal of global moves, and dqmc_mc_create's argument
checks, which come before the device check."""
import ctypes as C

import numpy as np
import pytest


def test_ising_model_lattice_choice(mc_amd):
    m = mc_amd.IsingModel(L=8, dims=2)
    assert m.L == 8 and m.dims == 2 and len(m.l) == 64
    assert isinstance(m.l, mc_amd.SquareLattice)
    m = mc_amd.IsingModel(dims=1, L=10)
    assert isinstance(m.l, mc_amd.Chain) and m.L == 10 and m.dims == 1 and len(m.l) == 10
    m = mc_amd.IsingModel(dims=3, L=3)
    assert isinstance(m.l, mc_amd.CubicLattice) and m.L == 3 and m.dims == 3 and len(m.l) == 27
    m = mc_amd.IsingModel(l=mc_amd.TriangularLattice(4))
    assert len(m.l) == 16 and m.l.neighs.shape == (6, 16)
    assert abs(mc_amd.IsingTc - 2.269185314213022) < 1e-12


def test_ising_energy_and_propose_local_fixtures(mc_amd):
    m3 = mc_amd.IsingModel(dims=3, L=3)
    assert m3.energy(np.arange(1, 28).reshape((3, 3, 3), order="F")) == -18333.0
    m2 = mc_amd.IsingModel(dims=2, L=8)
    conf = np.arange(1, 65).reshape((8, 8), order="F")
    assert m2.energy(conf) == -164320.0
    assert m2.propose_local(13, conf) == 1352.0


def test_global_moves_are_refused(mc_amd):
    with pytest.raises(NotImplementedError, match="global_move"):
        mc_amd.MC(mc_amd.IsingModel(dims=2, L=8), beta=0.35, global_moves=True)


def _create(mc_amd, l, n_sites=None, z=None, neighs=None):
    from montecarlo_jl_amd import _lib
    nb = np.asfortranarray(np.asarray(l.neighs if neighs is None else neighs, dtype=np.int64))
    bonds = np.asfortranarray(np.asarray(l.bonds, dtype=np.int64)[:, :2])
    p = _lib.McParams(n_sites=len(l) if n_sites is None else n_sites, z=nb.shape[0] if z is None else z, n_walkers=4,
                      device_id=0, n_bonds=bonds.shape[0], series_capacity=0,
                      neighs=nb.ctypes.data_as(C.POINTER(C.c_int64)), bonds=bonds.ctypes.data_as(C.POINTER(C.c_int64)))
    h = C.c_void_p()
    rc = _lib.lib().dqmc_mc_create(C.byref(p), C.byref(h))
    return rc, h, _lib.lib().dqmc_mc_last_error(None).decode()


def test_mc_create_validates_before_the_device(mc_amd):
    from montecarlo_jl_amd import _lib
    l = mc_amd.SquareLattice(8)
    bad = l.neighs.copy()
    bad[2, 17] = 65
    rc, h, msg = _create(mc_amd, l, neighs=bad)
    assert rc == _lib.ERR_INVALID and "neighbour index" in msg and not h.value
    bad[2, 17] = 0
    assert _create(mc_amd, l, neighs=bad)[0] == _lib.ERR_INVALID
    # 129 x 129 sites: above the 16384 the LDS holds (the table is never read past the size check)
    big = mc_amd.SquareLattice(129)
    rc, h, msg = _create(mc_amd, big)
    assert rc == _lib.ERR_INVALID and "16384" in msg and not h.value
    z9 = np.vstack([l.neighs, l.neighs, l.neighs[:1]])  # 9 rows
    rc, h, msg = _create(mc_amd, l, neighs=z9)
    assert rc == _lib.ERR_INVALID and "z must be" in msg and not h.value


def test_mc_create_without_a_device_or_with_one(mc_amd):
    """No device: DQMC_ERR_NO_DEVICE and MC(...) raises.  With one (the GPU box runs this file too), the same valid
    arguments create a handle."""
    from montecarlo_jl_amd import _lib
    l = mc_amd.SquareLattice(8)
    rc, h, msg = _create(mc_amd, l)
    if mc_amd.device_count() == 0:
        assert rc == _lib.ERR_NO_DEVICE and "no HIP device" in msg
        with pytest.raises(mc_amd.DQMCError) as e:
            mc_amd.MC(mc_amd.IsingModel(dims=2, L=8), beta=0.35)
        assert e.value.code == _lib.ERR_NO_DEVICE
    else:
        assert rc == 0 and h.value
        assert _lib.lib().dqmc_mc_destroy(h) == 0
