"""montecarlo.jl_amd — MI355X-native DQMC sweep engine behind the plugin surface of
ffreyer/MonteCarlo.jl's DQMC flavor (src/flavors/DQMC + src/linalg).

Python here is host plumbing only: lattice/model construction, loop control and the
ctypes binding of libdqmc_hip.so.  All numerics run in hand-written gfx950 kernels;
there is no CPU fallback (importing without the built library raises)."""
from ._lib import DQMCError, lib  # noqa: F401
from .configurations import (CompressedConf, ConfigRecorder, Discarder, compress,  # noqa: F401
                             decompress)
from . import lattices  # noqa: F401
from .lattices import (BilayerSquareLattice, Chain, EachLocalQuadByDistance, EachLocalQuadBySyncedDistance, EachSitePairByDistance,  # noqa: F401
                       CubicLattice, HoneycombLattice, RectangularLattice, SquareLattice, TriangularLattice, build_checkerboard,
                       bond_classes, momentum_grid,
                       strip_subsystem, sublattice_sign)
from .models import (HubbardModel, HubbardModelAttractive, HubbardModelRepulsive,  # noqa: F401
                     rand_conf)
from .sharding import (Communicator, reduce_accumulators, walker_block, walker_range,  # noqa: F401
                       walker_seeds)
from .dqmc import (DQMC, DQMCParameters, CurrentTauSums, matsubara_trapezoid, calculate_greens_AVX, device_count,  # noqa: F401
                   check_covariance_bins, checkerboard_exponentials, checkerboard_seqs, checkerboard_slab, checkerboard_tables,
                   tau_covariance_from_moments,
                   entanglement_from_pair_sums, finish_moments, hopping_exponentials, logdet_matrices, mfma_f64_peak, rdivp, square_tp_factors, triangular_factors,
                   udt_AVX_pivot, vmul)

from .mc import MC, IsingModel, IsingTc, greedy_colouring, reciprocal_vectors  # noqa: F401
from . import qstate  # noqa: F401
from .qstate import ClockModel, PottsModel, QStateMC, QStateModel, qstate_tables, twist_tables  # noqa: F401
from . import sac  # noqa: F401
from .sac import SAC, boson_symmetric_kernel, fermion_kernel  # noqa: F401

lib()  # fail loudly at import time if the HIP library has not been built
