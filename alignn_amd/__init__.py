"""alignn_amd: MI355X (gfx950) native implementation of ALIGNN's message-passing hot path.

Public surface mirrors ``alignn.models.alignn`` of the reference; see ``alignn_amd.alignn``.
"""

from .alignn import ALIGNN, ALIGNNConfig, ALIGNNConv, EdgeGatedGraphConv, MLPLayer, RBFExpansion  # noqa: F401
from .alignn_atomwise import ALIGNNAtomWise, ALIGNNAtomWiseConfig  # noqa: F401
from .cells import CellResult, conventional_cell, primitive_cell  # noqa: F401
from .defects import EV_A2_TO_J_M2, SurfaceResult, VacancyResult, miller_basis, surface_energy, vacancy_formation  # noqa: F401
from .elastic import ElasticResult, elastic_fit, elastic_tensor  # noqa: F401
from .eos import EOS_FORMS, EV_A3_TO_GPA, EVResult, eos_fit, ev_curve  # noqa: F401
from .dynamics import MDResult, run_md  # noqa: F401
from .phonons import EV_TO_CM1, EV_TO_THZ, PhononResult, phonons  # noqa: F401
from .ealignn_atomwise import eALIGNNAtomWise, eALIGNNAtomWiseConfig  # noqa: F401
from .interface import InterfaceResult, MatchResult, interface_energy, match_lattices  # noqa: F401
from .graph import CSRGraph, GraphBatch, build_csr  # noqa: F401
from .neb import NEBResult, neb, neb_interpolate  # noqa: F401
from .idpp import IDPPResult, idpp_forces, idpp_interpolate  # noqa: F401
from .local_order import BondOrderResult, CNAResult, bond_order, cna  # noqa: F401
from .order import (MAX_HKL, MAX_L, MAX_NEIGHBORS, ADFResult, SQResult, SteinhardtResult, adf, steinhardt,  # noqa: F401
                    structure_factor)
from .relax import RelaxResult, relax  # noqa: F401
from .symmetry import (SymmetryResult, distinct_miller_indices, find_symmetry, symmetrize_forces,  # noqa: F401
                       symmetrize_positions, symmetrize_stress)
from .thermo import QHAResult, ThermalResult, qha, thermal_properties, thermal_sums  # noqa: F401
from .trajectory import (A2_FS_TO_CM2_S, DiffusionResult, MSDResult, RDFResult, TrajectoryAnalysis, VACFResult,  # noqa: F401
                         VDOSResult, analyze_md, diffusion, green_kubo, msd, pair_row, rdf, vacf, vdos)
from .vanhove import (FqtResult, VanHoveDistinctResult, VanHoveSelfResult, intermediate_scattering,  # noqa: F401
                      van_hove_distinct, van_hove_self)
from .voronoi import VoronoiResult, voronoi, voronoi_census  # noqa: F401

__version__ = "0.1.0"
