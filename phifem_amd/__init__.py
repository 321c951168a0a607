"""phifem_amd -- MI355X-native hot path of phi-FEM behind phiFEM's Python API.

Host side (this package) mirrors the reference's interface for the path:
  * `phifem_amd.mesh_scripts.compute_tags_measures`  <- src/phifem/mesh_scripts.py:571-653
  * `phifem_amd.interpolate`                         <- dolfinx `Function.interpolate` into Lagrange degree 1-3, the
    level-set of the `discretize=True` leg of tests/test_compute_meshtags.py:153-158
  * `phifem_amd.solver.PhiFEMSolver`                 <- the "define form -> assemble -> solve"
    sequence of demo/weak-dirichlet/flower/main.py:102-186
  * `phifem_amd.solver.StrongDirichletSolver`        <- demo/strong-dirichlet/flower/main.py:83-182
  * `phifem_amd.solver.NeumannRobinSolver`           <- demo/robin/square/main.py:98-190 (simplices) and
    demo/neumann/square/main.py:49-158 (quadrilaterals)
  * `phifem_amd.solver.InterfaceElasticitySolver`    <- demo/interface-elasticity/main.py:145-289
  * `phifem_amd.solver.ElasticitySolver`             <- no counterpart: one-material linear elasticity with the
    displacement prescribed on {phi = 0}, the vector analogue of the weak-Dirichlet scheme (P1^d x P1^d)
  * `phifem_amd.solver.ReactionSolver`, `phifem_amd.solver.HeatSolver`  <- no counterpart: c u - Lap u = f + c g in the
    weak-Dirichlet scheme, and backward Euler / BDF2 time stepping of the heat equation on top of it
  * `phifem_amd.solver.DiffusionSolver`          <- no counterpart: c u - div(kappa grad u) = f + c g with a nodal P1
    conductivity kappa_h > 0 in the same scheme (`HeatSolver(..., kappa=kappa_h)` steps the heat equation with it)
  * `phifem_amd.solver.ConvectionDiffusionSolver` <- no counterpart: c u + beta . grad u - div(kappa grad u) = f + c g with
    a nodal P1 velocity beta_h and optional SUPG (`HeatSolver(..., velocity=beta_h)` steps the transport equation with it)
  * `phifem_amd.partition_cells`, `phifem_amd.distributed.PartitionedProblem`  <- no counterpart: unstructured
    background meshes partitioned over the ranks (the reference is serial, src/phifem/mesh_scripts.py:264)
  * `phifem_amd.refine`, `phifem_amd.prolongate`     <- dolfinx.mesh.refine (demo/interface-elasticity/main.py:390),
    uniform or marked by a cell / edge mask, and the nested coarse -> fine transfer of P1 / P2 nodal functions
  * `phifem_amd.locate`, `phifem_amd.evaluate`, `phifem_amd.interpolate_nonmatching`  <- dolfinx `Function.eval`
    with a bounding-box tree and `interpolate_nonmatching`: P1 / P2 / Q1 functions at arbitrary points
  * `phifem_amd.estimate`, `phifem_amd.mark_dorfler` <- no counterpart (dolfinx users write the residual forms in UFL):
    residual error indicators of the weak-Dirichlet scheme per cell and the Doerfler selection, on the device
  * `phifem_amd.recover_gradient`, `phifem_amd.estimate_zz` <- no counterpart (dolfinx users project the gradient with
    a mass solve): the volume-weighted vertex average of the cell-wise gradient and the Zienkiewicz-Zhu indicator built
    on it, for every solver here
  * `phifem_amd.io`                              <- XDMFFile.write_mesh / write_function / read_mesh
Everything numerical runs in `libphifem_hip.so` (hand-written HIP for gfx950) through the C ABI
declared in `include/phifem_hip.h`.  There is no CPU fallback.
"""
from . import _lib  # noqa: F401  (fails loudly when the HIP library is missing)
from .mesh import Mesh, MeshTags, create_box, create_rectangle, prolongate, refine, restrict  # noqa: F401
from .evaluate import evaluate, interpolate_nonmatching, locate, locator_info  # noqa: F401
from .estimate import estimate, mark_dorfler  # noqa: F401
from .recover import estimate_zz, recover_gradient  # noqa: F401
from . import io  # noqa: F401
from .mesh_scripts import (DeviceExpression, NodalFunction, Quadric, compute_tags_measures,  # noqa: F401
                           interpolate)
from .partition import partition_cells, partition_layout  # noqa: F401
from .distributed import PartitionedProblem  # noqa: F401
from .solver import (ConvectionDiffusionSolver, DiffusionSolver, ElasticitySolver, HeatSolver,  # noqa: F401
                     InterfaceElasticitySolver, NeumannRobinSolver, PhiFEMSolver, ReactionSolver, StrongDirichletSolver)
