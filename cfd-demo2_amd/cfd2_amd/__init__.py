"""cfd2_amd — MI355X-native coupled incompressible-flow step (drop-in for
``cfd2::solver::gpu::GpuSolver`` of TSultanov/cfd-demo2).

Python mirror of the reference API over the C ABI in include/cfd2_amd.h.
"""
from . import image, mesh, penalty, surface  # noqa: F401
from .mesh import (BackwardsStep, ChannelWithObstacle, CircleObstacle, Mesh,  # noqa: F401
                   RectangularChannel, generate_cut_cell_mesh)
from .solver import (GpuGroup, GpuSolver, adaptive_dt_rule, dist_plan, dist_unique_id,  # noqa: F401,E402
                     scalar_config_default, scalar_scheme_default, scalar_solver_default)
from ._ffi import (Config, Constants, FlowDiag, ScalarConfig, ScalarParams, ScalarScheme,  # noqa: F401,E402
                   ScalarSchemeStats, ScalarSolver, ScalarSolverStats, ScalarSource, ScalarStats, ScalarWall,
                   ScalarWallFlux, build_id, default_config)
