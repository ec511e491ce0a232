"""ctypes binding of include/cfd2_amd.h (the C ABI of the native library).

The library is built in-tree by ``__graft_entry__.build()`` into
``cfd2_amd/_lib/libcfd2_amd.so``.  There is no fallback: if the library is
missing, importing the solver raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CFD2_AMD_LIB selects an alternative build of the same library (A/B variants
# made by tools/ab_variants.py); default: the in-tree build.
LIB_PATH = os.environ.get("CFD2_AMD_LIB") or os.path.join(_HERE, "_lib", "libcfd2_amd.so")

u32p = C.POINTER(C.c_uint32)
f64p = C.POINTER(C.c_double)


class MeshView(C.Structure):
    _fields_ = [
        ("num_cells", C.c_uint32),
        ("num_faces", C.c_uint32),
        ("face_owner", u32p),
        ("face_neighbor", u32p),
        ("face_boundary", u32p),
        ("face_area", f64p),
        ("face_nx", f64p),
        ("face_ny", f64p),
        ("face_cx", f64p),
        ("face_cy", f64p),
        ("cell_cx", f64p),
        ("cell_cy", f64p),
        ("cell_vol", f64p),
        ("cell_face_offsets", u32p),
        ("cell_faces", u32p),
    ]


class Geometry(C.Structure):
    _fields_ = [("kind", C.c_int32), ("p", C.c_double * 8)]


class Constants(C.Structure):
    _fields_ = [
        ("dt", C.c_float),
        ("dt_old", C.c_float),
        ("time", C.c_float),
        ("viscosity", C.c_float),
        ("density", C.c_float),
        ("component", C.c_uint32),
        ("alpha_p", C.c_float),
        ("scheme", C.c_uint32),
        ("alpha_u", C.c_float),
        ("stride_x", C.c_uint32),
        ("time_scheme", C.c_uint32),
        ("inlet_velocity", C.c_float),
        ("ramp_time", C.c_float),
        ("precond_type", C.c_uint32),
    ]


class Config(C.Structure):
    _fields_ = [
        ("n_outer_correctors", C.c_int32),
        ("convergence_lag", C.c_int32),
        ("fixed_outer", C.c_int32),
        ("fixed_inner", C.c_int32),
        ("max_restart", C.c_int32),
        ("max_outer_restarts", C.c_int32),
        ("fgmres_rtol", C.c_float),
        ("fgmres_atol", C.c_float),
        ("log_level", C.c_int32),
        ("amg_rebuild_interval", C.c_int32),
        ("amg_local_aggregation", C.c_int32),
        ("comm_timeout_s", C.c_float),
    ]


class LinearStats(C.Structure):
    _fields_ = [
        ("iterations", C.c_uint32),
        ("residual", C.c_float),
        ("converged", C.c_int32),
        ("diverged", C.c_int32),
        ("time_s", C.c_double),
    ]


class StepInfo(C.Structure):
    _fields_ = [
        ("should_stop", C.c_int32),
        ("degenerate_count", C.c_uint32),
        ("steady_state_count", C.c_uint32),
        ("outer_residual_u", C.c_float),
        ("outer_residual_p", C.c_float),
        ("outer_iterations", C.c_uint32),
        ("stats_p", LinearStats),
        ("total_linear_iterations", C.c_uint32),
    ]


class CommTimingEntry(C.Structure):  # cfd_comm_timing_entry
    _fields_ = [
        ("category", C.c_int32),
        ("level", C.c_int32),
        ("calls", C.c_uint64),
        ("bytes", C.c_uint64),
        ("wait_us", C.c_double),
        ("comm_us", C.c_double),
    ]


COMM_CATEGORIES = {0: "krylov_halo", 1: "state_halo", 2: "reduction_allgather", 3: "replicated_level_allgather",
                   4: "amg_halo"}


class CommStats(C.Structure):  # cfd_comm_stats
    _fields_ = [
        ("transport", C.c_int32),
        ("comm_count", C.c_int32),
        ("comm_rank", C.c_int32),
        ("device", C.c_int32),
        ("exchanges", C.c_uint64),
        ("allgathers", C.c_uint64),
        ("bytes_sent", C.c_uint64),
        ("bytes_gathered", C.c_uint64),
    ]


TRANSPORTS = {0: "none", 1: "rccl", 2: "in-process", 3: "host-staged"}


class FlowDiag(C.Structure):  # cfd_flow_diag
    _fields_ = [
        ("max_speed", C.c_double),
        ("max_vorticity", C.c_double),
        ("max_divergence", C.c_double),
        ("kinetic_energy", C.c_double),
        ("enstrophy", C.c_double),
        ("force_pressure", C.c_double * 2),
        ("force_viscous", C.c_double * 2),
        ("region_faces", C.c_uint32),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self) -> dict:
        return dict(max_speed=self.max_speed, max_vorticity=self.max_vorticity,
                    max_divergence=self.max_divergence, kinetic_energy=self.kinetic_energy,
                    enstrophy=self.enstrophy, force_pressure=tuple(self.force_pressure),
                    force_viscous=tuple(self.force_viscous), region_faces=self.region_faces)


class ScalarParams(C.Structure):  # cfd_scalar_params
    _fields_ = [("diffusivity", C.c_float), ("inlet_value", C.c_float)]


class ScalarConfig(C.Structure):  # cfd_scalar_config
    _fields_ = [
        ("tol", C.c_float),
        ("max_sweeps", C.c_int32),
        ("check_interval", C.c_int32),
        ("reserved", C.c_int32),
    ]


class ScalarStats(C.Structure):  # cfd_scalar_stats
    _fields_ = [
        ("sweeps", C.c_uint32),
        ("converged", C.c_int32),
        ("last_delta", C.c_float),
        ("dt_used", C.c_float),
        ("min", C.c_double),
        ("max", C.c_double),
        ("integral", C.c_double),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class ScalarSolver(C.Structure):  # cfd_scalar_solver
    _fields_ = [
        ("method", C.c_int32),
        ("max_iters", C.c_int32),
        ("check_interval", C.c_int32),
        ("reserved", C.c_int32),
    ]


class ScalarSolverStats(C.Structure):  # cfd_scalar_solver_stats
    _fields_ = [
        ("method", C.c_int32),
        ("iterations", C.c_int32),
        ("stop_reason", C.c_int32),
        ("polish_sweeps", C.c_uint32),
        ("krylov_residual", C.c_float),
        ("reserved", C.c_int32),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class ScalarScheme(C.Structure):  # cfd_scalar_scheme
    _fields_ = [("scheme", C.c_int32), ("reserved", C.c_int32 * 3)]


class ScalarSchemeStats(C.Structure):  # cfd_scalar_scheme_stats
    _fields_ = [("scheme", C.c_int32), ("clamped_cells", C.c_uint32), ("reserved", C.c_int32 * 2)]

    def as_dict(self) -> dict:
        return {"scheme": self.scheme, "clamped_cells": self.clamped_cells}


class ScalarWall(C.Structure):  # cfd_scalar_wall
    _fields_ = [("kind", C.c_int32), ("value", C.c_float),
                ("x0", C.c_double), ("y0", C.c_double), ("x1", C.c_double), ("y1", C.c_double)]


class ScalarSource(C.Structure):  # cfd_scalar_source
    _fields_ = [("rate", C.c_float), ("reserved", C.c_int32),
                ("x0", C.c_double), ("y0", C.c_double), ("x1", C.c_double), ("y1", C.c_double)]


class ScalarWallFlux(C.Structure):  # cfd_scalar_wall_flux
    _fields_ = [("flux", C.c_double), ("area", C.c_double), ("phi_area", C.c_double),
                ("faces", C.c_uint32), ("kind", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class Buoyancy(C.Structure):  # cfd_buoyancy
    _fields_ = [("gx", C.c_float), ("gy", C.c_float), ("fields", C.c_int32), ("active", C.c_int32),
                ("beta", C.c_float * 4), ("ref", C.c_float * 4)]


class BuoyancyForce(C.Structure):  # cfd_buoyancy_force
    _fields_ = [("force", C.c_double * 2), ("fields", C.c_uint32), ("reserved", C.c_uint32)]


class BoundaryVelocity(C.Structure):  # cfd_boundary_velocity
    _fields_ = [("inlet_faces", C.c_uint32), ("wall_faces", C.c_uint32), ("inlet_scale", C.c_float),
                ("wall_scale", C.c_float), ("active", C.c_int32), ("reserved", C.c_int32),
                ("max_normal_removed", C.c_double)]


class ViscosityModel(C.Structure):  # cfd_viscosity_model
    _fields_ = [("kind", C.c_int32), ("K", C.c_float), ("n", C.c_float), ("gamma_min", C.c_float),
                ("mu0", C.c_float), ("mu_inf", C.c_float), ("lam", C.c_float), ("mu_min", C.c_float),
                ("mu_max", C.c_float)]


class ViscosityStats(C.Structure):  # cfd_viscosity_stats
    _fields_ = [("mu_min", C.c_float), ("mu_max", C.c_float), ("clamped_below", C.c_uint32),
                ("clamped_above", C.c_uint32)]


class PenaltyInfo(C.Structure):  # cfd_penalty_info
    _fields_ = [("active", C.c_int32), ("has_forch", C.c_int32), ("has_target", C.c_int32),
                ("target_scale", C.c_float), ("max_vol_sigma", C.c_double)]


class PenaltyForce(C.Structure):  # cfd_penalty_force
    _fields_ = [("force", C.c_double * 2), ("torque", C.c_double), ("power", C.c_double), ("cells", C.c_uint32),
                ("reserved", C.c_uint32)]


class WallMotion(C.Structure):  # cfd_wall_motion
    _fields_ = [("torque_pressure", C.c_double), ("torque_viscous", C.c_double), ("power", C.c_double),
                ("region_faces", C.c_uint32), ("moving_faces", C.c_uint32)]


class AmgLevel(C.Structure):  # cfd_amg_level
    _fields_ = [
        ("n", C.c_uint32), ("nc", C.c_uint32), ("nnz", C.c_uint64), ("r_nnz", C.c_uint64),
        ("wide", C.c_int32), ("use16", C.c_int32),
        ("row", C.POINTER(C.c_uint32)), ("col", C.POINTER(C.c_uint32)), ("val", C.POINTER(C.c_float)),
        ("dv", C.POINTER(C.c_float)), ("de", C.POINTER(C.c_float)),
        ("agg", C.POINTER(C.c_uint32)), ("r_row", C.POINTER(C.c_uint32)), ("r_col", C.POINTER(C.c_uint32)),
        ("m4", C.POINTER(C.c_int32)), ("m4_more", C.POINTER(C.c_int32)),
    ]


def amg_level_readback(call) -> dict:
    """The two-call read-back of one AMG level (cfd_debug_amg_level and the
    oracle's mirror): ``call(ptr)`` runs the entry on a cfd_amg_level.  Returns
    plain numpy arrays; agg / r_row / r_col / m4 / m4_more are None on a level
    without a coarse level."""
    import numpy as np
    lv = AmgLevel()
    call(C.byref(lv))
    n, nc, nnz, rn = int(lv.n), int(lv.nc), int(lv.nnz), int(lv.r_nnz)
    out = dict(n=n, nc=nc, nnz=nnz, wide=bool(lv.wide), use16=bool(lv.use16),
               row=np.zeros(n + 1, np.uint32), col=np.zeros(nnz, np.uint32), val=np.zeros(nnz, np.float32),
               dv=np.zeros(n, np.float32), de=np.zeros(n, np.float32),
               agg=None, r_row=None, r_col=None, m4=None, m4_more=None)
    if nc:
        out.update(agg=np.zeros(n, np.uint32), r_row=np.zeros(nc + 1, np.uint32), r_col=np.zeros(rn, np.uint32),
                   m4=np.zeros(4 * nc, np.int32), m4_more=np.zeros(nc, np.int32))
    for name, ctype in (("row", C.c_uint32), ("col", C.c_uint32), ("val", C.c_float), ("dv", C.c_float),
                        ("de", C.c_float), ("agg", C.c_uint32), ("r_row", C.c_uint32), ("r_col", C.c_uint32),
                        ("m4", C.c_int32), ("m4_more", C.c_int32)):
        if out[name] is not None:
            setattr(lv, name, out[name].ctypes.data_as(C.POINTER(ctype)))
    call(C.byref(lv))
    assert (int(lv.n), int(lv.nc), int(lv.nnz), int(lv.r_nnz)) == (n, nc, nnz, rn)
    if nc:
        out["m4"] = out["m4"].reshape(nc, 4)
    return out


class StateFileHeader(C.Structure):  # cfd_state_file_header (512 bytes)
    _fields_ = [
        ("magic", C.c_char * 8),
        ("version", C.c_uint32),
        ("header_bytes", C.c_uint32),
        ("num_cells", C.c_uint64),
        ("num_faces", C.c_uint64),
        ("amg_nnz", C.c_uint64),
        ("step_index", C.c_int32),
        ("have_prev", C.c_int32),
        ("inner_has_last", C.c_int32),
        ("inner_last", C.c_float),
        ("n_variance", C.c_uint32),
        ("reserved0", C.c_uint32),
        ("variance", (C.c_double * 2) * 10),
        ("constants", Constants),
        ("info", StepInfo),
        ("amg_age", C.c_uint32),
        ("amg_local_aggregation", C.c_int32),
        ("nranks", C.c_int32),
        ("reserved", C.c_uint8 * 164),
    ]


class ParticleConfig(C.Structure):  # cfd_particle_config
    _fields_ = [("hop_cap", C.c_int32), ("reserved", C.c_int32 * 3)]


class ParticleStats(C.Structure):  # cfd_particle_stats
    _fields_ = [("count", C.c_uint64 * 5), ("wall_contacts", C.c_uint64), ("hops_total", C.c_uint64),
                ("hops_max", C.c_uint64), ("capped", C.c_uint64), ("capacity", C.c_uint64)]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k in ("wall_contacts", "hops_total", "hops_max", "capped", "capacity")}
        d.update({name: int(self.count[k]) for k, name in enumerate(PARTICLE_STATUS)})
        return d


# the status values of a particle slot (CFD_PARTICLE_* of include/cfd2_amd.h) in order
PARTICLE_STATUS = ("empty", "alive", "exited_outlet", "exited_inlet", "outside")


class TstatsConfig(C.Structure):  # cfd_tstats_config
    _fields_ = [("second_moments", C.c_int32), ("scalars", C.c_int32), ("reserved", C.c_int32 * 2)]


class SurfaceInfo(C.Structure):  # cfd_surface_info
    _fields_ = [("faces", C.c_uint32), ("channels", C.c_uint32), ("samples", C.c_uint64), ("total_weight", C.c_double),
                ("stats_on", C.c_int32), ("reserved", C.c_int32)]


# cfd_tstats_get's kind argument (CFD_TSTATS_* of include/cfd2_amd.h) by name
TSTATS_KINDS = {"u": 0, "v": 1, "p": 2, "uu": 3, "uv": 4, "vv": 5, "pp": 6, "phi": 7, "phiphi": 8, "uphi": 9, "vphi": 10}


# cfd_render's field argument (CFD_RENDER_* of include/cfd2_amd.h) by name
RENDER_FIELDS = {"speed": 0, "ux": 1, "uy": 2, "p": 3, "vorticity": 4, "divergence": 5, "scalar": 6}


def default_config(**overrides) -> Config:
    cfg = Config(
        n_outer_correctors=20,
        convergence_lag=1,
        fixed_outer=0,
        fixed_inner=0,
        max_restart=50,
        max_outer_restarts=20,
        fgmres_rtol=1e-5,
        fgmres_atol=1e-7,
        log_level=0,
        amg_rebuild_interval=0,
        amg_local_aggregation=0,
        comm_timeout_s=180.0,
    )
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


# Every symbol include/cfd2_amd.h declares (checked by tests/test_capi.py).
EXPORTED = [
    "cfd_last_error", "cfd_build_id",
    "cfd_mesh_generate_cut_cell", "cfd_mesh_generate_voronoi", "cfd_mesh_generate_delaunay", "cfd_mesh_get_topology", "cfd_mesh_smooth", "cfd_mesh_max_skewness", "cfd_mesh_get_view",
    "cfd_mesh_get_vertices", "cfd_mesh_save", "cfd_mesh_load", "cfd_mesh_destroy",
    "cfd_config_default", "cfd_solver_create", "cfd_solver_destroy", "cfd_set_u", "cfd_set_p",
    "cfd_get_constants", "cfd_set_constants", "cfd_set_dt", "cfd_set_viscosity", "cfd_set_alpha_p",
    "cfd_set_alpha_u", "cfd_set_density", "cfd_set_scheme", "cfd_set_time_scheme",
    "cfd_set_inlet_velocity", "cfd_set_ramp_time", "cfd_set_precond_type", "cfd_update_constants",
    "cfd_initialize_history", "cfd_step", "cfd_get_u", "cfd_get_p", "cfd_get_d_p",
    "cfd_get_step_info", "cfd_set_stop_state", "cfd_set_n_outer_correctors", "cfd_num_cells", "cfd_num_faces", "cfd_state_save", "cfd_state_load", "cfd_synchronize",
    "cfd_group_state_save", "cfd_profile_enable", "cfd_profile_reset",
    "cfd_profile_smoother", "cfd_graph_enable", "cfd_graph_stats", "cfd_amg_levels", "cfd_step_algorithmic_bytes", "cfd_smoother_layout_bytes", "cfd_step_layout_bytes", "cfd_debug_buffer",
    "cfd_debug_buffer_len", "cfd_debug_prepare_assemble", "cfd_debug_reference_semantics", "cfd_debug_amg_info",
    "cfd_debug_column_widths", "cfd_debug_amg_level", "cfd_debug_amg_vcycle",
    "cfd_debug_apply_precond",
    "cfd_dist_unique_id", "cfd_solver_create_dist", "cfd_solver_create_dist_host", "cfd_group_create",
    "cfd_group_step",
    "cfd_dist_info", "cfd_dist_plan", "cfd_debug_rccl_selftest", "cfd_debug_comm_watchdog", "cfd_dist_comm_stats",
    "cfd_debug_group_fault", "cfd_debug_group_fault_midstep", "cfd_group_reset", "cfd_group_needs_restore",
    "cfd_comm_timing_enable", "cfd_comm_timing",
    "cfd_flow_diagnostics", "cfd_get_derived", "cfd_set_force_region", "cfd_min_cell_size",
    "cfd_adaptive_dt_rule", "cfd_adapt_dt", "cfd_group_flow_diagnostics", "cfd_group_adapt_dt",
    "cfd_scalar_config_default", "cfd_scalars_enable", "cfd_set_scalar_params", "cfd_set_scalar", "cfd_get_scalar",
    "cfd_scalar_advance", "cfd_scalar_stats_get",
    "cfd_scalar_solver_default", "cfd_set_scalar_solver", "cfd_scalar_solver_stats_get",
    "cfd_scalar_scheme_default", "cfd_set_scalar_scheme", "cfd_scalar_scheme_stats_get",
    "cfd_set_scalar_wall", "cfd_set_scalar_source", "cfd_scalar_wall_flux_get",
    "cfd_set_scalar_buoyancy", "cfd_set_gravity", "cfd_buoyancy_get", "cfd_buoyancy_force_get",
    "cfd_set_boundary_velocity", "cfd_set_boundary_velocity_scale", "cfd_boundary_velocity_get",
    "cfd_wall_motion_get",
    "cfd_set_viscosity_field", "cfd_get_viscosity_field", "cfd_set_viscosity_model", "cfd_viscosity_evaluate",
    "cfd_get_shear_rate", "cfd_viscosity_stats_get", "cfd_debug_pow_det",
    "cfd_set_penalty", "cfd_set_penalty_scale", "cfd_get_penalty", "cfd_penalty_force_get",
    "cfd_particles_set_mesh", "cfd_particle_config_default", "cfd_particles_enable", "cfd_particles_seed",
    "cfd_particles_advance", "cfd_particles_get", "cfd_particles_stats_get", "cfd_render_particles",
    "cfd_tstats_enable", "cfd_tstats_disable", "cfd_tstats_reset", "cfd_tstats_accumulate", "cfd_tstats_info",
    "cfd_tstats_get", "cfd_tstats_raw_get", "cfd_tstats_raw_set", "cfd_tstats_raw_set_totals",
    "cfd_monitor_enable", "cfd_monitor_disable", "cfd_monitor_record", "cfd_monitor_count", "cfd_monitor_info",
    "cfd_monitor_get",
    "cfd_surface_select", "cfd_surface_geometry_get", "cfd_surface_info_get", "cfd_surface_sample",
    "cfd_surface_stats_enable", "cfd_surface_stats_reset", "cfd_surface_stats_accumulate", "cfd_surface_stats_get",
]

_lib = None


def lib() -> C.CDLL:
    """Load the native library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"native library not built: {LIB_PATH} (run __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.cfd_last_error.restype = C.c_char_p
    L.cfd_build_id.restype = C.c_char_p
    L.cfd_mesh_generate_cut_cell.argtypes = [C.POINTER(Geometry), C.c_double, C.c_double, C.c_double,
                                             C.c_double, C.c_double, C.POINTER(vp)]
    u32pp = C.POINTER(C.POINTER(C.c_uint32))
    L.cfd_mesh_get_topology.argtypes = [vp, u32pp, u32pp, u32pp, u32pp]
    for fn in (L.cfd_mesh_generate_voronoi, L.cfd_mesh_generate_delaunay):
        fn.argtypes = [C.POINTER(Geometry), C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                       C.c_uint64, C.POINTER(vp)]
    L.cfd_mesh_smooth.argtypes = [vp, C.POINTER(Geometry), C.c_double, C.c_int32, C.POINTER(C.c_int32)]
    L.cfd_mesh_max_skewness.argtypes = [vp]
    L.cfd_mesh_max_skewness.restype = C.c_double
    L.cfd_mesh_get_view.argtypes = [vp, C.POINTER(MeshView)]
    L.cfd_mesh_get_vertices.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(f64p), C.POINTER(f64p),
                                        C.POINTER(C.POINTER(C.c_uint8))]
    L.cfd_mesh_save.argtypes = [vp, C.c_char_p]
    L.cfd_mesh_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.cfd_mesh_destroy.argtypes = [vp]
    L.cfd_mesh_destroy.restype = None
    _lib = L
    return L


def build_id() -> str:
    """cfd_build_id(): the source hash the loaded library was built from."""
    return lib().cfd_build_id().decode()


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = lib().cfd_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {status}): {msg}")
