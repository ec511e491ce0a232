"""``GpuSolver`` — Python mirror of the reference's ``cfd2::solver::gpu::GpuSolver``
(src/solver/gpu/structs.rs, solver.rs) over the C ABI.  Every method is one
C call into libcfd2_amd.so; the HIP kernels run on the library's own stream.
There is no CPU fallback: constructing a solver without a GPU raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

from . import _ffi

_vp = C.c_void_p
_bound = False

# GpuSolver.buoyancy_force(): the two force components and the number of driving fields
BuoyancyForce = collections.namedtuple("BuoyancyForce", "fx fy fields")
# GpuSolver.wall_motion(): torques of the pressure and viscous force on the force
# region's walls, the power its selected moving walls deliver, and the face counts
WallMotion = collections.namedtuple("WallMotion", "torque_pressure torque_viscous power region_faces moving_faces")
# GpuSolver.penalty_force(): the force of the fluid on the penalised medium, its torque, the rate
# of work of that force on the moving medium (negative where the body drives the fluid) and the
# number of penalised cells
PenaltyForce = collections.namedtuple("PenaltyForce", "force torque power cells")
# GpuSolver.particles(): float32 x, y and age, uint32 cell and status (CFD_PARTICLE_*), one entry per slot
Particles = collections.namedtuple("Particles", "x y cell status age")


# cfd_exchange_fn / cfd_allgather_fn (include/cfd2_amd.h)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                          C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64))
ALLGATHER_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)


def _bind():
    global _bound
    if _bound:
        return _ffi.lib()
    L = _ffi.lib()
    dp = C.POINTER(C.c_double)
    L.cfd_config_default.argtypes = [C.POINTER(_ffi.Config)]
    L.cfd_config_default.restype = None
    L.cfd_solver_create.argtypes = [C.POINTER(_ffi.MeshView), C.POINTER(_ffi.Config), C.c_int32,
                                    C.POINTER(_vp)]
    L.cfd_solver_destroy.argtypes = [_vp]
    L.cfd_solver_destroy.restype = None
    for n in ("cfd_set_u", "cfd_set_p", "cfd_get_u", "cfd_get_p", "cfd_get_d_p"):
        getattr(L, n).argtypes = [_vp, dp]
    L.cfd_get_constants.argtypes = [_vp, C.POINTER(_ffi.Constants)]
    L.cfd_set_constants.argtypes = [_vp, C.POINTER(_ffi.Constants)]
    for n in ("cfd_set_dt", "cfd_set_viscosity", "cfd_set_alpha_p", "cfd_set_alpha_u",
              "cfd_set_density", "cfd_set_inlet_velocity", "cfd_set_ramp_time"):
        getattr(L, n).argtypes = [_vp, C.c_float]
    for n in ("cfd_set_scheme", "cfd_set_time_scheme", "cfd_set_precond_type"):
        getattr(L, n).argtypes = [_vp, C.c_uint32]
    for n in ("cfd_update_constants", "cfd_initialize_history", "cfd_step", "cfd_synchronize"):
        getattr(L, n).argtypes = [_vp]
    L.cfd_get_step_info.argtypes = [_vp, C.POINTER(_ffi.StepInfo)]
    L.cfd_set_stop_state.argtypes = [_vp, C.c_int32, C.c_uint32, C.c_uint32]
    L.cfd_set_n_outer_correctors.argtypes = [_vp, C.c_int32]
    L.cfd_num_cells.argtypes = [_vp]
    L.cfd_num_cells.restype = C.c_uint32
    L.cfd_num_faces.argtypes = [_vp]
    L.cfd_num_faces.restype = C.c_uint32
    L.cfd_profile_enable.argtypes = [_vp, C.c_int32]
    L.cfd_profile_reset.argtypes = [_vp]
    L.cfd_profile_smoother.argtypes = [_vp, dp, C.POINTER(C.c_uint64), dp]
    L.cfd_graph_enable.argtypes = [_vp, C.c_int32]
    L.cfd_graph_stats.argtypes = [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.cfd_amg_levels.argtypes = [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint64)]
    L.cfd_step_algorithmic_bytes.argtypes = [_vp]
    L.cfd_step_algorithmic_bytes.restype = C.c_double
    L.cfd_smoother_layout_bytes.argtypes = [_vp]
    L.cfd_smoother_layout_bytes.restype = C.c_double
    L.cfd_step_layout_bytes.argtypes = [_vp]
    L.cfd_step_layout_bytes.restype = C.c_double
    L.cfd_debug_buffer_len.argtypes = [_vp, C.c_int32]
    L.cfd_debug_buffer_len.restype = C.c_size_t
    L.cfd_debug_buffer.argtypes = [_vp, C.c_int32, C.POINTER(C.c_float), C.c_size_t]
    L.cfd_debug_prepare_assemble.argtypes = [_vp, C.c_int32]
    L.cfd_debug_reference_semantics.argtypes = [_vp, C.c_int32]
    L.cfd_debug_amg_info.argtypes = [_vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    L.cfd_debug_column_widths.argtypes = [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.cfd_debug_amg_level.argtypes = [_vp, C.c_int32, C.POINTER(_ffi.AmgLevel)]
    L.cfd_debug_apply_precond.argtypes = [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t]
    L.cfd_debug_amg_vcycle.argtypes = [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                       C.c_size_t]
    u8p = C.POINTER(C.c_uint8)
    u32p = C.POINTER(C.c_uint32)
    L.cfd_dist_unique_id.argtypes = [u8p]
    L.cfd_solver_create_dist.argtypes = [C.POINTER(_ffi.MeshView), C.POINTER(_ffi.Config), C.c_int32,
                                         C.c_int32, C.c_int32, u8p, C.POINTER(_vp)]
    L.cfd_solver_create_dist_host.argtypes = [C.POINTER(_ffi.MeshView), C.POINTER(_ffi.Config), C.c_int32,
                                              C.c_int32, C.c_int32, EXCHANGE_FN, ALLGATHER_FN, _vp,
                                              C.POINTER(_vp)]
    L.cfd_group_create.argtypes = [C.POINTER(_ffi.MeshView), C.POINTER(_ffi.Config), C.c_int32,
                                   C.POINTER(C.c_int32), C.POINTER(_vp)]
    L.cfd_group_step.argtypes = [C.POINTER(_vp), C.c_int32]
    L.cfd_dist_info.argtypes = [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), u32p, u32p, u32p]
    L.cfd_dist_plan.argtypes = [C.POINTER(_ffi.MeshView), C.c_int32, C.c_int32, u32p, u32p, u32p, u32p,
                                u32p, u32p, C.POINTER(C.c_int32), u32p, u32p, u32p]
    L.cfd_debug_rccl_selftest.argtypes = [C.c_int32]
    L.cfd_state_save.argtypes = [_vp, C.c_char_p]
    L.cfd_state_load.argtypes = [_vp, C.c_char_p]
    L.cfd_group_state_save.argtypes = [C.POINTER(_vp), C.c_int32, C.c_char_p]
    L.cfd_dist_comm_stats.argtypes = [_vp, C.POINTER(_ffi.CommStats), C.c_int32]
    L.cfd_debug_group_fault.argtypes = [C.POINTER(_vp), C.c_int32, C.c_int32]
    L.cfd_debug_group_fault_midstep.argtypes = [C.POINTER(_vp), C.c_int32, C.c_int32]
    L.cfd_group_reset.argtypes = [C.POINTER(_vp), C.c_int32]
    L.cfd_group_needs_restore.argtypes = [C.POINTER(_vp), C.c_int32]
    L.cfd_group_needs_restore.restype = C.c_int32
    L.cfd_comm_timing_enable.argtypes = [_vp, C.c_int32]
    L.cfd_comm_timing.argtypes = [_vp, C.POINTER(_ffi.CommTimingEntry), C.c_int32, C.POINTER(C.c_int32)]
    L.cfd_flow_diagnostics.argtypes = [_vp, C.POINTER(_ffi.FlowDiag)]
    L.cfd_get_derived.argtypes = [_vp, C.c_int32, dp]
    L.cfd_set_force_region.argtypes = [_vp, C.c_double, C.c_double, C.c_double, C.c_double, u32p]
    L.cfd_min_cell_size.argtypes = [_vp]
    L.cfd_min_cell_size.restype = C.c_double
    L.cfd_adaptive_dt_rule.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, dp, C.POINTER(C.c_int32)]
    L.cfd_adapt_dt.argtypes = [_vp, C.c_double, C.POINTER(C.c_float)]
    L.cfd_group_flow_diagnostics.argtypes = [C.POINTER(_vp), C.c_int32, C.POINTER(_ffi.FlowDiag)]
    L.cfd_group_adapt_dt.argtypes = [C.POINTER(_vp), C.c_int32, C.c_double, C.POINTER(C.c_float)]
    L.cfd_scalar_config_default.argtypes = [C.POINTER(_ffi.ScalarConfig)]
    L.cfd_scalar_config_default.restype = None
    L.cfd_scalars_enable.argtypes = [_vp, C.c_int32, C.POINTER(_ffi.ScalarConfig)]
    L.cfd_set_scalar_params.argtypes = [_vp, C.c_int32, C.POINTER(_ffi.ScalarParams)]
    L.cfd_set_scalar.argtypes = [_vp, C.c_int32, dp]
    L.cfd_get_scalar.argtypes = [_vp, C.c_int32, dp]
    L.cfd_scalar_advance.argtypes = [_vp, C.c_float]
    L.cfd_scalar_stats_get.argtypes = [_vp, C.c_int32, C.POINTER(_ffi.ScalarStats)]
    L.cfd_scalar_solver_default.argtypes = [C.POINTER(_ffi.ScalarSolver)]
    L.cfd_scalar_solver_default.restype = None
    L.cfd_set_scalar_solver.argtypes = [_vp, C.c_int32, C.POINTER(_ffi.ScalarSolver)]
    L.cfd_scalar_solver_stats_get.argtypes = [_vp, C.c_int32, C.POINTER(_ffi.ScalarSolverStats)]
    L.cfd_scalar_scheme_default.argtypes = [C.POINTER(_ffi.ScalarScheme)]
    L.cfd_scalar_scheme_default.restype = None
    L.cfd_set_scalar_scheme.argtypes = [_vp, C.c_int32, C.POINTER(_ffi.ScalarScheme)]
    L.cfd_scalar_scheme_stats_get.argtypes = [_vp, C.c_int32, C.POINTER(_ffi.ScalarSchemeStats)]
    L.cfd_set_scalar_wall.argtypes = [_vp, C.c_int32, C.POINTER(_ffi.ScalarWall), u32p]
    L.cfd_set_scalar_source.argtypes = [_vp, C.c_int32, C.POINTER(_ffi.ScalarSource), u32p]
    L.cfd_scalar_wall_flux_get.argtypes = [_vp, C.c_int32, C.POINTER(_ffi.ScalarWallFlux)]
    L.cfd_set_scalar_buoyancy.argtypes = [_vp, C.c_int32, C.c_float, C.c_float]
    L.cfd_set_gravity.argtypes = [_vp, C.c_float, C.c_float]
    L.cfd_buoyancy_get.argtypes = [_vp, C.POINTER(_ffi.Buoyancy)]
    L.cfd_buoyancy_force_get.argtypes = [_vp, C.POINTER(_ffi.BuoyancyForce)]
    fp = C.POINTER(C.c_float)
    L.cfd_set_boundary_velocity.argtypes = [_vp, C.c_uint32, u32p, fp, fp, u32p]
    L.cfd_set_boundary_velocity_scale.argtypes = [_vp, C.c_float, C.c_float]
    L.cfd_boundary_velocity_get.argtypes = [_vp, C.POINTER(_ffi.BoundaryVelocity)]
    L.cfd_wall_motion_get.argtypes = [_vp, C.c_double, C.c_double, C.POINTER(_ffi.WallMotion)]
    L.cfd_set_viscosity_field.argtypes = [_vp, fp, C.c_uint32]
    L.cfd_get_viscosity_field.argtypes = [_vp, fp]
    L.cfd_set_viscosity_model.argtypes = [_vp, C.POINTER(_ffi.ViscosityModel)]
    L.cfd_viscosity_evaluate.argtypes = [_vp]
    L.cfd_get_shear_rate.argtypes = [_vp, fp]
    L.cfd_viscosity_stats_get.argtypes = [_vp, C.POINTER(_ffi.ViscosityStats)]
    dp_ = C.POINTER(C.c_double)
    L.cfd_debug_pow_det.argtypes = [dp_, dp_, dp_, C.c_uint32]
    L.cfd_set_penalty.argtypes = [_vp, fp, fp, fp, C.c_uint32]
    L.cfd_set_penalty_scale.argtypes = [_vp, C.c_float]
    L.cfd_get_penalty.argtypes = [_vp, C.POINTER(_ffi.PenaltyInfo), fp, fp, fp]
    L.cfd_penalty_force_get.argtypes = [_vp, C.c_double, C.c_double, dp_, C.POINTER(_ffi.PenaltyForce)]
    L.cfd_render_set_polygons.argtypes = [_vp, C.c_uint32, dp, dp, u32p, u32p]
    L.cfd_render_set_view.argtypes = [_vp, C.c_int32, C.c_int32, dp, u32p]
    L.cfd_render.argtypes = [_vp, C.c_int32, C.c_int32, fp, u8p, fp]
    L.cfd_render_owner_get.argtypes = [_vp, u32p]
    L.cfd_particles_set_mesh.argtypes = [_vp, C.c_uint32, dp, dp, u32p, u32p, u32p, u32p]
    L.cfd_particle_config_default.argtypes = [C.POINTER(_ffi.ParticleConfig)]
    L.cfd_particle_config_default.restype = None
    L.cfd_particles_enable.argtypes = [_vp, C.c_uint32, C.POINTER(_ffi.ParticleConfig)]
    L.cfd_particles_seed.argtypes = [_vp, C.c_uint32, C.c_uint32, dp, dp]
    L.cfd_particles_advance.argtypes = [_vp, C.c_float]
    L.cfd_particles_get.argtypes = [_vp, C.c_uint32, C.c_uint32, fp, fp, u32p, u32p, fp]
    L.cfd_particles_stats_get.argtypes = [_vp, C.POINTER(_ffi.ParticleStats)]
    L.cfd_render_particles.argtypes = [_vp, C.c_uint32, u8p]
    u64p = C.POINTER(C.c_uint64)
    L.cfd_tstats_enable.argtypes = [_vp, C.POINTER(_ffi.TstatsConfig)]
    for n in ("cfd_tstats_disable", "cfd_tstats_reset", "cfd_monitor_disable", "cfd_monitor_record"):
        getattr(L, n).argtypes = [_vp]
    L.cfd_tstats_accumulate.argtypes = [_vp, C.c_float]
    L.cfd_tstats_info.argtypes = [_vp, u64p, dp, u32p]
    L.cfd_tstats_get.argtypes = [_vp, C.c_int32, C.c_int32, dp]
    L.cfd_tstats_raw_get.argtypes = [_vp, C.c_uint32, dp]
    L.cfd_tstats_raw_set.argtypes = [_vp, C.c_uint32, dp]
    L.cfd_tstats_raw_set_totals.argtypes = [_vp, C.c_uint64, C.c_double]
    L.cfd_monitor_enable.argtypes = [_vp, C.c_uint32, C.c_uint32, u32p, C.c_int32]
    L.cfd_monitor_count.argtypes = [_vp, u64p, u64p]
    L.cfd_monitor_info.argtypes = [_vp, u32p, u32p, u32p, C.POINTER(C.c_int32)]
    L.cfd_monitor_get.argtypes = [_vp, C.c_uint64, C.c_uint64, fp, fp, fp, C.POINTER(_ffi.FlowDiag)]
    L.cfd_surface_select.argtypes = [_vp, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int32)]
    L.cfd_surface_geometry_get.argtypes = [_vp, u32p, u32p, dp, dp, dp, dp, dp, dp]
    L.cfd_surface_info_get.argtypes = [_vp, C.POINTER(_ffi.SurfaceInfo)]
    L.cfd_surface_sample.argtypes = [_vp, dp]
    L.cfd_surface_stats_enable.argtypes = [_vp, C.c_int32]
    L.cfd_surface_stats_reset.argtypes = [_vp]
    L.cfd_surface_stats_accumulate.argtypes = [_vp, C.c_double]
    L.cfd_surface_stats_get.argtypes = [_vp, C.c_int32, dp]
    _bound = True
    return L


def _boundary_faces(mesh):
    """(face ids, types, f64 centres x, y) of the inlet (1) and wall (3) boundary
    faces of ``mesh``, copied: the solver keeps no reference to the mesh."""
    if mesh is None or not hasattr(mesh, "arrays"):
        return None
    a = mesh.arrays()
    bt = np.asarray(a["face_boundary"]) & 3
    ids = np.nonzero((np.asarray(a["face_neighbor"]) == 0xFFFFFFFF) & ((bt == 1) | (bt == 3)))[0]
    return (ids.astype(np.uint32), bt[ids].astype(np.uint32), np.array(a["face_cx"][ids], np.float64),
            np.array(a["face_cy"][ids], np.float64))


class GpuSolver:
    """Drop-in for ``GpuSolver`` (init/mod.rs:15).  ``mesh`` is a cfd2_amd.Mesh."""

    JACOBI = 0
    AMG = 1

    def __init__(self, mesh, config: _ffi.Config | None = None, device: int = 0, _handle=None,
                  **cfg_overrides):
        L = _bind()
        # the library copies what it needs at creation: no reference to the mesh is kept
        cfg = config if config is not None else _ffi.default_config(**cfg_overrides)
        self._cfg = cfg
        self._n_outer = int(cfg.n_outer_correctors)
        if _handle is None:
            view = mesh.view()
            h = _vp()
            _ffi.check(L.cfd_solver_create(C.byref(view), C.byref(cfg), int(device), C.byref(h)),
                       "cfd_solver_create")
        else:
            h = _handle
        self._h = h
        self.num_cells = int(L.cfd_num_cells(h))
        self.num_faces = int(L.cfd_num_faces(h))
        r, n, c0, c1, ng = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _ffi.check(L.cfd_dist_info(h, C.byref(r), C.byref(n), C.byref(c0), C.byref(c1), C.byref(ng)),
                   "cfd_dist_info")
        self.rank, self.nranks = r.value, n.value
        self.owned = (c0.value, c1.value)  # global cell range this handle owns
        self._render_polygons, self._render_shape, self.last_render_range = False, None, None  # set_render_mesh, set_view
        self.num_global_cells = ng.value
        self._particle_capacity = 0  # enable_particles
        self._bnd = _boundary_faces(mesh)  # set_inlet_profile, set_wall_motion

    @classmethod
    def create_dist(cls, mesh, nranks: int, rank: int, unique_id: bytes, device: int = 0,
                    config: _ffi.Config | None = None, **cfg_overrides):
        """One rank of the RCCL-distributed solver (one process per GPU).  Collective."""
        L = _bind()
        cfg = config if config is not None else _ffi.default_config(**cfg_overrides)
        view = mesh.view()
        uid = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        h = _vp()
        _ffi.check(L.cfd_solver_create_dist(C.byref(view), C.byref(cfg), int(device), int(nranks), int(rank),
                                            uid, C.byref(h)), "cfd_solver_create_dist")
        return cls(mesh, config=cfg, _handle=h)

    @classmethod
    def create_dist_host(cls, mesh, nranks: int, rank: int, device: int = 0,
                         config: _ffi.Config | None = None, **cfg_overrides):
        """One rank of the distributed solver over the host-staged transport
        (test / rehearsal mode: torch.distributed's process group -- gloo --
        carries every halo and all-gather; several ranks may share one GPU).
        torch.distributed must be initialised.  Collective."""
        import torch
        import torch.distributed as dist
        L = _bind()
        cfg = config if config is not None else _ffi.default_config(**cfg_overrides)
        view = mesh.view()

        def buf(addr, nbytes):
            return torch.frombuffer((C.c_uint8 * int(nbytes)).from_address(addr), dtype=torch.uint8)

        def exchange(_user, n, peer, send, sbytes, recv, rbytes):
            try:
                reqs, ks, kr = [], {}, {}
                for i in range(n):
                    q = int(peer[i])
                    if sbytes[i]:
                        reqs.append(dist.isend(buf(send[i], sbytes[i]), q, tag=ks.setdefault(q, 0)))
                        ks[q] += 1
                    if rbytes[i]:
                        reqs.append(dist.irecv(buf(recv[i], rbytes[i]), q, tag=kr.setdefault(q, 0)))
                        kr[q] += 1
                for r in reqs:
                    r.wait()
                return 0
            except Exception as e:  # noqa: BLE001 -- reported through the status code
                print("cfd2 host transport exchange failed:", e, flush=True)
                return 1

        def allgather(_user, send, recv, nbytes):
            try:
                out = [buf(recv + r * nbytes, nbytes) for r in range(nranks)] if nbytes else None
                if nbytes:
                    dist.all_gather(out, buf(send, nbytes).clone())
                return 0
            except Exception as e:  # noqa: BLE001
                print("cfd2 host transport allgather failed:", e, flush=True)
                return 1

        ex_cb, ag_cb = EXCHANGE_FN(exchange), ALLGATHER_FN(allgather)
        h = _vp()
        _ffi.check(L.cfd_solver_create_dist_host(C.byref(view), C.byref(cfg), int(device), int(nranks), int(rank),
                                                 ex_cb, ag_cb, None, C.byref(h)), "cfd_solver_create_dist_host")
        s = cls(mesh, config=cfg, _handle=h)
        s._transport = (ex_cb, ag_cb)  # the callbacks must outlive the handle
        return s

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            _ffi.lib().cfd_solver_destroy(h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- constants (public `constants` field + setters, solver.rs:36-95) --------
    @property
    def constants(self) -> _ffi.Constants:
        c = _ffi.Constants()
        _ffi.check(_ffi.lib().cfd_get_constants(self._h, C.byref(c)), "cfd_get_constants")
        return c

    @constants.setter
    def constants(self, c: _ffi.Constants) -> None:
        _ffi.check(_ffi.lib().cfd_set_constants(self._h, C.byref(c)), "cfd_set_constants")

    def _call(self, name, *args):
        _ffi.check(getattr(_ffi.lib(), name)(self._h, *args), name)

    def set_dt(self, dt): self._call("cfd_set_dt", float(dt))
    def set_viscosity(self, v): self._call("cfd_set_viscosity", float(v))
    def set_alpha_p(self, v): self._call("cfd_set_alpha_p", float(v))
    def set_alpha_u(self, v): self._call("cfd_set_alpha_u", float(v))
    def set_density(self, v): self._call("cfd_set_density", float(v))
    def set_scheme(self, v): self._call("cfd_set_scheme", int(v))
    def set_time_scheme(self, v): self._call("cfd_set_time_scheme", int(v))
    def set_inlet_velocity(self, v): self._call("cfd_set_inlet_velocity", float(v))
    def set_ramp_time(self, v): self._call("cfd_set_ramp_time", float(v))
    def set_precond_type(self, v): self._call("cfd_set_precond_type", int(v))
    def update_constants(self): self._call("cfd_update_constants")

    # -- state ------------------------------------------------------------------
    def set_u(self, u):
        a = np.ascontiguousarray(np.asarray(u, dtype=np.float64).reshape(-1))
        if a.size != 2 * self.num_global_cells:
            raise ValueError("set_u expects one (u, v) pair per mesh cell")
        self._call("cfd_set_u", a.ctypes.data_as(C.POINTER(C.c_double)))

    def set_p(self, p):
        a = np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1))
        if a.size != self.num_global_cells:
            raise ValueError("set_p expects one value per mesh cell")
        self._call("cfd_set_p", a.ctypes.data_as(C.POINTER(C.c_double)))

    def initialize_history(self): self._call("cfd_initialize_history")
    def step(self): self._call("cfd_step")
    def synchronize(self): self._call("cfd_synchronize")

    # set_u / set_p take GLOBAL arrays (a distributed rank keeps its cells + ghosts)
    def _global_len(self):
        return self.num_global_cells

    def get_u(self) -> np.ndarray:
        a = np.zeros(2 * self.num_cells)
        self._call("cfd_get_u", a.ctypes.data_as(C.POINTER(C.c_double)))
        return a.reshape(-1, 2)

    def get_p(self) -> np.ndarray:
        a = np.zeros(self.num_cells)
        self._call("cfd_get_p", a.ctypes.data_as(C.POINTER(C.c_double)))
        return a

    def get_d_p(self) -> np.ndarray:
        a = np.zeros(self.num_cells)
        self._call("cfd_get_d_p", a.ctypes.data_as(C.POINTER(C.c_double)))
        return a

    # -- flow diagnostics, derived fields, adaptive dt (one read-only GPU pass) --
    def flow_diagnostics(self) -> _ffi.FlowDiag:
        """cfd_flow_diagnostics: max speed / vorticity / divergence, kinetic
        energy, enstrophy and the force on the selected wall faces of the
        current state (collective on a distributed rank)."""
        d = _ffi.FlowDiag()
        self._call("cfd_flow_diagnostics", C.byref(d))
        return d

    def _derived(self, kind) -> np.ndarray:
        a = np.zeros(self.num_cells)
        self._call("cfd_get_derived", int(kind), a.ctypes.data_as(C.POINTER(C.c_double)))
        return a

    def speed(self) -> np.ndarray: return self._derived(0)
    def vorticity(self) -> np.ndarray: return self._derived(1)
    def divergence(self) -> np.ndarray: return self._derived(2)

    def set_force_region(self, x0, y0, x1, y1) -> int:
        """Select the wall faces whose centre lies in the closed box (x1 < x0:
        none) for the force sums; returns the faces selected over the whole mesh."""
        n = C.c_uint32()
        self._call("cfd_set_force_region", float(x0), float(y0), float(x1), float(y1), C.byref(n))
        return int(n.value)

    @property
    def min_cell_size(self) -> float:
        """min sqrt(cell_vol) over the whole mesh (the reference's actual_min_cell_size)."""
        return float(_ffi.lib().cfd_min_cell_size(self._h))

    def adapt_dt(self, target_cfl) -> float:
        """The reference's adaptive time step from the current state; returns the dt now set."""
        dt = C.c_float()
        self._call("cfd_adapt_dt", float(target_cfl), C.byref(dt))
        return float(dt.value)

    def step_adaptive(self, target_cfl) -> float:
        """step(), then adapt_dt(target_cfl): one turn of the reference's driver loop."""
        self.step()
        return self.adapt_dt(target_cfl)

    # -- passive scalars (dye, temperature) advected by the solved flow -----------
    def enable_scalars(self, count, tol=None, max_sweeps=None, check_interval=None) -> None:
        """cfd_scalars_enable: (re)allocate ``count`` (1..4) zero fields; 0 frees them.
        Unset options keep cfd_scalar_config_default's values."""
        cfg = scalar_config_default()
        if tol is not None:
            cfg.tol = float(tol)
        if max_sweeps is not None:
            cfg.max_sweeps = int(max_sweeps)
        if check_interval is not None:
            cfg.check_interval = int(check_interval)
        self._call("cfd_scalars_enable", int(count), C.byref(cfg))

    def set_scalar_params(self, field, diffusivity, inlet_value) -> None:
        p = _ffi.ScalarParams(float(diffusivity), float(inlet_value))
        self._call("cfd_set_scalar_params", int(field), C.byref(p))

    def set_scalar(self, field, phi) -> None:
        a = np.ascontiguousarray(np.asarray(phi, dtype=np.float64).reshape(-1))
        if a.size != self.num_cells:
            raise ValueError("set_scalar expects one value per cell")
        self._call("cfd_set_scalar", int(field), a.ctypes.data_as(C.POINTER(C.c_double)))

    def get_scalar(self, field) -> np.ndarray:
        a = np.zeros(self.num_cells)
        self._call("cfd_get_scalar", int(field), a.ctypes.data_as(C.POINTER(C.c_double)))
        return a

    def advance_scalars(self, dt=None) -> None:
        """cfd_scalar_advance: every enabled field one implicit step of ``dt``
        (default: the dt the last step() used) on the fluxes that step left."""
        self._call("cfd_scalar_advance", 0.0 if dt is None else float(dt))

    def scalar_stats(self, field) -> _ffi.ScalarStats:
        st = _ffi.ScalarStats()
        self._call("cfd_scalar_stats_get", int(field), C.byref(st))
        return st

    def set_scalar_solver(self, field, method="bicgstab", max_iters=None, check_interval=None) -> None:
        """cfd_set_scalar_solver: ``method`` "jacobi" (0, the default of every
        field) or "bicgstab" (1): BiCGStab on the Jacobi-scaled system, then
        the Jacobi loop from its answer, which decides ``converged`` as before.
        BiCGStab is for diffusion-dominated fields on fine meshes (D dt / h^2
        well above 1: a temperature), where Jacobi needs thousands of sweeps; a
        dye (D dt / h^2 below 1) converges in a few Jacobi sweeps and gains
        nothing.  Unset options keep cfd_scalar_solver_default's values."""
        cfg = scalar_solver_default()
        methods = {"jacobi": 0, "bicgstab": 1}
        cfg.method = methods[method] if method in methods else int(method)
        if max_iters is not None:
            cfg.max_iters = int(max_iters)
        if check_interval is not None:
            cfg.check_interval = int(check_interval)
        self._call("cfd_set_scalar_solver", int(field), C.byref(cfg))

    def scalar_solver_stats(self, field) -> _ffi.ScalarSolverStats:
        st = _ffi.ScalarSolverStats()
        self._call("cfd_scalar_solver_stats_get", int(field), C.byref(st))
        return st

    def set_scalar_scheme(self, field, scheme="vanleer") -> None:
        """cfd_set_scalar_scheme: ``scheme`` "upwind" (0, the default of every
        field) or "vanleer" (1, "limited linear"): a van Leer-limited
        linear-upwind face value as a deferred correction on phi_old, clamped to
        the local extrema of phi_old so a dye in [0, 1] stays there as under
        upwind.  It costs one gradient pass and a wider assembly per advance
        and keeps a front about half as wide at small CFL.  Takes effect at the
        next advance_scalars()."""
        cfg = scalar_scheme_default()
        schemes = {"upwind": 0, "vanleer": 1}
        cfg.scheme = schemes[scheme] if scheme in schemes else int(scheme)
        self._call("cfd_set_scalar_scheme", int(field), C.byref(cfg))

    def scalar_scheme_stats(self, field) -> _ffi.ScalarSchemeStats:
        st = _ffi.ScalarSchemeStats()
        self._call("cfd_scalar_scheme_stats_get", int(field), C.byref(st))
        return st

    def set_scalar_wall(self, field, kind, value=0.0, box=(0.0, 0.0, -1.0, 0.0)) -> int:
        """cfd_set_scalar_wall: the wall faces whose centre lies in the closed
        ``box`` (x0, y0, x1, y1; x1 < x0: none) get ``kind`` "adiabatic" (0, the
        default of every wall), "value" (1: phi = ``value`` on them, a heated
        obstacle) or "flux" (2: ``value`` is the flux of density * phi per unit
        area into the fluid).  One box and kind per field; takes effect at the
        next advance_scalars().  Returns the faces in the box."""
        kinds = {"adiabatic": 0, "value": 1, "flux": 2}
        x0, y0, x1, y1 = (float(v) for v in box)
        cfg = _ffi.ScalarWall(kinds[kind] if kind in kinds else int(kind), float(value), x0, y0, x1, y1)
        n = C.c_uint32()
        self._call("cfd_set_scalar_wall", int(field), C.byref(cfg), C.byref(n))
        return int(n.value)

    def set_scalar_source(self, field, rate, box=(0.0, 0.0, -1.0, 0.0)) -> int:
        """cfd_set_scalar_source: ``rate`` (density * phi per unit volume and
        time) in the cells whose centre lies in the closed ``box``; rate 0: none.
        Returns the cells in the box."""
        x0, y0, x1, y1 = (float(v) for v in box)
        cfg = _ffi.ScalarSource(float(rate), 0, x0, y0, x1, y1)
        n = C.c_uint32()
        self._call("cfd_set_scalar_source", int(field), C.byref(cfg), C.byref(n))
        return int(n.value)

    def scalar_wall_flux(self, field) -> _ffi.ScalarWallFlux:
        """cfd_scalar_wall_flux_get: the rate at which the selected wall faces
        give density * phi to the fluid (current field), their area and the
        area-weighted sum of the adjacent cell values."""
        st = _ffi.ScalarWallFlux()
        self._call("cfd_scalar_wall_flux_get", int(field), C.byref(st))
        return st

    # -- Boussinesq buoyancy: a scalar field drives the flow ----------------------
    def set_scalar_buoyancy(self, field, beta, ref=0.0) -> None:
        """cfd_set_scalar_buoyancy: field ``field`` drives the momentum equation
        with -density * beta * (phi - ref) * g per unit volume (beta 0, the
        default: it does not).  Explicit coupling: step() reads the field as it
        stands; alternate step() and advance_scalars().  enable_scalars()
        clears it; a checkpoint does not store it."""
        self._call("cfd_set_scalar_buoyancy", int(field), float(beta), float(ref))

    def set_gravity(self, gx, gy) -> None:
        """cfd_set_gravity: the gravity vector of the buoyancy term, e.g. (0, -9.81); (0, 0), the default: none."""
        self._call("cfd_set_gravity", float(gx), float(gy))

    def buoyancy(self) -> dict:
        """cfd_buoyancy_get: ``g``, ``beta`` and ``ref`` per enabled field, and
        ``active``: whether the next step() assembles in the buoyant form."""
        b = _ffi.Buoyancy()
        self._call("cfd_buoyancy_get", C.byref(b))
        n = int(b.fields)
        return dict(g=(float(b.gx), float(b.gy)), beta=[float(v) for v in b.beta[:n]],
                    ref=[float(v) for v in b.ref[:n]], active=bool(b.active))

    def buoyancy_force(self) -> BuoyancyForce:
        """cfd_buoyancy_force_get: (fx, fy, fields): the body force the buoyancy
        term puts on the fluid, summed over the cells in f64 (current fields and
        density), and the number of driving fields.  (+0, +0) when off."""
        f = _ffi.BuoyancyForce()
        self._call("cfd_buoyancy_force_get", C.byref(f))
        return BuoyancyForce(float(f.force[0]), float(f.force[1]), int(f.fields))

    # -- prescribed boundary velocities: inlet profiles and moving walls ------------
    def set_boundary_velocity(self, faces, v) -> int:
        """cfd_set_boundary_velocity: global face indices ``faces`` (inlet or
        wall boundary faces) get the velocities ``v`` [n, 2] in place of
        inlet_velocity * ramp along +x (inlet) or rest (wall); the ramp and the
        scales still multiply them.  A wall entry loses its normal component
        (walls stay impermeable).  A later entry replaces an earlier one of the
        same face; an empty list clears the whole selection.  Takes effect at the
        next step(); a checkpoint does not store it.  Returns the faces selected
        afterwards.  One GPU only."""
        f = np.ascontiguousarray(np.asarray(faces, np.int64).reshape(-1))
        if f.size and (f.min() < 0 or f.max() > 0xFFFFFFFF):
            raise ValueError("face index out of range")
        f = f.astype(np.uint32)
        vv = np.asarray(v, np.float64).reshape(-1, 2)
        if len(vv) != len(f):
            raise ValueError("faces and v differ in length")
        vx = np.ascontiguousarray(vv[:, 0], np.float32)
        vy = np.ascontiguousarray(vv[:, 1], np.float32)
        n = C.c_uint32()
        fpt = C.POINTER(C.c_float)
        self._call("cfd_set_boundary_velocity", len(f), f.ctypes.data_as(C.POINTER(C.c_uint32)),
                   vx.ctypes.data_as(fpt), vy.ctypes.data_as(fpt), C.byref(n))
        return int(n.value)

    def clear_boundary_velocity(self) -> None:
        """The empty selection: the next step() launches the plain kernels again."""
        self._call("cfd_set_boundary_velocity", 0, None, None, None, None)

    def _boundary(self):
        if self._bnd is None:
            raise ValueError("this handle was created without a mesh: use set_boundary_velocity(faces, v)")
        return self._bnd

    def set_inlet_profile(self, fn) -> int:
        """``fn(x, y)`` -> (u, v), evaluated on the host in float64 at every
        inlet face centre (arrays in, arrays or scalars out), e.g. a parabolic
        profile ``lambda x, y: (6 * y * (H - y) / H**2, 0 * y)``.  Returns the
        faces selected afterwards."""
        ids, bt, cx, cy = self._boundary()
        m = bt == 1
        u, v = fn(cx[m], cy[m])
        vel = np.stack([np.broadcast_to(np.asarray(u, np.float64), cx[m].shape),
                        np.broadcast_to(np.asarray(v, np.float64), cx[m].shape)], 1)
        return self.set_boundary_velocity(ids[m], vel)

    def set_wall_motion(self, box, velocity=(0.0, 0.0), omega=0.0, centre=None) -> int:
        """Rigid-body motion of the wall faces whose centre (x, y) lies in the
        closed ``box`` (x0, y0, x1, y1): (U - omega (y - yc), V + omega (x - xc))
        with ``velocity`` = (U, V) and ``centre`` = (xc, yc) (default: the centre
        of the box): a rotating cylinder, a moving belt.  Returns the faces
        selected afterwards."""
        ids, bt, cx, cy = self._boundary()
        x0, y0, x1, y1 = (float(t) for t in box)
        xc, yc = (0.5 * (x0 + x1), 0.5 * (y0 + y1)) if centre is None else (float(centre[0]), float(centre[1]))
        m = (bt == 3) & (cx >= x0) & (cx <= x1) & (cy >= y0) & (cy <= y1)
        if not m.any():
            return int(sum(self.boundary_velocity()[k] for k in ("inlet_faces", "wall_faces")))
        vel = np.stack([float(velocity[0]) - float(omega) * (cy[m] - yc),
                        float(velocity[1]) + float(omega) * (cx[m] - xc)], 1)
        return self.set_boundary_velocity(ids[m], vel)

    def set_boundary_velocity_scale(self, inlet_scale=1.0, wall_scale=1.0) -> None:
        """cfd_set_boundary_velocity_scale: two factors applied on the device to
        the selected inlet and wall velocities (a pulsatile inlet, an oscillating
        rotation: no new upload).  Takes effect at the next step()."""
        self._call("cfd_set_boundary_velocity_scale", float(inlet_scale), float(wall_scale))

    def boundary_velocity(self) -> dict:
        """cfd_boundary_velocity_get: the selected inlet and wall faces, the two
        scales, ``active`` (the next step() runs the BCV kernels) and the largest
        normal component removed from a wall entry."""
        b = _ffi.BoundaryVelocity()
        self._call("cfd_boundary_velocity_get", C.byref(b))
        return dict(inlet_faces=int(b.inlet_faces), wall_faces=int(b.wall_faces), inlet_scale=float(b.inlet_scale),
                    wall_scale=float(b.wall_scale), active=bool(b.active),
                    max_normal_removed=float(b.max_normal_removed))

    def wall_motion(self, x0=0.0, y0=0.0) -> WallMotion:
        """cfd_wall_motion_get: over the wall faces of set_force_region(): the
        torque about (x0, y0) of the pressure and of the viscous force of the
        fluid on them, and the power the selected moving walls deliver to the
        fluid (-sum F_on_wall . u_wall), in f64."""
        w = _ffi.WallMotion()
        self._call("cfd_wall_motion_get", float(x0), float(y0), C.byref(w))
        return WallMotion(float(w.torque_pressure), float(w.torque_viscous), float(w.power), int(w.region_faces),
                          int(w.moving_faces))

    # -- variable viscosity: a viscosity per cell -----------------------------------
    def set_viscosity_field(self, mu) -> None:
        """cfd_set_viscosity_field: ``mu`` [num_cells], every value finite and
        > 0, rounded to float32: the viscosity of each cell, in place of the one
        of set_viscosity().  A face between two cells takes the arithmetic mean,
        a boundary face its cell's value.  Enables the field or replaces its
        values (one upload; nothing is re-captured); takes effect at the next
        step().  Not stored in a checkpoint.  One GPU only."""
        m = np.ascontiguousarray(np.asarray(mu, dtype=np.float64).reshape(-1).astype(np.float32))
        if len(m) == 0:
            raise ValueError("an empty viscosity field: clear_viscosity_field() clears it")
        self._call("cfd_set_viscosity_field", m.ctypes.data_as(C.POINTER(C.c_float)), len(m))

    def clear_viscosity_field(self) -> None:
        """The next step() runs the plain kernels again, with set_viscosity()'s value."""
        self._call("cfd_set_viscosity_field", None, 0)

    def viscosity_field(self) -> np.ndarray:
        """cfd_get_viscosity_field: the float32 field the next step() will read.
        Raises when none is set."""
        out = np.empty(self.num_cells, dtype=np.float32)
        self._call("cfd_get_viscosity_field", out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    VISCOSITY_KINDS = {"none": 0, "power_law": 1, "carreau": 2}

    def set_viscosity_model(self, kind, K=0.0, n=1.0, gamma_min=0.0, mu0=0.0, mu_inf=0.0, lam=0.0, mu_min=0.0,
                            mu_max=0.0) -> None:
        """cfd_set_viscosity_model: ``"power_law"`` (mu = K max(gdot, gamma_min)^(n-1))
        or ``"carreau"`` (mu = mu_inf + (mu0 - mu_inf) (1 + (lam gdot)^2)^((n-1)/2)),
        clamped to [mu_min, mu_max]; evaluated on the device at the start of
        every step() from the velocity the step starts from.  ``"none"`` stops
        the evaluation and leaves the field.  Not stored in a checkpoint."""
        k = self.VISCOSITY_KINDS[kind] if isinstance(kind, str) else int(kind)
        m = _ffi.ViscosityModel(k, float(K), float(n), float(gamma_min), float(mu0), float(mu_inf), float(lam),
                                float(mu_min), float(mu_max))
        self._call("cfd_set_viscosity_model", C.byref(m))

    def viscosity_evaluate(self) -> None:
        """cfd_viscosity_evaluate: the model on the current state, now."""
        self._call("cfd_viscosity_evaluate")

    def shear_rate(self) -> np.ndarray:
        """cfd_get_shear_rate: the float32 shear rate of the last evaluation."""
        out = np.empty(self.num_cells, dtype=np.float32)
        self._call("cfd_get_shear_rate", out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def viscosity_stats(self) -> dict:
        """cfd_viscosity_stats_get: min and max of the field and the cells clamped
        below and above, of the last evaluation."""
        st = _ffi.ViscosityStats()
        self._call("cfd_viscosity_stats_get", C.byref(st))
        return dict(mu_min=float(st.mu_min), mu_max=float(st.mu_max), clamped_below=int(st.clamped_below),
                    clamped_above=int(st.clamped_above))

    # -- volume penalisation: porous zones and immersed bodies ----------------------
    def set_penalty(self, sigma, forch=None, target=None) -> None:
        """cfd_set_penalty: ``sigma`` [num_cells] >= 0, the linear drag
        coefficient of each cell in  -s (u - u_t),  s = sigma + forch |u|;
        ``forch`` [num_cells] >= 0 or None; ``target`` [num_cells, 2], the
        velocity u_t the drag pulls towards, or None (rest).  All rounded to
        float32.  Sets the field or replaces its values (one upload; nothing is
        re-captured); takes effect at the next step().  Refused above the
        handle's limit on vol * sigma (``penalty()["max_vol_sigma"]``).  Not
        stored in a checkpoint.  One GPU only.  penalty.py builds fields."""
        f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1).astype(np.float32))  # noqa: E731
        fp = C.POINTER(C.c_float)
        sg = f32(sigma)
        if len(sg) == 0:
            raise ValueError("an empty penalty field: clear_penalty() clears it")
        fo = None if forch is None else f32(forch)
        tg = None if target is None else f32(target)
        if (fo is not None and len(fo) != len(sg)) or (tg is not None and len(tg) != 2 * len(sg)):
            raise ValueError("penalty: forch [n] and target [n, 2] must match sigma [n]")
        ptr = lambda a: None if a is None else a.ctypes.data_as(fp)  # noqa: E731
        self._call("cfd_set_penalty", ptr(sg), ptr(fo), ptr(tg), len(sg))

    def clear_penalty(self) -> None:
        """The next step() runs the kernels it ran before the field was set."""
        self._call("cfd_set_penalty", None, None, None, 0)

    def set_penalty_scale(self, s) -> None:
        """cfd_set_penalty_scale: the factor on the target velocity, a kernel
        argument (an oscillating body costs no upload)."""
        self._call("cfd_set_penalty_scale", float(s))

    def penalty(self) -> dict:
        """cfd_get_penalty: active (False on a rank handle and in the reference-
        semantics modes, where no field can be set), target_scale, max_vol_sigma and, with a field
        set, the float32 sigma, forch (or None) and target [n, 2] (or None)."""
        info = _ffi.PenaltyInfo()
        self._call("cfd_get_penalty", C.byref(info), None, None, None)
        out = dict(active=bool(info.active), target_scale=float(info.target_scale),
                   max_vol_sigma=float(info.max_vol_sigma), sigma=None, forch=None, target=None)
        if info.active:
            fp = C.POINTER(C.c_float)
            n = self.num_cells
            sg = np.empty(n, np.float32)
            fo = np.empty(n, np.float32) if info.has_forch else None
            tg = np.empty((n, 2), np.float32) if info.has_target else None
            ptr = lambda a: None if a is None else a.ctypes.data_as(fp)  # noqa: E731
            self._call("cfd_get_penalty", None, ptr(sg), ptr(fo), ptr(tg))
            out.update(sigma=sg, forch=fo, target=tg)
        return out

    def penalty_force(self, centre=(0.0, 0.0), box=None) -> PenaltyForce:
        """cfd_penalty_force_get: the force of the fluid on the penalised medium,
        its torque about ``centre``, the rate of work of that force on the moving
        medium (``power``: negative where the body drives the fluid, which then
        receives ``-power``) and the number of penalised cells, over the cells whose centre lies in ``box`` (x0, y0,
        x1, y1; None: every cell), on the current state.  Read-only."""
        b = None if box is None else (C.c_double * 4)(*[float(v) for v in box])
        out = _ffi.PenaltyForce()
        self._call("cfd_penalty_force_get", float(centre[0]), float(centre[1]), b, C.byref(out))
        return PenaltyForce((float(out.force[0]), float(out.force[1])), float(out.torque), float(out.power),
                            int(out.cells))

    # -- frames on the device: a cell field as an RGBA8 image ---------------------
    def set_render_mesh(self, mesh) -> None:
        """cfd_render_set_polygons: upload ``mesh``'s vertices and CCW cell
        polygons (Mesh.vertices(), Mesh.topology()); drops the view.  ``None``
        releases the renderer's device memory.  A MappedMesh has no vertices
        and cannot render.  One GPU only."""
        if mesh is None:
            self._call("cfd_render_set_polygons", 0, None, None, None, None)
            self._render_polygons, self._render_shape, self.last_render_range = False, None, None
            return
        if not hasattr(mesh, "vertices") or not hasattr(mesh, "topology"):
            raise ValueError("set_render_mesh needs a Mesh with vertices and cell polygons: a "
                             f"{type(mesh).__name__} has none and cannot render")
        vx, vy, _ = mesh.vertices()
        t = mesh.topology()
        self.set_render_polygons(vx, vy, t["cell_vertex_offsets"], t["cell_vertices"])

    def set_render_polygons(self, vx, vy, cell_vertex_offsets, cell_vertices) -> None:
        """cfd_render_set_polygons from arrays: one offset per cell plus one,
        ``cell_vertices[offsets[c]:offsets[c + 1]]`` the CCW polygon of cell c."""
        vx = np.ascontiguousarray(vx, dtype=np.float64)
        vy = np.ascontiguousarray(vy, dtype=np.float64)
        off = np.ascontiguousarray(cell_vertex_offsets, dtype=np.uint32)
        idx = np.ascontiguousarray(cell_vertices, dtype=np.uint32)
        if vx.ndim != 1 or vx.shape != vy.shape or len(vx) == 0:
            raise ValueError("set_render_polygons expects two vertex arrays of one length > 0")
        if off.shape != (self.num_global_cells + 1,):  # (a distributed handle is refused by the library)
            raise ValueError("set_render_polygons expects one offset per cell plus one")
        if idx.ndim != 1 or len(idx) < int(off[-1]):
            raise ValueError("set_render_polygons: cell_vertices is shorter than cell_vertex_offsets[-1]")
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
        self._call("cfd_render_set_polygons", len(vx), vx.ctypes.data_as(dp), vy.ctypes.data_as(dp),
                   off.ctypes.data_as(up), idx.ctypes.data_as(up))  # a refused call changes nothing
        self._render_polygons, self._render_shape, self.last_render_range = True, None, None

    def set_view(self, width, height, box=None) -> int:
        """cfd_render_set_view: build the ownership map of a ``height`` x
        ``width`` image (1..8192 each) of the world box ``(x0, y0, x1, y1)``;
        ``None``: the bounding box of the polygons.  Once per view, not per
        frame.  Returns the pixels that have an owner."""
        b = None
        if box is not None:
            if len(box) != 4:
                raise ValueError("box = (x0, y0, x1, y1)")
            b = (C.c_double * 4)(*[float(v) for v in box])
        n = C.c_uint32(0)
        self._render_shape = None  # a refused call leaves no view
        self._call("cfd_render_set_view", int(width), int(height), b, C.byref(n))
        self._render_shape = (int(height), int(width))
        return int(n.value)

    def _render_need_view(self):
        # the output is sized by the view this object set: refused here, in the library's words, without one
        if not self._render_polygons:
            raise RuntimeError("render failed: no polygons (set_render_mesh)")
        if self._render_shape is None:
            raise RuntimeError("render failed: no view (set_view)")
        return self._render_shape

    def render(self, field="speed", range=None, scalar=None) -> np.ndarray:
        """cfd_render: the current state's ``field`` ("speed", "ux", "uy", "p",
        "vorticity", "divergence", "scalar", or 0..6) as an (H, W, 4) uint8
        RGBA image, row 0 the top, through the reference's blue-green-red map
        over ``range`` = (lo, hi); ``None``: the minimum and maximum over all
        cells, found on the device.  ``scalar``: the field index of "scalar"
        (default 0).  The range used is kept as ``last_render_range``.  Pixels
        off the mesh are (0, 0, 0, 0), NaN cells (0, 0, 0, 255)."""
        if isinstance(field, str):
            if field not in _ffi.RENDER_FIELDS:
                raise ValueError(f"render: unknown field {field!r} (one of {', '.join(_ffi.RENDER_FIELDS)})")
            field = _ffi.RENDER_FIELDS[field]
        h, w = self._render_need_view()
        out = np.empty((h, w, 4), dtype=np.uint8)
        r = None if range is None else (C.c_float * 2)(float(range[0]), float(range[1]))
        used = (C.c_float * 2)()
        self._call("cfd_render", int(field), 0 if scalar is None else int(scalar), r,
                   out.ctypes.data_as(C.POINTER(C.c_uint8)), used)
        self.last_render_range = (np.float32(used[0]), np.float32(used[1]))
        return out

    def render_owner(self) -> np.ndarray:
        """cfd_render_owner_get: the (H, W) uint32 ownership map of the view:
        the cell under each pixel centre, 0xFFFFFFFF where there is none."""
        h, w = self._render_need_view()
        out = np.empty((h, w), dtype=np.uint32)
        self._call("cfd_render_owner_get", out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    # -- tracer particles on the device -------------------------------------------
    def set_particle_mesh(self, mesh) -> None:
        """cfd_particles_set_mesh: upload ``mesh``'s vertices, CCW cell polygons
        and face vertices (Mesh.vertices(), Mesh.topology()); frees the particle
        set of an earlier mesh.  ``None`` releases the module's device memory.
        One GPU only."""
        if mesh is None:
            self._call("cfd_particles_set_mesh", 0, None, None, None, None, None, None)
            self._particle_capacity = 0
            return
        if not hasattr(mesh, "vertices") or not hasattr(mesh, "topology"):
            raise ValueError("set_particle_mesh needs a Mesh with vertices and cell polygons: a "
                             f"{type(mesh).__name__} has none")
        vx, vy, _ = mesh.vertices()
        t = mesh.topology()
        self.set_particle_polygons(vx, vy, t["cell_vertex_offsets"], t["cell_vertices"], t["face_v1"], t["face_v2"])

    def set_particle_polygons(self, vx, vy, cell_vertex_offsets, cell_vertices, face_v1, face_v2) -> None:
        """cfd_particles_set_mesh from arrays."""
        vx = np.ascontiguousarray(vx, dtype=np.float64)
        vy = np.ascontiguousarray(vy, dtype=np.float64)
        off = np.ascontiguousarray(cell_vertex_offsets, dtype=np.uint32)
        idx = np.ascontiguousarray(cell_vertices, dtype=np.uint32)
        v1 = np.ascontiguousarray(face_v1, dtype=np.uint32)
        v2 = np.ascontiguousarray(face_v2, dtype=np.uint32)
        if vx.ndim != 1 or vx.shape != vy.shape or len(vx) == 0:
            raise ValueError("set_particle_polygons expects two vertex arrays of one length > 0")
        if off.shape != (self.num_global_cells + 1,):  # (a distributed handle is refused by the library)
            raise ValueError("set_particle_polygons expects one offset per cell plus one")
        if idx.ndim != 1 or len(idx) < int(off[-1]):
            raise ValueError("set_particle_polygons: cell_vertices is shorter than cell_vertex_offsets[-1]")
        # (a distributed handle, which holds a part of the faces, is refused by the library)
        if self.nranks == 1 and (v1.shape != (self.num_faces,) or v2.shape != (self.num_faces,)):
            raise ValueError("set_particle_polygons expects two vertex indices per face")
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
        self._call("cfd_particles_set_mesh", len(vx), vx.ctypes.data_as(dp), vy.ctypes.data_as(dp),
                   off.ctypes.data_as(up), idx.ctypes.data_as(up), v1.ctypes.data_as(up), v2.ctypes.data_as(up))
        self._particle_capacity = 0  # a refused call changes nothing; an accepted one frees the set

    def enable_particles(self, n, hop_cap=64) -> None:
        """cfd_particles_enable: ``n`` slots (1..2^24), all EMPTY; 0 frees them.
        ``hop_cap``: the face crossings a particle may make in one advance."""
        cfg = _ffi.ParticleConfig(hop_cap=int(hop_cap))
        self._call("cfd_particles_enable", int(n), C.byref(cfg))
        self._particle_capacity = int(n)

    def seed_particles(self, xy, first=0) -> None:
        """cfd_particles_seed: overwrite slots ``[first, first + len(xy))`` with
        the (n, 2) positions ``xy`` (rounded to float32 once), age 0, and locate
        them on the device.  Re-seeding a ring of slots at a rake every step
        draws a streakline."""
        xy = np.asarray(xy, dtype=np.float64)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("seed_particles expects an (n, 2) array")
        x, y = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
        dp = C.POINTER(C.c_double)
        self._call("cfd_particles_seed", int(first), len(x), x.ctypes.data_as(dp), y.ctypes.data_as(dp))

    def advance_particles(self, dt=None) -> None:
        """cfd_particles_advance: carry every ALIVE particle through the current
        velocity field for ``dt`` (None: the dt of the last step)."""
        self._call("cfd_particles_advance", 0.0 if dt is None else float(dt))

    def particles(self) -> Particles:
        """cfd_particles_get of every slot: a ``Particles`` tuple of float32 x, y,
        age and uint32 cell, status arrays."""
        n = self._particle_capacity
        if not n:
            raise RuntimeError("particles failed: particles are not enabled (enable_particles)")
        x, y, age = (np.empty(n, np.float32) for _ in range(3))
        cell, status = np.empty(n, np.uint32), np.empty(n, np.uint32)
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        self._call("cfd_particles_get", 0, n, x.ctypes.data_as(fp), y.ctypes.data_as(fp), cell.ctypes.data_as(up),
                   status.ctypes.data_as(up), age.ctypes.data_as(fp))
        return Particles(x, y, cell, status, age)

    def particle_stats(self) -> dict:
        """cfd_particles_stats_get: the slots per status (by name), wall_contacts,
        hops_total / hops_max / capped of the last advance, and the capacity."""
        st = _ffi.ParticleStats()
        self._call("cfd_particles_stats_get", C.byref(st))
        return st.as_dict()

    def render_particles(self, colour=(255, 255, 255, 255)) -> np.ndarray:
        """cfd_render_particles: the last ``render()`` frame with every ALIVE
        particle in the view stamped as one pixel of ``colour`` (R, G, B, A)."""
        h, w = self._render_need_view()
        r, g, b, a = (int(v) & 0xFF for v in colour)
        out = np.empty((h, w, 4), dtype=np.uint8)
        self._call("cfd_render_particles", r | g << 8 | b << 16 | a << 24, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out

    # -- time-averaged fields and Reynolds stresses, accumulated on the device ------
    def enable_time_stats(self, second_moments=True, scalars=True) -> None:
        """cfd_tstats_enable: allocate and zero the f64 planes: the means of u, v,
        p; with ``second_moments`` the M planes of uu, uv, vv, pp; with
        ``scalars`` every scalar field enabled now (mean and variance, and with
        second moments the fluxes u phi, v phi).  A second call starts afresh."""
        cfg = _ffi.TstatsConfig(1 if second_moments else 0, 1 if scalars else 0)
        self._call("cfd_tstats_enable", C.byref(cfg))

    def disable_time_stats(self) -> None:
        self._call("cfd_tstats_disable")

    def reset_time_stats(self) -> None:
        """cfd_tstats_reset: no samples, zero weight, zero planes."""
        self._call("cfd_tstats_reset")

    def accumulate_time_stats(self, weight=None) -> None:
        """cfd_tstats_accumulate: the current state enters the statistics with
        ``weight`` (None: the dt of the last step).  Asynchronous."""
        self._call("cfd_tstats_accumulate", 0.0 if weight is None else float(weight))

    def time_stats_info(self) -> dict:
        """cfd_tstats_info: ``samples``, ``total_weight`` and ``planes``."""
        n, w, p = C.c_uint64(), C.c_double(), C.c_uint32()
        self._call("cfd_tstats_info", C.byref(n), C.byref(w), C.byref(p))
        return dict(samples=int(n.value), total_weight=float(w.value), planes=int(p.value))

    def time_stats(self, kind, field=0) -> np.ndarray:
        """cfd_tstats_get: one float64 value per cell of ``kind``: a mean "u",
        "v", "p", "phi", or a covariance "uu", "uv", "vv", "pp", "phiphi",
        "uphi", "vphi" (or 0..10); ``field``: the scalar field of the phi kinds."""
        if isinstance(kind, str):
            if kind not in _ffi.TSTATS_KINDS:
                raise ValueError(f"time_stats: unknown kind {kind!r} (one of {', '.join(_ffi.TSTATS_KINDS)})")
            kind = _ffi.TSTATS_KINDS[kind]
        a = np.zeros(self.num_cells)
        self._call("cfd_tstats_get", int(kind), int(field), a.ctypes.data_as(C.POINTER(C.c_double)))
        return a

    def export_time_stats(self) -> dict:
        """The statistics as they stand: ``planes`` (P, N) float64 (cfd_tstats_raw_get
        of every plane), ``samples`` and ``total_weight``.  Checkpoints do not
        hold them: keep this next to the state file."""
        info = self.time_stats_info()
        planes = np.zeros((info["planes"], self.num_cells))
        for q in range(info["planes"]):
            self._call("cfd_tstats_raw_get", q, planes[q].ctypes.data_as(C.POINTER(C.c_double)))
        return dict(planes=planes, samples=info["samples"], total_weight=info["total_weight"])

    def import_time_stats(self, d) -> None:
        """Put back what ``export_time_stats`` returned, into statistics enabled the
        same way: the run continues bit for bit."""
        planes = np.ascontiguousarray(d["planes"], dtype=np.float64)
        info = self.time_stats_info()
        if planes.shape != (info["planes"], self.num_cells):
            raise ValueError(f"import_time_stats expects planes of shape {(info['planes'], self.num_cells)}: enable "
                             "the statistics as they were enabled for the export")
        for q in range(info["planes"]):
            self._call("cfd_tstats_raw_set", q, planes[q].ctypes.data_as(C.POINTER(C.c_double)))
        self._call("cfd_tstats_raw_set_totals", int(d["samples"]), float(d["total_weight"]))

    # -- wall surface distributions: pressure, shear and heat flux per wall face ------
    def select_surface(self, box) -> int:
        """cfd_surface_select: the wall faces whose centre lies in the closed box
        ``(x0, y0, x1, y1)`` (set_force_region's rule), ordered by cell, then
        slot; returns their number.  ``x1 < x0`` clears the surface.  A second
        call replaces the surface and resets its statistics."""
        x0, y0, x1, y1 = (float(v) for v in box)
        n = C.c_int32()
        self._call("cfd_surface_select", x0, y0, x1, y1, C.byref(n))
        return int(n.value)

    def surface_info(self) -> dict:
        """cfd_surface_info_get: ``faces``, ``channels``, ``samples``,
        ``total_weight`` and ``stats_on``."""
        d = _ffi.SurfaceInfo()
        self._call("cfd_surface_info_get", C.byref(d))
        return dict(faces=int(d.faces), channels=int(d.channels), samples=int(d.samples),
                    total_weight=float(d.total_weight), stats_on=bool(d.stats_on))

    def surface_geometry(self) -> dict:
        """cfd_surface_geometry_get: per face ``cell``, ``slot``, the float64 face
        centre ``cx``, ``cy`` the selection tested, and the float32 ``nx``,
        ``ny`` (out of the cell), ``area``, ``dist_e`` the channels use, widened."""
        n = self.surface_info()["faces"]
        g = dict(cell=np.zeros(n, np.uint32), slot=np.zeros(n, np.uint32))
        for k in ("cx", "cy", "nx", "ny", "area", "dist_e"):
            g[k] = np.zeros(n)
        u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        self._call("cfd_surface_geometry_get", g["cell"].ctypes.data_as(u32p), g["slot"].ctypes.data_as(u32p),
                   *(g[k].ctypes.data_as(dp) for k in ("cx", "cy", "nx", "ny", "area", "dist_e")))
        return g

    @staticmethod
    def _surface_dict(ch) -> dict:
        nf = (len(ch) - 5) // 2
        return dict(p=ch[0], force_p=np.stack([ch[1], ch[2]], 1), force_v=np.stack([ch[3], ch[4]], 1),
                    flux=[ch[5 + 2 * f] for f in range(nf)], phi=[ch[6 + 2 * f] for f in range(nf)], channels=ch)

    def _surface_read(self, name, *args) -> dict:
        info = self.surface_info()
        ch = np.zeros((info["channels"], info["faces"]))
        self._call(name, *args, ch.ctypes.data_as(C.POINTER(C.c_double)))
        return self._surface_dict(ch)

    def surface(self) -> dict:
        """cfd_surface_sample: the float64 channels of the current state, per face:
        ``p``, ``force_p`` (n, 2) and ``force_v`` (n, 2), the pressure and viscous
        force of the fluid on the face (the terms of flow_diagnostics' sums), and
        per scalar field ``flux[f]`` (the term of scalar_wall_flux's sum) and
        ``phi[f]``; ``channels`` holds them all, (5 + 2 fields, n)."""
        return self._surface_read("cfd_surface_sample")

    def enable_surface_stats(self, on=True) -> None:
        """cfd_surface_stats_enable: running mean and variance of every channel."""
        self._call("cfd_surface_stats_enable", 1 if on else 0)

    def reset_surface_stats(self) -> None:
        self._call("cfd_surface_stats_reset")

    def accumulate_surface_stats(self, weight=None) -> None:
        """cfd_surface_stats_accumulate: the current state's channels enter the
        statistics with ``weight`` (None: the dt of the last step).  Asynchronous."""
        self._call("cfd_surface_stats_accumulate", 0.0 if weight is None else float(weight))

    def surface_stats(self, kind="mean") -> dict:
        """cfd_surface_stats_get: ``surface()``'s layout holding the ``"mean"`` (0)
        or the ``"variance"`` (1) of every channel."""
        kinds = {"mean": 0, "variance": 1}
        if isinstance(kind, str):
            if kind not in kinds:
                raise ValueError(f"surface_stats: unknown kind {kind!r} (one of {', '.join(kinds)})")
            kind = kinds[kind]
        return self._surface_read("cfd_surface_stats_get", int(kind))

    # -- monitor history: probes and the flow diagnostics recorded on the device ----
    def enable_monitor(self, capacity, probe_cells=(), diagnostics=True) -> None:
        """cfd_monitor_enable: a ring of ``capacity`` samples (1..2^20) of the
        cells ``probe_cells`` (at most 1024) and, with ``diagnostics``, of the
        flow diagnostics."""
        cells = np.ascontiguousarray(probe_cells, dtype=np.int64).reshape(-1)
        if cells.size and (cells.min() < 0 or cells.max() > 0xFFFFFFFF):
            raise ValueError("enable_monitor: probe cells are cell indices")
        c32 = cells.astype(np.uint32)
        self._call("cfd_monitor_enable", int(capacity), len(c32), c32.ctypes.data_as(C.POINTER(C.c_uint32)),
                   1 if diagnostics else 0)

    def disable_monitor(self) -> None:
        self._call("cfd_monitor_disable")

    def record_monitor(self) -> None:
        """cfd_monitor_record: one sample of the current state.  Asynchronous:
        nothing is copied to the host and nothing waits."""
        self._call("cfd_monitor_record")

    def monitor_count(self) -> tuple:
        """cfd_monitor_count: (samples ever recorded, samples held)."""
        t, h = C.c_uint64(), C.c_uint64()
        self._call("cfd_monitor_count", C.byref(t), C.byref(h))
        return int(t.value), int(h.value)

    def monitor(self) -> dict:
        """cfd_monitor_get of every held sample, oldest first: float32 ``time``
        and ``dt`` (n,), ``probes`` (n, P, 3 + scalar fields): u.x, u.y, p and the
        fields; ``total``; and with diagnostics ``diag``, a dict of float64
        arrays by the names of FlowDiag (``region_faces`` uint32), and
        ``diag_raw``, the n FlowDiag structures as they came."""
        total, held = self.monitor_count()
        _, npr, fields, with_diag = self.monitor_info()
        t, dt = np.zeros(held, np.float32), np.zeros(held, np.float32)
        fp = C.POINTER(C.c_float)
        probes = np.zeros((held, npr, 3 + fields), np.float32)
        diag = (_ffi.FlowDiag * max(held, 1))()
        if held:
            self._call("cfd_monitor_get", 0, held, t.ctypes.data_as(fp), dt.ctypes.data_as(fp),
                       probes.ctypes.data_as(fp), diag if with_diag else None)
        out = dict(time=t, dt=dt, probes=probes, total=total)
        if with_diag:
            raw = [_ffi.FlowDiag.from_buffer_copy(bytes(diag[k])) for k in range(held)]
            cols = {}
            for name, ctype in _ffi.FlowDiag._fields_:
                if name == "reserved":
                    continue
                vals = [getattr(d, name) for d in raw]
                if name in ("force_pressure", "force_viscous"):
                    cols[name] = np.array([tuple(v) for v in vals], dtype=np.float64).reshape(held, 2)
                else:
                    cols[name] = np.array(vals, dtype=np.uint32 if name == "region_faces" else np.float64)
            out["diag"], out["diag_raw"] = cols, raw
        return out

    def monitor_info(self) -> tuple:
        """cfd_monitor_info: (capacity, probes, scalar fields per probe, with diagnostics)."""
        v = [C.c_uint32() for _ in range(3)]
        d = C.c_int32()
        self._call("cfd_monitor_info", C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(d))
        return int(v[0].value), int(v[1].value), int(v[2].value), bool(d.value)

    # -- public status fields of the reference struct -------------------------
    def step_info(self) -> _ffi.StepInfo:
        i = _ffi.StepInfo()
        self._call("cfd_get_step_info", C.byref(i))
        return i

    # should_stop / degenerate_count / steady_state_count are plain public
    # fields in the reference (structs.rs:244-247): the GUI clears should_stop
    # before it resumes stepping (src/ui/app.rs:852-857)
    def set_stop_state(self, should_stop, degenerate_count, steady_state_count):
        self._call("cfd_set_stop_state", 1 if should_stop else 0, int(degenerate_count), int(steady_state_count))

    def _set_stop_field(self, **kw):
        i = self.step_info()
        cur = dict(should_stop=i.should_stop, degenerate_count=i.degenerate_count,
                   steady_state_count=i.steady_state_count)
        cur.update(kw)
        self.set_stop_state(**cur)

    @property
    def should_stop(self) -> bool: return bool(self.step_info().should_stop)
    @should_stop.setter
    def should_stop(self, v): self._set_stop_field(should_stop=bool(v))
    @property
    def degenerate_count(self) -> int: return int(self.step_info().degenerate_count)
    @degenerate_count.setter
    def degenerate_count(self, v): self._set_stop_field(degenerate_count=int(v))
    @property
    def steady_state_count(self) -> int: return int(self.step_info().steady_state_count)
    @steady_state_count.setter
    def steady_state_count(self, v): self._set_stop_field(steady_state_count=int(v))
    @property
    def outer_iterations(self) -> int: return int(self.step_info().outer_iterations)

    # n_outer_correctors: a public field as well (structs.rs:238), read by every
    # step (coupled_solver.rs:111); its initial value comes from the config
    @property
    def n_outer_correctors(self) -> int: return int(self._n_outer)
    @n_outer_correctors.setter
    def n_outer_correctors(self, v):
        self._call("cfd_set_n_outer_correctors", int(v))
        self._n_outer = int(v)

    # -- instrumentation --------------------------------------------------------
    def profile_enable(self, on=True): self._call("cfd_profile_enable", 1 if on else 0)
    def profile_reset(self): self._call("cfd_profile_reset")

    def graph_enable(self, on=True): self._call("cfd_graph_enable", 1 if on else 0)

    def graph_stats(self):
        """(enabled, graphs captured, iterations replayed) of the FGMRES iteration graphs."""
        e, c, r = C.c_int32(), C.c_uint64(), C.c_uint64()
        self._call("cfd_graph_stats", C.byref(e), C.byref(c), C.byref(r))
        return bool(e.value), c.value, r.value

    def profile_smoother(self):
        ms, n, b = C.c_double(), C.c_uint64(), C.c_double()
        self._call("cfd_profile_smoother", C.byref(ms), C.byref(n), C.byref(b))
        return ms.value, n.value, b.value

    def amg_levels(self):
        nl = C.c_int32()
        rows = (C.c_uint32 * 20)()
        nnz = (C.c_uint64 * 20)()
        self._call("cfd_amg_levels", C.byref(nl), rows, nnz)
        return [(int(rows[i]), int(nnz[i])) for i in range(nl.value)]

    def amg_setup_info(self):
        """(setup path: 0 not built / 1 host / 2 device, [digest of every level image])."""
        path = C.c_int32()
        dig = []
        for li in range(len(self.amg_levels())):
            d = C.c_uint64()
            self._call("cfd_debug_amg_info", li, C.byref(path), C.byref(d))
            dig.append(int(d.value))
        return int(path.value), dig

    def column_widths(self):
        """(coupled use16, [use16 of every built AMG level]): 1 = the row kernels
        read 16-bit column deltas, 0 = 32-bit absolute columns
        (cfd_debug_column_widths; host fields only, nothing is launched)."""
        cu, nl = C.c_int32(), C.c_int32()
        lv = (C.c_int32 * 20)()
        self._call("cfd_debug_column_widths", C.byref(cu), C.byref(nl), lv)
        return int(cu.value), [int(lv[i]) for i in range(min(nl.value, 20))]

    def step_algorithmic_bytes(self) -> float:
        return float(_ffi.lib().cfd_step_algorithmic_bytes(self._h))

    def step_layout_bytes(self) -> float:
        """Layout-true bytes of one fixed-schedule step (cfd_step_layout_bytes)."""
        return float(_ffi.lib().cfd_step_layout_bytes(self._h))

    def smoother_layout_bytes(self) -> float:
        """Layout-true bytes of one level-0 smoother sweep (cfd_smoother_layout_bytes)."""
        return float(_ffi.lib().cfd_smoother_layout_bytes(self._h))

    def debug_buffer(self, bid: int) -> np.ndarray:
        n = _ffi.lib().cfd_debug_buffer_len(self._h, bid)
        a = np.zeros(n, dtype=np.float32)
        self._call("cfd_debug_buffer", int(bid), a.ctypes.data_as(C.POINTER(C.c_float)), n)
        return a

    # checkpoint / resume (cfd_state_file_header; read the file with cfd2_amd.state)
    def save_state(self, path):
        """Write the whole solver state to ``path`` (collective on a distributed rank)."""
        self._call("cfd_state_save", os.fsencode(path))

    def load_state(self, path):
        """Replace the state with a saved one (drops this solver's AMG hierarchy)."""
        self._call("cfd_state_load", os.fsencode(path))

    def debug_prepare_assemble(self, assemble=True):
        self._call("cfd_debug_prepare_assemble", 1 if assemble else 0)

    def debug_apply_precond(self, v) -> np.ndarray:
        """z = M^-1 v, one application of the FGMRES preconditioner outside the
        solve (cfd_debug_apply_precond); v, z: 3 num_cells floats, (u, v, p) per cell."""
        v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
        assert v.size == 3 * self.num_cells
        z = np.zeros(v.size, dtype=np.float32)
        fp = C.POINTER(C.c_float)
        self._call("cfd_debug_apply_precond", v.ctypes.data_as(fp), z.ctypes.data_as(fp), v.size)
        return z

    def debug_amg_level(self, level: int) -> dict:
        """Level ``level`` of the built hierarchy as plain CSR with its diagonals
        and transfer operators, expanded from the device image
        (cfd_debug_amg_level; _ffi.amg_level_readback for the keys)."""
        return _ffi.amg_level_readback(lambda p: self._call("cfd_debug_amg_level", int(level), p))

    def debug_amg_vcycle(self, x0, b) -> np.ndarray:
        """One V-cycle of the preconditioner on (x0, b), outside the solve
        (cfd_debug_amg_vcycle); f32 in, f32 out."""
        x0 = np.ascontiguousarray(x0, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        assert x0.shape == b.shape == (self.num_cells,)
        out = np.zeros(self.num_cells, dtype=np.float32)
        fp = C.POINTER(C.c_float)
        self._call("cfd_debug_amg_vcycle", x0.ctypes.data_as(fp), b.ctypes.data_as(fp), out.ctypes.data_as(fp),
                   self.num_cells)
        return out

    def debug_reference_semantics(self, flags):
        """Test mode: the reference's own semantics (oracle flag bits 1 / 4 /
        8) instead of the canonical resolutions (cfd_debug_reference_semantics;
        one GPU)."""
        self._call("cfd_debug_reference_semantics", int(flags))

    def comm_stats(self, reset=False) -> dict:
        """Transport of this handle (RCCL: ncclCommCount / ncclCommUserRank),
        its HIP device, and the collective traffic since the last reset."""
        c = _ffi.CommStats()
        self._call("cfd_dist_comm_stats", C.byref(c), 1 if reset else 0)
        d = {k: getattr(c, k) for k, _ in _ffi.CommStats._fields_}
        d["transport"] = _ffi.TRANSPORTS.get(c.transport, str(c.transport))
        return d

    def comm_timing_enable(self, enable=True) -> None:
        """cfd_comm_timing_enable: time every halo / all-gather (resets the totals)."""
        self._call("cfd_comm_timing_enable", 1 if enable else 0)

    def comm_timing(self) -> list:
        """cfd_comm_timing: per category (AMG halos per level) the calls, bytes,
        the compute stream's exposed wait and the transport's own time (us)."""
        cap = 64
        buf = (_ffi.CommTimingEntry * cap)()
        n = C.c_int32(0)
        self._call("cfd_comm_timing", buf, cap, C.byref(n))
        out = []
        for e in buf[:n.value]:
            out.append({"category": _ffi.COMM_CATEGORIES.get(e.category, str(e.category)), "level": e.level,
                        "calls": e.calls, "bytes": e.bytes, "wait_us": e.wait_us, "comm_us": e.comm_us})
        return out


def scalar_solver_default() -> _ffi.ScalarSolver:
    """cfd_scalar_solver_default (no handle and no GPU needed)."""
    cfg = _ffi.ScalarSolver()
    _bind().cfd_scalar_solver_default(C.byref(cfg))
    return cfg


def scalar_scheme_default() -> _ffi.ScalarScheme:
    """cfd_scalar_scheme_default (no handle and no GPU needed)."""
    cfg = _ffi.ScalarScheme()
    _bind().cfd_scalar_scheme_default(C.byref(cfg))
    return cfg


def scalar_config_default() -> _ffi.ScalarConfig:
    """cfd_scalar_config_default (no handle and no GPU needed)."""
    cfg = _ffi.ScalarConfig()
    _bind().cfd_scalar_config_default(C.byref(cfg))
    return cfg


def adaptive_dt_rule(current_dt, target_cfl, min_cell_size, max_vel):
    """cfd_adaptive_dt_rule, the reference's driver-loop rule (src/ui/app.rs:897-909)
    in f64; no handle and no GPU needed.  Returns (next_dt, changed)."""
    L = _bind()
    nxt, ch = C.c_double(), C.c_int32()
    _ffi.check(L.cfd_adaptive_dt_rule(float(current_dt), float(target_cfl), float(min_cell_size), float(max_vel),
                                      C.byref(nxt), C.byref(ch)), "cfd_adaptive_dt_rule")
    return float(nxt.value), bool(ch.value)


def dist_unique_id() -> bytes:
    """RCCL unique id (rank 0 creates it, every rank passes it to create_dist)."""
    L = _bind()
    buf = (C.c_uint8 * 128)()
    _ffi.check(L.cfd_dist_unique_id(buf), "cfd_dist_unique_id")
    return bytes(buf)


class GpuGroup:
    """In-process distributed solver: ``nranks`` ranks on ``devices`` (default
    all on GPU 0), one host thread per rank inside the library.  Same surface
    as GpuSolver; getters return global arrays (owned slices concatenated)."""

    def __init__(self, mesh, nranks: int, devices=None, config: _ffi.Config | None = None,
                 **cfg_overrides):
        L = _bind()
        cfg = config if config is not None else _ffi.default_config(**cfg_overrides)
        view = mesh.view()
        devs = list(devices) if devices is not None else [0] * nranks
        if len(devs) != nranks:
            raise ValueError("one device per rank")
        darr = (C.c_int32 * nranks)(*devs)
        harr = (_vp * nranks)()
        _ffi.check(L.cfd_group_create(C.byref(view), C.byref(cfg), int(nranks), darr, harr),
                   "cfd_group_create")
        self._harr = harr
        self.ranks = [GpuSolver(mesh, config=cfg, _handle=_vp(harr[r])) for r in range(nranks)]
        self.nranks = nranks
        self.num_cells = self.ranks[0].num_global_cells

    def close(self):
        for r in self.ranks:
            r.close()
        self.ranks = []

    def __getattr__(self, name):
        # setters / state writers apply to every rank
        if name.startswith("set_") or name in ("update_constants", "initialize_history",
                                               "profile_enable", "profile_reset", "synchronize",
                                               "enable_scalars", "scalar_solver_stats", "scalar_scheme_stats",
                                               "enable_particles", "enable_time_stats", "enable_monitor"):
            # scalars, particles, time statistics, monitor: refused by every rank, one GPU only
            def f(*a, **k):
                for r in self.ranks:
                    getattr(r, name)(*a, **k)
            return f
        raise AttributeError(name)

    @property
    def constants(self):
        return self.ranks[0].constants

    @constants.setter
    def constants(self, c):
        for r in self.ranks:
            r.constants = c

    def step(self):
        _ffi.check(_bind().cfd_group_step(self._harr, self.nranks), "cfd_group_step")

    def _gather(self, getter, comps):
        out = np.zeros((self.num_cells, comps) if comps > 1 else self.num_cells)
        for r in self.ranks:
            c0, c1 = r.owned
            out[c0:c1] = getattr(r, getter)()
        return out

    def debug_fault(self, fail_rank: int) -> None:
        """cfd_debug_group_fault: raises (the injected failure of ``fail_rank``)."""
        _ffi.check(_bind().cfd_debug_group_fault(self._harr, self.nranks, int(fail_rank)),
                   "cfd_debug_group_fault")

    def debug_fault_midstep(self, fail_rank: int) -> None:
        """cfd_debug_group_fault_midstep: a group step in which ``fail_rank``
        fails right after its first prepare(); raises, and the group is then
        marked needs-restore."""
        _ffi.check(_bind().cfd_debug_group_fault_midstep(self._harr, self.nranks, int(fail_rank)),
                   "cfd_debug_group_fault_midstep")

    @property
    def needs_restore(self) -> bool:
        return bool(_bind().cfd_group_needs_restore(self._harr, self.nranks))

    def reset(self) -> None:
        """cfd_group_reset: accept the ranks' current state after a failed step."""
        _ffi.check(_bind().cfd_group_reset(self._harr, self.nranks), "cfd_group_reset")

    def save_state(self, path):
        _ffi.check(_bind().cfd_group_state_save(self._harr, self.nranks, os.fsencode(path)),
                   "cfd_group_state_save")

    def load_state(self, path):
        for r in self.ranks:
            r.load_state(path)

    def get_u(self): return self._gather("get_u", 2)
    def get_p(self): return self._gather("get_p", 1)
    def get_d_p(self): return self._gather("get_d_p", 1)

    # diagnostics: the group calls are collective; every rank returns the same bytes
    def flow_diagnostics(self) -> _ffi.FlowDiag:
        out = (_ffi.FlowDiag * self.nranks)()
        _ffi.check(_bind().cfd_group_flow_diagnostics(self._harr, self.nranks, out), "cfd_group_flow_diagnostics")
        first = bytes(out[0])
        assert all(bytes(out[r]) == first for r in range(self.nranks)), "ranks disagree on the flow diagnostics"
        return _ffi.FlowDiag.from_buffer_copy(first)

    # derived fields: per rank, not collective (the pass reads current ghosts)
    def speed(self): return self._gather("speed", 1)
    def vorticity(self): return self._gather("vorticity", 1)
    def divergence(self): return self._gather("divergence", 1)

    def set_force_region(self, x0, y0, x1, y1) -> int:
        return [r.set_force_region(x0, y0, x1, y1) for r in self.ranks][0]

    @property
    def min_cell_size(self) -> float:
        return self.ranks[0].min_cell_size

    def adapt_dt(self, target_cfl) -> float:
        dt = C.c_float()
        _ffi.check(_bind().cfd_group_adapt_dt(self._harr, self.nranks, float(target_cfl), C.byref(dt)),
                   "cfd_group_adapt_dt")
        return float(dt.value)

    def step_adaptive(self, target_cfl) -> float:
        self.step()
        return self.adapt_dt(target_cfl)

    # frames: one GPU only, as the scalars (set_render_mesh / set_view reach every rank, which refuses)
    def render(self, *a, **k):
        raise RuntimeError("render failed: rendering runs on one GPU only: a group's ranks each hold a part of the fields")

    render_owner = render

    # surfaces: one GPU only (the name has no forwarded prefix: say so here instead of an AttributeError)
    def select_surface(self, *a, **k):
        raise RuntimeError("select_surface failed: surface distributions run on one GPU only: a group's ranks each hold "
                           "a part of the fields")

    def step_info(self): return self.ranks[0].step_info()
    def amg_levels(self): return self.ranks[0].amg_levels()

    def column_widths(self):
        w = [r.column_widths() for r in self.ranks]
        assert all(x == w[0] for x in w), f"ranks disagree on the column widths: {w}"
        return w[0]

    @property
    def should_stop(self): return self.ranks[0].should_stop
    @should_stop.setter
    def should_stop(self, v):
        for r in self.ranks:
            r.should_stop = v
    @property
    def degenerate_count(self): return self.ranks[0].degenerate_count
    @property
    def steady_state_count(self): return self.ranks[0].steady_state_count
    @property
    def n_outer_correctors(self): return self.ranks[0].n_outer_correctors
    @n_outer_correctors.setter
    def n_outer_correctors(self, v):
        for r in self.ranks:
            r.n_outer_correctors = v


def dist_plan(mesh, nranks: int, rank: int) -> dict:
    """Host-only halo plan of one rank (no GPU): owned range, ghost ids, and per
    peer the receive / send counts and the owned ids sent."""
    L = _bind()
    view = mesh.view()
    c0, c1, ng, npeer, ns = (C.c_uint32() for _ in range(5))
    z = None
    _ffi.check(L.cfd_dist_plan(C.byref(view), nranks, rank, C.byref(c0), C.byref(c1), C.byref(ng),
                               C.byref(npeer), C.byref(ns), z, z, z, z, z), "cfd_dist_plan")
    ghost = np.zeros(max(ng.value, 1), dtype=np.uint32)
    prank = np.zeros(max(npeer.value, 1), dtype=np.int32)
    precv = np.zeros(max(npeer.value, 1), dtype=np.uint32)
    psend = np.zeros(max(npeer.value, 1), dtype=np.uint32)
    sendg = np.zeros(max(ns.value, 1), dtype=np.uint32)
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    _ffi.check(L.cfd_dist_plan(C.byref(view), nranks, rank, None, None, None, None, None, u32(ghost),
                               prank.ctypes.data_as(C.POINTER(C.c_int32)), u32(precv), u32(psend),
                               u32(sendg)), "cfd_dist_plan")
    n = npeer.value
    return dict(c0=c0.value, c1=c1.value, ghost=ghost[:ng.value], peers=prank[:n].tolist(),
                recv=precv[:n].tolist(), send=psend[:n].tolist(), send_ids=sendg[:ns.value])


def rccl_selftest(device: int = 0) -> None:
    """RCCL transport plumbing check on one GPU (raises on failure)."""
    _ffi.check(_bind().cfd_debug_rccl_selftest(int(device)), "cfd_debug_rccl_selftest")
