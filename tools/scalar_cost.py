"""Cost of the passive-scalar advance, and its sweep kernel against the level-0
AMG smoother of the same session.

At each bench configuration (default c1 and c2), on one handle after 2 steps
(AMG preconditioner, the level-0 smoother timed during the second):
  (a) the median of 20 fenced advance_scalars() calls (cfd_synchronize on both
      sides) for one field with the default config (tol 1e-6, batches of 4
      sweeps, one host read per batch), and the sweeps each call took;
  (b) the same with max_sweeps = check_interval = 64: 64 sweeps and one host
      read per call, so time / 64 is the sweep kernel's own time (plus 1/64 of
      the assembly and the read); its layout bytes / that time is the rate;
  (c) the level-0 smoother's layout-true rate from cfd_profile_smoother /
      cfd_smoother_layout_bytes -- the yardstick: both kernels are one Jacobi
      sweep over a slot-major ELL with a gather.
Writes profiles/r08/scalar_cost.json.

    python tools/scalar_cost.py [--configs c1 c2] [--mesh-cache-dir DIR]

--krylov: instead, Jacobi against BiCGStab + polish (set_scalar_solver) for one
field at dt = 1e-3, D = 1e-4 (a dye) and D = 0.01 (diffusion dominated), every
advance from the same step profile: sweeps / iterations and the median of 5
fenced calls each (Jacobi with max_sweeps raised until it converges); the time
of one BiCGStab iteration as (128 iterations - 64 iterations) / 64 at tol = 0,
its layout bytes over that time, and the sweep kernel's rate as in (b).
Writes profiles/r09/scalar_krylov.json.

--scheme: instead, the extra time of a scheme-1 ("limited linear", van Leer)
advance over a scheme-0 advance (set_scalar_scheme) on one handle in one
session: one field at dt = 1e-3, D = 1e-4, every advance from the same step
profile and exactly 4 sweeps long, medians of 20 fenced calls, scheme 0 timed
before and after scheme 1; beside it the layout bytes of the two new passes
less those of the assembly they replace, at the sweep kernel's rate of the
same session.  Writes profiles/r10/scalar_hr.json.

--wall: instead, the extra time of the boundary-condition forms of the
assemblies (set_scalar_wall: the obstacle's faces at a fixed value) over their
plain siblings under scheme 0 and under scheme 1, on one handle in one session
as --scheme times its pair: the plain advance before and after the one with the
wall; the median of 20 fenced scalar_wall_flux() calls (k_scalar_wall_flux, the
one-block finish and a 24-byte read: a whole host call, not the kernel's own
time, which a kernel trace of this run gives); the extra layout bytes (4 B per
cell per pass that reads the selection image) over the extra times, left null
where the extra is below the spread of the two plain runs that bracket it,
beside the sweep kernel's rate of the same session.  Writes profiles/r12/scalar_bc.json.

--buoyancy: instead, the extra time of a step whose assembly runs in its
buoyant form (set_scalar_buoyancy + set_gravity: one driving field) over the
plain step, on one handle in one session under the fixed schedule (5 Picard x
30 FGMRES, so a step's work does not depend on the state): medians of 10 fenced
step() calls with buoyancy off, on, and off again; the median of 20 fenced
buoyancy_force() calls (k_buoyancy_force, the one-block finish and a 16-byte
read: a whole host call, not the kernel's own time, which a kernel trace of
this run gives); beside the extra, the expected cost outer iterations x 4 B x N
at the sweep kernel's rate of the same session.  Writes profiles/r13/buoyancy.json.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cfd-demo2_amd"))
sys.path.insert(0, ROOT)

H = {"c1": 0.001723, "c2": 5.449e-4}  # bench.py CONFIGS
# a dye: at D = 1e-4 and dt = 1e-3 the diffusion number D dt / h^2 is 0.03 (C1) and 0.34 (C2), below the
# cell CFL, so Jacobi converges in tens of sweeps; it needs about (1 + CFL + 4 D dt / h^2) ln(1 / tol) of them
DIFFUSIVITY = 1e-4


def sweep_layout_bytes(mesh) -> float:
    """Layout bytes of one k_scalar_sweep, each element once: per used face slot
    the column (fs.other) and the coefficient (4 B each); per cell nface, diag,
    b and the phi written (4 B each); the phi gathers counted once (4 B per cell)."""
    slots = float(mesh.arrays()["cell_face_offsets"][-1])
    return 8.0 * slots + 16.0 * mesh.num_cells() + 4.0 * mesh.num_cells()


def krylov_layout_bytes(mesh) -> float:
    """Layout bytes of one BiCGStab iteration, each element of a pass once: the
    two operator passes read every used slot's column and coefficient (16 B per
    slot); per cell, 4 B each: v = A p: nface, diag, p, rh, v; s: r, v, s; t = A
    s: nface, diag, s, t; x / r: x twice, p, s, t, rh, r; p: r, v, p twice (92 B)."""
    slots = float(mesh.arrays()["cell_face_offsets"][-1])
    return 16.0 * slots + 92.0 * mesh.num_cells()


def krylov_rows(s, mesh, name, np):
    x = mesh.arrays()["cell_cx"]
    dye = np.where(x < 0.5, 1.0, 0.0)

    def run(D, method, reps=5, **cfg):
        kw = {k: cfg.pop(k) for k in ("max_iters", "check_interval_k") if k in cfg}
        s.enable_scalars(1, **cfg)
        s.set_scalar_params(0, D, 1.0)
        if method:
            s.set_scalar_solver(0, "bicgstab", max_iters=kw.get("max_iters"), check_interval=kw.get("check_interval_k"))
        ts = []
        for r in range(reps + 1):  # the first call is the warm-up
            s.set_scalar(0, dye)
            s.synchronize()
            t0 = time.perf_counter()
            s.advance_scalars()
            s.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts[1:]), s.scalar_stats(0), s.scalar_solver_stats(0)

    rows = []
    for D in (1e-4, 0.01):
        j_t, j_st, _ = run(D, False, max_sweeps=200000)
        k_t, k_st, k_ks = run(D, True)
        rows.append(dict(config=name, cells=mesh.num_cells(), dt=1e-3, diffusivity=D,
                         jacobi_sweeps=int(j_st.sweeps), jacobi_converged=int(j_st.converged), jacobi_ms=1e3 * j_t,
                         bicgstab_iterations=int(k_ks.iterations), bicgstab_reason=int(k_ks.stop_reason),
                         polish_sweeps=int(k_ks.polish_sweeps), bicgstab_converged=int(k_st.converged),
                         bicgstab_ms=1e3 * k_t, bicgstab_faster=bool(k_t < j_t)))
    t64, _, k64 = run(0.01, True, tol=0.0, max_sweeps=4, max_iters=64, check_interval_k=64)
    t128, _, k128 = run(0.01, True, tol=0.0, max_sweeps=4, max_iters=128, check_interval_k=128)
    assert (k64.iterations, k128.iterations) == (64, 128), (k64.iterations, k128.iterations)
    it_s = (t128 - t64) / 64
    s.enable_scalars(1, max_sweeps=64, check_interval=64)
    s.set_scalar_params(0, 0.01, 1.0)
    s.set_scalar(0, dye)
    s.advance_scalars()
    b_med, _, _ = fenced(s, s.advance_scalars, reps=10)
    kb, sb = krylov_layout_bytes(mesh), sweep_layout_bytes(mesh)
    rate = dict(config=name, cells=mesh.num_cells(), iteration_us=1e6 * it_s, iteration_layout_bytes=kb,
                iteration_gbs=kb / it_s / 1e9, sweep_us=1e6 * b_med / 64, sweep_layout_bytes=sb,
                sweep_gbs=sb / (b_med / 64) / 1e9)
    return rows, rate


def scheme_layout_bytes(mesh) -> dict:
    """Layout bytes, each element of a pass once.  k_scalar_assemble: per used
    slot other, meta, flux_s, area, dist_e and the coef written (24 B); per cell
    nface, vol, phi_old, diag, b (20 B).  k_scalar_grad: per used slot other,
    meta, area, nx, ny, lam_s (24 B); per cell nface, vol, the phi_old gathers
    counted once, the 8-byte g written (20 B).  k_scalar_assemble_limited: the
    assembly's slot streams plus dvx, dvy (32 B); per cell the assembly's 20 B
    and the g gathers counted once (28 B)."""
    slots, n = float(mesh.arrays()["cell_face_offsets"][-1]), float(mesh.num_cells())
    return dict(assemble=24.0 * slots + 20.0 * n, grad=24.0 * slots + 20.0 * n, limited=32.0 * slots + 28.0 * n)


def scheme_row(s, mesh, name, np):
    """One advance under scheme 0 and under scheme 1 on one handle: every call
    starts from the same step profile and runs exactly one batch of 4 sweeps
    (max_sweeps = check_interval = 4), so the two differ by the assembly alone;
    medians of 20 fenced calls, scheme 0 timed before and after scheme 1."""
    x = mesh.arrays()["cell_cx"]
    dye = np.where(x < 0.5, 1.0, 0.0)

    def run(scheme, reps=20, **cfg):
        s.enable_scalars(1, **cfg)
        s.set_scalar_params(0, DIFFUSIVITY, 1.0)
        s.set_scalar_scheme(0, scheme)
        ts = []
        for _ in range(reps + 1):  # the first call is the warm-up
            s.set_scalar(0, dye)
            s.synchronize()
            t0 = time.perf_counter()
            s.advance_scalars()
            s.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts[1:]), min(ts[1:]), s.scalar_scheme_stats(0)

    one = dict(max_sweeps=4, check_interval=4)
    u0, u0_min, _ = run("upwind", **one)
    v, v_min, hs = run("vanleer", **one)
    u1, u1_min, _ = run("upwind", **one)
    t64, _, _ = run("upwind", reps=10, max_sweeps=64, check_interval=64)
    sweep = (t64 - 0.5 * (u0 + u1)) / 60.0  # 60 more sweeps, the same assembly and one read
    lb, sb = scheme_layout_bytes(mesh), sweep_layout_bytes(mesh)
    extra = v - 0.5 * (u0 + u1)
    extra_bytes = lb["grad"] + lb["limited"] - lb["assemble"]
    rate = sb / sweep
    return dict(config=name, cells=mesh.num_cells(), dt=1e-3, diffusivity=DIFFUSIVITY, sweeps_per_call=4,
                upwind_ms=1e3 * u0, upwind_min_ms=1e3 * u0_min, vanleer_ms=1e3 * v, vanleer_min_ms=1e3 * v_min,
                upwind_again_ms=1e3 * u1, upwind_again_min_ms=1e3 * u1_min, clamped_cells=int(hs.clamped_cells),
                extra_us=1e6 * extra, extra_layout_bytes=extra_bytes, extra_gbs=extra_bytes / extra / 1e9,
                sweep_us=1e6 * sweep, sweep_layout_bytes=sb, sweep_gbs=rate / 1e9,
                extra_at_sweep_rate_us=1e6 * extra_bytes / rate, extra_in_sweeps=extra / sweep,
                layout_bytes=lb)


OBSTACLE_BOX = (0.85, 0.36, 1.15, 0.66)  # around bench_channel's obstacle ((1.0, 0.51), r = 0.1), off the channel walls


def wall_row(s, mesh, name, np):
    """scheme_row's protocol (one batch of 4 sweeps from the same step profile
    per call, medians of 20 fenced calls) for a field with and without a
    fixed-value wall on the obstacle, under scheme 0 and scheme 1."""
    x = mesh.arrays()["cell_cx"]
    dye = np.where(x < 0.5, 1.0, 0.0)
    n = float(mesh.num_cells())

    def run(scheme, wall, reps=20, **cfg):
        s.enable_scalars(1, **cfg)
        s.set_scalar_params(0, DIFFUSIVITY, 1.0)
        s.set_scalar_scheme(0, scheme)
        faces = s.set_scalar_wall(0, "value", 1.0, OBSTACLE_BOX) if wall else 0
        ts = []
        for _ in range(reps + 1):  # the first call is the warm-up
            s.set_scalar(0, dye)
            s.synchronize()
            t0 = time.perf_counter()
            s.advance_scalars()
            s.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts[1:]), faces

    one = dict(max_sweeps=4, check_interval=4)
    out = dict(config=name, cells=mesh.num_cells(), dt=1e-3, diffusivity=DIFFUSIVITY, sweeps_per_call=4)
    plain = {}
    for scheme, passes in (("upwind", 1), ("vanleer", 2)):
        p0, _ = run(scheme, False, **one)
        w, faces = run(scheme, True, **one)
        p1, _ = run(scheme, False, **one)
        plain[scheme] = 0.5 * (p0 + p1)
        extra, spread = w - plain[scheme], abs(p1 - p0)
        out[scheme] = dict(plain_ms=1e3 * p0, wall_ms=1e3 * w, plain_again_ms=1e3 * p1, extra_us=1e6 * extra,
                           plain_spread_us=1e6 * spread, extra_layout_bytes=4.0 * n * passes,
                           extra_gbs=4.0 * n * passes / extra / 1e9 if extra > spread else None)
        out["faces"] = faces
    # the wall-flux call on the field the last wall run left
    run("upwind", True, reps=1, **one)
    ts = []
    for _ in range(21):
        s.synchronize()
        t0 = time.perf_counter()
        wf = s.scalar_wall_flux(0)
        ts.append(time.perf_counter() - t0)
    f = statistics.median(ts[1:])
    t64, _ = run("upwind", False, reps=10, max_sweeps=64, check_interval=64)
    sweep = (t64 - plain["upwind"]) / 60.0
    sb = sweep_layout_bytes(mesh)
    out.update(wall_flux_call_us=1e6 * f, wall_flux_layout_bytes=4.0 * n, wall_flux=wf.as_dict(), sweep_us=1e6 * sweep, sweep_layout_bytes=sb, sweep_gbs=sb / sweep / 1e9)
    return out


def buoyancy_row(s, mesh, name, np, outer):
    """Steps with buoyancy off, on and off again on one handle; beta is small, so
    the flow stays the bench flow while the buoyant kernel does all its work."""
    x = mesh.arrays()["cell_cx"]
    dye = np.where(x < 0.5, 1.0, 0.0)
    n = float(mesh.num_cells())
    s.enable_scalars(1, max_sweeps=4, check_interval=4)
    s.set_scalar_params(0, DIFFUSIVITY, 1.0)
    s.set_scalar(0, dye)
    s.set_scalar_buoyancy(0, 1e-3, 0.5)

    def steps(on, reps=10):
        s.set_gravity(0.0, -9.81 if on else 0.0)
        assert s.buoyancy()["active"] == on
        ts = []
        for _ in range(reps + 1):  # the first call is the warm-up
            s.synchronize()
            t0 = time.perf_counter()
            s.step()
            s.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts[1:]), min(ts[1:]), s.step_layout_bytes()

    off0, off0_min, bytes_off = steps(False)
    on, on_min, bytes_on = steps(True)
    off1, off1_min, _ = steps(False)
    s.set_gravity(0.0, -9.81)
    ts = []
    for _ in range(21):
        s.synchronize()
        t0 = time.perf_counter()
        force = s.buoyancy_force()
        ts.append(time.perf_counter() - t0)
    f = statistics.median(ts[1:])
    s.set_gravity(0.0, 0.0)

    def advance(reps, **cfg):
        s.enable_scalars(1, **cfg)
        s.set_scalar_params(0, DIFFUSIVITY, 1.0)
        ts = []
        for _ in range(reps + 1):
            s.set_scalar(0, dye)
            s.synchronize()
            t0 = time.perf_counter()
            s.advance_scalars()
            s.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts[1:])

    t4 = advance(10, max_sweeps=4, check_interval=4)
    t64 = advance(10, max_sweeps=64, check_interval=64)
    sweep = (t64 - t4) / 60.0
    sb = sweep_layout_bytes(mesh)
    rate = sb / sweep
    extra, spread = on - 0.5 * (off0 + off1), abs(off1 - off0)
    extra_bytes = outer * 4.0 * n
    return dict(config=name, cells=mesh.num_cells(), dt=1e-3, outer_iterations=outer, driving_fields=1,
                step_off_ms=1e3 * off0, step_off_min_ms=1e3 * off0_min, step_on_ms=1e3 * on, step_on_min_ms=1e3 * on_min,
                step_off_again_ms=1e3 * off1, step_off_again_min_ms=1e3 * off1_min, extra_us=1e6 * extra,
                off_spread_us=1e6 * spread, extra_layout_bytes=extra_bytes,
                step_layout_bytes_off=bytes_off, step_layout_bytes_on=bytes_on,
                extra_gbs=extra_bytes / extra / 1e9 if extra > spread else None,
                sweep_us=1e6 * sweep, sweep_layout_bytes=sb, sweep_gbs=rate / 1e9,
                extra_at_sweep_rate_us=1e6 * extra_bytes / rate,
                buoyancy_force_call_us=1e6 * f, buoyancy_force_layout_bytes=8.0 * n,
                buoyancy_force=dict(fx=force.fx, fy=force.fy, fields=force.fields))


def fenced(solver, fn, reps=20):
    ts, sweeps = [], []
    for _ in range(reps):
        solver.synchronize()
        t0 = time.perf_counter()
        fn()
        solver.synchronize()
        ts.append(time.perf_counter() - t0)
        sweeps.append(int(solver.scalar_stats(0).sweeps))
    return statistics.median(ts), min(ts), sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c1", "c2"], choices=sorted(H))
    ap.add_argument("--mesh-cache-dir", default=None, help="load / save <dir>/<config>.mesh (bench.py --mesh-cache files)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--krylov", action="store_true", help="Jacobi against BiCGStab (profiles/r09/scalar_krylov.json)")
    ap.add_argument("--scheme", action="store_true", help="scheme 1 against scheme 0 (profiles/r10/scalar_hr.json)")
    ap.add_argument("--wall", action="store_true", help="the wall-condition forms against the plain ones (profiles/r12/scalar_bc.json)")
    ap.add_argument("--buoyancy", action="store_true", help="the buoyant step against the plain one (profiles/r13/buoyancy.json)")
    args = ap.parse_args()
    if args.krylov + args.scheme + args.wall + args.buoyancy > 1:
        ap.error("--krylov, --scheme, --wall and --buoyancy are separate runs")
    if args.out is None:
        where = ("r13", "buoyancy.json") if args.buoyancy else ("r12", "scalar_bc.json") if args.wall else ("r10", "scalar_hr.json") if args.scheme else ("r09", "scalar_krylov.json") if args.krylov else ("r08", "scalar_cost.json")
        args.out = os.path.join(ROOT, "profiles", *where)
    import numpy as np
    from cfd2_amd import GpuSolver, build_id, default_config
    from cfd2_amd.mesh import Mesh, bench_channel

    rows, rates = [], []
    for name in args.configs:
        cache = os.path.join(args.mesh_cache_dir, name + ".mesh") if args.mesh_cache_dir else None
        if cache and os.path.exists(cache):
            mesh = Mesh.load(cache)
        else:
            mesh = bench_channel(H[name], 100)
            if cache:
                mesh.save(cache)
        s = GpuSolver(mesh, config=default_config(fixed_outer=5, fixed_inner=30))
        s.set_dt(1e-3)
        s.set_viscosity(0.01)
        s.set_density(1.0)
        s.set_alpha_u(0.7)
        s.set_alpha_p(0.3)
        s.set_precond_type(1)
        s.initialize_history()
        if args.buoyancy:
            s.step()
            s.step()
            row = buoyancy_row(s, mesh, name, np, 5)
            row["build"] = build_id()
            print(json.dumps(row), flush=True)
            rows.append(row)
            s.close()
            del mesh
            continue
        if args.scheme or args.wall:
            s.step()
            s.step()
            row = (wall_row if args.wall else scheme_row)(s, mesh, name, np)
            row["build"] = build_id()
            print(json.dumps(row), flush=True)
            rows.append(row)
            s.close()
            del mesh
            continue
        if args.krylov:
            s.step()
            s.step()
            r, rate = krylov_rows(s, mesh, name, np)
            for row in r + [rate]:
                print(json.dumps(row), flush=True)
            rows += r
            rates.append(rate)
            s.close()
            del mesh
            continue
        s.profile_enable(True)
        s.step()           # includes the AMG setup
        s.profile_reset()  # the smoother's times of the second step only
        s.step()
        sm_ms, sm_n, _ = s.profile_smoother()
        s.profile_enable(False)
        sm_bytes = s.smoother_layout_bytes()
        x = mesh.arrays()["cell_cx"]
        dye = np.where(x < 0.5, 1.0, 0.0)

        def start(**cfg):
            s.enable_scalars(1, **cfg)
            s.set_scalar_params(0, DIFFUSIVITY, 1.0)
            s.set_scalar(0, dye)
            s.advance_scalars()  # warm-up: the first launches load the code objects

        start()
        a_med, a_min, a_sweeps = fenced(s, s.advance_scalars)
        st = s.scalar_stats(0)
        start(max_sweeps=64, check_interval=64)
        b_med, b_min, b_sweeps = fenced(s, s.advance_scalars)
        assert set(b_sweeps) == {64}
        nbytes = sweep_layout_bytes(mesh)
        row = dict(config=name, cells=mesh.num_cells(), build=build_id(), dt=1e-3, diffusivity=DIFFUSIVITY,
                   advance_ms=1e3 * a_med, advance_min_ms=1e3 * a_min, advance_sweeps=a_sweeps,
                   advance_converged=int(st.converged), phi_min=st.min, phi_max=st.max,
                   fixed64_ms=1e3 * b_med, fixed64_min_ms=1e3 * b_min, sweep_us=1e6 * b_med / 64,
                   sweep_layout_bytes=nbytes, sweep_gbs=nbytes / (b_med / 64) / 1e9,
                   smoother_launches=int(sm_n), smoother_us=1e3 * sm_ms / max(sm_n, 1),
                   smoother_layout_bytes=sm_bytes, smoother_gbs=sm_bytes / (1e-3 * sm_ms / max(sm_n, 1)) / 1e9)
        row["sweep_rate_over_smoother_rate"] = row["sweep_gbs"] / row["smoother_gbs"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        s.close()
        del mesh
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if args.buoyancy:
        with open(args.out, "w") as fh:
            json.dump(dict(what="one handle after 2 steps, fixed schedule 5 Picard x 30 FGMRES / AMG, dt 1e-3, one driving "
                                "field with beta 1e-3 (tools/scalar_cost.py --buoyancy): medians of 10 fenced step() calls "
                                "with g = (0, 0) (the plain k_assemble), g = (0, -9.81) (k_assemble_buoyant) and g = (0, 0) "
                                "again; extra = on - the mean of the two off, extra_gbs null where it is not above their "
                                "spread; extra layout bytes = outer iterations x 4 B x cells, beside them that many bytes at "
                                "the sweep kernel's rate of the same session (one sweep = (64 sweeps - 4 sweeps) / 60); "
                                "buoyancy_force_call_us = the median of 20 fenced buoyancy_force() calls (two launches, a "
                                "16-byte read, a synchronisation: not the kernel's time)",
                           rows=rows), fh, indent=1)
            fh.write("\n")
        return
    if args.wall:
        with open(args.out, "w") as fh:
            json.dump(dict(what="one field, dt 1e-3, D 1e-4, one handle after 2 steps, every advance from the same step "
                                "profile and one batch of 4 sweeps long (tools/scalar_cost.py --wall): medians of 20 fenced "
                                "advance_scalars() calls without a wall condition, with the obstacle's faces at a fixed "
                                "value, and without again, under scheme 0 (upwind) and scheme 1 (vanleer); extra = with - "
                                "the mean of the two without, extra_gbs null where it is not above their spread; "
                                "wall_flux_call_us = the median of 20 fenced scalar_wall_flux() calls (two launches, a "
                                "24-byte read, a synchronisation: not the kernel's time); one sweep = (64 sweeps - 4 sweeps) / 60; extra layout bytes = 4 B per cell per "
                                "pass that reads the selection image",
                           rows=rows), fh, indent=1)
            fh.write("\n")
        return
    if args.scheme:
        with open(args.out, "w") as fh:
            json.dump(dict(what="one field, dt 1e-3, D 1e-4, one handle after 2 steps, every advance from the same step "
                                "profile and one batch of 4 sweeps long (tools/scalar_cost.py --scheme): medians of 20 "
                                "fenced advance_scalars() calls under scheme 0, scheme 1 and scheme 0 again; extra = "
                                "scheme 1 - the mean of the two scheme-0 medians; one sweep = (64 sweeps - 4 sweeps) / 60; "
                                "layout bytes with each element of a pass once",
                           rows=rows), fh, indent=1)
            fh.write("\n")
        return
    if args.krylov:
        with open(args.out, "w") as fh:
            json.dump(dict(what="one field, dt 1e-3, one handle after 2 steps, every advance from the same step profile "
                                "(tools/scalar_cost.py --krylov): medians of 5 fenced advance_scalars() calls; Jacobi with "
                                "max_sweeps raised to 200,000; rates: one BiCGStab iteration = (128 - 64 iterations) / 64 "
                                "at tol 0, one sweep = 64 sweeps / 64, layout bytes with each element of a pass once",
                           build=build_id(), rows=rows, rates=rates), fh, indent=1)
            fh.write("\n")
        return
    with open(args.out, "w") as fh:
        json.dump(dict(what="median of 20 fenced advance_scalars() calls for one field, one handle, after 2 steps "
                            "(tools/scalar_cost.py); advance_* = the default config (a whole host call: the assembly, "
                            "batches of 4 sweeps, one 4-byte read and stream synchronisation per batch); fixed64_* = "
                            "64 sweeps and one read per call; smoother_* = the level-0 AMG smoother timed by device "
                            "events during the second step of the same session",
                       rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
