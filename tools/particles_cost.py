"""Cost of tracer particles on the device against the read-back a host tracer needs.

At each bench configuration (default c1 and c2), on one handle after 2 steps,
with 10^5 and 10^6 particles seeded on a uniform lattice over the mesh's bounds,
medians of 5 fenced host calls (cfd_synchronize on both sides; the first call
of each kind is a warm-up and is not counted):
  set_mesh      set_particle_mesh(mesh), once per configuration and not fenced
                (host work: the per-slot vertex pairs and the bin grid, then the
                upload); the time of the Python call, topology arrays included
  seed          seed_particles(lattice): f64 -> f32, the upload, k_particles_locate
  advance       advance_particles(dt) at the bench's dt (1e-3), with the mean
                and the maximum hops per particle of the last of them
  advance_far   the same with dt = 4 h / max speed (flow_diagnostics): after 2 steps
                the flow is still starting and the bench's dt moves a particle
                by a small part of a cell, so this row is the one that hops
  advance_uniform  after everything else the state is overwritten with u = (1, 0)
                (set_u) and the lattice seeded again: advance_particles(4 h), every
                particle crossing about four cells, the hop loop at several hops
                per particle (a developed flow moves about as far per step as its
                CFL number says; this is the loop's cost at CFL 4)
  stats         particle_stats(): k_particles_stats and 72 bytes to the host
  render        render_particles() over a 1920 x 1080 frame of the whole domain:
                the frame's copy on the device, k_particles_stamp, 4 W H bytes
                to the host
  get           particles(): 20 B per particle to the host
  readback      get_u(): what a tracer on the host needs per step (N cells to
                the host, widened to 16 N bytes of doubles)
Writes profiles/r14/particles_cost.json.

    python tools/particles_cost.py [--configs c1 c2] [--counts 100000 1000000] [--mesh-cache-dir DIR]
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
W_PX, H_PX = 1920, 1080
DT = 1e-3


def fenced(s, fn, reps=5):
    ts = []
    for _ in range(reps + 1):  # the first call is the warm-up
        s.synchronize()
        t0 = time.perf_counter()
        fn()
        s.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts[1:]), 1e3 * min(ts[1:])


def solver_for(mesh):
    from cfd2_amd import GpuSolver, default_config
    s = GpuSolver(mesh, config=default_config(fixed_outer=5, fixed_inner=30))
    s.set_dt(DT)
    s.set_viscosity(0.01)
    s.set_density(1.0)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_precond_type(1)
    s.initialize_history()
    s.step()
    s.step()
    return s


def lattice(np, n, box):
    """n points, the cell centres of a uniform lattice over the box, row by row"""
    x0, y0, x1, y1 = box
    nx = max(1, int(np.ceil(np.sqrt(n * (x1 - x0) / (y1 - y0)))))
    ny = -(-n // nx)
    k = np.arange(n)
    return np.stack([x0 + (k % nx + 0.5) * (x1 - x0) / nx, y0 + (k // nx + 0.5) * (y1 - y0) / ny], 1)


def rows_for(s, mesh, name, counts, np):
    t0 = time.perf_counter()
    s.set_particle_mesh(mesh)
    s.synchronize()
    set_mesh = 1e3 * (time.perf_counter() - t0)
    wf = int(np.diff(np.asarray(mesh.arrays()["cell_face_offsets"], np.int64)).max())  # the widest cell's faces
    vx, vy, _ = mesh.vertices()
    box = (float(np.min(vx)), float(np.min(vy)), float(np.max(vx)), float(np.max(vy)))
    s.set_render_mesh(mesh)
    s.set_view(W_PX, H_PX)
    s.render("speed", range=(0.0, 1.5))
    r_med, r_min = fenced(s, s.get_u)
    rows = []
    for n in counts:
        xy = lattice(np, n, box)
        s.enable_particles(n)
        seed = fenced(s, lambda: s.seed_particles(xy))
        after_seed = s.particle_stats()
        adv = fenced(s, lambda: s.advance_particles(DT))
        st = s.particle_stats()
        dt_far = 4.0 * H[name] / max(s.flow_diagnostics().max_speed, 1e-30)
        far = fenced(s, lambda: s.advance_particles(dt_far))
        sf = s.particle_stats()
        stats = fenced(s, s.particle_stats)
        stamp = fenced(s, s.render_particles)
        get = fenced(s, s.particles)
        moving = max(1, after_seed["alive"])
        rows.append(dict(config=name, cells=mesh.num_cells(), particles=n, dt=DT, set_mesh_ms=set_mesh,
                         wf=wf, slot_bytes=8 * wf * mesh.num_cells(),
                         seed_ms=seed[0], seed_min_ms=seed[1], alive_after_seed=after_seed["alive"],
                         outside_after_seed=after_seed["outside"],
                         advance_ms=adv[0], advance_min_ms=adv[1], hops_mean=st["hops_total"] / moving,
                         hops_max=st["hops_max"], capped=st["capped"], wall_contacts=st["wall_contacts"],
                         alive_after_advances=st["alive"],
                         advance_far_dt=dt_far, advance_far_ms=far[0], advance_far_min_ms=far[1],
                         far_hops_mean=sf["hops_total"] / max(1, sf["alive"]), far_hops_max=sf["hops_max"],
                         far_capped=sf["capped"], far_alive=sf["alive"],
                         stats_ms=stats[0], stats_min_ms=stats[1],
                         render_particles_ms=stamp[0], render_particles_min_ms=stamp[1], width=W_PX, height=H_PX,
                         get_ms=get[0], get_min_ms=get[1],
                         readback_get_u_ms=r_med, readback_get_u_min_ms=r_min,
                         advance_over_readback=adv[0] / r_med))
    # the hop loop at several hops per particle: a uniform field, 4 cells per advance
    s.set_u(np.tile(np.array([1.0, 0.0]), (mesh.num_cells(), 1)))
    for row, n in zip(rows, counts):
        xy = lattice(np, n, box)
        s.enable_particles(n)
        s.seed_particles(xy)
        uni = fenced(s, lambda: s.advance_particles(4.0 * H[name]))
        su = s.particle_stats()
        row.update(advance_uniform_dt=4.0 * H[name], advance_uniform_ms=uni[0], advance_uniform_min_ms=uni[1],
                   uniform_hops_mean=su["hops_total"] / max(1, su["alive"]), uniform_hops_max=su["hops_max"],
                   uniform_capped=su["capped"], uniform_alive=su["alive"], uniform_wall_contacts=su["wall_contacts"])
        print(json.dumps(row), flush=True)
    s.enable_particles(0)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c1", "c2"], choices=sorted(H))
    ap.add_argument("--counts", nargs="+", type=int, default=[100_000, 1_000_000])
    ap.add_argument("--mesh-cache-dir", default=None, help="load / save <dir>/<config>.mesh (bench.py --mesh-cache files)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "particles_cost.json"))
    args = ap.parse_args()
    import numpy as np
    from cfd2_amd import build_id
    from cfd2_amd.mesh import Mesh, bench_channel

    rows = []
    for name in args.configs:
        cache = os.path.join(args.mesh_cache_dir, name + ".mesh") if args.mesh_cache_dir else None
        if cache and os.path.exists(cache):
            mesh = Mesh.load(cache)
        else:
            mesh = bench_channel(H[name], 100)
            if cache:
                mesh.save(cache)
        s = solver_for(mesh)
        for row in rows_for(s, mesh, name, args.counts, np):
            row["build"] = build_id()
            rows.append(row)
        s.close()
        del mesh
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="one handle after 2 steps (fixed schedule 5 Picard x 30 FGMRES / AMG, dt 1e-3), particles on a "
                            "uniform lattice over the mesh's bounds (tools/particles_cost.py): medians of 5 fenced host "
                            "calls each, milliseconds. set_mesh = set_particle_mesh once, Python call and host build "
                            "included; seed = seed_particles (upload + locate); advance = advance_particles(1e-3), hops of "
                            "the last one (mean over the particles ALIVE after seeding); advance_far = the same with dt = 4 h / max "
                            "speed, hops over the particles still ALIVE; stats = particle_stats; "
                            "advance_uniform = advance_particles(4 h) after set_u(1, 0) and a fresh seeding, the hop loop at about 4 "
                            "hops per particle; wf = the widest cell's faces, slot_bytes = 8 wf N, the per-slot vertex pairs; "
                            "render_particles over a 1920 x 1080 frame; get = particles(); readback_get_u = get_u(), what "
                            "a tracer on the host reads per step",
                       rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
