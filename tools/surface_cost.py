"""Cost of the wall surface distributions against the path they replace.

At each bench configuration (default c1 and c2), on one handle after 2 steps,
with every wall face of the mesh selected: the median of 20 fenced calls
(cfd_synchronize on both sides, after one warm-up call each) of
  (a) surface()                     -- one launch, one copy of the channels
  (b) accumulate_surface_stats(1)   -- one launch, no copy
  (c) get_u() + get_p() + numpy extraction of the same five channels on the
      same faces                     -- what a caller does without the module
  (d) (c) plus a numpy West update of mean and M2 -- the path (b) replaces
Writes profiles/r17/surface_cost.json.

    python tools/surface_cost.py [--configs c1 c2] [--mesh-cache-dir DIR]
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


def fenced_median(solver, fn, reps=20):
    fn()  # warm-up: first-use allocations, page faults of the host buffers
    ts = []
    for _ in range(reps):
        solver.synchronize()
        t0 = time.perf_counter()
        fn()
        solver.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c1", "c2"], choices=sorted(H))
    ap.add_argument("--mesh-cache-dir", default=None, help="load / save <dir>/<config>.mesh (bench.py --mesh-cache files)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "surface_cost.json"))
    args = ap.parse_args()
    import numpy as np
    from cfd2_amd import GpuSolver, build_id, default_config
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
        s = GpuSolver(mesh, config=default_config(fixed_outer=5, fixed_inner=30))
        s.set_dt(1e-3)
        s.set_viscosity(0.01)
        s.set_density(1.0)
        s.set_alpha_u(0.7)
        s.set_alpha_p(0.3)
        s.set_precond_type(1)
        s.initialize_history()
        s.step()
        s.step()
        faces = s.select_surface((-1e30, -1e30, 1e30, 1e30))
        s.enable_surface_stats()
        g = s.surface_geometry()
        cell = g["cell"].astype(np.int64)
        nu = float(np.float32(0.01))
        k = nu * g["area"] / g["dist_e"]
        pnx, pny = g["nx"] * g["area"], g["ny"] * g["area"]
        state = dict(mean=np.zeros((5, faces)), m2=np.zeros((5, faces)), W=0.0)

        def replaced():
            u, p = s.get_u(), s.get_p()
            pc, uc = p[cell], u[cell]
            return np.stack([pc, pc * pnx, pc * pny, uc[:, 0] * k, uc[:, 1] * k])

        def replaced_stats():
            x = replaced()
            Wn = state["W"] + 1.0
            d = x - state["mean"]
            state["mean"] += (1.0 / Wn) * d
            state["m2"] += d * (x - state["mean"])
            state["W"] = Wn

        dev = s.surface()["channels"]
        assert np.allclose(dev, replaced(), rtol=1e-12, atol=0.0), "the module and the host path disagree"
        a_med, a_min = fenced_median(s, s.surface)
        b_med, b_min = fenced_median(s, lambda: s.accumulate_surface_stats(1.0))
        c_med, c_min = fenced_median(s, replaced)
        d_med, d_min = fenced_median(s, replaced_stats)
        row = dict(config=name, cells=mesh.num_cells(), faces=faces, build=build_id(),
                   surface_ms=1e3 * a_med, surface_min_ms=1e3 * a_min,
                   accumulate_ms=1e3 * b_med, accumulate_min_ms=1e3 * b_min,
                   readback_extract_ms=1e3 * c_med, readback_extract_min_ms=1e3 * c_min,
                   readback_stats_ms=1e3 * d_med, readback_stats_min_ms=1e3 * d_min,
                   speedup_surface=c_med / a_med, speedup_accumulate=d_med / b_med)
        print(json.dumps(row), flush=True)
        rows.append(row)
        s.close()
        del mesh
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="median of 20 fenced host calls after one warm-up call, one handle, after 2 steps, every "
                            "wall face of the mesh selected (tools/surface_cost.py); surface() is a whole host call: "
                            "the info call, one launch, one 2-D copy and a stream synchronisation",
                       rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
