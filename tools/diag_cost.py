"""Cost of the flow-diagnostics pass against the path it replaces.

At each bench configuration (default c1 and c2), on one handle after 2 steps:
the median of 20 fenced calls (cfd_synchronize on both sides) of
  (a) flow_diagnostics()            -- the scalar-only pass
  (b) vorticity()                   -- the pass with its field outputs + the copy out
  (c) get_u() + numpy max of |u|    -- what a driver loop does without the pass
and the scalar pass's layout bytes / time.  Writes profiles/r07/diag_cost.json.

    python tools/diag_cost.py [--configs c1 c2] [--mesh-cache-dir DIR]
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


def scalar_pass_bytes(mesh, solver) -> float:
    """Layout bytes of the scalar-only pass, each element once: per used face
    slot meta, other, area, nx, ny (4 B each) and lam_s on internal slots; per
    cell nface, vol (4 B), u (8 B; the neighbour gathers re-read it); the six
    f64 unit partials and the three u64 block maxima."""
    import numpy as np
    a = mesh.arrays()
    n = mesh.num_cells()
    slots = float(a["cell_face_offsets"][-1])
    internal = 2.0 * float(np.count_nonzero(a["face_neighbor"] != 0xFFFFFFFF))
    chunks = -(-n // 256)
    g = 0
    while g < 8 and (n >> (g + 1)) >= 16384:
        g += 1
    units = -(-chunks // min(1 << g, 4))
    blocks = -(-n // 1024)
    return 20.0 * slots + 4.0 * internal + 16.0 * n + 48.0 * units + 24.0 * blocks


def fenced_median(solver, fn, reps=20):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "diag_cost.json"))
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

        def replaced():
            u = s.get_u()
            return float(np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]).max())

        d = s.flow_diagnostics()  # first call allocates
        assert d.max_speed == replaced(), "the pass and the host loop disagree on max_vel"
        s.vorticity()
        a_med, a_min = fenced_median(s, s.flow_diagnostics)
        b_med, b_min = fenced_median(s, s.vorticity)
        c_med, c_min = fenced_median(s, replaced)
        nbytes = scalar_pass_bytes(mesh, s)
        row = dict(config=name, cells=mesh.num_cells(), build=build_id(),
                   flow_diagnostics_ms=1e3 * a_med, flow_diagnostics_min_ms=1e3 * a_min,
                   vorticity_ms=1e3 * b_med, vorticity_min_ms=1e3 * b_min,
                   get_u_numpy_max_ms=1e3 * c_med, get_u_numpy_max_min_ms=1e3 * c_min,
                   scalar_pass_bytes=nbytes, scalar_pass_gbs=nbytes / a_med / 1e9,
                   speedup_vs_get_u=c_med / a_med, max_speed=d.max_speed)
        print(json.dumps(row), flush=True)
        rows.append(row)
        s.close()
        del mesh
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="median of 20 fenced calls, one handle, after 2 steps (tools/diag_cost.py); the "
                            "flow_diagnostics time is a whole host call: two kernel launches, the final sum, "
                            "one 72-byte copy and a stream synchronisation",
                       rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
