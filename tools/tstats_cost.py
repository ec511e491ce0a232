"""Cost of the time statistics and the monitor history against the read-back they replace.

At each bench configuration (default c1 and c2), on one handle after 2 steps
(the level-0 smoother is profiled during them), medians of 5 fenced host calls
(cfd_synchronize on both sides; the first call of each kind is a warm-up and is
not counted):
  accumulate    accumulate_time_stats(1.0) for every kernel form: means only or
                second moments, with 0, 1 and 4 scalar fields; the time, the
                bytes of the model (12 B of state + 16 B per plane, 4 B more per
                field, per cell) and the two divided, beside the HBM peak
  record        record_monitor() with 64 probes, with and without the flow
                diagnostics
  readback      get_u(): what a caller who averages on the host pays per sample
  smoother      the level-0 AMG smoother's layout-true GB/s and fraction of the
                HBM peak over the 2 steps (cfd_profile_smoother): the project's
                roofline of record, on the same box in the same session
Writes profiles/r15/tstats_cost.json.

    python tools/tstats_cost.py [--configs c1 c2] [--mesh-cache-dir DIR]
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
HBM_PEAK_GBS = 8000.0                 # bench.py
DT = 1e-3
FORMS = [(m2, nf) for m2 in (False, True) for nf in (0, 1, 4)]


def fenced(s, fn, reps=5):
    ts = []
    for _ in range(reps + 1):  # the first call is the warm-up
        s.synchronize()
        t0 = time.perf_counter()
        fn()
        s.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts[1:]), 1e3 * min(ts[1:])


def model_bytes(n, m2, nf):
    planes = 3 + (4 if m2 else 0) + nf * (4 if m2 else 2)
    return n * (12 + 4 * nf + 16 * planes), planes


def rows_for(mesh, name, np):
    from cfd2_amd import GpuSolver, default_config
    s = GpuSolver(mesh, config=default_config(fixed_outer=5, fixed_inner=30))
    s.set_dt(DT)
    s.set_viscosity(0.01)
    s.set_density(1.0)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_precond_type(1)
    s.initialize_history()
    s.profile_enable(True)
    s.step()
    s.step()
    s.synchronize()
    sm_ms, sm_n, sm_bytes = s.profile_smoother()
    s.profile_enable(False)
    n = s.num_cells
    # as bench.py: the layout-true bytes of one sweep over the mean time of a sweep
    sm_gbs = s.smoother_layout_bytes() / (sm_ms * 1e-3 / sm_n) / 1e9 if sm_n and sm_ms > 0 else None
    base = dict(config=name, cells=n, smoother_gbs=sm_gbs, smoother_launches=int(sm_n), smoother_avg_us=1e3 * sm_ms / max(sm_n, 1),
                smoother_frac=sm_gbs / HBM_PEAK_GBS if sm_gbs else None)
    r_med, r_min = fenced(s, s.get_u)
    base.update(readback_get_u_ms=r_med, readback_get_u_min_ms=r_min)
    rows = []
    rng = np.random.default_rng(1)
    for m2, nf in FORMS:
        s.enable_scalars(nf)
        for f in range(nf):
            s.set_scalar(f, rng.random(n))
        s.enable_time_stats(second_moments=m2, scalars=True)
        med, mn = fenced(s, lambda: s.accumulate_time_stats(1.0))
        b, planes = model_bytes(n, m2, nf)
        gbs = b / (med * 1e-3) / 1e9
        rows.append(dict(base, what="accumulate", second_moments=m2, fields=nf, planes=planes, model_bytes=b,
                         ms=med, min_ms=mn, gbs=gbs, frac=gbs / HBM_PEAK_GBS,
                         frac_over_smoother=gbs / sm_gbs if sm_gbs else None, over_readback=med / r_med))
        print(json.dumps(rows[-1]), flush=True)
        s.disable_time_stats()
    s.enable_scalars(0)
    cells = np.linspace(0, n - 1, 64).astype(np.int64)
    for diag in (False, True):
        s.enable_monitor(1024, cells, diagnostics=diag)
        med, mn = fenced(s, s.record_monitor)
        rows.append(dict(base, what="record_monitor", probes=64, diagnostics=diag, ms=med, min_ms=mn))
        print(json.dumps(rows[-1]), flush=True)
    s.disable_monitor()
    s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c1", "c2"], choices=sorted(H))
    ap.add_argument("--mesh-cache-dir", default=None, help="load / save <dir>/<config>.mesh (bench.py --mesh-cache files)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "tstats_cost.json"))
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
        for row in rows_for(mesh, name, np):
            row["build"] = build_id()
            rows.append(row)
        del mesh
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="one handle after 2 steps (fixed schedule 5 Picard x 30 FGMRES / AMG, dt 1e-3) "
                            "(tools/tstats_cost.py): medians of 5 fenced host calls each, milliseconds. accumulate = "
                            "accumulate_time_stats(1.0) per kernel form; model_bytes = N (12 + 4 fields + 16 planes), "
                            "gbs = model_bytes / ms, frac = gbs / 8000 (the HBM peak bench.py uses), frac_over_smoother "
                            "= gbs / smoother_gbs; smoother_* = the level-0 AMG smoother over the same 2 steps "
                            "(cfd_profile_smoother, layout-true bytes); record_monitor with 64 probes; readback_get_u = "
                            "get_u(), what averaging on the host reads per sample",
                       rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
