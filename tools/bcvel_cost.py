"""Cost of the boundary-velocity forms of prepare and the assembly against the plain kernels.

On the C1 bench mesh (bench.py CONFIGS), one handle, one process, after 2
warm-up steps; medians of 7 fenced host calls (cfd_synchronize on both sides;
the first call of each kind is a warm-up and is not counted):
  prepare            debug_prepare_assemble(assemble=False): k_prepare / k_prepare_bcv
  prepare+assemble   debug_prepare_assemble(): + k_assemble / k_assemble_bcv
  step               one whole step (5 outer x 30 inner, AMG), plain then BCV then
                     plain again, so a drift of the box shows as the difference of
                     the two plain figures
with the empty selection (the plain kernels) and with a rotating obstacle plus a
parabolic inlet (the BCV kernels).  Writes profiles/r16/bcvel_cost.json.

    python tools/bcvel_cost.py [--config c1]
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

H = {"c0": 0.0138, "c1": 0.001723}  # bench.py CONFIGS
OBSTACLE_BOX = (0.85, 0.36, 1.15, 0.66)  # bench geometry: centre (1.0, 0.51), radius 0.1


def fenced(s, fn, reps=7):
    ts = []
    for _ in range(reps + 1):  # the first call is the warm-up
        s.synchronize()
        t0 = time.perf_counter()
        fn()
        s.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts[1:]), 1e3 * min(ts[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c1", choices=sorted(H))
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    from cfd2_amd import GpuSolver, build_id, default_config
    from cfd2_amd.mesh import bench_channel
    mesh = bench_channel(H[args.config], 100)
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

    def select(on):
        if on:
            s.set_inlet_profile(lambda x, y: (6.0 * y * (1.0 - y), 0.0 * y))
            s.set_wall_motion(OBSTACLE_BOX, omega=2.0, centre=(1.0, 0.51))
        else:
            s.clear_boundary_velocity()

    def steps():
        for _ in range(args.steps):
            s.step()

    out = dict(config=args.config, cells=s.num_cells, build=build_id(), steps_per_sample=args.steps, rows=[])
    for label, on in (("plain", False), ("bcv", True), ("plain again", False)):
        select(on)
        bv = s.boundary_velocity()
        row = dict(form=label, selected_faces=bv["inlet_faces"] + bv["wall_faces"])
        row["prepare_ms"], row["prepare_min_ms"] = fenced(s, lambda: s.debug_prepare_assemble(False))
        row["prepare_assemble_ms"], row["prepare_assemble_min_ms"] = fenced(s, s.debug_prepare_assemble)
        med, mn = fenced(s, steps, reps=3)
        row["step_ms"], row["step_min_ms"] = med / args.steps, mn / args.steps
        print(row, flush=True)
        out["rows"].append(row)
    p, b = out["rows"][0], out["rows"][1]
    out["ratio_prepare"] = b["prepare_ms"] / p["prepare_ms"]
    out["ratio_prepare_assemble"] = b["prepare_assemble_ms"] / p["prepare_assemble_ms"]
    out["ratio_step"] = b["step_ms"] / (0.5 * (p["step_ms"] + out["rows"][2]["step_ms"]))
    print({k: v for k, v in out.items() if k.startswith("ratio")}, flush=True)
    dst = os.path.join(ROOT, "profiles", "r16")
    os.makedirs(dst, exist_ok=True)
    with open(os.path.join(dst, "bcvel_cost.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
