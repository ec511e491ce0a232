"""Writes profiles/r07/f64_residual_deviation.txt: over the solve case list of
tests/fv_cases.py, run on the CPU oracle, the worst deviation of the reported
linear residual from |b - A x| recomputed in float64, per mesh and
preconditioner and by what the solve reports.  tests/fv_cases.RESIDUAL_TOL and
ESTIMATE_FLOOR_EPS are 4 x the two worst figures.

    python tools/f64_residual_deviation.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cfd-demo2_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import fv_cases as fc  # noqa: E402
from tests import fv_checks as fv  # noqa: E402
from tests.oracle_py import OracleSolver  # noqa: E402


def main():
    lines = ["# worst over max_restart {50,3,1} x convergence_lag {0,1} x 3 steps (18 solves per line; monotone: 8",
             "# fixed-schedule solves), by what the solve reports (fv_checks.reports_estimate):",
             "# computed = | |b - A x|_f64 - reported | / reported over the solves that report a computed b - A x",
             "# est_eps  = | |b - A x|_f64 - reported | / |eps32 (|b| + |A||x|)|_2 over the solves that may report",
             "#            the Givens estimate (converged, report below max(rtol |b|, atol))",
             "# est_raw  = the same deviation relative to the reported value (why no relative bound fits them)",
             f"{'group':34s} {'n_comp':>6s} {'computed':>10s} {'n_est':>6s} {'est_eps':>9s} {'est_raw':>10s}"]
    worst_c = worst_e = 0.0
    groups = [(m, p, False) for m in fc.MESHES for p in (0, 1)] + [(m, p, True) for m in fc.MONOTONE_MESHES
                                                                    for p in (0, 1)]
    for mesh_name, precond, mono in groups:
        rec = []
        if mono:
            fc.monotone_residuals(OracleSolver, fc.mesh_of(mesh_name), precond, record=rec)
        else:
            fc.run_solve(OracleSolver, mesh_name, precond, record=rec)
        comp = eps = raw = 0.0
        nc = ne = 0
        for _, sysm, stats, cfg in rec:
            d = abs(fv.true_residual(sysm) - stats.residual)
            if fv.reports_estimate(sysm, stats, cfg):
                ne += 1
                eps, raw = max(eps, d / fv.residual_resolution(sysm)), max(raw, d / stats.residual)
            else:
                nc += 1
                comp = max(comp, d / stats.residual)
        worst_c, worst_e = max(worst_c, comp), max(worst_e, eps)
        name = f"{'monotone ' if mono else ''}{mesh_name} precond {precond}"
        lines.append(f"{name:34s} {nc:6d} {comp:10.3e} {ne:6d} {eps:9.3f} {raw:10.3e}")
    lines.append(f"worst computed = {worst_c:.3e}: RESIDUAL_TOL = 4 x = {4 * worst_c:.3e}")
    lines.append(f"worst est_eps = {worst_e:.3f}: ESTIMATE_FLOOR_EPS = 4 x = {4 * worst_e:.3f}")
    out = os.path.join(ROOT, "profiles", "r07", "f64_residual_deviation.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
