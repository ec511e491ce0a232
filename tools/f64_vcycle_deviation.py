"""Writes profiles/r07/f64_vcycle_deviation.txt: over the case list of
tests/amg_cases.py (every mesh at both densities, four vector pairs each, and
the block-shuffled 32-bit-column mesh of tests/test_gpu_wide_columns.py), run
on the CPU oracle, the worst deviation of one AMG V-cycle from the float64
cycle of tests/amg_checks.py in units of eps32 x the majorant cycle, per row.
tests/amg_cases.VCYCLE_WORST_MEASURED is the worst figure; K is 4 x it.

    python tools/f64_vcycle_deviation.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cfd-demo2_amd"))
sys.path.insert(0, ROOT)

from tests import amg_cases as ac  # noqa: E402
from tests.oracle_py import OracleSolver  # noqa: E402


def main():
    lines = ["# ratio = max over the rows of |x_oracle - x_f64| / (eps32 M): x_oracle one V-cycle of the CPU oracle",
             "# (debug_amg_vcycle), x_f64 the float64 cycle over the read-back levels, M the majorant cycle",
             "# (every matrix, x0 and b by magnitude, every subtraction an addition), all on the same (x0, b)",
             f"{'case':66s} {'ratio':>10s}"]
    worst = 0.0
    for name in ac.MESHES:
        for density in ac.DENSITIES:
            rec = []
            ac.run_case(OracleSolver, name, density, record=rec)
            for what, ratio in rec:
                worst = max(worst, ratio)
                lines.append(f"{what:66s} {ratio:10.3e}")
    rec = []
    ac.run_wide_columns(OracleSolver, record=rec)
    for what, ratio in rec:
        worst = max(worst, ratio)
        lines.append(f"{what:66s} {ratio:10.3e}")
    lines.append(f"worst = {worst:.3e}: K = 4 x = {4 * worst:.3e}")
    out = os.path.join(ROOT, "profiles", "r07", "f64_vcycle_deviation.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
