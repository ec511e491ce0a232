"""cfd_step_layout_bytes pinned to recorded values (tests/golden/layout_bytes.json).

The count is a sum over the V-cycle's launch schedule, so every op kind's cost
and every scheduling decision shows in it.  The golden file holds, for three
small meshes under six knob settings, step_layout_bytes() and amg_levels()
after one step of a 2 x 8 fixed schedule, recorded before the V-cycle schedule
became a value built once at setup.  The bytes are sums of integers far below
2^53, so the doubles compare exactly.
"""
import json
import os

import pytest

from cfd2_amd import GpuSolver, default_config
from tests.meshes import backwards_step, channel_obstacle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_bytes.json")

KNOBS = ("CFD_AMG_TAIL_ROWS", "CFD_AMG_TAIL", "CFD_AMG_FUSED_PAIR", "CFD_AMG_FUSED_RR_ROWS",
         "CFD_AMG_FUSED_PROLONG_ROWS")
SETTINGS = {
    "default": {},
    "no_tail_pair0": {"CFD_AMG_TAIL_ROWS": "0", "CFD_AMG_FUSED_PAIR": "0"},
    "no_tail_pair2": {"CFD_AMG_TAIL_ROWS": "0", "CFD_AMG_FUSED_PAIR": "2"},
    "no_tail_pair0_rr0": {"CFD_AMG_TAIL_ROWS": "0", "CFD_AMG_FUSED_PAIR": "0", "CFD_AMG_FUSED_RR_ROWS": "0"},
    "no_tail_prolong0": {"CFD_AMG_TAIL_ROWS": "0", "CFD_AMG_FUSED_PROLONG_ROWS": "0"},
    "tail_lds": {"CFD_AMG_TAIL": "lds"},
}
MESHES = ("amg_test", "graded", "channel_012")

_meshes = {}


def make_mesh(name):
    if name not in _meshes:
        if name == "amg_test":
            _meshes[name] = backwards_step()
        elif name == "graded":
            from cfd2_amd.mesh import ChannelWithObstacle, generate_cut_cell_mesh
            geo = ChannelWithObstacle(length=3.0, height=1.0, obstacle_center=(1.0, 0.5), obstacle_radius=0.15)
            _meshes[name] = generate_cut_cell_mesh(geo, 0.02, 0.08, 1.2, (3.0, 1.0))
        else:
            _meshes[name] = channel_obstacle(h=0.012)
    return _meshes[name]


def measure(mesh_name, setting, setenv, delenv, log_level=0):
    """(step_layout_bytes, amg_levels as lists) after one step of a 2 x 8 schedule."""
    from tests.test_gpu_parity import _setup_amg_test
    mesh = make_mesh(mesh_name)
    for k in KNOBS:
        delenv(k)
    for k, v in SETTINGS[setting].items():
        setenv(k, v)
    g = GpuSolver(mesh, config=default_config(log_level=log_level, fixed_outer=2, fixed_inner=8))
    _setup_amg_test(g, mesh, 1)
    g.step()
    out = (g.step_layout_bytes(), [list(x) for x in g.amg_levels()])
    g.close()
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("mesh_name", MESHES)
def test_step_layout_bytes_pinned(mesh_name, setting, monkeypatch):
    with open(GOLDEN) as fh:
        want = json.load(fh)[mesh_name][setting]
    got, levels = measure(mesh_name, setting, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert levels == want["amg_levels"], f"hierarchy differs: {levels} vs {want['amg_levels']}"
    assert got == want["step_layout_bytes"], (got, want["step_layout_bytes"])
