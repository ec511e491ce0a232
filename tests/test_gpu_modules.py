"""The five opt-in post-processing modules (renderer, tracer particles, time
statistics, monitor, wall surface) are independent of one another and of the
step: releasing one leaves every other module's output byte for byte what it
was, whatever the order, a released module refuses in its documented words, and
the step afterwards gives the bits of a solver that never enabled any."""
import numpy as np
import pytest

from cfd2_amd import GpuSolver
from tests.meshes import channel_obstacle

pytestmark = pytest.mark.gpu

MODULES = ("render", "particles", "tstats", "monitor", "surface")
BODY = (0.7, 0.2, 1.3, 0.8)
INVERTED = (1.0, 0.0, 0.0, 1.0)
STEPS = 3


@pytest.fixture(scope="module")
def mesh():
    return channel_obstacle(h=0.1)  # 296 cells around the disc: two 256-cell chunks, the second ragged


def _flow(mesh):
    """one dye field, the force region around the body, three steps"""
    s = GpuSolver(mesh)
    s.set_dt(0.001)
    s.set_viscosity(0.001)
    s.set_inlet_velocity(1.0)
    s.set_precond_type(1)
    s.initialize_history()
    s.enable_scalars(1)
    s.set_scalar_params(0, 1e-3, 1.0)
    assert s.set_force_region(*BODY) > 0
    for _ in range(STEPS):
        s.step()
        s.advance_scalars()
    return s


def _enable_all(s, mesh):
    n = mesh.num_cells()
    s.set_render_mesh(mesh)
    assert s.set_view(64, 48) > 0
    s.set_particle_mesh(mesh)
    s.enable_particles(100)
    rng = np.random.default_rng(5)
    s.seed_particles(np.stack([rng.uniform(0.05, 2.95, 100), rng.uniform(0.05, 0.95, 100)], 1))
    s.advance_particles()
    s.enable_time_stats(second_moments=True)
    s.enable_monitor(4, [0, n - 1])
    assert s.select_surface(BODY) > 0
    s.enable_surface_stats()
    for w in (0.5, 0.25):  # every accumulating module holds two samples of the current state
        s.accumulate_time_stats(w)
        s.record_monitor()
        s.accumulate_surface_stats(w)
    assert s.particle_stats()["alive"] > 0 and s.render("speed").any()
    assert s.time_stats_info()["samples"] == 2 and s.monitor_count() == (2, 2) and s.surface_info()["samples"] == 2


def _output(s, name, on):
    """what module `name` returns now, as bytes; `on`: the modules still enabled"""
    if name == "render":
        out = [s.render("speed").tobytes(), repr(s.last_render_range)]
        out += [s.render("vorticity").tobytes(), repr(s.last_render_range)]  # through the flow diagnostics
        out += [s.render("scalar", scalar=0).tobytes(), s.render_owner().tobytes()]
        return out
    if name == "particles":
        out = [a.tobytes() for a in s.particles()] + [repr(sorted(s.particle_stats().items()))]
        if "render" in on:  # the overlay reads the renderer's last frame
            s.render("speed", range=(0.0, 2.0))
            out.append(s.render_particles((10, 200, 30, 128)).tobytes())
        return out
    if name == "tstats":
        e = s.export_time_stats()
        return [e["planes"].tobytes(), e["samples"], e["total_weight"], s.time_stats("uu").tobytes(),
                s.time_stats("uphi").tobytes()]
    if name == "monitor":
        m = s.monitor()
        return [m["time"].tobytes(), m["dt"].tobytes(), m["probes"].tobytes(), [bytes(d) for d in m["diag_raw"]],
                s.monitor_count(), s.monitor_info()]
    if name == "surface":
        return [s.surface()["channels"].tobytes(), s.surface_stats("mean")["channels"].tobytes(),
                s.surface_stats("variance")["channels"].tobytes(), repr(sorted(s.surface_info().items()))]
    raise KeyError(name)


def _reference(s):
    ref = {name: _output(s, name, MODULES) for name in MODULES}
    ref["particles (no overlay)"] = ref["particles"][:-1]
    return ref


def _release(s, name):
    if name == "render":
        s.set_render_mesh(None)
    elif name == "particles":
        s.set_particle_mesh(None)
    elif name == "tstats":
        s.disable_time_stats()
    elif name == "monitor":
        s.disable_monitor()
    else:
        assert s.select_surface(INVERTED) == 0


def _assert_refuses(s, name):
    if name == "render":
        with pytest.raises(RuntimeError, match="no polygons"):
            s.set_view(64, 48)  # the library's refusal
        with pytest.raises(RuntimeError, match="no polygons"):
            s.render("speed")
    elif name == "particles":
        for call in (s.advance_particles, s.particle_stats, s.particles):
            with pytest.raises(RuntimeError, match="not enabled"):
                call()
        with pytest.raises(RuntimeError, match="no mesh"):
            s.enable_particles(4)
    elif name == "tstats":
        for call in (s.accumulate_time_stats, s.time_stats_info, s.export_time_stats):
            with pytest.raises(RuntimeError, match=r"status 1.*time statistics are not enabled"):
                call()
    elif name == "monitor":
        for call in (s.record_monitor, s.monitor_count, s.monitor_info, s.monitor):
            with pytest.raises(RuntimeError, match=r"status 1.*the monitor is not enabled"):
                call()
    else:
        for call in (s.surface, s.surface_info, s.accumulate_surface_stats):
            with pytest.raises(RuntimeError, match=r"status 1.*no surface is selected"):
                call()


def _step_bits(s):
    s.step()
    return s.get_u().tobytes(), s.get_p().tobytes()


@pytest.fixture(scope="module")
def untouched(mesh):
    """the step after the three, of a solver that never enabled a module"""
    s = _flow(mesh)
    out = _step_bits(s)
    s.close()
    return out


@pytest.mark.parametrize("order", (MODULES, MODULES[::-1]), ids=("in order", "reversed"))
def test_release_one_at_a_time(mesh, untouched, order):
    s = _flow(mesh)
    _enable_all(s, mesh)
    ref = _reference(s)
    assert _reference(s) == ref, "reading the modules twice"
    on = list(MODULES)
    for name in order:
        _release(s, name)
        on.remove(name)
        _assert_refuses(s, name)
        for other in on:
            key = "particles (no overlay)" if other == "particles" and "render" not in on else other
            assert _output(s, other, on) == ref[key], f"{other} after releasing {name}"
    assert _step_bits(s) == untouched
    s.close()
