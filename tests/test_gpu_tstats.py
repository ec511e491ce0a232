"""Time statistics and the monitor history on the GPU: every plane and total
bit for bit against the numpy restatement (tests/tstats_ref.py) after every
accumulate, the exact checks (tests/tstats_checks.py) on the device's own
read-back, the round trips, a solved flow, the monitor's ring, the refusals, and
that neither module touches the solver's state."""
import ctypes as C

import numpy as np
import pytest

from cfd2_amd import GpuGroup, GpuSolver
from tests import tstats_cases as TC
from tests import tstats_checks as K
from tests import tstats_ref as R
from tests.meshes import channel_obstacle
from tests.synthetic import strip

pytestmark = pytest.mark.gpu

F = np.float32


def same_bits(a, b, what=""):
    """uint64 patterns equal; a NaN only has to be a NaN (its payload is the hardware's)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), what + ": NaN cells differ"
    assert np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)), what


def feed(s, sample, drive):
    """one sample onto the device; set_u zeroes p and set_p zeroes u, as the sequences do"""
    if drive == "u":
        s.set_u(np.stack([sample["u"], sample["v"]], 1))
    else:
        s.set_p(sample["p"])
    for f, phi in enumerate(sample["phi"]):
        s.set_scalar(f, phi)


def same_as(s, st, what):
    d = s.export_time_stats()
    same_bits(d["planes"], st.planes, what)
    assert d["samples"] == st.samples and np.float64(d["total_weight"]).view(np.uint64) == np.float64(st.W).view(np.uint64)
    info = s.time_stats_info()
    assert info == dict(samples=st.samples, total_weight=float(st.W), planes=len(st.planes))


def drive_and_compare(s, n, m2, nf, kind, drive, check=True):
    seq = TC.sequence(n, nf, kind, drive)
    st = R.Stats(n, m2, nf)
    for k, (sample, w) in enumerate(zip(seq, TC.WEIGHTS)):
        feed(s, sample, drive)
        s.accumulate_time_stats(w)
        st.accumulate(sample["u"], sample["v"], sample["p"], sample["phi"], w)
        same_as(s, st, f"n {n} m2 {m2} nf {nf} {kind} {drive} after sample {k}")
    for kd, f in st.kinds():  # the public getter: a mean is its plane, a covariance M / W in f64
        same_bits(s.time_stats(kd, f), st.get(kd, f), kd)
    if check:  # the mathematics on the device's own read-back
        K.check_all(s.time_stats, st.kinds(), seq, TC.WEIGHTS)
    return seq, st


@pytest.mark.parametrize("n", TC.STRIPS)
def test_every_form_matches_restatement_and_passes_the_checks(n):
    """strips around the odd last cell of the two-cells-per-lane kernel and both
    sides of a block's 512 cells; every kernel form; three kinds of values"""
    s = GpuSolver(strip(n))
    for m2, nf in TC.FORMS:
        s.enable_scalars(nf)
        for kind in TC.KINDS:
            s.enable_time_stats(second_moments=m2, scalars=True)
            assert s.time_stats_info() == dict(samples=0, total_weight=0.0, planes=R.plane_count(m2, nf))
            drive_and_compare(s, n, m2, nf, kind, "u")
        s.reset_time_stats()
        drive_and_compare(s, n, m2, nf, "unit", "p")
    s.close()


def test_obstacle_mesh():
    mesh = channel_obstacle()
    s = GpuSolver(mesh)
    s.enable_scalars(4)
    s.enable_time_stats()
    drive_and_compare(s, mesh.num_cells(), True, 4, "unit", "u")
    s.close()


def test_reset_and_export_import_round_trips():
    n, m2, nf = 513, True, 1
    s = GpuSolver(strip(n))
    s.enable_scalars(nf)
    s.enable_time_stats()
    seq, st = drive_and_compare(s, n, m2, nf, "unit", "u", check=False)
    first = s.export_time_stats()
    s.reset_time_stats()
    assert s.time_stats_info()["samples"] == 0 and not s.export_time_stats()["planes"].any()
    drive_and_compare(s, n, m2, nf, "unit", "u", check=False)
    again = s.export_time_stats()
    same_bits(again["planes"], first["planes"], "reset, then the same sequence")
    # 3 samples, export, import into a fresh handle, 2 more == 5 straight
    s.reset_time_stats()
    for sample, w in zip(seq[:3], TC.WEIGHTS):
        feed(s, sample, "u")
        s.accumulate_time_stats(w)
    saved = s.export_time_stats()
    s.close()
    t = GpuSolver(strip(n))
    t.enable_scalars(nf)
    t.enable_time_stats()
    t.import_time_stats(saved)
    back = t.export_time_stats()
    same_bits(back["planes"], saved["planes"], "raw round trip")
    assert (back["samples"], back["total_weight"]) == (3, saved["total_weight"])
    for sample, w in zip(seq[3:], TC.WEIGHTS[3:]):
        feed(t, sample, "u")
        t.accumulate_time_stats(w)
    same_as(t, st, "3 + import + 2")
    t.close()


def _flow(mesh, dye=True):
    s = GpuSolver(mesh)
    s.set_dt(0.001)
    s.set_viscosity(0.001)
    s.set_inlet_velocity(1.0)
    s.set_precond_type(1)
    s.initialize_history()
    if dye:
        s.enable_scalars(1)
        s.set_scalar_params(0, 1e-3, 1.0)
    return s


def test_solved_flow_with_a_dye():
    """3 adaptive steps past the obstacle, each step's state accumulated with the
    step's own dt; the restatement is fed with the handle's own read-backs"""
    mesh = channel_obstacle()
    n = mesh.num_cells()
    s = _flow(mesh)
    s.enable_time_stats()
    s.enable_monitor(8, [0, n // 2, n - 1])
    st = R.Stats(n, True, 1)
    seq, weights, diags = [], [], []
    for k in range(3):
        dt = F(s.constants.dt)  # the dt this step uses
        s.step_adaptive(0.5)
        s.advance_scalars()
        s.accumulate_time_stats()
        s.record_monitor()
        u, p, phi = s.get_u().astype(F), s.get_p().astype(F), s.get_scalar(0).astype(F)
        st.accumulate(u[:, 0].copy(), u[:, 1].copy(), p, [phi], dt)
        seq.append(dict(u=u[:, 0].copy(), v=u[:, 1].copy(), p=p, phi=[phi]))
        weights.append(dt)
        diags.append((float(s.constants.time), dt))
        same_as(s, st, f"after step {k}")
    assert len(set(float(w) for w in weights)) > 1, "the adaptive steps should differ in dt"
    K.check_all(s.time_stats, st.kinds(), seq, np.array(weights, F))
    m = s.monitor()
    assert np.array_equal(m["time"], np.array([d[0] for d in diags], F)) and np.array_equal(m["dt"], np.array(weights, F))
    for j, c in enumerate((0, n // 2, n - 1)):  # the probes' signals are the fields at those cells
        assert np.array_equal(m["probes"][:, j, 0], np.array([q["u"][c] for q in seq]))
        assert np.array_equal(m["probes"][:, j, 3], np.array([q["phi"][0][c] for q in seq]))
    s.close()


@pytest.mark.parametrize("P", (0, 1, 63, 64, 65, 257))
def test_monitor_ring_probes_and_diagnostics(P):
    """capacity 3, 5 records: the wrap and the oldest-first order; probe values and
    diagnostics equal the getters' at the same state, bit for bit"""
    mesh = channel_obstacle()
    n = mesh.num_cells()
    s = GpuSolver(mesh)
    s.enable_scalars(2)
    assert s.set_force_region(0.7, 0.2, 1.3, 0.8) > 0
    cells = np.random.default_rng(P).integers(0, n, P)
    if P:
        cells[0], cells[-1] = n - 1, 0
    s.enable_monitor(3, cells)
    assert s.monitor_count() == (0, 0) and s.monitor_info() == (3, P, 2, True)
    assert s.monitor()["probes"].shape == (0, P, 5)
    seq = TC.sequence(n, 2, "unit", seed=P)
    want = []
    for k, sample in enumerate(seq):
        feed(s, sample, "u")
        if k == 3:
            s.set_force_region(0.0, 0.0, 3.0, 1.0)  # the region of the moment is part of the record
        c = s.constants
        c.time = 0.25 * k
        s.constants = c
        s.record_monitor()
        u, p = s.get_u().astype(F), s.get_p().astype(F)
        phis = [s.get_scalar(f).astype(F) for f in range(2)]
        pr = np.stack([u[cells, 0], u[cells, 1], p[cells]] + [ph[cells] for ph in phis], 1).reshape(P, 5)
        want.append((F(0.25 * k), pr, bytes(s.flow_diagnostics())))
        numbers, _ = R.ring(k + 1, 3)
        assert s.monitor_count() == (k + 1, len(numbers))
        m = s.monitor()
        assert m["total"] == k + 1
        assert np.array_equal(m["time"], np.array([want[j][0] for j in numbers], F))
        assert np.array_equal(m["dt"], np.zeros(len(numbers), F))  # no step yet
        for i, j in enumerate(numbers):
            assert np.array_equal(m["probes"][i].view(np.uint32), want[j][1].view(np.uint32)), (k, j)
            assert bytes(m["diag_raw"][i]) == want[j][2], (k, j)
        assert m["diag"]["kinetic_energy"].shape == (len(numbers),) and m["diag"]["force_pressure"].shape == (len(numbers), 2)
    assert len({w[2] for w in want}) == 5 and m["diag"]["region_faces"][-1] > m["diag"]["region_faces"][0]
    # without diagnostics: the same probes, no diag
    s.enable_monitor(2, cells, diagnostics=False)
    s.record_monitor()
    m = s.monitor()
    assert "diag" not in m and np.array_equal(m["probes"][0].view(np.uint32), want[-1][1].view(np.uint32))
    s.close()


def test_both_modules_leave_the_state_alone():
    mesh = channel_obstacle()

    def run(on):
        s = _flow(mesh, dye=False)
        layout = s.step_layout_bytes()
        if on:
            s.enable_time_stats()
            s.enable_monitor(2, [1, 5, 7])
            assert s.step_layout_bytes() == layout
        for _ in range(3):
            s.step()
            if on:
                s.accumulate_time_stats()
                s.record_monitor()
        if on:
            assert s.time_stats_info()["samples"] == 3 and s.monitor_count() == (3, 2)
        out = s.get_u().tobytes(), s.get_p().tobytes(), s.step_layout_bytes()
        s.close()
        return out

    assert run(True) == run(False)


def test_refusals_change_nothing():
    n = 257
    mesh = strip(n)
    s = GpuSolver(mesh)
    for call in (s.accumulate_time_stats, s.reset_time_stats, s.time_stats_info, lambda: s.time_stats("u"),
                 s.export_time_stats):
        with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
            call()
    for call in (s.record_monitor, s.monitor_count, s.monitor):
        with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
            call()
    s.enable_scalars(1)
    s.enable_time_stats(second_moments=False)
    with pytest.raises(RuntimeError, match=r"status 1.*there was none"):  # no step yet: no dt to take
        s.accumulate_time_stats()
    with pytest.raises(RuntimeError, match=r"status 1.*there was none"):
        s.accumulate_time_stats(-1.0)
    for w in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(RuntimeError, match=r"status 1.*finite"):
            s.accumulate_time_stats(w)
    with pytest.raises(RuntimeError, match=r"status 1.*no sample"):
        s.time_stats("u")
    assert s.time_stats_info() == dict(samples=0, total_weight=0.0, planes=5)
    seq = TC.sequence(n, 1, "unit")
    feed(s, seq[0], "u")
    s.accumulate_time_stats(0.5)
    before = s.export_time_stats()
    for kind in ("uu", "uv", "vv", "pp", "uphi", "vphi"):  # planes that are off
        with pytest.raises(RuntimeError, match=r"status 1.*second_moments"):
            s.time_stats(kind)
    for kind, f in (("phi", 1), ("phi", -1), ("phiphi", 4)):
        with pytest.raises(RuntimeError, match=r"status 1.*scalar index"):
            s.time_stats(kind, f)
    with pytest.raises(RuntimeError, match=r"status 1.*kind"):
        s.time_stats(11)
    with pytest.raises(ValueError):
        s.time_stats("w")
    with pytest.raises(RuntimeError, match=r"status 1.*plane"):
        s._call("cfd_tstats_raw_get", 5, np.zeros(n).ctypes.data_as(C.POINTER(C.c_double)))
    with pytest.raises(RuntimeError, match=r"status 1.*finite"):
        s.import_time_stats(dict(before, total_weight=float("nan")))
    s.import_time_stats(before)
    # the scalar count changes under the statistics and the monitor
    s.enable_monitor(4, [0, n - 1])
    s.record_monitor()
    s.enable_scalars(2)
    with pytest.raises(RuntimeError, match=r"status 1.*scalar fields"):
        s.accumulate_time_stats(1.0)
    with pytest.raises(RuntimeError, match=r"status 1.*scalar fields"):
        s.record_monitor()
    s.enable_scalars(1)
    for f, phi in enumerate(seq[0]["phi"]):
        s.set_scalar(f, phi)
    after = s.export_time_stats()
    same_bits(after["planes"], before["planes"], "refused calls")
    assert (after["samples"], after["total_weight"]) == (1, 0.5) and s.monitor_count() == (1, 1)
    # the monitor's arguments: a refused enable leaves the old monitor
    for cap, cells, what in ((0, [0], "capacity"), ((1 << 20) + 1, [0], "capacity"), (4, [n], "outside"),
                             (4, [0, n - 1, n], "outside"), (4, np.zeros(1025, np.int64), "num_probes")):
        with pytest.raises(RuntimeError, match=r"status 1.*" + what):
            s.enable_monitor(cap, cells)
    assert s.monitor_info() == (4, 2, 1, True) and s.monitor_count() == (1, 1)
    s.record_monitor()
    m = s.monitor()
    assert m["probes"].shape == (2, 2, 4) and np.array_equal(m["probes"][0], m["probes"][1])
    with pytest.raises(RuntimeError, match=r"status 1.*held"):
        s._call("cfd_monitor_get", 1, 2, None, None, None, None)
    s.disable_time_stats()
    s.disable_monitor()
    with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
        s.accumulate_time_stats(1.0)
    with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
        s.record_monitor()
    s.close()
    # distributed handles: a 2-rank group and each of its members
    g = GpuGroup(channel_obstacle(), 2)
    for call in (g.enable_time_stats, lambda: g.enable_monitor(4, [0])):
        with pytest.raises(RuntimeError, match=r"status 1.*one GPU only"):
            call()
    for r in g.ranks:
        for call in (r.enable_time_stats, r.accumulate_time_stats, r.disable_time_stats, lambda: r.enable_monitor(4, [0]),
                     r.record_monitor, r.disable_monitor, r.monitor_count):
            with pytest.raises(RuntimeError, match=r"status 1.*one GPU only"):
                call()
    g.close()
