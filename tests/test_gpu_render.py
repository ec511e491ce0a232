"""Frames on the GPU: the ownership map and the image of every field kind,
bit for bit against the numpy restatement (tests/render_ref.py), the map
against the float64 check (tests/render_checks.py), the refusals, and that
rendering leaves the solver's state alone."""
import numpy as np
import pytest

from cfd2_amd import GpuGroup, GpuSolver
from cfd2_amd.mesh import MappedMesh, save_view_file
from tests import render_cases as RC
from tests import render_checks as K
from tests import render_ref as R
from tests.test_gpu_flow_diag import _fields

pytestmark = pytest.mark.gpu

F = np.float32
FIXED = (0.2, 1.1)


def _solver(mesh):
    s = GpuSolver(mesh)
    u, p = RC.with_nan(mesh, *_fields(mesh))
    s.set_u(u)
    s.set_p(p)
    return s


def _values(s):
    """the f32 cell values of every field kind as the handle reports them"""
    u, p = s.get_u().astype(F), s.get_p().astype(F)
    return dict(u=u, p=p, vorticity=s.vorticity().astype(F), divergence=s.divergence().astype(F))


def _same_range(got, want):
    return np.array_equal(np.array(got, F).view(np.uint32), np.array(want, F).view(np.uint32))


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_map_and_image_match_restatement(name):
    mesh, W, H, box, full, ref_owner = RC.case(name)
    s = _solver(mesh)
    s.set_render_mesh(mesh)
    covered = s.set_view(W, H, box)
    owner = s.render_owner()
    assert owner.shape == (H, W) and owner.dtype == np.uint32
    assert np.array_equal(owner, ref_owner)
    assert covered == int((ref_owner != R.NONE).sum())
    if name == "outside":
        assert covered == 0
    vals = _values(s)
    for field in ("speed", "ux", "uy", "p", "vorticity", "divergence"):
        v = R.field_values(field, **vals)
        for rng in (FIXED, None):
            img = s.render(field, range=rng)
            ref, used = R.render(ref_owner, v, rng)
            assert img.shape == (H, W, 4) and img.dtype == np.uint8
            assert np.array_equal(img, ref), (field, rng)
            assert _same_range(s.last_render_range, used), (field, rng, s.last_render_range, used)
    if name == "outside":
        assert not s.render("speed").any()
    # the NaN cell, where it is on the image, is opaque black
    k = RC.nan_cell(mesh)
    img = s.render("p", range=FIXED)
    assert (img[owner == k] == (0, 0, 0, 255)).all() and (img[owner == R.NONE] == 0).all()
    # the float64 check of the device's own map
    vx, vy, off, idx = RC.polygons_of(RC.CASES[name][0])
    K.assert_owner_map(vx, vy, off, idx, full, owner, cap=1.0 if name in RC.UNCAPPED else 0.05)
    assert np.array_equal(s.render(0, range=FIXED), s.render("speed", range=FIXED))  # a field by its number
    s.close()


def test_speed_is_the_correctly_rounded_sqrt():
    mesh = RC.mesh_of("big")
    s = GpuSolver(mesh)
    rng = np.random.default_rng(11)
    u = (rng.standard_normal((mesh.num_cells(), 2)) * 10.0 ** rng.uniform(-22, 18, (mesh.num_cells(), 1))).astype(F)
    s.set_u(u.astype(np.float64))
    s.set_render_mesh(mesh)
    s.set_view(128, 64)
    s.render("speed")
    want = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1])  # np.sqrt on f32 is correctly rounded
    assert _same_range(s.last_render_range, (want.min(), want.max()))
    # each cell's value through a range that isolates it: the image is ref's for the very same f32 values
    owner = s.render_owner()
    assert np.array_equal(s.render("speed", range=(0.0, 1.0)), R.shade(owner, want, 0.0, 1.0))
    s.close()


def test_scalar_field_renders_like_get_scalar():
    mesh, W, H, box, full, ref_owner = RC.case("obstacle")
    s = GpuSolver(mesh)
    s.set_dt(0.001)
    s.set_viscosity(0.001)
    s.set_inlet_velocity(1.0)
    s.initialize_history()
    s.step()
    s.enable_scalars(1)
    s.set_scalar_params(0, 1e-3, 1.0)
    s.set_scalar(0, np.where(mesh.arrays()["cell_cx"] < 1.0, 1.0, 0.0))
    s.advance_scalars()
    s.set_render_mesh(mesh)
    s.set_view(W, H, box)
    phi = s.get_scalar(0).astype(F)
    for rng in ((0.0, 1.0), None):
        ref, used = R.render(ref_owner, phi, rng)
        assert np.array_equal(s.render("scalar", range=rng, scalar=0), ref)
        assert _same_range(s.last_render_range, used)
    with pytest.raises(RuntimeError, match="scalar field index"):
        s.render("scalar", scalar=1)
    s.close()


def test_refusals(tmp_path):
    mesh, W, H, box, full, ref_owner = RC.case("obstacle")
    s = GpuSolver(mesh)
    with pytest.raises(RuntimeError, match="no polygons"):
        s.render("speed")
    with pytest.raises(RuntimeError, match="no polygons"):
        s.set_view(8, 8)
    with pytest.raises(RuntimeError, match="no polygons"):
        s.render_owner()
    s.set_render_mesh(mesh)
    with pytest.raises(RuntimeError, match="no view"):
        s.render("speed")
    with pytest.raises(RuntimeError, match="no view"):
        s.render_owner()
    for w, h in ((0, 8), (8, 0), (8193, 8), (8, 8193)):
        with pytest.raises(RuntimeError, match="1..8192"):
            s.set_view(w, h)
    for bad in ((1.0, 0.0, 1.0, 1.0), (0.0, 1.0, 3.0, 0.5), (0.0, 0.0, np.nan, 1.0), (0.0, 0.0, np.inf, 1.0)):
        with pytest.raises(RuntimeError, match="box"):
            s.set_view(8, 8, bad)
    with pytest.raises(RuntimeError, match="no view"):  # a refused set_view leaves none
        s.render("speed")
    s.set_view(W, H)
    with pytest.raises(RuntimeError, match="field must be"):
        s.render(7)
    with pytest.raises(RuntimeError, match="field must be"):
        s.render(-1)
    with pytest.raises(ValueError, match="unknown field"):
        s.render("enstrophy")
    with pytest.raises(RuntimeError, match="not enabled"):
        s.render("scalar")
    # malformed polygons: a refused call changes nothing
    vx, vy, off, idx = RC.polygons_of("obstacle")
    for o in (np.r_[1, off[1:]], np.r_[off[:5], off[3], off[6:]]):
        with pytest.raises(RuntimeError, match="cell_vertex_offsets"):
            s.set_render_polygons(vx, vy, o, idx)
    bad_idx = idx.copy()
    bad_idx[17] = len(vx)
    with pytest.raises(RuntimeError, match="vertex index"):
        s.set_render_polygons(vx, vy, off, bad_idx)
    with pytest.raises(ValueError):
        s.set_render_polygons(vx, vy, off[:-1], idx)
    assert np.array_equal(s.render_owner(), ref_owner)
    # a mesh view without vertices cannot render
    path = str(tmp_path / "view.mesh")
    save_view_file(mesh, path)
    with pytest.raises(ValueError, match="cannot render"):
        s.set_render_mesh(MappedMesh(path))
    s.close()
    g = GpuGroup(mesh, 2)
    with pytest.raises(RuntimeError, match="one GPU only"):
        g.set_render_mesh(mesh)
    with pytest.raises(RuntimeError, match="one GPU only"):
        g.render("speed")
    g.close()


def test_second_view_replaces_the_first_and_release():
    mesh, W, H, box, full, ref_owner = RC.case("obstacle")
    mesh2, W2, H2, box2, full2, ref2 = RC.case("zoom")
    assert mesh2 is mesh
    s = _solver(mesh)
    s.set_render_mesh(mesh)
    s.set_view(W, H, box)
    s.set_view(W2, H2, box2)
    assert np.array_equal(s.render_owner(), ref2)
    s.set_view(W, H, box)  # and back, through a reallocation of the map
    assert np.array_equal(s.render_owner(), ref_owner)
    a = s.render("speed")
    assert np.array_equal(s.render("speed"), a)  # a frame does not disturb the next
    s.set_render_mesh(None)
    with pytest.raises(RuntimeError, match="no polygons"):
        s.render("speed")
    s.set_render_mesh(mesh)  # and usable again
    s.set_view(W, H, box)
    assert np.array_equal(s.render("speed"), a)
    s.close()


def test_rendering_is_read_only():
    """two steps with a render of every kind between and after them: u, p and the
    step info (all of it but the solve's wall-clock time) are byte-equal to a twin
    that never rendered"""
    mesh, W, H, box, full, ref_owner = RC.case("obstacle")

    def run(render):
        s = GpuSolver(mesh)
        s.set_dt(0.001)
        s.set_viscosity(0.001)
        s.set_inlet_velocity(1.0)
        s.set_precond_type(1)
        s.enable_scalars(1)
        s.initialize_history()
        if render:
            s.set_render_mesh(mesh)
            s.set_view(W, H, box)
        for _ in range(2):
            s.step()
            if render:
                for field in R.FIELDS:
                    s.render(field)
                    s.render(field, range=FIXED)
                s.render_owner()
        info = s.step_info()
        info.stats_p.time_s = 0.0  # the wall-clock time of the last solve: the one field that is not state
        out = s.get_u().tobytes(), s.get_p().tobytes(), bytes(info)
        s.close()
        return out

    assert run(True) == run(False)
