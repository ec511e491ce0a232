"""Float64 checks of the flow side (tests/flow_checks.py) over the case list of
tests/flow_cases.py on the CPU oracle: the face flux, the gradients, d_p, every
matrix entry, the right-hand side and the update; and the proof that the checks
resolve wrong conventions.  tests/test_gpu_flow_f64.py runs the same cases
through the same drivers on the HIP path, so every bound it asserts is first
shown to hold here.  Run with -s for the worst error / bound per check and mesh."""
import functools

import pytest

from tests import flow_cases as cs
from tests import flow_checks as fl
from tests.oracle_py import OracleSolver


@pytest.mark.parametrize("density", cs.DENSITIES)
@pytest.mark.parametrize("name", cs.MESHES)
def test_flow_stages_satisfy_the_float64_formulas(name, density):
    """Schemes {0, 1, 2} x time schemes {0, 1} of one mesh and density: every
    face's flux, every cell's gradients and d_p, every stored matrix entry and
    every row of the right-hand side, each to its derived bound (the counts
    are asserted by the driver)."""
    worst = {}
    cover = cs.run_mesh(OracleSolver, name, density, worst)
    print(name, density, cover, {k: f"{r:.3f} ({w})" for k, (r, w) in worst.items()})


def test_case_list_covers_what_can_go_wrong():
    """Over the list: every face kind, both upwind directions, a degenerate
    weight and a floored distance occur, and at most 1 % of a case's faces
    took either branch; the channel mesh gives the 8-way block remapping of
    row_id() a quotient and a remainder within 2,500 to 3,800 cells."""
    kinds = {0: 0, fl.INLET: 0, fl.OUTLET: 0, fl.WALL: 0}
    out = back = degenerate = floored = 0
    for name in cs.MESHES:
        cover = cs.run_mesh(OracleSolver, name, 1.0)
        faces = cs.mesh_of(name).num_faces()
        assert cover["either"] <= cs.MAX_EITHER_SHARE * faces, (name, cover)
        for k, v in cover["kinds"].items():
            kinds[k] += v
        if cs.mesh_of(name).num_cells() >= 100:
            assert min(cover["kinds"].values()) > 0 and min(cover["upwind"][:2]) > 0, (name, cover)
        out, back = out + cover["upwind"][0], back + cover["upwind"][1]
        degenerate, floored = degenerate + cover["degenerate"], floored + cover["floored"]
    assert min(kinds.values()) > 0 and out > 0 and back > 0, (kinds, out, back)
    assert degenerate > 0 and floored > 0
    big = cs.mesh_of("channel13")
    assert 2500 <= big.num_cells() <= 3800
    assert cs.blocks(big) >= 9 and cs.blocks(big) % 8 != 0, cs.blocks(big)


@pytest.mark.parametrize("name", cs.UPDATE_MESHES)
def test_update_and_max_difference_fold(name):
    print(name, f"check_update worst {cs.run_update(OracleSolver, name):.3f}")


def test_distance_sum_at_the_floor_takes_either_branch():
    """A strip of side 1e-6: every distance sum is the floor itself to within
    rounding, so both lambdas are evaluated (here they agree: 1/2) and the
    faces are counted; the share bound of the drivers is what keeps such a
    mesh out of the case list."""
    from tests.synthetic import strip
    mesh = strip(3, h=1e-6)
    st = cs.flow_state(OracleSolver, mesh, 2, 1, 1000.0)
    assert fl.Geometry(st.arrays).ambiguous.sum() == 2
    for check in cs.CHECKS:
        out = getattr(fl, check)(st)
        assert out.get("either", 2) >= 2, (check, out)
    with pytest.raises(AssertionError):
        cs.run_checks(st)  # 2 of 10 faces: above the 1 % share


# ---------------------------------------------------------------- wrong conventions
WRONG_MESHES = ["voronoi", "graded", "strip7", "wheel100"]
# error -> the checks that must see it (on at least one mesh each)
WRONG_SEEN_BY = {
    "matrix_dist_c": ["check_matrix_entries"],  # dist_c for dist_n in the matrix
    "d_p_dist_n": ["check_d_p"],  # dist_n for dist_c in d_p
    "lambda_swapped": ["check_flux", "check_gradients", "check_matrix_entries"],
    "rhie_chow_sign": ["check_flux"],
    "quick_swapped": ["check_rhs"],  # 3/8 phi_U + 5/8 phi_D
    "bdf2_r": ["check_rhs"],  # r / (1 + r) for r^2 / (1 + r)
    "no_ramp": ["check_flux", "check_gradients", "check_rhs"],
    "outlet_p": ["check_gradients"],  # p_i on an outlet face instead of 0
    "nu_scaled": ["check_matrix_entries"],  # nu (1 + 2^-10)
}


@functools.lru_cache(maxsize=None)
def _state(name):
    return cs.flow_state(OracleSolver, cs.mesh_of(name), 2, 1, 1000.0)  # QUICK, BDF2


def test_every_wrong_convention_is_listed():
    assert set(WRONG_SEEN_BY) == set(fl.WRONG)


@pytest.mark.parametrize("wrong", list(WRONG_SEEN_BY))
def test_checks_resolve_wrong_conventions(wrong):
    """Each deliberate error in the float64 formulas exceeds its bound on the
    oracle's output (scheme 2, BDF2 with r = 0.75, density 1000; the right
    formulas pass: the test above).  As run, error / bound of the worst element:

    - matrix_dist_c: check_matrix_entries on voronoi (6.7e4 x) and graded; the
      strips and the wheel are orthogonal (dist_c = dist_n) and cannot show it;
    - d_p_dist_n: check_d_p on voronoi (3.0 x) and graded (573 x); the
      diffusive part of that diagonal is small against a_t at density 1000;
    - lambda_swapped: check_flux, check_gradients and check_matrix_entries on
      voronoi, graded and wheel100 (1e4 x and more); every face of a strip has
      lambda = 1/2;
    - rhie_chow_sign: check_flux on all four (5e5 x and more);
    - quick_swapped: check_rhs on all four (5e3 x on strip7, 5e4 x and more);
    - bdf2_r: check_rhs on all four (2.6e4 x);
    - no_ramp: check_flux, check_gradients and check_rhs on all four (1e5 x);
    - outlet_p: check_gradients on all four (2e5 x and more);
    - nu_scaled: check_matrix_entries on all four (512 x: 2^-10 over 16 eps32,
      on the entries that are diffusion alone), check_d_p on graded (4.2 x)."""
    caught = []
    for name in WRONG_MESHES:
        for check in cs.CHECKS:
            try:
                getattr(fl, check)(_state(name), (wrong,))
            except AssertionError as e:
                assert f"f64 {check}" in str(e), e  # the check's own failure
                caught.append((name, check))
    print(wrong, caught)
    for check in WRONG_SEEN_BY[wrong]:
        assert any(c == check for _, c in caught), f"{wrong}: {check} passes on every one of {WRONG_MESHES}"
