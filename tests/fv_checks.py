"""Float64 checks of the assembled coupled system and of the FGMRES solve,
written from the maths and not from any restatement of the kernels.

HELPER MODULE, not a test: numpy and scipy.sparse only.  Every function takes
a mesh (its `arrays()`) and the debug buffers of a solver object -- GpuSolver
and OracleSolver share the `debug_buffer` / `constants` / `step_info`
surface -- computes in float64 from the f32 buffers and raises AssertionError
naming the worst cell or row.

What is checked follows from the discretisation being a conservative finite
volume scheme on closed cells and from FGMRES being a minimal-residual method:

- momentum conservation: an interior row of A_uu (and A_vv) sums to the time
  coefficient plus the net mass flux out of the cell (central diffusion
  cancels, upwind convection leaves the flux);
- geometric closure: the pressure-gradient row of an interior cell sums to
  sum_f A_f n_f = 0, the two interpolation weights of a face add to 1, and the
  divergence block repeats the gradient block;
- the pressure operator is a symmetric, weakly diagonally dominant M-matrix
  with zero interior row sums, and the scalar (AMG) matrix is rho times it;
- the stored diagonal inverses invert the diagonals they belong to;
- the reported linear residual is the true residual |b - A x| of the stored
  system, from both sides; a converged solve meets its tolerance; the true
  residual does not grow with the Krylov dimension.

"Interior cell": a cell none of whose faces is a boundary face.

Tolerance of every assembled-system identity: TOL_ROW = 16 eps32 times the
sum of the magnitudes of the terms of that row's identity -- a rounding bound
(a row has about a dozen f32 terms, each a product of a few rounded factors),
not a measurement.
"""
import numpy as np
import scipy.sparse as sp

EPS32 = float(np.finfo(np.float32).eps)
TOL_ROW = 16.0 * EPS32
NONE = 0xFFFFFFFF
SAFE_INVERSE_GUARD = 1e-14  # |d| <= guard: the stored inverse is 0 (safe_inverse, oracle.cpp)


# --------------------------------------------------------------------- layout
def _coupled_csr(mesh, vals):
    """Reference coupled CSR (init/linear_solver/mod.rs:180-216) as scipy from the
    scalar pattern: block row i holds sub-rows u, v, p, each listing
    (3j, 3j+1, 3j+2) for the neighbours j of i in ascending order."""
    import scipy.sparse as sp
    srow, scol = _scalar_csr_fast(mesh)
    n = len(srow) - 1
    deg = np.diff(srow)
    base3 = (3 * scol[:, None] + np.arange(3)[None, :]).reshape(-1)
    pos = np.arange(9 * len(scol))
    row = np.repeat(np.arange(n), 9 * deg)
    off = pos - 9 * srow[row]
    sub = off // (3 * deg[row])
    cols = base3[3 * srow[row] + off % (3 * deg[row])]
    return sp.csr_matrix((vals, (3 * row + sub, cols)), shape=(3 * n, 3 * n))


def _scalar_csr_fast(mesh):
    a = mesh.arrays()
    n = len(a["cell_cx"])
    own = a["face_owner"].astype(np.int64)
    nb = a["face_neighbor"].astype(np.int64)
    m = nb != 0xFFFFFFFF
    r = np.concatenate([np.arange(n), own[m], nb[m]])
    c = np.concatenate([np.arange(n), nb[m], own[m]])
    key = np.unique(r * n + c)
    rr, cc = key // n, key % n
    srow = np.zeros(n + 1, dtype=np.int64)
    np.add.at(srow, rr + 1, 1)
    return np.cumsum(srow), cc


def interior_mask(mesh):
    """True for the cells none of whose faces is a boundary face."""
    a = mesh.arrays()
    n = len(a["cell_cx"])
    own = a["face_owner"].astype(np.int64)
    nb = a["face_neighbor"].astype(np.int64)
    mask = np.ones(n, dtype=bool)
    mask[own[nb == NONE]] = False
    return mask


class System:
    """The buffers of one solver after an assembly (or a step), in float64.
    Plain attributes, so that a test can mutate a copy."""

    def __init__(self, mesh, solver):
        self.mesh = mesh
        self.constants = solver.constants
        self.flux = solver.debug_buffer(0).astype(np.float64)
        self.rhs = solver.debug_buffer(3).astype(np.float64)
        self.x = solver.debug_buffer(4).astype(np.float64)
        self.dinv = [solver.debug_buffer(i).astype(np.float64) for i in (5, 6, 7)]
        self.scalar = solver.debug_buffer(8).astype(np.float64)
        self.coupled = solver.debug_buffer(9).astype(np.float64)

    def copy(self):
        import copy
        c = copy.copy(self)
        for k in ("flux", "rhs", "x", "scalar", "coupled"):
            setattr(c, k, getattr(self, k).copy())
        c.dinv = [d.copy() for d in self.dinv]
        return c

    def matrix(self):
        return _coupled_csr(self.mesh, self.coupled)

    def block(self, r, c):
        """Block (r, c) of the coupled matrix, r and c in 'u', 'v', 'p'."""
        i, j = "uvp".index(r), "uvp".index(c)
        return self.matrix()[i::3, j::3].tocsr()

    def scalar_matrix(self):
        srow, scol = _scalar_csr_fast(self.mesh)
        n = len(srow) - 1
        return sp.csr_matrix((self.scalar, scol, srow), shape=(n, n))


def _abs_rowsum(M):
    return np.asarray(abs(M).sum(axis=1)).ravel()


def _rowsum(M):
    return np.asarray(M.sum(axis=1)).ravel()


def _assert_rows(err, scale, rows, what, extra=""):
    """|err[i]| <= TOL_ROW * scale[i] on the given rows; names the worst row."""
    if not np.any(rows):
        return 0
    idx = np.nonzero(rows)[0]
    e, s = np.abs(err[idx]), scale[idx]
    assert np.all(np.isfinite(e)) and np.all(np.isfinite(s)), f"{what}: non-finite entries"
    over = e - TOL_ROW * s
    w = int(np.argmax(over))
    assert over[w] <= 0.0, (f"{what}: row/cell {idx[w]}: |error| {e[w]:.3e} > 16 eps32 * {s[w]:.3e} "
                            f"= {TOL_ROW * s[w]:.3e} ({e[w] / max(s[w], 1e-300) / EPS32:.2f} eps32){extra}")
    return len(idx)


# ------------------------------------------------------------- assembled system
def time_coefficient(mesh, constants):
    """vol rho / dt (Euler); times (1 + 2r)/(1 + r), r = dt/dt_old (BDF2, variable step)."""
    c = constants
    vol = mesh.arrays()["cell_vol"].astype(np.float32).astype(np.float64)
    tc = vol * float(c.density) / float(c.dt)
    if int(c.time_scheme) == 1:
        r = float(c.dt) / float(c.dt_old)
        tc = tc * (1.0 + 2.0 * r) / (1.0 + r)
    return tc


def net_flux(mesh, flux):
    """(sum_f s_f flux_f, sum_f |flux_f|) per cell over the internal faces:
    s_f = +1 for the owner, -1 for the neighbour."""
    a = mesh.arrays()
    n = len(a["cell_cx"])
    own = a["face_owner"].astype(np.int64)
    nb = a["face_neighbor"].astype(np.int64)
    m = nb != NONE
    net, mag = np.zeros(n), np.zeros(n)
    np.add.at(net, own[m], flux[m])
    np.add.at(net, nb[m], -flux[m])
    np.add.at(mag, own[m], np.abs(flux[m]))
    np.add.at(mag, nb[m], np.abs(flux[m]))
    return net, mag


def check_momentum(sysm):
    """Interior rows: sum_j A_uu[i,j] = tc_i + sum_f s_f flux_f, the same for
    A_vv; every A_uv / A_vu entry is zero.  Returns the interior rows checked."""
    mesh = sysm.mesh
    inner = interior_mask(mesh)
    tc = time_coefficient(mesh, sysm.constants)
    net, mag = net_flux(mesh, sysm.flux)
    count = 0
    for comp in "uv":
        A = sysm.block(comp, comp)
        err = _rowsum(A) - tc - net
        scale = _abs_rowsum(A) + np.abs(tc) + mag
        count = _assert_rows(err, scale, inner, f"momentum conservation A_{comp}{comp}")
    for r, c in ("uv", "vu"):
        A = sysm.block(r, c)
        assert A.nnz == 0 or np.abs(A.data).max() == 0.0, f"A_{r}{c} has a non-zero entry"
    return count


def check_closure(sysm):
    """Interior rows: sum_j A_up[i,j] = 0 = sum_j A_vp[i,j] (sum of A n over a
    closed cell; the two weights of a face add to 1), and the divergence rows
    A_pu, A_pv repeat A_up, A_vp.  Returns the interior rows checked."""
    inner = interior_mask(sysm.mesh)
    count = 0
    for comp in "uv":
        G = sysm.block(comp, "p")
        count = _assert_rows(_rowsum(G), _abs_rowsum(G), inner, f"geometric closure A_{comp}p")
        D = sysm.block("p", comp)
        diff = (D - G).tocsr()
        _assert_rows(_abs_rowsum(diff), _abs_rowsum(D) + _abs_rowsum(G), inner, f"A_p{comp} == A_{comp}p")
    return count


def check_face_weights(sysm):
    """Every internal face, whatever its cells: A_up[o,n] - A_up[n,o] = A_f nx_f
    (owner side (1 - w) A n, neighbour side -w A n: the weights add to 1); the
    same with ny for A_vp.  Sees a weight swapped within one row, which no
    row sum can.  Returns the faces checked."""
    a = sysm.mesh.arrays()
    own = a["face_owner"].astype(np.int64)
    nb = a["face_neighbor"].astype(np.int64)
    m = (nb != NONE) & (nb != own)
    o, n = own[m], nb[m]
    if len(o) == 0:
        return 0
    area = a["face_area"].astype(np.float32).astype(np.float64)[m]
    for comp, key in (("u", "face_nx"), ("v", "face_ny")):
        G = sysm.block(comp, "p")
        g_on = np.asarray(G[o, n]).ravel()
        g_no = np.asarray(G[n, o]).ravel()
        an = area * a[key].astype(np.float32).astype(np.float64)[m]
        err = g_on - g_no - an
        scale = np.abs(g_on) + np.abs(g_no) + np.abs(an)
        faces = np.nonzero(m)[0]
        over = np.abs(err) - TOL_ROW * scale
        w = int(np.argmax(over))
        assert over[w] <= 0.0, (f"face weights A_{comp}p: face {faces[w]} (cells {o[w]}, {n[w]}): "
                                f"|error| {abs(err[w]):.3e} > {TOL_ROW * scale[w]:.3e}")
    return len(o)


def check_pressure(sysm):
    """A_pp and the scalar matrix: symmetric, interior rows sum to zero, no
    positive off-diagonal, diagonal >= sum of off-diagonal magnitudes (what the
    Jacobi-smoothed AMG relies on); scalar == rho * A_pp.  Returns the
    interior rows checked."""
    inner = interior_mask(sysm.mesh)
    rho = float(sysm.constants.density)
    App, S = sysm.block("p", "p"), sysm.scalar_matrix()
    every = np.ones(App.shape[0], dtype=bool)
    count = 0
    for name, M in (("A_pp", App), ("scalar matrix", S)):
        asym = (M - M.T).tocsr()
        # per row: the worst pair against the magnitudes of that pair
        pair = (abs(M) + abs(M.T)).tocsr()
        bad = (abs(asym) - TOL_ROW * pair).tocsr()
        worst = bad.max() if bad.nnz else 0.0
        if worst > 0.0:
            coo = bad.tocoo()
            k = int(np.argmax(coo.data))
            raise AssertionError(f"{name} not symmetric: entry ({coo.row[k]}, {coo.col[k]}) = {M[coo.row[k], coo.col[k]]:.9e}"
                                 f" vs ({coo.col[k]}, {coo.row[k]}) = {M[coo.col[k], coo.row[k]]:.9e}")
        count = _assert_rows(_rowsum(M), _abs_rowsum(M), inner, f"{name} interior row sum")
        diag = M.diagonal()
        offd = (M - sp.diags(diag)).tocsr()
        offd.eliminate_zeros()
        if offd.nnz:
            coo = offd.tocoo()
            k = int(np.argmax(coo.data))
            assert coo.data[k] <= 0.0, f"{name}: positive off-diagonal {coo.data[k]:.3e} at ({coo.row[k]}, {coo.col[k]})"
        offsum = _abs_rowsum(offd)
        _assert_rows(np.minimum(diag - offsum, 0.0), np.abs(diag) + offsum, every, f"{name} diagonal dominance")
    diff = (S - rho * App).tocsr()
    err, scale = _abs_rowsum(diff), _abs_rowsum(S) + rho * _abs_rowsum(App)
    # entrywise: the worst entry of a row against that entry's own magnitudes
    pair = (abs(S) + rho * abs(App)).tocsr()
    bad = (abs(diff) - TOL_ROW * pair).tocsr()
    if bad.nnz and bad.max() > 0.0:
        coo = bad.tocoo()
        k = int(np.argmax(coo.data))
        i, j = coo.row[k], coo.col[k]
        raise AssertionError(f"scalar matrix != rho * A_pp at ({i}, {j}): {S[i, j]:.9e} vs {rho} * {App[i, j]:.9e}")
    _assert_rows(err, scale, every, "scalar matrix == rho * A_pp")
    return count


def check_diagonal_inverses(sysm):
    """ids 5, 6, 7 times the diagonal each inverts equal 1: the A_uu diagonal,
    the A_vv diagonal and -- id 7 -- the diagonal of the SCALAR pressure matrix
    (id 8, rho-scaled; oracle.cpp assemble(): safe_inverse(scalar_diag_p)),
    not A_pp's.  Rows under the guard |d| <= 1e-14 hold 0.  Returns rows checked."""
    diags = (sysm.block("u", "u").diagonal(), sysm.block("v", "v").diagonal(), sysm.scalar_matrix().diagonal())
    n = len(diags[0])
    for name, d, inv in zip(("diag_u_inv (5)", "diag_v_inv (6)", "diag_p_inv (7)"), diags, sysm.dinv):
        guarded = np.abs(d) <= SAFE_INVERSE_GUARD
        assert np.all(inv[guarded] == 0.0), f"{name}: guarded row {np.nonzero(guarded & (inv != 0))[0][:1]} not 0"
        prod = inv * d
        _assert_rows(prod - 1.0, np.abs(prod) + 1.0, ~guarded, f"{name} * diagonal == 1")
    return n


def check_assembled(sysm):
    """Every assembled-system check.  Returns what each ran on, so that a
    caller can see that none was vacuous: `interior` rows (momentum, closure,
    pressure row sums), `rows` (symmetry, signs, dominance, scalar = rho A_pp,
    diagonal inverses: every row) and `faces` (face weights: every internal face)."""
    n = check_momentum(sysm)
    assert check_closure(sysm) == n
    faces = check_face_weights(sysm)
    assert check_pressure(sysm) == n
    rows = check_diagonal_inverses(sysm)
    return {"interior": n, "rows": rows, "faces": faces}


# ------------------------------------------------------------------------ solve
# What a solve reports, by the exit it took (oracle.cpp solve(); the reference's
# coupled_solver_fgmres.rs in brackets):
#  - "computed": an f32 evaluation of |b - A x| -- cap reached, the fixed
#    schedule, the early exit, the stagnation exit [:2406-2413], convergence seen
#    at a restart [:2364];
#  - "estimate": the Givens estimate of the iteration that broke the inner loop
#    [:2278], which is below the target rtol |b| (or, under convergence_lag 1,
#    follows one that was).
# From outside: a `converged` natural-schedule solve whose report is below the
# target max(rtol |b|, atol) may be an estimate; everything else is computed
# (a report above the target under lag 1 is the stale read, an estimate far
# above what f32 resolves, and meets the computed bound all the same).
def true_residual(sysm, x=None):
    """|b - A x| in float64 over the stored system."""
    x = sysm.x if x is None else x
    return float(np.linalg.norm(sysm.rhs - sysm.matrix() @ x))


def residual_resolution(sysm):
    """|eps32 (|b| + |A||x|)|_2: one rounding of every term of the rows
    r_i = b_i - sum_j A_ij x_j, the unit in which the Givens estimate's
    undershoot of the true residual is measured."""
    return float(np.linalg.norm(EPS32 * (abs(sysm.matrix()) @ np.abs(sysm.x) + np.abs(sysm.rhs))))


def target_residual(sysm, cfg):
    """max(rtol |b|, atol): the reference's target [:1855]."""
    return max(float(cfg.fgmres_rtol) * float(np.linalg.norm(sysm.rhs)), float(cfg.fgmres_atol))


def reports_estimate(sysm, stats, cfg):
    """True where the reported residual may be the Givens estimate (see above)."""
    return bool(stats.converged) and int(cfg.fixed_inner) == 0 and int(stats.iterations) > 0 \
        and float(stats.residual) < target_residual(sysm, cfg)


def check_residual(sysm, reported, tol, floor_eps=0.0, what=""):
    """Two-sided: | |b - A x|_f64 - reported | <= tol * reported
    (+ floor_eps * residual_resolution where the report is an estimate:
    pass floor_eps only then).  Returns the true residual."""
    reported = float(reported)
    assert np.isfinite(reported) and reported > 0.0, f"{what}: reported residual {reported}"
    r = true_residual(sysm)
    assert np.isfinite(r), f"{what}: non-finite true residual"
    floor = floor_eps * residual_resolution(sysm) if floor_eps else 0.0
    assert abs(r - reported) <= tol * reported + floor, (
        f"{what}: true residual {r:.9e} vs reported {reported:.9e}: deviation {abs(r - reported):.3e} > "
        f"{tol:.3e} * reported + {floor:.3e} (relative {abs(r - reported) / reported:.3e})")
    return r


def check_solve(sysm, stats, cfg, tol, floor_eps, what=""):
    """check_residual with the bound of the exit the solve took."""
    est = reports_estimate(sysm, stats, cfg)
    return check_residual(sysm, stats.residual, tol, floor_eps if est else 0.0, what + (" [estimate]" if est else " [computed]"))


def iteration_cap(cfg):
    """Iterations of a natural-schedule solve that neither converges nor
    diverges: max_outer_restarts restarts of max_restart iterations
    (oracle.cpp solve(): `for outer < max_outer` x `for j < m`, m = max_restart)."""
    return int(cfg.max_restart) * int(cfg.max_outer_restarts)


def check_convergence_contract(sysm, stats, cfg, tol, floor_eps, what=""):
    """What `converged` means in the reference's loop (and so in the oracle
    and the HIP path), on the true residual r = |b - A x|_f64.  The target is
    relative to |b|, not to |b - A x0| ([:1855] `(tol * rhs_norm).max(abstol)`,
    [:2278], [:2364]; oracle.cpp solve()).

    - converged, report below the target: r <= target (1 + tol) +
      floor_eps * residual_resolution;
    - converged, report at or above the target, convergence_lag 0: only the
      stagnation exit does that (three restarts that each improve by less than
      1e-3, [:2406-2413]): iterations is a multiple of max_restart, at least
      3 of them;
    - converged, report at or above the target, convergence_lag 1: the stale
      read -- the check of a cycle's first iteration reads the last estimate
      of the previous cycle or of the PREVIOUS solve (the async reader is
      never reset) -- or stagnation: no bound on r;
    - neither converged nor diverged: iterations == iteration_cap(cfg).

    Returns which of these was asserted: "target", "stagnation", "stale", "cap", "diverged"."""
    r = true_residual(sysm)
    it, m = int(stats.iterations), int(cfg.max_restart)
    if stats.converged:
        target = target_residual(sysm, cfg)
        if float(stats.residual) < target:
            bound = target * (1.0 + tol) + floor_eps * residual_resolution(sysm)
            assert r <= bound, (f"{what}: converged after {it} iterations but |b - A x| = {r:.6e} > "
                                f"target (1 + tol) + floor = {bound:.6e} (target {target:.6e})")
            return "target"
        if int(cfg.convergence_lag) == 0:
            assert it >= 3 * m and it % m == 0, (
                f"{what}: converged with report {stats.residual:.6e} >= target {target:.6e} after {it} iterations: "
                f"not a stagnation exit of max_restart {m}")
            return "stagnation"
        return "stale"
    if stats.diverged:
        return "diverged"
    assert it == iteration_cap(cfg), f"{what}: not converged, not diverged, {it} iterations != cap {iteration_cap(cfg)}"
    return "cap"


def check_monotone(residuals, tol, what=""):
    """True residuals r(1..K) of fixed_inner = 1..K from one state: non-increasing
    up to (1 + tol) (FGMRES minimises over nested spaces), and r(K) < 0.5 r(1)."""
    r = np.asarray(residuals, dtype=np.float64)
    for k in range(1, len(r)):
        assert r[k] <= r[k - 1] * (1.0 + tol), (
            f"{what}: residual grows from k={k} ({r[k - 1]:.9e}) to k={k + 1} ({r[k]:.9e})")
    assert r[-1] < 0.5 * r[0], f"{what}: r({len(r)}) = {r[-1]:.6e} not below half of r(1) = {r[0]:.6e}"
