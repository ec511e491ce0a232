"""Float64 checks of the aggregation-AMG hierarchy and its V-cycle, written
from the definitions (linear_solver/amg.rs:84-235, 246-595, 666-770 and
amg.wgsl as mathematics), not from oracle/oracle.cpp or the HIP kernels.

HELPER MODULE, not a test.  numpy and scipy.sparse only.  The input is the
read-back of a built hierarchy (`debug_amg_level` of GpuSolver and of
OracleSolver): every level as plain CSR in f32 with its raw diagonal `dv`, its
smoother diagonal `de` and, where it has a coarse level, the aggregate of every
row (`agg`), R's rows (`r_row`, `r_col`) and the four-member image of R (`m4`,
`m4_more`).

Every check raises AssertionError whose message starts with the check's name
and names the level and the worst row or entry; it returns how many rows,
entries or levels it ran on, so that a caller can assert it was not vacuous.

Bounds.  DERIVED, no measurement behind them:
- Galerkin: a coarse entry is a k-term f32 sum of exact products (P's values
  are 1), so |stored - exact| <= k eps32 sum|terms|;
- the row identities (symmetry, dominance, row sums) carry TOL_ROW = 16 eps32
  of tests/fv_checks.py on level 0 and, level by level, the sum of the members'
  bounds plus the Galerkin bound of the coarse row;
- off-diagonals <= 0 exactly: a float sum of non-positive terms is non-positive.
MEASURED against the CPU oracle: K of the V-cycle agreement (tests/amg_cases.py).
"""
import numpy as np
import scipy.sparse as sp

EPS32 = float(np.finfo(np.float32).eps)
TOL_ROW = 16.0 * EPS32  # tests/fv_checks.py
DIAG_GUARD = 1e-14      # amg.wgsl:46: |diagonal| below it smooths with 1.0
OMEGA = 0.8
COARSEST_SWEEPS = 10
MAX_LEVELS = 20
MIN_COARSEN_ROWS = 100  # a level of more rows is coarsened (amg.rs:246-595)


class Level:
    """One read-back level.  Plain attributes (f32 / integer arrays as read
    back), so that a test can mutate a copy."""

    KEYS = ("row", "col", "val", "dv", "de", "agg", "r_row", "r_col", "m4", "m4_more")

    def __init__(self, d):
        self.n, self.nc, self.nnz = int(d["n"]), int(d["nc"]), int(d["nnz"])
        self.wide, self.use16 = bool(d.get("wide", False)), bool(d.get("use16", False))
        for k in self.KEYS:
            v = d[k]
            setattr(self, k, None if v is None else np.array(v))

    def copy(self):
        import copy
        c = copy.copy(self)
        for k in self.KEYS:
            v = getattr(self, k)
            setattr(c, k, None if v is None else v.copy())
        return c

    @property
    def has_op(self):
        return self.nc > 0

    def rows_of_entries(self):
        return np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.row.astype(np.int64)))

    def matrix(self):
        """The level in f64, explicit zeros kept."""
        return sp.csr_matrix((self.val.astype(np.float64), self.col.astype(np.int64), self.row.astype(np.int64)),
                             shape=(self.n, self.n))

    def off_diagonal(self):
        """The level without its diagonal entries (f64 CSR)."""
        r, c = self.rows_of_entries(), self.col.astype(np.int64)
        m = r != c
        return sp.csr_matrix((self.val.astype(np.float64)[m], (r[m], c[m])), shape=(self.n, self.n))

    def prolongation(self):
        """P: n x nc, one 1 per row."""
        return sp.csr_matrix((np.ones(self.n), (np.arange(self.n), self.agg.astype(np.int64))), shape=(self.n, self.nc))


def read_hierarchy(solver):
    """Every level of the solver's built hierarchy."""
    return [Level(solver.debug_amg_level(li)) for li in range(len(solver.amg_levels()))]


def _fail(check, level, msg):
    raise AssertionError(f"{check}: level {level}: {msg}")


# --------------------------------------------------------------------- source
def check_source(levels, scalar_pattern=None, scalar_values=None):
    """Level 0 is, bit for bit, the scalar matrix the hierarchy was built from
    (pattern: (row pointers, columns); values: debug buffer 8 in f32); on every
    level the columns ascend, dv is the CSR's diagonal entry and de == dv
    except 1.0 where |dv| < 1e-14.  Returns the rows checked."""
    rows = 0
    for li, L in enumerate(levels):
        row, col = L.row.astype(np.int64), L.col.astype(np.int64)
        if len(row) != L.n + 1 or row[0] != 0 or row[-1] != L.nnz or len(col) != L.nnz or len(L.val) != L.nnz:
            _fail("source", li, f"CSR sizes: {len(row)} row pointers, {len(col)} columns for n {L.n}, nnz {L.nnz}")
        if np.any(np.diff(row) < 0):
            _fail("source", li, "row pointers decrease")
        r = L.rows_of_entries()
        if L.nnz and (col.min() < 0 or col.max() >= L.n):
            _fail("source", li, f"column {col.max()} outside [0, {L.n})")
        same = r[1:] == r[:-1]
        bad = np.nonzero(same & (np.diff(col) <= 0))[0]
        if len(bad):
            _fail("source", li, f"row {r[bad[0]]}: columns do not ascend at entry {bad[0] + 1}")
        if li == 0 and scalar_pattern is not None:
            srow, scol = (np.asarray(a, dtype=np.int64) for a in scalar_pattern)
            if not (np.array_equal(srow, row) and np.array_equal(scol, col)):
                _fail("source", 0, "pattern differs from the scalar matrix")
        if li == 0 and scalar_values is not None:
            sv = np.asarray(scalar_values, dtype=np.float32)
            diff = np.nonzero(sv.view(np.uint32) != L.val.astype(np.float32).view(np.uint32))[0] \
                if len(sv) == L.nnz else np.array([0])
            if len(diff):
                k = int(diff[0])
                _fail("source", 0, f"row {r[k]} entry {k}: {L.val[k]!r} is not the scalar matrix's {sv[k] if len(sv) == L.nnz else 'length'}")
        isd = r == col
        cnt = np.bincount(r[isd], minlength=L.n)
        if np.any(cnt != 1):
            _fail("source", li, f"row {int(np.argmax(cnt != 1))}: {cnt[np.argmax(cnt != 1)]} diagonal entries")
        diag = np.zeros(L.n, dtype=np.float32)
        diag[r[isd]] = L.val[isd]
        bad = np.nonzero(diag.view(np.uint32) != L.dv.astype(np.float32).view(np.uint32))[0]
        if len(bad):
            _fail("source", li, f"row {bad[0]}: dv {L.dv[bad[0]]!r} is not the diagonal entry {diag[bad[0]]!r}")
        want = np.where(np.abs(L.dv.astype(np.float64)) < DIAG_GUARD, np.float32(1.0), L.dv.astype(np.float32))
        bad = np.nonzero(want.view(np.uint32) != L.de.astype(np.float32).view(np.uint32))[0]
        if len(bad):
            _fail("source", li, f"row {bad[0]}: de {L.de[bad[0]]!r}, expected {want[bad[0]]!r} (dv {L.dv[bad[0]]!r})")
        rows += L.n
    return rows


# ------------------------------------------------------------------ partition
def check_partition(levels):
    """agg is a partition of the rows into nc < n non-empty aggregates; R is its
    transpose with members ascending; the four-member image lists the same
    first members and flags exactly the larger aggregates; the lowest row of
    an aggregate is its seed -- every other member is a graph neighbour of it
    in A_l (greedy aggregation in index order, no strength test,
    amg.rs:84-116) -- and aggregate ids increase with their seeds.  Returns
    the rows checked."""
    rows = 0
    for li, L in enumerate(levels):
        if not L.has_op:
            continue
        n, nc = L.n, L.nc
        agg = L.agg.astype(np.int64)
        if len(agg) != n:
            _fail("partition", li, f"{len(agg)} aggregate ids for {n} rows")
        if agg.min() < 0 or agg.max() >= nc:
            w = int(np.argmax((agg < 0) | (agg >= nc)))
            _fail("partition", li, f"row {w}: aggregate {agg[w]} outside [0, {nc})")
        cnt = np.bincount(agg, minlength=nc)
        if np.any(cnt == 0):
            _fail("partition", li, f"aggregate {int(np.argmax(cnt == 0))} has no member (an orphan id)")
        if not nc < n:
            _fail("partition", li, f"nc {nc} is not below n {n}")
        if li + 1 >= len(levels) or levels[li + 1].n != nc:
            _fail("partition", li, f"nc {nc} is not the next level's row count")
        r_row, r_col = L.r_row.astype(np.int64), L.r_col.astype(np.int64)
        want_row = np.concatenate([[0], np.cumsum(cnt)])
        want_col = np.argsort(agg, kind="stable")  # members of aggregate 0 ascending, then of 1, ...
        if not np.array_equal(r_row, want_row):
            w = int(np.argmax(r_row != want_row)) if len(r_row) == len(want_row) else 0
            _fail("partition", li, f"R row pointer {w}: {r_row[w] if w < len(r_row) else None}, the transpose of agg has {want_row[w]}")
        if not np.array_equal(r_col, want_col):
            w = int(np.argmax(r_col != want_col)) if len(r_col) == len(want_col) else 0
            I = int(np.searchsorted(want_row, w, side="right") - 1)
            _fail("partition", li, f"aggregate {I}: R member {r_col[w] if w < len(r_col) else None} at entry {w}, "
                                   f"the transpose of agg (members ascending) has {want_col[w]}")
        m4 = L.m4.astype(np.int64).reshape(nc, 4)
        q = np.arange(4)[None, :]
        idx = np.minimum(want_row[:-1, None] + q, len(want_col) - 1)
        want4 = np.where(q < cnt[:, None], want_col[idx], -1)
        if not np.array_equal(m4, want4):
            w = int(np.argmax(np.any(m4 != want4, axis=1)))
            _fail("partition", li, f"aggregate {w}: four-member image {m4[w].tolist()}, R has {want4[w].tolist()}")
        more = L.m4_more.astype(np.int64) != 0
        if not np.array_equal(more, cnt > 4):
            w = int(np.argmax(more != (cnt > 4)))
            _fail("partition", li, f"aggregate {w}: {cnt[w]} members, more-than-four flag {bool(more[w])}")
        seed = want_col[want_row[:-1]]  # lowest member of each aggregate
        if np.any(np.diff(seed) <= 0):
            w = int(np.argmax(np.diff(seed) <= 0))
            _fail("partition", li, f"aggregate {w + 1}: seed {seed[w + 1]} is not above aggregate {w}'s seed {seed[w]}")
        pat = sp.csr_matrix((np.ones(L.nnz), L.col.astype(np.int64), L.row.astype(np.int64)), shape=(n, n))
        member = np.nonzero(seed[agg] != np.arange(n))[0]
        if len(member):
            linked = np.asarray(pat[seed[agg[member]], member]).ravel() != 0
            if not np.all(linked):
                w = int(member[np.argmax(~linked)])
                _fail("partition", li, f"row {w}: in aggregate {agg[w]} but no neighbour of its seed {seed[agg[w]]}")
        rows += n
    return rows


# ------------------------------------------------------------------- Galerkin
def galerkin_terms(fine):
    """Of A_c = P^T A_l P in f64 from the stored f32 level: the sums G, the
    number of terms K and the sum of the terms' magnitudes S of every coarse
    entry, as CSR matrices of one pattern (every (I, J) with a contributing
    entry, explicit zeros counted)."""
    agg = fine.agg.astype(np.int64)
    I, J = agg[fine.rows_of_entries()], agg[fine.col.astype(np.int64)]
    v = fine.val.astype(np.float64)
    shape = (fine.nc, fine.nc)
    K = sp.coo_matrix((np.ones(len(v)), (I, J)), shape=shape).tocsr()
    G = sp.coo_matrix((v, (I, J)), shape=shape).tocsr()
    S = sp.coo_matrix((np.abs(v), (I, J)), shape=shape).tocsr()
    for M in (K, G, S):
        M.sort_indices()
    assert np.array_equal(K.indptr, G.indptr) and np.array_equal(K.indices, G.indices)
    assert np.array_equal(K.indptr, S.indptr) and np.array_equal(K.indices, S.indices)
    return G, K, S


def check_galerkin(levels):
    """Every level with a coarse level against the stored level above it (so
    nothing accumulates down the hierarchy): the coarse pattern is exactly the
    set of (I, J) with a contributing fine entry, and
    |A_c[I,J] - sum| <= k eps32 sum|terms| (the rounding bound of a k-term f32
    sum of exact products).  Returns the coarse entries checked."""
    entries = 0
    for li, F in enumerate(levels[:-1]):
        if not F.has_op:
            _fail("galerkin", li, "no operators but a level below")
        C = levels[li + 1]
        G, K, S = galerkin_terms(F)
        crow, ccol = C.row.astype(np.int64), C.col.astype(np.int64)
        if C.n != F.nc or not np.array_equal(crow, K.indptr) or not np.array_equal(ccol, K.indices):
            have = sp.csr_matrix((np.ones(len(ccol)), ccol, crow), shape=(C.n, C.n)) if C.n == F.nc else None
            where = ""
            if have is not None:
                d = (have - (K > 0).astype(np.float64)).tocoo()
                nz = np.nonzero(d.data)[0]
                if len(nz):
                    k = int(nz[0])
                    where = (f": entry ({d.row[k]}, {d.col[k]}) "
                             f"{'stored without a contributing fine entry' if d.data[k] > 0 else 'missing'}")
            _fail("galerkin", li + 1, f"pattern is not that of P^T A P{where}")
        err = np.abs(C.val.astype(np.float64) - G.data)
        tol = K.data * EPS32 * S.data
        over = err - tol
        if len(over) and over.max() > 0.0:
            k = int(np.argmax(over))
            I = int(np.searchsorted(crow, k, side="right") - 1)
            _fail("galerkin", li + 1, f"entry ({I}, {ccol[k]}): stored {C.val[k]!r}, sum of {int(K.data[k])} fine entries "
                                      f"{G.data[k]:.9e}: |error| {err[k]:.3e} > k eps32 sum|a| = {tol[k]:.3e}")
        entries += len(err)
    return entries


# ------------------------------------------------- consequences a level keeps
def _rowsum(M):
    return np.asarray(M.sum(axis=1)).ravel()


def check_consequences(levels):
    """Symmetry, no positive off-diagonal, diagonal >= sum of off-diagonal
    magnitudes on every level; row sum of coarse row I = the sum of its
    members' row sums.  Level 0 takes the TOL_ROW bounds of fv_checks; a coarse
    level the sum of its members' bounds plus the Galerkin rounding bound of
    its own entries (k-scaled).  Returns the rows checked."""
    rows = 0
    sym_tol = dom_tol = None
    for li, L in enumerate(levels):
        A = L.matrix()
        off = L.off_diagonal()
        diag = L.dv.astype(np.float64)
        if li == 0:
            sym_tol = (TOL_ROW * (abs(A) + abs(A.T))).tocsr()
            dom_tol = TOL_ROW * (np.abs(diag) + _rowsum(abs(off)))
        else:
            F = levels[li - 1]
            _, K, S = galerkin_terms(F)
            KS = K.multiply(S).tocsr() * EPS32
            P = F.prolongation()
            sym_tol = (P.T @ sym_tol @ P + KS + KS.T).tocsr()
            dom_tol = P.T @ dom_tol + _rowsum(KS)
            fine_sum, coarse_sum = P.T @ _rowsum(F.matrix()), _rowsum(A)
            over = np.abs(coarse_sum - fine_sum) - _rowsum(KS)
            if over.max() > 0.0:
                w = int(np.argmax(over))
                _fail("consequences", li, f"row {w}: row sum {coarse_sum[w]:.9e}, its members' row sums add to "
                                          f"{fine_sum[w]:.9e} (bound {_rowsum(KS)[w]:.3e})")
        asym = abs(A - A.T).tocsr()
        bad = (asym - sym_tol).tocoo()
        if bad.nnz and bad.data.max() > 0.0:
            k = int(np.argmax(bad.data))
            i, j = int(bad.row[k]), int(bad.col[k])
            _fail("consequences", li, f"not symmetric: entry ({i}, {j}) = {A[i, j]:.9e} vs ({j}, {i}) = {A[j, i]:.9e} "
                                      f"(bound {sym_tol[i, j]:.3e})")
        if off.nnz and off.data.max() > 0.0:
            c = off.tocoo()
            k = int(np.argmax(c.data))
            _fail("consequences", li, f"positive off-diagonal {c.data[k]:.3e} at ({c.row[k]}, {c.col[k]})")
        slack = diag - _rowsum(abs(off))
        over = -slack - dom_tol
        if over.max() > 0.0:
            w = int(np.argmax(over))
            _fail("consequences", li, f"row {w}: diagonal {diag[w]:.9e} below the off-diagonal magnitudes "
                                      f"{diag[w] - slack[w]:.9e} (bound {dom_tol[w]:.3e})")
        rows += L.n
    return rows


# ------------------------------------------------------------------ stop rule
def check_stop_rule(levels, reported):
    """A level is coarsened iff it has more than 100 rows, is not the 20th and
    aggregation shrank it (a structurally symmetric level with any
    off-diagonal entry shrinks under greedy aggregation); the last level has
    no operators; `reported` (amg_levels(): rows, nnz per level) equals the
    read-back.  Returns the levels checked."""
    if not 1 <= len(levels) <= MAX_LEVELS:
        _fail("stop rule", len(levels) - 1, f"{len(levels)} levels")
    if [(L.n, L.nnz) for L in levels] != [tuple(r) for r in reported]:
        _fail("stop rule", 0, f"amg_levels() reports {list(reported)}, read back {[(L.n, L.nnz) for L in levels]}")
    for li, L in enumerate(levels):
        last = li == len(levels) - 1
        if L.has_op == last:
            _fail("stop rule", li, "the last level has operators" if last else "no operators but a level below")
        may = L.n > MIN_COARSEN_ROWS and li < MAX_LEVELS - 1
        if L.has_op and not may:
            _fail("stop rule", li, f"coarsened with {L.n} rows")
        if may and not L.has_op and L.off_diagonal().nnz:
            _fail("stop rule", li, f"{L.n} rows and off-diagonal entries, yet not coarsened")
    return len(levels)


def check_hierarchy(levels, reported, scalar_pattern=None, scalar_values=None):
    """Every hierarchy check, in the order source, partition, Galerkin,
    consequences, stop rule.  Returns what each ran on."""
    return {
        "source": check_source(levels, scalar_pattern, scalar_values),
        "partition": check_partition(levels),
        "galerkin": check_galerkin(levels),
        "consequences": check_consequences(levels),
        "stop": check_stop_rule(levels, reported),
    }


# -------------------------------------------------------------------- V-cycle
def vcycle64(levels, x0, b, omega=OMEGA, post_sweep=True, coarsest_sweeps=COARSEST_SWEEPS, drop_aggregate=None,
             majorant=False):
    """The V-cycle in f64 over the read-back levels: out-of-place Jacobi
    x <- x + omega (D_e^-1 (b - A x)) with the diagonal term excluded through
    de (x_new = (b - sum_{j != i} a_ij x_j) / de_i, x <- x + omega (x_new - x)),
    one pre-sweep, b_c = P^T (b - A x), x_c = 0, ten sweeps on the last level,
    x += P x_c, one post-sweep.

    majorant: the same recursion with every matrix, x0 and b replaced by their
    magnitudes and every subtraction by an addition -- per row, what the
    quantities of the cycle can add up to.  omega / post_sweep /
    coarsest_sweeps / drop_aggregate = (level, aggregate): the deliberate
    errors the agreement check must see."""
    sgn = 1.0 if majorant else -1.0
    mats = []
    for L in levels:
        A, off = L.matrix(), L.off_diagonal()
        de = L.de.astype(np.float64)
        if majorant:
            A, off, de = abs(A), abs(off), np.abs(de)
        mats.append((A, off, de))

    def sweep(li, x, rhs):
        _, off, de = mats[li]
        x_new = (rhs + sgn * (off @ x)) / de
        return x + omega * (x_new + sgn * x)

    def cycle(li, x, rhs):
        L = levels[li]
        if not L.has_op:
            for _ in range(coarsest_sweeps):
                x = sweep(li, x, rhs)
            return x
        x = sweep(li, x, rhs)
        P = L.prolongation()
        r = rhs + sgn * (mats[li][0] @ x)
        xc = cycle(li + 1, np.zeros(L.nc), P.T @ r)
        if drop_aggregate is not None and drop_aggregate[0] == li:
            xc = xc.copy()
            xc[drop_aggregate[1]] = 0.0
        x = x + P @ xc
        return sweep(li, x, rhs) if post_sweep else x

    x0 = np.asarray(x0, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if majorant:
        x0, b = np.abs(x0), np.abs(b)
    return cycle(0, x0, b)


def vcycle_deviation(levels, x0, b, x_out):
    """max over the rows of |x_out - x_f64| / (eps32 M), M the majorant cycle,
    and the row it is at."""
    x64 = vcycle64(levels, x0, b)
    M = vcycle64(levels, x0, b, majorant=True)
    err = np.abs(np.asarray(x_out, dtype=np.float64) - x64)
    ratio = np.where(M > 0.0, err / np.where(M > 0.0, EPS32 * M, 1.0), np.where(err > 0.0, np.inf, 0.0))
    w = int(np.argmax(ratio))
    return float(ratio[w]), w


def check_vcycle_agreement(levels, x0, b, x_out, K, what=""):
    """|x_out - x_f64| <= K eps32 M per row.  Returns the rows checked."""
    assert np.all(np.isfinite(x_out)), f"agreement: {what}: the cycle's output is not finite"
    ratio, w = vcycle_deviation(levels, x0, b, x_out)
    assert ratio <= K, (f"agreement: {what}: level 0 row {w}: |x_out - x_f64| = {ratio:.3f} eps32 M, "
                        f"bound {K:.3f} eps32 M")
    return len(x_out)


def check_linearity(vcycle, x0, b, what=""):
    """`vcycle(x0, b)` is the solver's cycle in f32: V(0, 0) = 0, a repeated
    call gives the same bits (no stale scratch between calls), and
    V(a x0, a b) = a V(x0, b) exactly for a a power of two.  Returns the calls
    compared."""
    x0 = np.asarray(x0, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    ref = vcycle(x0, b)
    zero = vcycle(np.zeros_like(x0), np.zeros_like(b))
    assert not np.any(zero), f"linearity: {what}: V(0, 0) != 0 at row {int(np.argmax(zero != 0))}"
    again = vcycle(x0, b)
    assert np.array_equal(ref, again), (f"linearity: {what}: V(x0, b) after V(0, 0) differs at row "
                                        f"{int(np.argmax(ref != again))}")
    n = 2
    for a in (4.0, 0.125):
        out = vcycle((a * x0).astype(np.float32), (a * b).astype(np.float32))
        want = (np.float32(a) * ref).astype(np.float32)
        assert np.array_equal(out, want), (f"linearity: {what}: V({a} x0, {a} b) != {a} V(x0, b) at row "
                                           f"{int(np.argmax(out != want))}")
        n += 1
    return n


def energy_matrix(levels):
    """The symmetric part of level 0 in f64."""
    A = levels[0].matrix()
    return ((A + A.T) * 0.5).tocsr()


def a_norm(A, e):
    return float(np.sqrt(max(float(e @ (A @ e)), 0.0)))


def check_non_expansion(levels, x_star, x0, b, x_out=None, what=""):
    """Error in the energy norm of the symmetric part of level 0, x* the
    solution of b (b = A x* rounded to f32 as the solver gets it, or x* the
    sparse direct solve of a given b): the f64 cycle from x0 must reduce it,
    ||x* - V(x0, b)||_A < ||x* - x0||_A; a solver's x_out must reach
    rho_dev <= rho_64 + (1 - rho_64) / 2.  Returns (rho_64, rho_dev or None);
    (0, 0) on a one-row level whose start left nothing to contract (see below)."""
    A = energy_matrix(levels)
    x_star = np.asarray(x_star, dtype=np.float64)
    e0 = a_norm(A, x_star - np.asarray(x0, dtype=np.float64))
    floor = TOL_ROW * a_norm(A, x_star)
    if levels[0].n == 1 and e0 <= floor:
        # One-row level only (strip1 from x0 = D^-1 b): Jacobi's start is the
        # solution itself, and b and x0 are each rounded once, so the start
        # already is x* to what f32 resolves.  There is no error left to
        # contract; the cycles only have to stay within that resolution.  Any
        # other case keeps the strict assertion below.
        outs = [vcycle64(levels, x0, b)] + ([np.asarray(x_out, dtype=np.float64)] if x_out is not None else [])
        for o in outs:
            assert a_norm(A, x_star - o) <= floor, (f"non-expansion: {what}: from a start within f32 resolution "
                                                    f"of x* the error grew to {a_norm(A, x_star - o):.3e} > {floor:.3e}")
        return 0.0, (0.0 if x_out is not None else None)
    rho64 = a_norm(A, x_star - vcycle64(levels, x0, b)) / e0
    assert rho64 < 1.0, f"non-expansion: {what}: the f64 cycle's factor {rho64:.6f} is not below 1"
    rho_dev = None
    if x_out is not None:
        rho_dev = a_norm(A, x_star - np.asarray(x_out, dtype=np.float64)) / e0
        bound = rho64 + (1.0 - rho64) / 2.0
        assert rho_dev <= bound, (f"non-expansion: {what}: factor {rho_dev:.6f} above {bound:.6f} "
                                  f"(f64 cycle: {rho64:.6f})")
    return rho64, rho_dev


# -------------------------------------------------- preconditioner identity
def check_precond_identity(sysm, v, z, what=""):
    """z = M^-1 v of the Schur preconditioner (one application,
    debug_apply_precond), per row in f64 from the diagonal inverses (debug
    buffers 5, 6) and the coupled matrix (9) of `sysm` (an fv_checks.System):
    z_u = D_u^-1 (v_u - sum_j A_up[i,j] z_p[j]), the same for v.  Independent
    of how the pressure block was solved (Jacobi relaxation or the V-cycle).
    Bound: TOL_ROW times the magnitudes of the row's terms.  Returns the rows
    checked (two per cell)."""
    v = np.asarray(v, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    assert np.all(np.isfinite(z)), f"precond identity: {what}: z is not finite"
    zp = z[2::3]
    rows = 0
    for k, comp in enumerate("uv"):
        Axp = sysm.block(comp, "p")
        dinv = np.asarray(sysm.dinv[k], dtype=np.float64)
        zx, vx = z[k::3], v[k::3]
        want = dinv * (vx - Axp @ zp)
        scale = np.abs(zx) + np.abs(dinv) * (np.abs(vx) + abs(Axp) @ np.abs(zp))
        over = np.abs(zx - want) - TOL_ROW * scale
        w = int(np.argmax(over))
        assert over[w] <= 0.0, (f"precond identity: {what}: cell {w}: z_{comp} = {zx[w]:.9e}, "
                                f"D_{comp}^-1 (v_{comp} - A_{comp}p z_p) = {want[w]:.9e}: |error| "
                                f"{abs(zx[w] - want[w]):.3e} > 16 eps32 * {scale[w]:.3e}")
        rows += len(zx)
    return rows
