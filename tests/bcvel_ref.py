"""Prescribed boundary velocities restated in numpy float32 -- TEST INFRASTRUCTURE ONLY.

Written from the prose of include/cfd2_amd.h ("Arithmetic of boundary
velocities"), not from the kernels, on top of tests/refpy.py (whose prepare and
assemble are restated here with a velocity per boundary face where they have
one constant) and tests/buoyancy_ref.py (so a buoyant step with moving walls
is covered).  For a selected face with the uploaded (bx, by), every operation
one float32 rounding:

    g = scale * ramp;  ubx = bx * g;  uby = by * g

    prepare, inlet   flux = density * (ubx * nfx + uby * nfy) * area;  vfu, vfv = ubx, uby
    prepare, wall    flux and diagonal unchanged;  vfu, vfv = ubx, uby
    assemble, inlet  the plain branch with ubx, and uby for the literal 0
    assemble, wall   the plain branch, then rhs_u += diff * ubx;  rhs_v += diff * uby

An unselected inlet face keeps (inlet_velocity * ramp, 0), an unselected wall
face adds nothing.  The host's part is restated too: a wall entry loses (v . n)
n / (n . n) in float64 before it is rounded.  BcvRefSolver.step() replaces
refpy.prepare and refpy.assemble for its own duration.

The pieces a deliberately wrong variant replaces (tests/test_bcvel.py) are
methods of BoundaryVelocities: wall_sign, inlet_uby, gain, project.
"""
from __future__ import annotations

import numpy as np

from tests import refpy
from tests.buoyancy_ref import BuoyantRefSolver
from tests.refpy import F, _dist, _smoothstep

INLET, WALL = 1, 3


class BoundaryVelocities:
    """The selection: per face the uploaded float32 (bx, by), and the two scales."""

    def __init__(self, arrays):
        a = arrays
        self.F = len(a["face_area"])
        self.boundary = np.asarray(a["face_neighbor"]) == refpy.NONE
        self.bt = np.where(self.boundary, np.asarray(a["face_boundary"]).astype(np.int64) & 3, 0)
        self.n64 = np.stack([np.asarray(a["face_nx"], np.float64), np.asarray(a["face_ny"], np.float64)], 1)
        self.inlet_scale, self.wall_scale = F(1), F(1)
        self.clear()

    def clear(self):
        self.sel = np.zeros(self.F, bool)
        self.bx, self.by = np.zeros(self.F, F), np.zeros(self.F, F)
        self.max_normal_removed = 0.0

    # ---- the four pieces a wrong variant replaces -----------------------------
    def wall_sign(self):
        return F(1)

    def inlet_uby(self, uby):
        return uby

    def gain(self, scale, ramp):
        return F(scale) * ramp

    def project(self, v, n):
        """v [m, 2] without its component along n [m, 2], float64; and |v . n| / |n|"""
        nn = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]
        vn = (v[:, 0] * n[:, 0] + v[:, 1] * n[:, 1]) / nn
        return v - vn[:, None] * n, np.abs(vn) * np.sqrt(nn)

    # ---------------------------------------------------------------------------
    def set(self, faces, v):
        """cfd_set_boundary_velocity: returns the faces selected afterwards; ValueError
        (nothing changed) for a face that is no inlet or wall boundary face"""
        faces = np.asarray(faces, np.int64).reshape(-1)
        v = np.asarray(v, np.float64).reshape(-1, 2).astype(F).astype(np.float64)  # the interface takes float32
        if len(faces) == 0:
            self.clear()
            return 0
        if np.any(faces < 0) or np.any(faces >= self.F) or not np.all(np.isin(self.bt[faces], (INLET, WALL))):
            raise ValueError("not an inlet or wall boundary face")
        if not np.all(np.isfinite(v)):
            raise ValueError("velocities must be finite")
        v = v.copy()
        w = self.bt[faces] == WALL
        if np.any(w):
            v[w], removed = self.project(v[w], self.n64[faces[w]])
            self.max_normal_removed = max(self.max_normal_removed, float(np.max(removed)))
        for f, (x, y) in zip(faces, v):  # in order: a later entry replaces an earlier one
            self.sel[f], self.bx[f], self.by[f] = True, F(x), F(y)
        return int(self.sel.sum())

    def info(self):
        return dict(inlet_faces=int((self.sel & (self.bt == INLET)).sum()),
                    wall_faces=int((self.sel & (self.bt == WALL)).sum()), inlet_scale=float(self.inlet_scale),
                    wall_scale=float(self.wall_scale), active=bool(self.sel.any()),
                    max_normal_removed=float(self.max_normal_removed))

    def face_values(self, M, c, ramp):
        """(ubx [F], uby [F], selected wall [F]): the float32 boundary velocity of
        every face as the step uses it (meaningful on inlet faces and selected walls)"""
        ubx = np.full(self.F, c.inlet_velocity * ramp, F)
        uby = np.zeros(self.F, F)
        si, sw = self.sel & (self.bt == INLET), self.sel & (self.bt == WALL)
        gi, gw = self.gain(self.inlet_scale, ramp), self.gain(self.wall_scale, ramp)
        ubx[si], uby[si] = self.bx[si] * gi, self.inlet_uby(self.by[si] * gi)
        ubx[sw], uby[sw] = self.bx[sw] * gw, self.by[sw] * gw
        assert ubx.dtype == F and uby.dtype == F
        return ubx, uby, sw


# ------------------------------------------------------------------- kernels
def prepare(M, st, st_old, c, bv):
    """refpy.prepare with the boundary velocities ``bv`` (a BoundaryVelocities):
    the boundary value of face f is bv.face_values(c, ramp)[..][f] on an inlet
    face (selected or not) and on a selected wall face."""
    N = M.N
    with np.errstate(all="ignore"):
        time_coeff = M.vol * c.density / c.dt
        if c.time_scheme == 1:
            r = c.dt / c.dt_old
            time_coeff = M.vol * c.density / c.dt * (F(1) + F(2) * r) / (F(1) + r)
        diag = F(0) + time_coeff
        gpa = np.zeros((N, 2), F)
        g_u = np.zeros((N, 2), F)
        g_v = np.zeros((N, 2), F)
        fluxes = np.zeros(len(M.area), F)
        ramp = _smoothstep(0.0, c.ramp_time, c.time)
        UBX, UBY, WSEL = bv.face_values(M, c, ramp)
        u, p, dp, gp = st.u, st.p, st.d_p, st.grad_p
        for k in range(M.K):
            cells = np.nonzero(M.slot_face[:, k] >= 0)[0]
            f = M.slot_face[cells, k]
            owner, neigh, btype = M.own[f], M.nb[f], M.bt[f]
            area, fx, fy = M.area[f], M.fx[f], M.fy[f]
            isown = owner == cells
            nx = np.where(isown, M.nx[f], -M.nx[f])
            ny = np.where(isown, M.ny[f], -M.ny[f])
            cox, coy = M.cx[owner], M.cy[owner]
            nfx, nfy = M.nx[f].copy(), M.ny[f].copy()
            flip = (fx - cox) * nfx + (fy - coy) * nfy < F(0)
            nfx = np.where(flip, -nfx, nfx)
            nfy = np.where(flip, -nfy, nfy)
            internal = neigh >= 0
            n = np.where(internal, neigh, 0)
            # Rhie-Chow flux (:134-180)
            d_own = _dist(cox, coy, fx, fy)
            d_ngh = _dist(M.cx[n], M.cy[n], fx, fy)
            tot = d_own + d_ngh
            lam = np.where(tot > F(1e-6), d_ngh / tot, F(0.5))
            ufx = lam * u[owner, 0] + (F(1) - lam) * u[n, 0]
            ufy = lam * u[owner, 1] + (F(1) - lam) * u[n, 1]
            dpf = lam * dp[owner] + (F(1) - lam) * dp[n]
            gfx = lam * gp[owner, 0] + (F(1) - lam) * gp[n, 0]
            gfy = lam * gp[owner, 1] + (F(1) - lam) * gp[n, 1]
            dx, dy = M.cx[n] - cox, M.cy[n] - coy
            dist = np.maximum(np.abs(dx * nfx + dy * nfy), F(1e-6))
            gpn = gfx * nfx + gfy * nfy
            pgf = (p[n] - p[owner]) / dist
            rc = dpf * area * (gpn - pgf)
            un = ufx * nfx + ufy * nfy
            flux_int = c.density * (un * area + rc)
            ubx, uby, wsel = UBX[f], UBY[f], WSEL[f]
            flux_in = c.density * (ubx * nfx + uby * nfy) * area
            un_o = u[owner, 0] * nfx + u[owner, 1] * nfy
            flux_out = np.maximum(F(0), c.density * un_o * area)
            flux = np.where(internal, flux_int,
                            np.where(btype == 1, flux_in, np.where(btype == 2, flux_out, F(0)))).astype(F)
            fluxes[f[isown]] = flux[isown]
            # d_p diagonal (:202-254)
            fo = np.where(isown, flux, -flux)
            other = np.where(internal, np.where(isown, neigh, owner), 0)
            ocx = np.where(internal, M.cx[other], fx)
            ocy = np.where(internal, M.cy[other], fy)
            cx, cy = M.cx[cells], M.cy[cells]
            dvx, dvy = ocx - cx, ocy - cy
            dist_e = np.sqrt(dvx * dvx + dvy * dvy)
            diff = c.viscosity * area / dist_e
            conv = np.where(fo > F(0), fo, F(0))
            d = diag[cells]
            d_int = d + (diff + conv)
            d_iw = d + diff
            d_iw = np.where(fo > F(0), d_iw + fo, d_iw)
            d_out = np.where(fo > F(0), d + fo, d)
            diag[cells] = np.where(internal, d_int,
                                   np.where((btype == 1) | (btype == 3), d_iw, np.where(btype == 2, d_out, d)))
            # grad p (:256-279)
            d_c = _dist(cx, cy, fx, fy)
            d_o = _dist(ocx, ocy, fx, fy)
            tp = d_c + d_o
            lp = np.where(tp > F(1e-6), d_o / tp, F(0.5))
            pc = p[cells]
            vfp = np.where(internal, lp * pc + (F(1) - lp) * p[other], np.where(btype == 2, F(0), pc))
            gpa[cells, 0] += vfp * nx * area
            gpa[cells, 1] += vfp * ny * area
            # velocity gradients (:281-324)
            uc, vc = u[cells, 0], u[cells, 1]
            uo, vo = u[other, 0], u[other, 1]
            vfu_i = np.where(tp > F(1e-6), lp * uc + (F(1) - lp) * uo, F(0.5) * (uc + uo))
            vfv_i = np.where(tp > F(1e-6), lp * vc + (F(1) - lp) * vo, F(0.5) * (vc + vo))
            wall_u, wall_v = np.where(wsel, ubx, F(0)), np.where(wsel, uby, F(0))
            vfu = np.where(internal, vfu_i, np.where(btype == 1, ubx, np.where(btype == 3, wall_u, uc)))
            vfv = np.where(internal, vfv_i, np.where(btype == 1, uby, np.where(btype == 3, wall_v, vc)))
            g_u[cells, 0] += vfu * nx * area
            g_u[cells, 1] += vfu * ny * area
            g_v[cells, 0] += vfv * nx * area
            g_v[cells, 1] += vfv * ny * area
        st.d_p = np.where(np.abs(diag) > F(1e-20), M.vol / diag, F(0)).astype(F)
        st.grad_p = (gpa / M.vol[:, None]).astype(F)
        return fluxes, (g_u / M.vol[:, None]).astype(F), (g_v / M.vol[:, None]).astype(F)


def assemble(M, st, st_old, st_old_old, fluxes, grad_u, grad_v, c, bv):
    """refpy.assemble with the boundary velocities ``bv``: the inlet branch with
    the face's (ubx, uby), the wall branch followed by rhs += diff * ub on a
    selected wall face, each at the slot's place in the loop."""
    N = M.N
    nnz_s = len(M.scol)
    mv = np.zeros(9 * nnz_s, F)
    sv = np.zeros(nnz_s, F)
    with np.errstate(all="ignore"):
        coeff_time = M.vol * c.density / c.dt
        rtu = coeff_time * st_old.u[:, 0]
        rtv = coeff_time * st_old.u[:, 1]
        if c.time_scheme == 1:  # BDF2 (:114-127)
            r = c.dt / c.dt_old
            coeff_time = M.vol * c.density / c.dt * (F(1) + F(2) * r) / (F(1) + r)
            fn, fnm1 = F(1) + r, (r * r) / (F(1) + r)
            base = M.vol * c.density / c.dt
            rtu = base * (fn * st_old.u[:, 0] - fnm1 * st_old_old.u[:, 0])
            rtv = base * (fn * st_old.u[:, 1] - fnm1 * st_old_old.u[:, 1])
        diag_u = F(0) + coeff_time
        diag_v = F(0) + coeff_time
        rhs_u = F(0) + rtu
        rhs_v = F(0) + rtv
        rhs_p = np.zeros(N, F)
        sup, svp, spu, spv, spp, sdp = (np.zeros(N, F) for _ in range(6))
        nbr = np.diff(M.srow)
        ramp = _smoothstep(0.0, c.ramp_time, c.time)
        UBX, UBY, WSEL = bv.face_values(M, c, ramp)
        for k in range(M.K):
            cells = np.nonzero(M.slot_face[:, k] >= 0)[0]
            f = M.slot_face[cells, k]
            owner, neigh, btype = M.own[f], M.nb[f], M.bt[f]
            area, fx, fy = M.area[f], M.fx[f], M.fy[f]
            isown = owner == cells
            sign = np.where(isown, F(1), F(-1))
            nx = np.where(isown, M.nx[f], -M.nx[f])
            ny = np.where(isown, M.ny[f], -M.ny[f])
            flux = fluxes[f] * sign
            ubx, uby, wsel = UBX[f], UBY[f], WSEL[f]
            internal = neigh >= 0
            other = np.where(internal, np.where(isown, neigh, owner), 0)
            cx, cy = M.cx[cells], M.cy[cells]
            ocx = np.where(internal, M.cx[other], fx)
            ocy = np.where(internal, M.cy[other], fy)
            dpn = np.where(internal, st.d_p[other], st.d_p[cells])
            dvx, dvy = ocx - cx, ocy - cy
            dist = np.maximum(np.abs(dvx * nx + dvy * ny), F(1e-6))
            diff = c.viscosity * area / dist
            cdg = np.where(flux > F(0), flux, F(0))
            cof = np.where(flux > F(0), F(0), flux)
            # matrix slots (:195-214)
            so = M.srow[cells]
            rank = np.where(internal, M.slot_mat[cells, k] - so, 0)
            r0 = 9 * so
            r1 = r0 + 3 * nbr[cells]
            r2 = r0 + 6 * nbr[cells]
            ii = cells[internal]
            ri, r0i, r1i, r2i = rank[internal], r0[internal], r1[internal], r2[internal]
            # --- internal faces (:216-350)
            coeff = (-diff + cof)[internal]
            mv[r0i + 3 * ri + 0] = coeff
            mv[r0i + 3 * ri + 1] = F(0)
            mv[r1i + 3 * ri + 0] = F(0)
            mv[r1i + 3 * ri + 1] = coeff
            du = diag_u[cells]
            dv = diag_v[cells]
            du_i = du + (diff + cdg)
            dv_i = dv + (diff + cdg)
            if c.scheme != 0:  # deferred correction (:229-293)
                uo_x, uo_y = st.u[cells, 0], st.u[cells, 1]
                un_x, un_y = st.u[other, 0], st.u[other, 1]
                neg = flux < F(0)
                pu_u = np.where(neg, un_x, uo_x)
                pu_v = np.where(neg, un_y, uo_y)
                pos = flux > F(0)
                if c.scheme == 1:  # SOU
                    rxo, ryo = fx - cx, fy - cy
                    rxn, ryn = fx - ocx, fy - ocy
                    ho_u = np.where(pos, uo_x + (grad_u[cells, 0] * rxo + grad_u[cells, 1] * ryo),
                                    un_x + (grad_u[other, 0] * rxn + grad_u[other, 1] * ryn))
                    ho_v = np.where(pos, uo_y + (grad_v[cells, 0] * rxo + grad_v[cells, 1] * ryo),
                                    un_y + (grad_v[other, 0] * rxn + grad_v[other, 1] * ryn))
                else:  # QUICK
                    dcx, dcy = ocx - cx, ocy - cy
                    tu_o = grad_u[cells, 0] * dcx + grad_u[cells, 1] * dcy
                    tv_o = grad_v[cells, 0] * dcx + grad_v[cells, 1] * dcy
                    ncx, ncy = cx - ocx, cy - ocy
                    tu_n = grad_u[other, 0] * ncx + grad_u[other, 1] * ncy
                    tv_n = grad_v[other, 0] * ncx + grad_v[other, 1] * ncy
                    ho_u = np.where(pos, F(0.625) * uo_x + F(0.375) * un_x + F(0.125) * tu_o,
                                    F(0.625) * un_x + F(0.375) * uo_x + F(0.125) * tu_n)
                    ho_v = np.where(pos, F(0.625) * uo_y + F(0.375) * un_y + F(0.125) * tv_o,
                                    F(0.625) * un_y + F(0.375) * uo_y + F(0.125) * tv_n)
                rcu = rhs_u[cells] - flux * (ho_u - pu_u)
                rcv = rhs_v[cells] - flux * (ho_v - pu_v)
            else:
                rcu, rcv = rhs_u[cells], rhs_v[cells]
            d_own = _dist(cx, cy, fx, fy)
            d_ngh = _dist(ocx, ocy, fx, fy)
            tot = d_own + d_ngh
            lam = np.where(tot > F(1e-6), d_ngh / tot, F(0.5))
            pgx, pgy = area * nx, area * ny
            dcx_, dcy_ = nx * area, ny * area
            om = F(1) - lam
            mv[r0i + 3 * ri + 2] = (om * pgx)[internal]
            mv[r1i + 3 * ri + 2] = (om * pgy)[internal]
            mv[r2i + 3 * ri + 0] = (om * dcx_)[internal]
            mv[r2i + 3 * ri + 1] = (om * dcy_)[internal]
            dpf = lam * st.d_p[cells] + om * st.d_p[other]
            lap = dpf * area / dist
            mv[r2i + 3 * ri + 2] = (-lap)[internal]
            dpf_s = lam * st.d_p[cells] + om * dpn
            scoef = c.density * dpf_s * area / dist
            sv[M.slot_mat[ii, k]] = (-scoef)[internal]
            # --- boundary faces (:352-419)
            inl, wal, out = (~internal) & (btype == 1), (~internal) & (btype == 3), (~internal) & (btype == 2)
            # inlet
            du_in = du + diff
            dv_in = dv + diff
            ru_in = rhs_u[cells] + diff * ubx
            rv_in = rhs_v[cells] + diff * uby
            du_in = np.where(flux > F(0), du_in + flux, du_in)
            dv_in = np.where(flux > F(0), dv_in + flux, dv_in)
            ru_in = np.where(flux > F(0), ru_in, ru_in - flux * ubx)
            rv_in = np.where(flux > F(0), rv_in, rv_in - flux * uby)
            flux_bc = (ubx * nx + uby * ny) * area
            # wall
            du_w, dv_w = du + diff, dv + diff
            ru_w = rhs_u[cells] + bv.wall_sign() * (diff * ubx)
            rv_w = rhs_v[cells] + bv.wall_sign() * (diff * uby)
            # outlet
            du_o = np.where(flux > F(0), du + flux, du)
            dv_o = np.where(flux > F(0), dv + flux, dv)
            lap_o = st.d_p[cells] * area / dist
            sc_o = c.density * st.d_p[cells] * area / dist
            diag_u[cells] = np.where(internal, du_i, np.where(inl, du_in, np.where(wal, du_w, np.where(out, du_o, du))))
            diag_v[cells] = np.where(internal, dv_i, np.where(inl, dv_in, np.where(wal, dv_w, np.where(out, dv_o, dv))))
            rhs_u[cells] = np.where(internal, rcu, np.where(inl, ru_in, np.where(wal & wsel, ru_w, rhs_u[cells])))
            rhs_v[cells] = np.where(internal, rcv, np.where(inl, rv_in, np.where(wal & wsel, rv_w, rhs_v[cells])))
            rhs_p[cells] = np.where(inl, rhs_p[cells] - flux_bc, rhs_p[cells])
            sup[cells] = np.where(internal, sup[cells] + lam * pgx, np.where(inl | wal, sup[cells] + pgx, sup[cells]))
            svp[cells] = np.where(internal, svp[cells] + lam * pgy, np.where(inl | wal, svp[cells] + pgy, svp[cells]))
            spu[cells] = np.where(internal, spu[cells] + lam * dcx_, np.where(out, spu[cells] + dcx_, spu[cells]))
            spv[cells] = np.where(internal, spv[cells] + lam * dcy_, np.where(out, spv[cells] + dcy_, spv[cells]))
            spp[cells] = np.where(internal, spp[cells] + lap, np.where(out, spp[cells] + lap_o, spp[cells]))
            sdp[cells] = np.where(internal, sdp[cells] + scoef, np.where(out, sdp[cells] + sc_o, sdp[cells]))
        # diagonal block (:422-461)
        dr = M.diag_idx - M.srow[:-1]
        r0 = 9 * M.srow[:-1]
        r1 = r0 + 3 * nbr
        r2 = r0 + 6 * nbr
        mv[r0 + 3 * dr + 0] = diag_u
        mv[r0 + 3 * dr + 1] = F(0)
        mv[r0 + 3 * dr + 2] = sup
        mv[r1 + 3 * dr + 0] = F(0)
        mv[r1 + 3 * dr + 1] = diag_v
        mv[r1 + 3 * dr + 2] = svp
        mv[r2 + 3 * dr + 0] = spu
        mv[r2 + 3 * dr + 1] = spv
        mv[r2 + 3 * dr + 2] = F(0) + spp
        sv[M.diag_idx] = sdp
        rhs = np.zeros(3 * N, F)
        rhs[0::3], rhs[1::3], rhs[2::3] = rhs_u, rhs_v, rhs_p
        inv = lambda v: np.where(np.abs(v) > F(1e-14), F(1) / v, F(0)).astype(F)  # noqa: E731
        return mv, rhs, sv, inv(diag_u), inv(diag_v), inv(sdp)


# --------------------------------------------------------------------- solver
class BcvRefSolver(BuoyantRefSolver):
    """BuoyantRefSolver with GpuSolver's boundary-velocity surface.  bv_class: a
    BoundaryVelocities subclass (a wrong variant)."""

    def __init__(self, mesh, M=None, bv_class=BoundaryVelocities, **cfg):
        super().__init__(mesh, M=M, **cfg)
        self.bv = bv_class(self._arrays)
        self.region = np.zeros(self.bv.F, bool)

    # ---- the surface ------------------------------------------------------------
    def set_boundary_velocity(self, faces, v):
        return self.bv.set(faces, v)

    def clear_boundary_velocity(self):
        self.bv.clear()

    def set_boundary_velocity_scale(self, inlet_scale=1.0, wall_scale=1.0):
        self.bv.inlet_scale, self.bv.wall_scale = F(inlet_scale), F(wall_scale)

    def boundary_velocity(self):
        return self.bv.info()

    def set_inlet_profile(self, fn):
        a = self._arrays
        f = np.nonzero(self.bv.bt == INLET)[0]
        u, v = fn(a["face_cx"][f], a["face_cy"][f])
        return self.bv.set(f, np.stack([np.broadcast_to(np.asarray(u, np.float64), f.shape),
                                        np.broadcast_to(np.asarray(v, np.float64), f.shape)], 1))

    def set_wall_motion(self, box, velocity=(0.0, 0.0), omega=0.0, centre=None):
        a = self._arrays
        x0, y0, x1, y1 = box
        xc, yc = (0.5 * (x0 + x1), 0.5 * (y0 + y1)) if centre is None else centre
        x, y = a["face_cx"], a["face_cy"]
        f = np.nonzero((self.bv.bt == WALL) & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1))[0]
        if len(f) == 0:
            return int(self.bv.sel.sum())
        return self.bv.set(f, np.stack([velocity[0] - omega * (y[f] - yc), velocity[1] + omega * (x[f] - xc)], 1))

    def set_force_region(self, x0, y0, x1, y1):
        a = self._arrays
        x, y = a["face_cx"], a["face_cy"]
        self.region = (self.bv.bt == WALL) & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1) & (not x1 < x0)
        return int(self.region.sum())

    # ---- the step ---------------------------------------------------------------
    def _wrapped(self):
        bv = self.bv
        return (lambda M, st, old, c: prepare(M, st, old, c, bv),
                lambda M, st, old, oo, fl, gu, gv, c: assemble(M, st, old, oo, fl, gu, gv, c, bv))

    def step(self):
        if not self.bv.sel.any():  # the empty selection: the plain step
            return super().step()
        plain = refpy.prepare, refpy.assemble
        refpy.prepare, refpy.assemble = self._wrapped()
        try:
            super().step()
        finally:
            refpy.prepare, refpy.assemble = plain

    def debug_prepare_assemble(self):
        """cfd_debug_prepare_assemble: prepare and assemble on the current state, no
        rotation; dict of fluxes, grad_u, grad_v, mv, rhs (buoyancy added), sv, dui, dvi, dpi"""
        st, old, old_old = self.ring[self.i_state], self.ring[self.i_old], self.ring[self.i_old_old]
        prep, asm = self._wrapped() if self.bv.sel.any() else (refpy.prepare, refpy.assemble)
        fl, gu, gv = prep(self.M, st, old, self.c)
        mv, rhs, sv, dui, dvi, dpi = asm(self.M, st, old, old_old, fl, gu, gv, self.c)
        return dict(fluxes=fl, grad_u=gu, grad_v=gv, mv=mv, rhs=self.add_buoyancy(rhs), sv=sv, dui=dui, dvi=dvi, dpi=dpi)

    # ---- diagnostics --------------------------------------------------------------
    def _wall_terms(self):
        """per force-region wall face, float64 from the float32 values, in the order
        of the header: (faces, owner cells, F_p [m, 2], F_v [m, 2], ub [m, 2], selected)"""
        M, c = self.M, self.c
        st = self.ring[self.i_state]
        ramp = _smoothstep(0.0, c.ramp_time, c.time)
        ubx, uby, sw = self.bv.face_values(M, c, ramp)
        f = np.nonzero(self.region)[0]
        o = M.own[f]
        d = np.float64
        area = M.area[f].astype(d)
        dvx, dvy = M.fx[f] - M.cx[o], M.fy[f] - M.cy[o]
        dist = np.sqrt(dvx * dvx + dvy * dvy).astype(d)  # dist_e: float32 |face centre - cell centre|
        nx, ny = M.nx[f].astype(d), M.ny[f].astype(d)    # a boundary face: its owner's outward normal
        p = st.p[o].astype(d)
        sel = sw[f]
        bx, by = np.where(sel, ubx[f], F(0)).astype(d), np.where(sel, uby[f], F(0)).astype(d)
        rux = np.where(sel, st.u[o, 0].astype(d) - bx, st.u[o, 0].astype(d))
        ruy = np.where(sel, st.u[o, 1].astype(d) - by, st.u[o, 1].astype(d))
        nu = float(c.viscosity)
        Fp = np.stack([p * nx * area, p * ny * area], 1)
        Fv = np.stack([nu * rux * area / dist, nu * ruy * area / dist], 1)
        return f, o, Fp, Fv, np.stack([bx, by], 1), sel

    def _by_cell(self, faces, cells, terms):
        """canonical sum over the cells of each cell's terms added in slot order"""
        t = np.zeros(self.M.N)
        slot = {}
        for i in np.unique(cells):
            slot[i] = {int(fc): k for k, fc in enumerate(self.M.slot_face[i]) if fc >= 0}
        order = sorted(range(len(faces)), key=lambda j: (cells[j], slot[cells[j]][int(faces[j])]))
        for j in order:
            t[cells[j]] = t[cells[j]] + terms[j]
        return float(refpy.canon_sum(t))

    def wall_force(self):
        """cfd_flow_diag's force_pressure, force_viscous over the force region"""
        f, o, Fp, Fv, ub, sel = self._wall_terms()
        return ([self._by_cell(f, o, Fp[:, 0]), self._by_cell(f, o, Fp[:, 1])],
                [self._by_cell(f, o, Fv[:, 0]), self._by_cell(f, o, Fv[:, 1])])

    def wall_motion(self, x0=0.0, y0=0.0):
        """cfd_wall_motion_get: (torque_pressure, torque_viscous, power, region faces, moving faces)"""
        f, o, Fp, Fv, ub, sel = self._wall_terms()
        a = self._arrays
        rx, ry = a["face_cx"][f] - x0, a["face_cy"][f] - y0
        tp = rx * Fp[:, 1] - ry * Fp[:, 0]
        tv = rx * Fv[:, 1] - ry * Fv[:, 0]
        pw = np.where(sel, -((Fp[:, 0] + Fv[:, 0]) * ub[:, 0] + (Fp[:, 1] + Fv[:, 1]) * ub[:, 1]), 0.0)
        # the kernel subtracts the term from +0: the same value, and -(x) + 0 rounds alike
        return (self._by_cell(f, o, tp), self._by_cell(f, o, tv), self._by_cell(f, o, pw), int(len(f)),
                int(sel.sum()))

    def velocity_gradients(self):
        """the Green-Gauss gradients of the flow diagnostics: prepare's, on a copy of the state"""
        st = self.ring[self.i_state].copy()
        prep = self._wrapped()[0] if self.bv.sel.any() else refpy.prepare
        _, gu, gv = prep(self.M, st, self.ring[self.i_old], self.c)
        return gu, gv
