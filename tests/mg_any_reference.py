"""The any-size multigrid pressure solve of the cavity and Rayleigh-Benard
(CFD_POISSON_MULTIGRID_ANY) restated in numpy: the yardstick of
its GPU path (csrc/mg.hip, the scheme MgAny), which must give the same cycle
count, residual and pressure bit for bit.

The scheme is mg_reference's with sizes halved rounding up. In units of the
finest spacing h, cells 1 .. n_l - 1 of level l are W = 2^l wide and the last
cell is w_l = n_0 - (n_l - 1) W wide (1 <= w_l <= W), so the walls stay where
level 0 has them. The operator is the finite-volume one on that grid, in units
of ih2_l = 1 / (4^l h^2): every coefficient is 1 but across the face between
cells n_l - 1 and n_l, whose centres are (W + w_l) / 2 apart: the east (north)
coefficient of cell n_l - 1 is 2 W / (W + w_l), the west (south) coefficient of
cell n_l that times W / w_l. Row 1 keeps mg_reference's Dirichlet zero at
y = -h/2. The restriction is minus the volume-weighted mean of the children's
residuals (the last coarse cell has one child where n_l is odd), the
prolongation linear between the two nearest coarse centres and constant beyond
the last one.

Every expression is one IEEE double operation per operator in the written
order. The sweeps and the residual are mg_reference's own functions on this
module's coefficients: a coefficient of 1 multiplies to the same bits, so a
cell whose stencil touches no irregular face is computed as there, and a grid
on which mg_reference's plan ends with a smaller side below 8 gives its bits.
"""
from __future__ import annotations

import math

import numpy as np

import mg_reference as M

MAX_COARSE_CELLS = M.MAX_COARSE_CELLS
MAX_LEVELS = 16

sweep = M.sweep        # one red-black sweep (Gauss-Seidel, or the coarsest level's SOR) on a Level of this module
residual = M.residual  # (ny, nx) interior residual; at level 0 the reference's (cavity-01.cpp:670-673)
smoothing_launches = M.smoothing_launches
random_source = M.random_source


def plan(nx: int, ny: int):
    """[(nx_l, ny_l)]: n_{l+1} = ceil(n_l / 2) while the smaller side is at least 8. None
    where the grid has no valid plan: a smaller side below 8 (one level), more than 16
    levels, or a coarsest level of more than 4096 cells."""
    lv = [(nx, ny)]
    while min(lv[-1]) >= 8:
        if len(lv) == MAX_LEVELS:
            return None
        lv.append(((lv[-1][0] + 1) // 2, (lv[-1][1] + 1) // 2))
    if len(lv) < 2 or lv[-1][0] * lv[-1][1] > MAX_COARSE_CELLS:
        return None
    return lv


def tail(pl) -> int:
    return M.tail(pl)


def launches_per_cycle(pl, nu1: int, nu2: int, fused: bool = True) -> int:
    per_level = smoothing_launches(nu1, fused) + smoothing_launches(nu2, fused) + 2
    return tail(pl) * per_level + 2


class Direction:
    """One direction of level l: n cells of n0 finest ones, and what the transfer
    to the next level (nc cells) needs. The constants as mga_make_plan forms them."""

    def __init__(self, l: int, n0: int, n: int, has_next: bool):
        self.n = n
        self.W = W = float(2 ** l)
        self.w = w = float(n0 - (n - 1) * 2 ** l)
        self.irregular = w != W
        # the face between cells n - 1 and n: (east of n - 1, west of n)
        self.c_lo = (2.0 * W) / (W + w)
        self.c_hi = self.c_lo * (W / w)
        # the transfer to the next level: irregular where n is odd or the last cell is narrow
        self.t_irregular = has_next and (n % 2 == 1 or self.irregular)
        self.single = n % 2 == 1            # the last coarse cell has one child
        self.nc = nc = (n + 1) // 2
        self.r0, self.r1 = 0.5, 0.5         # restriction weights of the last coarse cell's children
        self.first = 2 * nc - 2             # the fine cells first .. n take the weights below
        self.pa = [0.75, 0.75, 0.75]        # (own coarse cell, the neighbour on the child's side)
        self.pb = [0.25, 0.25, 0.25]
        if not self.t_irregular:
            self.first = n + 1
            return
        wc = float(n0 - (nc - 1) * 2 ** (l + 1))
        if not self.single:
            self.r0 = W / (W + w)
            self.r1 = w / (W + w)
        D = W + 0.5 * wc                    # between the last two coarse centres
        self.pb[0] = (0.5 * W) / D
        self.pa[0] = 1.0 - self.pb[0]
        if self.single:
            self.pa[1], self.pb[1] = 1.0, 0.0
        else:
            self.pb[1] = (0.5 * w) / D
            self.pa[1] = 1.0 - self.pb[1]
        self.pa[2], self.pb[2] = 1.0, 0.0   # (n even: cell n lies beyond the last coarse centre)


class Level:
    """A level with mg_reference.Level's attributes, so that its sweep and residual serve."""

    def __init__(self, l: int, n0x: int, n0y: int, nx: int, ny: int, dx: float, has_next: bool):
        self.l, self.nx, self.ny = l, nx, ny
        self.h2 = (4.0 ** l) * (dx * dx)
        self.ih2 = 1.0 / self.h2
        d = 0.5 + 0.5 ** (l + 1)
        self.cS = 1.0 / d
        self.g = 1.0 - self.cS
        self.x, self.y = Direction(l, n0x, nx, has_next), Direction(l, n0y, ny, has_next)
        ew, ee = np.ones(nx), np.ones(nx)
        cs, en = np.ones(ny), np.ones(ny)
        ee[nx - 2], ew[nx - 1] = self.x.c_lo, self.x.c_hi
        en[ny - 2], cs[ny - 1] = self.y.c_lo, self.y.c_hi
        ew[0], ee[nx - 1], en[ny - 1], cs[0] = 0.0, 0.0, 0.0, self.cS
        self.ew, self.ee = ew[None, :], ee[None, :]
        self.en, self.cs = en[:, None], cs[:, None]
        self.rdiag = 1.0 / (((self.ew + self.ee) + self.en) + self.cs)  # (ny, nx)
        n = max(nx, ny)
        self.omega = 2.0 / (1.0 + math.sin(math.pi / (n + 1)))
        self.one_m_omega = 1.0 - self.omega
        self.omr = self.omega * self.rdiag
        self.coarse_sweeps = 4 * n


def make_levels(nx: int, ny: int, dx: float):
    pl = plan(nx, ny)
    if pl is None:
        raise ValueError(f"{nx}x{ny} has no valid any-size multigrid plan")
    return [Level(l, nx, ny, a, b, dx, l + 1 < len(pl)) for l, (a, b) in enumerate(pl)]


def restrict(L: Level, r: np.ndarray) -> np.ndarray:
    """(ncy + 2, ncx + 2) coarse source from the fine interior residual r (ny, nx):
    mg_reference's -1/4 ((rSW + rSE) + (rNW + rNE)) on the coarse cells with four
    children of regular directions; on the last coarse column / row of an irregular
    direction -(b0 hS + b1 hN), hS = a0 rSW + a1 rSE and hN alike, a direction's
    single child standing alone (h = rW; -hS)."""
    ny, nx = r.shape
    X, Y = L.x, L.y
    fc = np.zeros((Y.nc + 2, X.nc + 2))
    fx, fy = nx // 2, ny // 2  # coarse cells with two children per direction
    fc[1:fy + 1, 1:fx + 1] = -0.25 * ((r[0:2 * fy:2, 0:2 * fx:2] + r[0:2 * fy:2, 1:2 * fx:2])
                                      + (r[1:2 * fy:2, 0:2 * fx:2] + r[1:2 * fy:2, 1:2 * fx:2]))

    def general(Js, Is):
        for J in Js:
            for I in Is:
                lastx, lasty = X.t_irregular and I == X.nc, Y.t_irregular and J == Y.nc
                a0, a1 = (X.r0, X.r1) if lastx else (0.5, 0.5)
                b0, b1 = (Y.r0, Y.r1) if lasty else (0.5, 0.5)
                j, i = 2 * J - 2, 2 * I - 2  # r's indices of the south-west child
                sx, sy = lastx and X.single, lasty and Y.single
                hS = r[j, i] if sx else a0 * r[j, i] + a1 * r[j, i + 1]
                if sy:
                    fc[J, I] = -hS
                    continue
                hN = r[j + 1, i] if sx else a0 * r[j + 1, i] + a1 * r[j + 1, i + 1]
                fc[J, I] = -(b0 * hS + b1 * hN)

    if X.t_irregular:
        general(range(1, Y.nc + 1), [X.nc])
    if Y.t_irregular:
        general([Y.nc], range(1, X.nc + 1))
    return fc


def extend(Lc: Level, e: np.ndarray) -> None:
    M.extend(Lc, e)


def prolong_add(L: Level, p: np.ndarray, e: np.ndarray) -> None:
    """p += the interpolant of the extended coarse e. Fine cell (j, i) of coarse cell
    (J, I) = ((j+1)>>1, (i+1)>>1) takes c = e(J, I) and V / H / D, the coarse neighbours on
    the child's side (south for odd j, west for odd i): mg_reference's
    (((9 c + 3 V) + 3 H) + D) / 16, but where i >= x.first or j >= y.first: with (ax, bx)
    and (ay, by) the direction's weights there (3/4, 1/4 in a regular direction),
    ay (ax c + bx H) + by (ax V + bx D); a weight b = 0 drops its terms (a = 1)."""
    ny, nx = L.ny, L.nx
    X, Y = L.x, L.y
    j = np.arange(1, ny + 1)[:, None]
    i = np.arange(1, nx + 1)[None, :]
    J, I = (j + 1) >> 1, (i + 1) >> 1
    dj, di = np.where(j & 1, -1, 1), np.where(i & 1, -1, 1)
    c, V, H, D = e[J, I], e[J + dj, I], e[J, I + di], e[J + dj, I + di]
    corr = (((9.0 * c + 3.0 * V) + 3.0 * H) + D) * 0.0625

    def weights(Dn, n):
        a, b = np.full(n, 0.75), np.full(n, 0.25)
        for k in range(3):
            q = Dn.first + k
            if q <= n:
                a[q - 1], b[q - 1] = Dn.pa[k], Dn.pb[k]
        return a, b

    ax, bx = (v[None, :] for v in weights(X, nx))
    ay, by = (v[:, None] for v in weights(Y, ny))
    with np.errstate(invalid="ignore", over="ignore"):
        rc = np.where(bx != 0.0, ax * c + bx * H, c)
        rv = np.where(bx != 0.0, ax * V + bx * D, V)
        gen = np.where(by != 0.0, ay * rc + by * rv, rc)
    special = (i >= X.first) | (j >= Y.first)
    p[1:-1, 1:-1] += np.where(special, gen, corr)


def vcycle(levels, l: int, p: np.ndarray, f: np.ndarray, nu1: int, nu2: int) -> None:
    L = levels[l]
    if l == len(levels) - 1:
        for _ in range(L.coarse_sweeps):
            sweep(L, p, f, sor=True)
        return
    for _ in range(nu1):
        sweep(L, p, f)
    fc = restrict(L, residual(L, p, f))
    e = np.zeros_like(fc)
    vcycle(levels, l + 1, e, fc, nu1, nu2)
    extend(levels[l + 1], e)
    prolong_add(L, p, e)
    for _ in range(nu2):
        sweep(L, p, f)


def solve(f: np.ndarray, dx: float, tol_factor: float = 1e-9, nu1: int = 2, nu2: int = 2, max_cycles: int = 50):
    """mg_reference.solve's loop (cavity-01.cpp:617-689 with a V-cycle for the sweep):
    returns (cycles, residual, p, history of max|r| after each cycle)."""
    ny, nx = f.shape[0] - 2, f.shape[1] - 2
    levels = make_levels(nx, ny, dx)
    f = np.ascontiguousarray(f, dtype=np.float64)
    p = np.zeros_like(f)
    tol = tol_factor * float(np.abs(f[1:-1, 1:-1]).max())
    res, cycles, hist = 1.0, 0, []
    while res > tol and cycles < max_cycles:
        vcycle(levels, 0, p, f, nu1, nu2)
        res = float(np.abs(residual(levels[0], p, f)).max())
        cycles += 1
        hist.append(res)
    return cycles, res, p, hist


def oracle_step(o, cp, **mg_opts):
    """mg_reference.oracle_step with this module's solve."""
    rb = cp.case_id == 3
    o.velocity_bc(False)
    if rb:
        o.temperature_bc()
    o.tentative()
    if rb:
        o.thermal()
    o.source()
    cycles, res, p, _ = solve(o.field("src"), cp.dx, cp.tol_factor, **mg_opts)
    o.field("p")[...] = p
    o.correct()
    return cycles, res


def level_doubles(nx: int, ny: int, dx: float, l: int) -> list[float]:
    """Level l's constants in cfd_mg_any_level's order (include/cfd_amd.h), every one as
    this module forms it: what the kernels multiply with."""
    pl = plan(nx, ny)
    levels = make_levels(nx, ny, dx)
    L, t = levels[l], tail(pl)
    lds_p = lds_f = -1
    if l >= t:
        lds_p = sum(2 * (a + 2) * (b + 2) for a, b in pl[t:l])
        lds_f = lds_p + (L.nx + 2) * (L.ny + 2)
    out = [L.nx, L.ny, (L.nx + 3 + 15) // 16 * 16, lds_p, lds_f, L.coarse_sweeps, t,
           L.g, L.one_m_omega, L.h2, L.ih2, L.cS]
    # a direction's classes: cell 1, cells 2 .. n - 2, cell n - 1, cell n (every level has n >= 4)
    cols, rows = [0, 1, L.nx - 2, L.nx - 1], [0, 1, L.ny - 2, L.ny - 1]
    out += [L.rdiag[rows[k >> 2], cols[k & 3]] for k in range(16)]
    out += [L.omr[rows[k >> 2], cols[k & 3]] for k in range(16)]
    for D in (L.x, L.y):
        out += [D.n - 1 if D.irregular else D.n, D.nc if D.t_irregular else 0, int(D.single), D.first,
                D.c_lo, D.c_hi, D.r0, D.r1, *D.pa, *D.pb]
    return [float(v) for v in out]
