"""The any-size multigrid pressure solve of the channel
(CFD_POISSON_MULTIGRID_OPEN_ANY) restated in numpy: the yardstick
of its GPU path (csrc/mg.hip, the scheme MgChannelAny), which must give the same
cycle count, residual and pressure bit for bit.

The scheme is mg_open_reference's (the channel: dx != dy, Neumann west / south /
north, a Dirichlet zero in the east ghost column, semi-coarsening) with sizes
halved rounding up, as mg_any_reference does for the cavity. A direction that was
halved h times has, in units of its finest spacing, cells 1 .. n - 1 of width
W = 2^h and a last cell of width w = n0 - (n - 1) W (1 <= w <= W): the walls and
the east zero stay where level 0 has them. A direction a transfer does not halve
is carried over unchanged. The operator is the finite-volume one with
mg_open_reference's absolute coefficients cx = 1 / hx^2, cy = 1 / hy^2: across the
face between cells n - 1 and n, whose centres are (W + w) / 2 apart, the east
(north) coefficient of cell n - 1 is cx 2W / (W + w) and the west (south)
coefficient of cell n that times W / w. Column nx sees the east zero (w + 1) / 2
finest spacings from its centre: with d = (w + 1) / (2 W) its east coefficient is
cE = (cx / d) (W / w) - for w = W, d is mg_open_reference's 0.5 + 0.5^(a+1) and
W / w = 1: its cE, bit for bit. The restriction is minus the volume-weighted mean
of the children's residuals in each halved direction (the last coarse cell has
one child where n is odd), the prolongation linear between the two nearest
coarse centres, constant beyond a Neumann end and, beyond the last coarse x
centre, linear towards the east zero.

Every expression is one IEEE double operation per operator in the written
order. A coefficient that equals cx multiplies to the same bits, so a cell whose
stencil and transfer touch no irregular face is computed as in
mg_open_reference, and a grid on which that module's plan stops on a size below
8 gives its bits.
"""
from __future__ import annotations

import math

import numpy as np

import mg_open_reference as M

MAX_COARSE_CELLS = M.MAX_COARSE_CELLS
MAX_LEVELS = M.MAX_LEVELS
MIN_CELLS = 4  # per direction on every level: the classes cell 1, 2 .. n - 2, n - 1, n are distinct
FULL, X_ONLY, Y_ONLY = M.FULL, M.X_ONLY, M.Y_ONLY

kinds = M.kinds
tail = M.tail
smoothing_launches = M.smoothing_launches
launches_per_cycle = M.launches_per_cycle
refresh_ghosts = M.refresh_ghosts
residual_reference = M.residual_reference
tolerance = M.tolerance
random_source = M.random_source
random_field = M.random_field


def plan_levels(nx: int, ny: int, dx: float, dy: float):
    """[(nx_l, ny_l, a_l, b_l)]: mg_open_reference.plan_levels with "even and >= 8"
    replaced by ">= 8" and n // 2 by (n + 1) // 2. None where the grid has no valid
    plan: fewer than two levels, more than 16, a coarsest level over 4096 cells, or
    a level (level 0 included) with fewer than 4 cells in a direction."""
    lv = [(nx, ny, 0, 0)]
    while True:
        n, m, a, b = lv[-1]
        hx, hy = math.ldexp(dx, a), math.ldexp(dy, b)
        q = hy / hx
        r = q * q
        cx, cy = n >= 8, m >= 8
        if r > 2.0:
            nxt = ((n + 1) // 2, m, a + 1, b) if cx else None
        elif r < 0.5:
            nxt = (n, (m + 1) // 2, a, b + 1) if cy else None
        else:
            nxt = ((n + 1) // 2, (m + 1) // 2, a + 1, b + 1) if cx and cy else None
        if nxt is None or len(lv) > MAX_LEVELS:
            break
        lv.append(nxt)
    if len(lv) < 2 or len(lv) > MAX_LEVELS or lv[-1][0] * lv[-1][1] > MAX_COARSE_CELLS:
        return None
    if min(min(n, m) for n, m, _, _ in lv) < MIN_CELLS:
        return None
    return lv


def plan(nx: int, ny: int, dx: float, dy: float):
    """[(nx_l, ny_l)] of plan_levels, or None."""
    lv = plan_levels(nx, ny, dx, dy)
    return None if lv is None else [(n, m) for n, m, _, _ in lv]


class Direction:
    """One direction of a level: n cells of n0 finest ones after h halvings, with the
    absolute coefficient c (cx or cy), and what the transfer to the next level needs
    where that transfer halves this direction (`halved`). `east`: the direction ends
    on the Dirichlet zero (x), not on a Neumann wall (y)."""

    def __init__(self, h: int, n0: int, n: int, c: float, halved: bool, east: bool):
        self.n, self.h = n, h
        self.W = W = float(2 ** h)
        self.w = w = float(n0 - (n - 1) * 2 ** h)
        self.irregular = w != W
        # the face between cells n - 1 and n: (east of n - 1, west of n)
        self.c_lo = c * ((2.0 * W) / (W + w))
        self.c_hi = self.c_lo * (W / w)
        self.halved = halved
        self.t_irregular = halved and (n % 2 == 1 or self.irregular)
        self.single = halved and n % 2 == 1      # the last coarse cell has one child
        self.nc = nc = (n + 1) // 2 if halved else n
        self.r0, self.r1 = 0.5, 0.5              # restriction weights of the last coarse cell's children
        self.first = n + 1                       # the fine cells first .. n take the weights below
        self.pa = [0.75, 0.75, 0.75]             # (own coarse cell, the neighbour on the child's side)
        self.pb = [0.25, 0.25, 0.25]
        if not self.t_irregular:
            return
        self.first = 2 * nc - 2
        wc = float(n0 - (nc - 1) * 2 ** (h + 1))
        if not self.single:
            self.r0 = W / (W + w)
            self.r1 = w / (W + w)
        D = W + 0.5 * wc                         # between the last two coarse centres
        self.pb[0] = (0.5 * W) / D
        self.pa[0] = 1.0 - self.pb[0]
        if self.single:                          # cell n is the last coarse cell itself
            self.pa[1], self.pb[1] = 1.0, 0.0
        else:
            self.pb[1] = (0.5 * w) / D
            self.pa[1] = 1.0 - self.pb[1]
        # n even: cell n lies beyond the last coarse centre - constant (Neumann), or linear towards the
        # east zero z = n0 + 1/2: (z - x) / (z - X_c) = (w + 1) / (wc + 1) on the last coarse cell alone
        self.pa[2], self.pb[2] = ((w + 1.0) / (wc + 1.0) if east else 1.0), 0.0


class Level:
    def __init__(self, nx: int, ny: int, a: int, b: int, n0x: int, n0y: int, dx: float, dy: float, kind: int,
                 unit_east: bool = False):
        self.nx, self.ny, self.a, self.b, self.kind = nx, ny, a, b, kind
        hx, hy = math.ldexp(dx, a), math.ldexp(dy, b)
        self.cx = 1.0 / (hx * hx)
        self.cy = 1.0 / (hy * hy)
        self.x = X = Direction(a, n0x, nx, self.cx, kind in (FULL, X_ONLY), True)
        self.y = Y = Direction(b, n0y, ny, self.cy, kind in (FULL, Y_ONLY), False)
        d = 1.0 if unit_east else (X.w + 1.0) / (2.0 * X.W)
        self.cE = (self.cx / d) * (X.W / X.w)
        self.g = 1.0 - 1.0 / d
        i = np.arange(1, nx + 1)
        j = np.arange(1, ny + 1)
        self.has_w = (i > 1)[None, :]
        self.has_e = (i < nx)[None, :]
        self.has_s = (j > 1)[:, None]
        self.has_n = (j < ny)[:, None]
        cw, ce = np.full(nx, self.cx), np.full(nx, self.cx)
        cs, cn = np.full(ny, self.cy), np.full(ny, self.cy)
        ce[nx - 2], cw[nx - 1] = X.c_lo, X.c_hi
        cn[ny - 2], cs[ny - 1] = Y.c_lo, Y.c_hi
        cw[0], ce[nx - 1], cs[0], cn[ny - 1] = 0.0, self.cE, 0.0, 0.0
        # (a coefficient of an absent neighbour enters the diagonal only: the sweeps and the residual skip it)
        self.cw, self.ce = cw[None, :], ce[None, :]
        self.cs, self.cn = cs[:, None], cn[:, None]
        self.rdiag = 1.0 / ((self.cw + self.ce) + (self.cs + self.cn))  # (ny, nx)
        m = max(nx, ny)
        self.omega = 2.0 / (1.0 + math.sin(math.pi / (m + 1)))
        self.one_m_omega = 1.0 - self.omega
        self.omr = self.omega * self.rdiag
        self.coarse_sweeps = 4 * m


def make_levels(nx: int, ny: int, dx: float, dy: float, unit_east: bool = False):
    pl = plan_levels(nx, ny, dx, dy)
    if pl is None:
        raise ValueError(f"{nx}x{ny} has no valid any-size open multigrid plan")
    kd = kinds(pl) + [-1]
    # (the unit-east variant keeps level 0 as it is: there d = 1 anyway)
    return [Level(n, m, a, b, nx, ny, dx, dy, k, unit_east) for (n, m, a, b), k in zip(pl, kd)]


def _half_sweep(L: Level, p: np.ndarray, f: np.ndarray, colour: int, sor: bool) -> None:
    nx, ny = L.nx, L.ny
    for j0 in (1, 2):  # rows j0, j0 + 2, ...: the colour's cells start at the same column
        i0 = 1 + ((j0 + 1 + colour) & 1)
        if j0 > ny or i0 > nx:
            continue
        js, is_ = slice(j0, ny + 1, 2), slice(i0, nx + 1, 2)
        jn, js_ = slice(j0 + 1, ny + 2, 2), slice(j0 - 1, ny, 2)
        ie, iw = slice(i0 + 1, nx + 2, 2), slice(i0 - 1, nx, 2)
        kj, ki = slice(j0 - 1, ny, 2), slice(i0 - 1, nx, 2)  # the same cells in the constants
        tE = np.where(L.has_e[:, ki], L.ce[:, ki] * p[js, ie], 0.0)
        tW = np.where(L.has_w[:, ki], L.cw[:, ki] * p[js, iw], 0.0)
        tN = np.where(L.has_n[kj, :], L.cn[kj, :] * p[jn, is_], 0.0)
        tS = np.where(L.has_s[kj, :], L.cs[kj, :] * p[js_, is_], 0.0)
        s = ((tE + tW) + (tN + tS)) - f[js, is_]
        if sor:
            p[js, is_] = p[js, is_] * L.one_m_omega + L.omr[kj, ki] * s
        else:
            p[js, is_] = L.rdiag[kj, ki] * s


def sweep(L: Level, p: np.ndarray, f: np.ndarray, sor: bool = False) -> None:
    """One red-black sweep: colour 0 (row j starts at i = 1 + ((j+1)&1)), then colour 1."""
    _half_sweep(L, p, f, 0, sor)
    _half_sweep(L, p, f, 1, sor)


def residual(L: Level, p: np.ndarray, f: np.ndarray) -> np.ndarray:
    """(ny, nx) interior residual of the level operator: sum of coef (nb - c), minus f;
    column nx's east term is cE (0 - c)."""
    c = p[1:-1, 1:-1]
    tE = np.where(L.has_e, L.ce * (p[1:-1, 2:] - c), L.cE * (0.0 - c))
    tW = np.where(L.has_w, L.cw * (p[1:-1, :-2] - c), 0.0)
    tN = np.where(L.has_n, L.cn * (p[2:, 1:-1] - c), 0.0)
    tS = np.where(L.has_s, L.cs * (p[:-2, 1:-1] - c), 0.0)
    return ((tE + tW) + (tN + tS)) - f[1:-1, 1:-1]


def restrict(L: Level, r: np.ndarray) -> np.ndarray:
    """(ncy + 2, ncx + 2) coarse source from the fine interior residual r (ny, nx).
    mg_open_reference's expressions (-1/4 ((rSW + rSE) + (rNW + rNE)), -1/2 (rW + rE),
    -1/2 (rS + rN)) on the coarse cells that are not the last of an irregular halved
    direction; on those -(b0 hS + b1 hN) with hS = a0 rSW + a1 rSE and hN alike, where
    a direction's single child, and a direction the transfer does not halve, stand
    alone (h = rW; -hS)."""
    ny, nx = r.shape
    X, Y, kind = L.x, L.y, L.kind
    fc = np.zeros((Y.nc + 2, X.nc + 2))
    fx, fy = nx // 2, ny // 2  # coarse cells with two children in a halved direction
    if kind == FULL:
        fc[1:fy + 1, 1:fx + 1] = -0.25 * ((r[0:2 * fy:2, 0:2 * fx:2] + r[0:2 * fy:2, 1:2 * fx:2])
                                          + (r[1:2 * fy:2, 0:2 * fx:2] + r[1:2 * fy:2, 1:2 * fx:2]))
    elif kind == X_ONLY:
        fc[1:-1, 1:fx + 1] = -0.5 * (r[:, 0:2 * fx:2] + r[:, 1:2 * fx:2])
    else:
        fc[1:fy + 1, 1:-1] = -0.5 * (r[0:2 * fy:2, :] + r[1:2 * fy:2, :])

    def general(Js, Is):
        for J in Js:
            for I in Is:
                lastx, lasty = X.t_irregular and I == X.nc, Y.t_irregular and J == Y.nc
                a0, a1 = (X.r0, X.r1) if lastx else (0.5, 0.5)
                b0, b1 = (Y.r0, Y.r1) if lasty else (0.5, 0.5)
                # r's indices of the south-west child (the cell itself in a direction that is not halved)
                j = 2 * J - 2 if Y.halved else J - 1
                i = 2 * I - 2 if X.halved else I - 1
                sx, sy = not X.halved or (lastx and X.single), not Y.halved or (lasty and Y.single)
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
    """mg_open_reference.extend: rows (Neumann), then columns (west Neumann; east the
    line through the zero, e(J, nx) g - read only by a regular x's prolongation)."""
    M.extend(Lc, e)


def prolong_add(L: Level, p: np.ndarray, e: np.ndarray) -> None:
    """p += the interpolant of the extended coarse e. Fine cell (j, i) of coarse cell
    (J, I) takes c = e(J, I) and V / H / D, the coarse neighbours on the child's side
    (south for odd j, west for odd i) in the halved directions:
    mg_open_reference's (((9 c + 3 V) + 3 H) + D) / 16, (3 c + H) / 4 or (3 c + V) / 4,
    but where i >= x.first or j >= y.first, with (ax, bx) and (ay, by) the directions'
    weights there (3/4, 1/4 in a regular one): ay (ax c + bx H) + by (ax V + bx D) for
    a full transfer, ax c + bx H or ay c + by V along the one halved direction; a weight
    b = 0 drops its term and leaves a times the other."""
    ny, nx = L.ny, L.nx
    X, Y, kind = L.x, L.y, L.kind
    j = np.arange(1, ny + 1)[:, None]
    i = np.arange(1, nx + 1)[None, :]
    if Y.halved:
        J, dj = (j + 1) >> 1, np.where(j & 1, -1, 1)
    else:
        J, dj = j, 0 * j
    if X.halved:
        I, di = (i + 1) >> 1, np.where(i & 1, -1, 1)
    else:
        I, di = i, 0 * i
    c, V, H, D = e[J, I], e[J + dj, I], e[J, I + di], e[J + dj, I + di]

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
        if kind == FULL:
            corr = (((9.0 * c + 3.0 * V) + 3.0 * H) + D) * 0.0625
            rc = np.where(bx != 0.0, ax * c + bx * H, ax * c)
            rv = np.where(bx != 0.0, ax * V + bx * D, ax * V)
            gen = np.where(by != 0.0, ay * rc + by * rv, ay * rc)
        elif kind == X_ONLY:
            corr = (3.0 * c + H) * 0.25
            gen = np.where(bx != 0.0, ax * c + bx * H, ax * c)
        else:
            corr = (3.0 * c + V) * 0.25
            gen = np.where(by != 0.0, ay * c + by * V, ay * c)
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


def solve(f: np.ndarray, p0: np.ndarray, dx: float, dy: float, tol_factor: float = 1e-7, abs_tol: float = 0.0,
          nu1: int = 2, nu2: int = 2, max_cycles: int = 50, unit_east: bool = False):
    """mg_open_reference.solve's loop (channel-01.cpp:642-688 with a V-cycle for the
    sweep): a warm start from p0, the loop primed with tol + 1, ghosts refreshed after
    each cycle, the stop test on the reference's own residual. Returns (cycles,
    residual, p, history of max|r| after each cycle)."""
    ny, nx = f.shape[0] - 2, f.shape[1] - 2
    levels = make_levels(nx, ny, dx, dy, unit_east)
    f = np.ascontiguousarray(f, dtype=np.float64)
    p = np.array(p0, dtype=np.float64, order="C", copy=True)
    tol = tolerance(f, tol_factor, abs_tol)
    res, cycles, hist = tol + 1.0, 0, []
    while res > tol and cycles < max_cycles:
        vcycle(levels, 0, p, f, nu1, nu2)
        refresh_ghosts(p)
        res = float(np.abs(residual_reference(p, f, dx, dy)).max())
        cycles += 1
        hist.append(res)
    return cycles, res, p, hist


def oracle_step(o, cp, **mg_opts):
    """mg_open_reference.oracle_step with this module's solve."""
    o.tentative()
    o.velocity_bc(True)
    o.source()
    cycles, res, p, _ = solve(o.field("src"), o.field("p"), cp.dx, cp.dy, cp.tol_factor, cp.abs_tol, **mg_opts)
    o.field("p")[...] = p
    o.correct()
    o.velocity_bc(False)
    return cycles, res


def level_doubles(nx: int, ny: int, dx: float, dy: float, l: int) -> list[float]:
    """Level l's constants in cfd_mg_open_any_level's order (include/cfd_amd.h), every
    one as this module forms it: what the kernels multiply with."""
    pl = plan(nx, ny, dx, dy)
    levels = make_levels(nx, ny, dx, dy)
    L, t = levels[l], tail(pl)
    lds_p = lds_f = -1
    if l >= t:
        lds_p = sum(2 * (a + 2) * (b + 2) for a, b in pl[t:l])
        lds_f = lds_p + (L.nx + 2) * (L.ny + 2)
    out = [L.nx, L.ny, (L.nx + 3 + 15) // 16 * 16, lds_p, lds_f, L.coarse_sweeps, t, L.kind, L.a, L.b,
           L.cx, L.cy, L.cE, L.g, L.one_m_omega]
    # a direction's classes: cell 1, cells 2 .. n - 2, cell n - 1, cell n (every level has n >= 4)
    cols, rows = [0, 1, L.nx - 2, L.nx - 1], [0, 1, L.ny - 2, L.ny - 1]
    out += [L.rdiag[rows[k >> 2], cols[k & 3]] for k in range(16)]
    out += [L.omr[rows[k >> 2], cols[k & 3]] for k in range(16)]
    for D in (L.x, L.y):
        out += [D.n - 1 if D.irregular else D.n, D.nc if D.t_irregular else 0, int(D.single), D.first,
                D.c_lo, D.c_hi, D.r0, D.r1, *D.pa, *D.pb]
    return [float(v) for v in out]
