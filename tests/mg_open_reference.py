"""The multigrid pressure solve of the channel ("The channel")
restated in numpy: the yardstick of the GPU path (csrc/mg.hip, the mgo_*
kernels), which must give the same cycle count, residual and pressure bit for
bit. It stands beside mg_reference.py (the cavity's scheme) and shares nothing
with it but the plan's tail rule and the launch-count rule.

Operator (channel-01.cpp:642-688): dx != dy, Neumann west / south / north and a
Dirichlet zero in the east ghost column, i.e. p = 0 at x = L + dx/2. Level l has
spacings hx = 2^a dx and hy = 2^b dy (a, b: how often x and y were halved), cx =
1/hx^2, cy = 1/hy^2. It keeps the zero where the finest grid has it: column nx
sees it d = 0.5 + 0.5^(a+1) spacings away, so its east coefficient is cE = cx/d
with neighbour value 0 (level 0: d = 1, the reference's operator). Absent
neighbours are skipped by selects (np.where), never multiplied by 0: no ghost
cell's value reaches a result.

Semi-coarsening: with r = (hy/hx)^2, r > 2 halves x only, r < 1/2 halves y only,
otherwise both; a direction can be halved while its size is even and >= 8.

Every expression is one IEEE double operation per operator in the written order,
which is what the kernels compute with contraction off. Fields are (ny+2, nx+2)
arrays in the reference's indexing.
"""
from __future__ import annotations

import math

import numpy as np

MAX_COARSE_CELLS = 4096
MAX_LDS_DOUBLES = 18432
MAX_LEVELS = 16
FULL, X_ONLY, Y_ONLY = 0, 1, 2  # how a level is coarsened to the next


def plan_levels(nx: int, ny: int, dx: float, dy: float, semi: bool = True):
    """[(nx_l, ny_l, a_l, b_l)] from the solver's grid down, or None where the grid
    has no valid plan (fewer than two levels, more than 16, or a coarsest level
    over 4096 cells). semi=False: full coarsening only (the degraded variant)."""
    lv = [(nx, ny, 0, 0)]
    while True:
        n, m, a, b = lv[-1]
        hx, hy = math.ldexp(dx, a), math.ldexp(dy, b)
        q = hy / hx
        r = q * q
        cx, cy = n % 2 == 0 and n >= 8, m % 2 == 0 and m >= 8
        if semi and r > 2.0:
            nxt = (n // 2, m, a + 1, b) if cx else None
        elif semi and r < 0.5:
            nxt = (n, m // 2, a, b + 1) if cy else None
        else:
            nxt = (n // 2, m // 2, a + 1, b + 1) if cx and cy else None
        if nxt is None:
            break
        lv.append(nxt)
    if len(lv) < 2 or len(lv) > MAX_LEVELS or lv[-1][0] * lv[-1][1] > MAX_COARSE_CELLS:
        return None
    return lv


def plan(nx: int, ny: int, dx: float, dy: float, semi: bool = True):
    """[(nx_l, ny_l)] of plan_levels, or None."""
    lv = plan_levels(nx, ny, dx, dy, semi)
    return None if lv is None else [(n, m) for n, m, _, _ in lv]


def kinds(pl):
    """The transfer kind between each pair of consecutive levels of a plan."""
    out = []
    for (n, m, *_), (nc, mc, *_) in zip(pl[:-1], pl[1:]):
        out.append(FULL if (nc != n and mc != m) else X_ONLY if nc != n else Y_ONLY)
    return out


class Level:
    def __init__(self, nx: int, ny: int, a: int, b: int, dx: float, dy: float, unit_east: bool = False):
        self.nx, self.ny, self.a, self.b = nx, ny, a, b
        hx, hy = math.ldexp(dx, a), math.ldexp(dy, b)
        self.cx = 1.0 / (hx * hx)
        self.cy = 1.0 / (hy * hy)
        d = 1.0 if unit_east else 0.5 + math.ldexp(1.0, -(a + 1))
        self.cE = self.cx / d
        self.g = 1.0 - 1.0 / d
        i = np.arange(1, nx + 1)
        j = np.arange(1, ny + 1)
        self.w = (i > 1)[None, :]
        self.e = (i < nx)[None, :]
        self.s = (j > 1)[:, None]
        self.n = (j < ny)[:, None]
        cw = np.where(self.w, self.cx, 0.0)
        ce = np.where(self.e, self.cx, self.cE)
        cs = np.where(self.s, self.cy, 0.0)
        cn = np.where(self.n, self.cy, 0.0)
        self.rdiag = 1.0 / ((cw + ce) + (cs + cn))  # (ny, nx)
        m = max(nx, ny)
        self.omega = 2.0 / (1.0 + math.sin(math.pi / (m + 1)))
        self.one_m_omega = 1.0 - self.omega
        self.omr = self.omega * self.rdiag
        self.coarse_sweeps = 4 * m


def _half_sweep(L: Level, p: np.ndarray, f: np.ndarray, colour: int, sor: bool) -> None:
    nx, ny = L.nx, L.ny
    for j0 in (1, 2):  # rows j0, j0 + 2, ...: the colour's cells start at the same column
        i0 = 1 + ((j0 + 1 + colour) & 1)
        if j0 > ny or i0 > nx:
            continue
        js, is_ = slice(j0, ny + 1, 2), slice(i0, nx + 1, 2)
        jn, js_ = slice(j0 + 1, ny + 2, 2), slice(j0 - 1, ny, 2)
        ie, iw = slice(i0 + 1, nx + 2, 2), slice(i0 - 1, nx, 2)
        k = (slice(j0 - 1, ny, 2), slice(i0 - 1, nx, 2))  # the same cells in the (ny, nx) constants
        tE = np.where(L.e[:, k[1]], L.cx * p[js, ie], 0.0)
        tW = np.where(L.w[:, k[1]], L.cx * p[js, iw], 0.0)
        tN = np.where(L.n[k[0], :], L.cy * p[jn, is_], 0.0)
        tS = np.where(L.s[k[0], :], L.cy * p[js_, is_], 0.0)
        s = ((tE + tW) + (tN + tS)) - f[js, is_]
        if sor:
            p[js, is_] = p[js, is_] * L.one_m_omega + L.omr[k] * s
        else:
            p[js, is_] = L.rdiag[k] * s


def sweep(L: Level, p: np.ndarray, f: np.ndarray, sor: bool = False) -> None:
    """One red-black sweep: colour 0 (the oracle's red: row j starts at i = 1 + ((j+1)&1)), then colour 1."""
    _half_sweep(L, p, f, 0, sor)
    _half_sweep(L, p, f, 1, sor)


def residual(L: Level, p: np.ndarray, f: np.ndarray) -> np.ndarray:
    """(ny, nx) interior residual of the level operator: sum of coef (nb - c), minus f."""
    c = p[1:-1, 1:-1]
    tE = np.where(L.e, L.cx * (p[1:-1, 2:] - c), L.cE * (0.0 - c))
    tW = np.where(L.w, L.cx * (p[1:-1, :-2] - c), 0.0)
    tN = np.where(L.n, L.cy * (p[2:, 1:-1] - c), 0.0)
    tS = np.where(L.s, L.cy * (p[:-2, 1:-1] - c), 0.0)
    return ((tE + tW) + (tN + tS)) - f[1:-1, 1:-1]


def restrict(r: np.ndarray, kind: int) -> np.ndarray:
    """The coarse source, ghosts zero, from the fine interior residual."""
    ny, nx = r.shape
    if kind == FULL:
        fc = np.zeros((ny // 2 + 2, nx // 2 + 2))
        fc[1:-1, 1:-1] = -0.25 * ((r[0::2, 0::2] + r[0::2, 1::2]) + (r[1::2, 0::2] + r[1::2, 1::2]))
    elif kind == X_ONLY:
        fc = np.zeros((ny + 2, nx // 2 + 2))
        fc[1:-1, 1:-1] = -0.5 * (r[:, 0::2] + r[:, 1::2])
    else:
        fc = np.zeros((ny // 2 + 2, nx + 2))
        fc[1:-1, 1:-1] = -0.5 * (r[0::2, :] + r[1::2, :])
    return fc


def extend(Lc: Level, e: np.ndarray) -> None:
    """One ghost layer of the coarse correction: rows (Neumann), then columns
    (west Neumann; east the line through the zero, e(J, nx) (1 - 1/d))."""
    e[Lc.ny + 1, 1:-1] = e[Lc.ny, 1:-1]
    e[0, 1:-1] = e[1, 1:-1]
    e[:, 0] = e[:, 1]
    e[:, Lc.nx + 1] = e[:, Lc.nx] * Lc.g


def prolong_add(p: np.ndarray, e: np.ndarray, kind: int) -> None:
    """p += interpolant of the extended coarse e (cell-centred): bilinear, or linear in the halved direction."""
    c = e[1:-1, 1:-1]
    S, N = e[:-2, 1:-1], e[2:, 1:-1]
    W, E = e[1:-1, :-2], e[1:-1, 2:]
    if kind == FULL:
        SW, SE, NW, NE = e[:-2, :-2], e[:-2, 2:], e[2:, :-2], e[2:, 2:]
        p[1:-1:2, 1:-1:2] += (((9.0 * c + 3.0 * S) + 3.0 * W) + SW) * 0.0625
        p[1:-1:2, 2:-1:2] += (((9.0 * c + 3.0 * S) + 3.0 * E) + SE) * 0.0625
        p[2:-1:2, 1:-1:2] += (((9.0 * c + 3.0 * N) + 3.0 * W) + NW) * 0.0625
        p[2:-1:2, 2:-1:2] += (((9.0 * c + 3.0 * N) + 3.0 * E) + NE) * 0.0625
    elif kind == X_ONLY:
        p[1:-1, 1:-1:2] += (3.0 * c + W) * 0.25
        p[1:-1, 2:-1:2] += (3.0 * c + E) * 0.25
    else:
        p[1:-1:2, 1:-1] += (3.0 * c + S) * 0.25
        p[2:-1:2, 1:-1] += (3.0 * c + N) * 0.25


def vcycle(levels, kd, l: int, p: np.ndarray, f: np.ndarray, nu1: int, nu2: int) -> None:
    L = levels[l]
    if l == len(levels) - 1:
        for _ in range(L.coarse_sweeps):
            sweep(L, p, f, sor=True)
        return
    for _ in range(nu1):
        sweep(L, p, f)
    fc = restrict(residual(L, p, f), kd[l])
    e = np.zeros_like(fc)
    vcycle(levels, kd, l + 1, e, fc, nu1, nu2)
    extend(levels[l + 1], e)
    prolong_add(p, e, kd[l])
    for _ in range(nu2):
        sweep(L, p, f)


def make_levels(nx: int, ny: int, dx: float, dy: float, semi: bool = True, unit_east: bool = False):
    pl = plan_levels(nx, ny, dx, dy, semi)
    if pl is None:
        raise ValueError(f"{nx}x{ny} has no valid multigrid plan")
    # (the unit-east variant keeps level 0 as it is: there d = 1 anyway)
    return [Level(n, m, a, b, dx, dy, unit_east) for n, m, a, b in pl], kinds(pl)


def refresh_ghosts(p: np.ndarray) -> None:
    """channel-01.cpp:531-541: west and east columns, then south and north rows (corners untouched)."""
    p[1:-1, 0] = p[1:-1, 1]
    p[1:-1, -1] = 0.0
    p[0, 1:-1] = p[1, 1:-1]
    p[-1, 1:-1] = p[-2, 1:-1]


def residual_reference(p: np.ndarray, f: np.ndarray, dx: float, dy: float) -> np.ndarray:
    """channel-01.cpp:672-681 on the ghosts as stored: (pE - 2c + pW) idx2 + (pN - 2c + pS) idy2 - f."""
    idx2, idy2 = 1.0 / (dx * dx), 1.0 / (dy * dy)
    c = p[1:-1, 1:-1]
    lap = ((p[1:-1, 2:] - 2.0 * c) + p[1:-1, :-2]) * idx2 + ((p[2:, 1:-1] - 2.0 * c) + p[:-2, 1:-1]) * idy2
    return lap - f[1:-1, 1:-1]


def tolerance(f: np.ndarray, tol_factor: float, abs_tol: float) -> float:
    m = float(np.abs(f[1:-1, 1:-1]).max())
    return max(tol_factor * (m if m > 0 else 1.0), abs_tol)


def solve(f: np.ndarray, p0: np.ndarray, dx: float, dy: float, tol_factor: float = 1e-7, abs_tol: float = 0.0,
          nu1: int = 2, nu2: int = 2, max_cycles: int = 50, semi: bool = True, unit_east: bool = False):
    """The solve loop (channel-01.cpp:642-688 with a V-cycle for the sweep): a warm
    start from p0, the loop primed with tol + 1, ghosts refreshed after each cycle,
    the stop test on the reference's own residual. Returns (cycles, residual, p,
    history of max|r| after each cycle)."""
    ny, nx = f.shape[0] - 2, f.shape[1] - 2
    levels, kd = make_levels(nx, ny, dx, dy, semi, unit_east)
    f = np.ascontiguousarray(f, dtype=np.float64)
    p = np.array(p0, dtype=np.float64, order="C", copy=True)
    tol = tolerance(f, tol_factor, abs_tol)
    res, cycles, hist = tol + 1.0, 0, []
    while res > tol and cycles < max_cycles:
        vcycle(levels, kd, 0, p, f, nu1, nu2)
        refresh_ghosts(p)
        res = float(np.abs(residual_reference(p, f, dx, dy)).max())
        cycles += 1
        hist.append(res)
    return cycles, res, p, hist


def tail(pl) -> int:
    """The first level of the one-launch tail (the cavity plan's rule): walk from the
    last level down to level 1, stop at a level of more than 4096 cells or where p
    and f of it and every coarser level, ghosts included, pass 18432 doubles."""
    t = len(pl) - 1
    for l in range(len(pl) - 1, 0, -1):
        need = sum(2 * (lv[0] + 2) * (lv[1] + 2) for lv in pl[l:])
        if pl[l][0] * pl[l][1] > MAX_COARSE_CELLS or need > MAX_LDS_DOUBLES:
            break
        t = l
    return t


def smoothing_launches(nu: int, fused: bool) -> int:
    """Launches of nu sweeps of a multi-launch level: fused, nu cut into pieces of
    at most 3 with 4 cut as 2 + 2; otherwise one launch per colour."""
    if not fused:
        return 2 * nu
    n = 0
    while nu > 0:
        nu -= 2 if nu == 4 else min(nu, 3)
        n += 1
    return n


def launches_per_cycle(pl, nu1: int, nu2: int, fused: bool = True) -> int:
    """Each level below the tail: its smoothing launches, the restriction and the
    prolongation; then the tail, the ghost refresh and the residual pass."""
    per_level = smoothing_launches(nu1, fused) + smoothing_launches(nu2, fused) + 2
    return tail(pl) * per_level + 3


def oracle_step(o, cp, **mg_opts):
    """One timestep of the oracle `o` in the open cases' phase order
    (Oracle.step_phases) with solve() in place of its SOR loop, warm-started from
    the oracle's own p: returns (cycles, residual)."""
    o.tentative()
    o.velocity_bc(True)
    o.source()
    cycles, res, p, _ = solve(o.field("src"), o.field("p"), cp.dx, cp.dy, cp.tol_factor, cp.abs_tol, **mg_opts)
    o.field("p")[...] = p
    o.correct()
    o.velocity_bc(False)
    return cycles, res


def dense_operator(nx: int, ny: int, dx: float, dy: float) -> np.ndarray:
    """The level-0 operator as a matrix over the interior cells in row-major order,
    column by column from the pinned residual (residual_reference on refreshed
    ghosts) with a zero source: not from this file's Level."""
    n = nx * ny
    A = np.empty((n, n))
    z = np.zeros((ny + 2, nx + 2))
    for k in range(n):
        p = np.zeros_like(z)
        p[1 + k // nx, 1 + k % nx] = 1.0
        refresh_ghosts(p)
        A[:, k] = residual_reference(p, z, dx, dy).ravel()
    return A


def direct_solve(f: np.ndarray, dx: float, dy: float, refinements: int = 5):
    """A x = f on level 0 without multigrid: a dense float64 solve refined with
    np.longdouble residuals. Returns (x as a (ny+2, nx+2) field with refreshed
    ghosts, ||A^-1||_inf, max|f - A x| of the refined x in long double)."""
    ny, nx = f.shape[0] - 2, f.shape[1] - 2
    A = dense_operator(nx, ny, dx, dy)
    Ainv = np.linalg.inv(A)
    b = np.ascontiguousarray(f[1:-1, 1:-1], dtype=np.float64).ravel()
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    x = (Ainv @ b).astype(np.longdouble)
    for _ in range(refinements):
        r = bl - Al @ x
        x = x + (Ainv @ r.astype(np.float64)).astype(np.longdouble)
    rmax = float(np.abs(bl - Al @ x).max())
    out = np.zeros_like(f, dtype=np.float64)
    out[1:-1, 1:-1] = x.astype(np.float64).reshape(ny, nx)
    refresh_ghosts(out)
    return out, float(np.abs(Ainv).sum(axis=1).max()), rmax


def yardstick_bound(f: np.ndarray, dx: float, dy: float, p: np.ndarray, res: float, ainv_norm: float) -> float:
    """mg_reference.yardstick_bound's statement with the channel's coefficients:
    max|p - x| <= ||A^-1||_inf (res + 48 u max(idx2, idy2) max|p| + u max|f|), u = 2^-53."""
    u = 2.0 ** -53
    c = max(1.0 / (dx * dx), 1.0 / (dy * dy))
    return ainv_norm * (res + 48.0 * u * c * float(np.abs(p).max()) + u * float(np.abs(f).max()))


def random_source(nx: int, ny: int, seed: int) -> np.ndarray:
    """A random source with zero ghosts whose interior mean is removed."""
    rng = np.random.default_rng(seed)
    f = np.zeros((ny + 2, nx + 2))
    r = rng.standard_normal((ny, nx))
    f[1:-1, 1:-1] = r - r.mean()
    return f


def random_field(nx: int, ny: int, seed: int) -> np.ndarray:
    """A random p, ghosts included."""
    return np.random.default_rng(seed).standard_normal((ny + 2, nx + 2))
