"""The multigrid pressure solve restated in numpy: the yardstick
of the GPU path (csrc/mg.hip), which must give the same cycle count, residual
and pressure bit for bit.

Cavity-like operator (cavity-01.cpp:643-677): Neumann west / east / north, the
bottom ghost row held at 0 (eps_s = j_min = 1), i.e. a Dirichlet zero at the
finest grid's ghost centre y = -h/2. Coarse level l keeps that zero where it
is: its row 1 sees it at distance d_l = 0.5 + 0.5^(l+1) coarse spacings, so
its south coefficient is cS_l = 1/d_l (1 on every other row).

Every expression below is one IEEE double operation per operator in the
written order (numpy elementwise add / subtract / multiply; the divisions
only form the per-level constants), which is what the kernels compute with
contraction off. Fields are (ny+2, nx+2) arrays in the reference's indexing.
"""
from __future__ import annotations

import math

import numpy as np

MAX_COARSE_CELLS = 4096


def plan(nx: int, ny: int):
    """[(nx_l, ny_l)] from the solver's grid down, or None where the grid has
    no valid plan (fewer than two levels, or a coarsest level over 4096 cells)."""
    lv = [(nx, ny)]
    while lv[-1][0] % 2 == 0 and lv[-1][1] % 2 == 0 and min(lv[-1]) >= 8:
        lv.append((lv[-1][0] // 2, lv[-1][1] // 2))
    if len(lv) < 2 or lv[-1][0] * lv[-1][1] > MAX_COARSE_CELLS:
        return None
    return lv


class Level:
    def __init__(self, l: int, nx: int, ny: int, dx: float, unit_cs: bool = False):
        self.l, self.nx, self.ny = l, nx, ny
        self.h2 = (4.0 ** l) * (dx * dx)
        self.ih2 = 1.0 / self.h2
        d = 0.5 + 0.5 ** (l + 1)
        self.cS = 1.0 if unit_cs else 1.0 / d
        self.g = 1.0 - self.cS
        i = np.arange(1, nx + 1)
        j = np.arange(1, ny + 1)
        self.ew = (i > 1).astype(np.float64)[None, :]
        self.ee = (i < nx).astype(np.float64)[None, :]
        self.en = (j < ny).astype(np.float64)[:, None]
        self.cs = np.where(j == 1, self.cS, 1.0)[:, None]
        self.rdiag = 1.0 / (((self.ew + self.ee) + self.en) + self.cs)  # (ny, nx)
        n = max(nx, ny)
        self.omega = 2.0 / (1.0 + math.sin(math.pi / (n + 1)))
        self.one_m_omega = 1.0 - self.omega
        self.omr = self.omega * self.rdiag
        self.coarse_sweeps = 4 * n


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
        ee, ew = L.ee[:, k[1]], L.ew[:, k[1]]
        en, cs = L.en[k[0], :], L.cs[k[0], :]
        s = ((ee * p[js, ie] + ew * p[js, iw]) + (en * p[jn, is_] + cs * p[js_, is_])) - f[js, is_] * L.h2
        if sor:
            p[js, is_] = p[js, is_] * L.one_m_omega + L.omr[k] * s
        else:
            p[js, is_] = L.rdiag[k] * s


def sweep(L: Level, p: np.ndarray, f: np.ndarray, sor: bool = False) -> None:
    """One red-black sweep: colour 0 (row j starts at i = 1 + ((j+1)&1)), then colour 1."""
    _half_sweep(L, p, f, 0, sor)
    _half_sweep(L, p, f, 1, sor)


def residual(L: Level, p: np.ndarray, f: np.ndarray) -> np.ndarray:
    """(ny, nx) interior residual; at level 0 the reference's (cavity-01.cpp:670-673)."""
    c = p[1:-1, 1:-1]
    return L.ih2 * (((L.ee * (p[1:-1, 2:] - c) + L.ew * (p[1:-1, :-2] - c)) + L.en * (p[2:, 1:-1] - c))
                    + L.cs * (p[:-2, 1:-1] - c)) - f[1:-1, 1:-1]


def restrict(r: np.ndarray) -> np.ndarray:
    """(ny/2 + 2, nx/2 + 2) coarse source from the fine interior residual."""
    ny, nx = r.shape
    fc = np.zeros((ny // 2 + 2, nx // 2 + 2))
    fc[1:-1, 1:-1] = -0.25 * ((r[0::2, 0::2] + r[0::2, 1::2]) + (r[1::2, 0::2] + r[1::2, 1::2]))
    return fc


def extend(Lc: Level, e: np.ndarray) -> None:
    """One ghost layer of the coarse correction: rows, then columns."""
    e[Lc.ny + 1, 1:-1] = e[Lc.ny, 1:-1]
    e[0, 1:-1] = e[1, 1:-1] * Lc.g
    e[:, 0] = e[:, 1]
    e[:, Lc.nx + 1] = e[:, Lc.nx]


def prolong_add(p: np.ndarray, e: np.ndarray) -> None:
    """p += bilinear interpolant of the extended coarse e (cell-centred)."""
    c = e[1:-1, 1:-1]
    S, N = e[:-2, 1:-1], e[2:, 1:-1]
    W, E = e[1:-1, :-2], e[1:-1, 2:]
    SW, SE, NW, NE = e[:-2, :-2], e[:-2, 2:], e[2:, :-2], e[2:, 2:]
    p[1:-1:2, 1:-1:2] += (((9.0 * c + 3.0 * S) + 3.0 * W) + SW) * 0.0625
    p[1:-1:2, 2:-1:2] += (((9.0 * c + 3.0 * S) + 3.0 * E) + SE) * 0.0625
    p[2:-1:2, 1:-1:2] += (((9.0 * c + 3.0 * N) + 3.0 * W) + NW) * 0.0625
    p[2:-1:2, 2:-1:2] += (((9.0 * c + 3.0 * N) + 3.0 * E) + NE) * 0.0625


def vcycle(levels, l: int, p: np.ndarray, f: np.ndarray, nu1: int, nu2: int) -> None:
    L = levels[l]
    if l == len(levels) - 1:
        for _ in range(L.coarse_sweeps):
            sweep(L, p, f, sor=True)
        return
    for _ in range(nu1):
        sweep(L, p, f)
    fc = restrict(residual(L, p, f))
    e = np.zeros_like(fc)
    vcycle(levels, l + 1, e, fc, nu1, nu2)
    extend(levels[l + 1], e)
    prolong_add(p, e)
    for _ in range(nu2):
        sweep(L, p, f)


def make_levels(nx: int, ny: int, dx: float, unit_cs: bool = False):
    pl = plan(nx, ny)
    if pl is None:
        raise ValueError(f"{nx}x{ny} has no valid multigrid plan")
    return [Level(l, a, b, dx, unit_cs) for l, (a, b) in enumerate(pl)]


def solve(f: np.ndarray, dx: float, tol_factor: float = 1e-9, nu1: int = 2, nu2: int = 2, max_cycles: int = 50,
          unit_cs: bool = False):
    """The solve loop (mirrors cavity-01.cpp:617-689 with a V-cycle for the sweep):
    returns (cycles, residual, p, history of max|r| after each cycle)."""
    ny, nx = f.shape[0] - 2, f.shape[1] - 2
    levels = make_levels(nx, ny, dx, unit_cs)
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


MAX_LDS_DOUBLES = 18432


def tail(pl) -> int:
    """The first level of the one-launch tail (mg_make_plan's rule): walk from the
    last level down to level 1, stop at a level of more than 4096 cells or where
    p and f of it and every coarser level, ghosts included, pass 18432 doubles;
    the tail is the lowest level reached."""
    t = len(pl) - 1
    for l in range(len(pl) - 1, 0, -1):
        need = sum(2 * (a + 2) * (b + 2) for a, b in pl[l:])
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
    prolongation; then the tail and the residual pass."""
    per_level = smoothing_launches(nu1, fused) + smoothing_launches(nu2, fused) + 2
    return tail(pl) * per_level + 2


def oracle_step(o, cp, **mg_opts):
    """One timestep of the oracle `o` in its own phase order (Oracle.step_phases)
    with solve() in place of its SOR loop: returns (cycles, residual)."""
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


def dense_operator(L: Level) -> np.ndarray:
    """The level's operator as a matrix over the interior cells in row-major
    order, column by column from residual() with a zero source."""
    n = L.nx * L.ny
    A = np.empty((n, n))
    z = np.zeros((L.ny + 2, L.nx + 2))
    for k in range(n):
        p = np.zeros_like(z)
        p[1 + k // L.nx, 1 + k % L.nx] = 1.0
        A[:, k] = residual(L, p, z).ravel()
    return A


def direct_solve(f: np.ndarray, dx: float, refinements: int = 5):
    """A x = f on level 0 without multigrid: a dense float64 solve refined with
    np.longdouble residuals. Returns (x as a (ny+2, nx+2) field with zero
    ghosts, ||A^-1||_inf, max|f - A x| of the refined x in long double)."""
    ny, nx = f.shape[0] - 2, f.shape[1] - 2
    A = dense_operator(Level(0, nx, ny, dx))
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
    return out, float(np.abs(Ainv).sum(axis=1).max()), rmax


def yardstick_bound(f: np.ndarray, dx: float, p: np.ndarray, res: float, ainv_norm: float) -> float:
    """max|p - x| <= ||A^-1||_inf (res + 48 u ih2 max|p| + u max|f|), u = 2^-53: A (p - x) = r_exact, and the
    reference's own evaluation of r (the reported res) differs from r_exact by at most the rounding of its
    differences, products and sums (DESIGN.md §2's bound) plus that of the final subtraction of f."""
    u = 2.0 ** -53
    ih2 = 1.0 / (dx * dx)
    return ainv_norm * (res + 48.0 * u * ih2 * float(np.abs(p).max()) + u * float(np.abs(f).max()))


def cavity_source(us: np.ndarray, vs: np.ndarray, dx: float, dt: float, rho: float) -> np.ndarray:
    """source_term as the reference builds it (cavity-01.cpp:622-627); us / vs are
    (ny+2, nx+2) with u*(j, i) the east face of cell (j, i), v*(j, i) its north face."""
    f = np.zeros_like(us)
    tinv, hinv = 1.0 / dt, 1.0 / dx
    f[1:-1, 1:-1] = tinv * rho * ((us[1:-1, 1:-1] - us[1:-1, :-2]) * hinv + (vs[1:-1, 1:-1] - vs[:-2, 1:-1]) * hinv)
    return f


def random_source(nx: int, ny: int, dx: float, dt: float, seed: int) -> np.ndarray:
    """f from random u*, v* whose wall-normal faces are zero (a compatible source)."""
    rng = np.random.default_rng(seed)
    us = rng.standard_normal((ny + 2, nx + 2))
    vs = rng.standard_normal((ny + 2, nx + 2))
    us[:, 0] = us[:, nx] = 0.0
    vs[0, :] = vs[ny, :] = 0.0
    return cavity_source(us, vs, dx, dt, 1.0)
