"""The multigrid pressure solve of the backwards-facing step
restated in numpy: the yardstick of the GPU path (csrc/mg.hip, the mgs_*
kernels), which must give the same cycle count, residual and pressure bit for
bit. It stands beside mg_open_reference.py (the channel's scheme) and shares
nothing with it but the semi-coarsening rule by r, the plan's tail rule and the
launch-count rule.

Geometry: level l has a halvings of x and b of y, si = step_i >> a, jm =
inlet_jmax >> b; cell (J, I) is fluid iff I > si or J <= jm. Solid cells are no
unknowns: never written, and never read by a fluid cell's update.

Operator (backwards_step-01.cpp:872-939 on the ghosts and solids that
685-740 refresh): the channel's - cx = 1/hx^2, cy = 1/hy^2, Neumann west / south
/ north, a Dirichlet zero in the east ghost column seen d = 0.5 + 0.5^(a+1)
spacings away (cE = cx / d) - where a neighbour exists only if it is inside the
grid and fluid. The reference sets the block's corner solid C = (jm+1, si) to
(p_A + p_B) / 2 of its east fluid cell A = (jm+1, si+1) and its south fluid
cell B = (jm, si); substituted in, A's west term is (cx/2)(p_B - p_A) and B's
north term (cy/2)(p_A - p_B), on every level. A and B have the same colour:
both updates of a colour phase use the pre-phase values (the pair rule).

Absent neighbours are skipped by selects (np.where), never multiplied by 0.
Every expression is one IEEE double operation per operator in the written
order, which is what the kernels compute with contraction off. Fields are
(ny+2, nx+2) arrays in the reference's indexing.
"""
from __future__ import annotations

import math

import numpy as np

MAX_COARSE_CELLS = 4096
MAX_LDS_DOUBLES = 18432
MAX_LEVELS = 16
FULL, X_ONLY, Y_ONLY = 0, 1, 2  # how a level is coarsened to the next


def geometry_ok(ny: int, si: int, jm: int) -> bool:
    """The geometry rule: a block at least 2 columns wide, under it at least 2 rows, at least 2 rows high."""
    return si >= 2 and jm >= 2 and ny - jm >= 2


def plan_levels(nx: int, ny: int, dx: float, dy: float, si: int, jm: int, semi: bool = True):
    """[(nx_l, ny_l, a_l, b_l, si_l, jm_l)] from the solver's grid down, or None where the
    grid has no valid plan (fewer than two levels, more than 16, or a coarsest level over
    4096 cells). x can be halved while nx is even and >= 8 and si is even and >= 2; y while
    ny is even and >= 8, jm is even and >= 2 and ny - jm >= 2. semi=False: full coarsening only."""
    lv = [(nx, ny, 0, 0, si, jm)]
    while True:
        n, m, a, b, s, j = lv[-1]
        hx, hy = math.ldexp(dx, a), math.ldexp(dy, b)
        q = hy / hx
        r = q * q
        cx = n % 2 == 0 and n >= 8 and s % 2 == 0 and s >= 2
        cy = m % 2 == 0 and m >= 8 and j % 2 == 0 and j >= 2 and m - j >= 2
        if semi and r > 2.0:
            nxt = (n // 2, m, a + 1, b, s // 2, j) if cx else None
        elif semi and r < 0.5:
            nxt = (n, m // 2, a, b + 1, s, j // 2) if cy else None
        else:
            nxt = (n // 2, m // 2, a + 1, b + 1, s // 2, j // 2) if cx and cy else None
        if nxt is None:
            break
        lv.append(nxt)
    if len(lv) < 2 or len(lv) > MAX_LEVELS or lv[-1][0] * lv[-1][1] > MAX_COARSE_CELLS:
        return None
    return lv


def plan(nx: int, ny: int, dx: float, dy: float, si: int, jm: int, semi: bool = True):
    """[(nx_l, ny_l)] of plan_levels, or None."""
    lv = plan_levels(nx, ny, dx, dy, si, jm, semi)
    return None if lv is None else [(l[0], l[1]) for l in lv]


def plan_of(cp, semi: bool = True):
    """plan() of a CaseParams."""
    return plan(cp.nx, cp.ny, cp.dx, cp.dy, cp.step_i, cp.inlet_jmax, semi)


def kinds(pl):
    """The transfer kind between each pair of consecutive levels of a plan."""
    out = []
    for (n, m, *_), (nc, mc, *_) in zip(pl[:-1], pl[1:]):
        out.append(FULL if (nc != n and mc != m) else X_ONLY if nc != n else Y_ONLY)
    return out


def fluid_mask(nx: int, ny: int, si: int, jm: int) -> np.ndarray:
    """(ny, nx) over the interior cells."""
    i = np.arange(1, nx + 1)[None, :]
    j = np.arange(1, ny + 1)[:, None]
    return (i > si) | (j <= jm)


class Level:
    def __init__(self, nx, ny, a, b, si, jm, dx, dy, couple: bool = True):
        self.nx, self.ny, self.a, self.b, self.si, self.jm = nx, ny, a, b, si, jm
        self.couple = couple
        hx, hy = math.ldexp(dx, a), math.ldexp(dy, b)
        self.cx = 1.0 / (hx * hx)
        self.cy = 1.0 / (hy * hy)
        self.chx = self.cx * 0.5  # the pair's coefficients: A's west, B's north
        self.chy = self.cy * 0.5
        d = 0.5 + math.ldexp(1.0, -(a + 1))
        self.cE = self.cx / d
        self.g = 1.0 - 1.0 / d
        self.fluid = fluid_mask(nx, ny, si, jm)
        pad = np.zeros((ny + 2, nx + 2), dtype=bool)  # present: inside the grid and fluid
        pad[1:-1, 1:-1] = self.fluid
        self.present = pad
        self.w = pad[1:-1, :-2]
        self.e = np.broadcast_to((np.arange(1, nx + 1) < nx)[None, :], (ny, nx))  # (east of a fluid cell: fluid)
        self.s = np.broadcast_to((np.arange(1, ny + 1) > 1)[:, None], (ny, nx))  # (south of a fluid cell: fluid)
        self.n = pad[2:, 1:-1]
        cw = np.where(self.w, self.cx, 0.0)
        ce = np.where(self.e, self.cx, self.cE)
        cs = np.where(self.s, self.cy, 0.0)
        cn = np.where(self.n, self.cy, 0.0)
        self.A = (jm, si)  # (jm+1, si+1) as an index of the (ny, nx) interior arrays
        self.B = (jm - 1, si - 1)  # (jm, si)
        if couple:
            cw = cw.copy()
            cn = cn.copy()
            cw[self.A] = self.chx
            cn[self.B] = self.chy
        self.rdiag = 1.0 / ((cw + ce) + (cs + cn))  # (ny, nx)
        m = max(nx, ny)
        self.omega = 2.0 / (1.0 + math.sin(math.pi / (m + 1)))
        self.one_m_omega = 1.0 - self.omega
        self.omr = self.omega * self.rdiag
        self.coarse_sweeps = 4 * m
        ii = np.arange(1, nx + 1)[None, :]
        jj = np.arange(1, ny + 1)[:, None]
        self.colour = [self.fluid & (((ii + jj) & 1) == c) for c in (0, 1)]  # colour 0: i + j even (the oracle's red)


def _update(L: Level, p: np.ndarray, f: np.ndarray, sor: bool) -> np.ndarray:
    """The update of every interior cell from p as it stands (solid cells: unused values)."""
    c = p[1:-1, 1:-1]
    tE = np.where(L.e, L.cx * p[1:-1, 2:], 0.0)
    tW = np.where(L.w, L.cx * p[1:-1, :-2], 0.0)
    tN = np.where(L.n, L.cy * p[2:, 1:-1], 0.0)
    tS = np.where(L.s, L.cy * p[:-2, 1:-1], 0.0)
    if L.couple:
        tW[L.A] = L.chx * c[L.B]
        tN[L.B] = L.chy * c[L.A]
    s = ((tE + tW) + (tN + tS)) - f[1:-1, 1:-1]
    return c * L.one_m_omega + L.omr * s if sor else L.rdiag * s


def _half_sweep(L: Level, p: np.ndarray, f: np.ndarray, colour: int, sor: bool, pair_gs: bool = False) -> None:
    sel = L.colour[colour]
    with np.errstate(all="ignore"):
        new = _update(L, p, f, sor)
        p[1:-1, 1:-1][sel] = new[sel]
        if pair_gs and L.couple and sel[L.A]:  # the degraded variant: B again, from A's new value
            p[1:-1, 1:-1][L.B] = _update(L, p, f, sor)[L.B]


def sweep(L: Level, p: np.ndarray, f: np.ndarray, sor: bool = False, pair_gs: bool = False) -> None:
    """One red-black sweep over the fluid cells: colour 0 (i + j even), then colour 1."""
    _half_sweep(L, p, f, 0, sor, pair_gs)
    _half_sweep(L, p, f, 1, sor, pair_gs)


def residual(L: Level, p: np.ndarray, f: np.ndarray) -> np.ndarray:
    """(ny, nx) residual of the level operator: sum of coef (nb - c), minus f; 0 in solid cells."""
    c = p[1:-1, 1:-1]
    with np.errstate(all="ignore"):
        tE = np.where(L.e, L.cx * (p[1:-1, 2:] - c), L.cE * (0.0 - c))
        tW = np.where(L.w, L.cx * (p[1:-1, :-2] - c), 0.0)
        tN = np.where(L.n, L.cy * (p[2:, 1:-1] - c), 0.0)
        tS = np.where(L.s, L.cy * (p[:-2, 1:-1] - c), 0.0)
        if L.couple:
            tW[L.A] = L.chx * (c[L.B] - c[L.A])
            tN[L.B] = L.chy * (c[L.A] - c[L.B])
        r = ((tE + tW) + (tN + tS)) - f[1:-1, 1:-1]
    return np.where(L.fluid, r, 0.0)


def restrict(r: np.ndarray, kind: int, Lc: Level) -> np.ndarray:
    """The coarse source, ghosts and solid cells zero, from the fine interior residual."""
    fc = np.zeros((Lc.ny + 2, Lc.nx + 2))
    if kind == FULL:
        v = -0.25 * ((r[0::2, 0::2] + r[0::2, 1::2]) + (r[1::2, 0::2] + r[1::2, 1::2]))
    elif kind == X_ONLY:
        v = -0.5 * (r[:, 0::2] + r[:, 1::2])
    else:
        v = -0.5 * (r[0::2, :] + r[1::2, :])
    fc[1:-1, 1:-1] = np.where(Lc.fluid, v, 0.0)
    return fc


def _corr(Lc: Level, e: np.ndarray, kind: int, dj: int, di: int) -> np.ndarray:
    """(ny_c, nx_c) correction of each coarse cell's child on the side (dj, di). A horizontal or
    vertical neighbour that is missing (solid, or beyond a Neumann side) takes the centre value c,
    the east ghost c g; a missing diagonal the H value if V is missing, else the V value if H is
    missing, else c; an east-ghost diagonal V' g."""
    ny, nx = Lc.ny, Lc.nx
    J = np.arange(1, ny + 1)[:, None]
    I = np.arange(1, nx + 1)[None, :]
    c = e[1:-1, 1:-1]
    pr = Lc.present
    Vp = pr[J + dj, I + 0 * di]
    V = np.where(Vp, e[J + dj, I + 0 * di], c)
    if kind == Y_ONLY:
        return (3.0 * c + V) * 0.25
    east = np.broadcast_to(I + di == nx + 1, c.shape)
    Hp = pr[J + 0 * dj, I + di]
    H = np.where(east, c * Lc.g, np.where(Hp, e[J + 0 * dj, I + di], c))
    if kind == X_ONLY:
        return (3.0 * c + H) * 0.25
    Dp = pr[J + dj, I + di]
    D = np.where(east, V * Lc.g, np.where(Dp, e[J + dj, I + di], np.where(~Vp, H, np.where(~Hp, V, c))))
    return (((9.0 * c + 3.0 * V) + 3.0 * H) + D) * 0.0625


def prolong_add(L: Level, Lc: Level, p: np.ndarray, e: np.ndarray, kind: int) -> None:
    """p += interpolant of the coarse e (cell-centred) on the fluid cells: bilinear, or linear in the halved direction."""
    add = np.zeros((L.ny, L.nx))
    if kind == FULL:
        add[0::2, 0::2] = _corr(Lc, e, kind, -1, -1)
        add[0::2, 1::2] = _corr(Lc, e, kind, -1, 1)
        add[1::2, 0::2] = _corr(Lc, e, kind, 1, -1)
        add[1::2, 1::2] = _corr(Lc, e, kind, 1, 1)
    elif kind == X_ONLY:
        add[:, 0::2] = _corr(Lc, e, kind, 0, -1)
        add[:, 1::2] = _corr(Lc, e, kind, 0, 1)
    else:
        add[0::2, :] = _corr(Lc, e, kind, -1, 0)
        add[1::2, :] = _corr(Lc, e, kind, 1, 0)
    c = p[1:-1, 1:-1]
    c[L.fluid] = (c + add)[L.fluid]


def vcycle(levels, kd, l: int, p: np.ndarray, f: np.ndarray, nu1: int, nu2: int, pair_gs: bool = False) -> None:
    L = levels[l]
    if l == len(levels) - 1:
        for _ in range(L.coarse_sweeps):
            sweep(L, p, f, sor=True, pair_gs=pair_gs)
        return
    for _ in range(nu1):
        sweep(L, p, f, pair_gs=pair_gs)
    fc = restrict(residual(L, p, f), kd[l], levels[l + 1])
    e = np.zeros_like(fc)
    vcycle(levels, kd, l + 1, e, fc, nu1, nu2, pair_gs)
    prolong_add(L, levels[l + 1], p, e, kd[l])
    for _ in range(nu2):
        sweep(L, p, f, pair_gs=pair_gs)


def make_levels(nx, ny, dx, dy, si, jm, semi: bool = True, couple: bool = True):
    if not geometry_ok(ny, si, jm):
        raise ValueError(f"step_i {si}, inlet_jmax {jm} on {ny} rows: geometry rule")
    pl = plan_levels(nx, ny, dx, dy, si, jm, semi)
    if pl is None:
        raise ValueError(f"{nx}x{ny} has no valid multigrid plan")
    return [Level(n, m, a, b, s, j, dx, dy, couple) for n, m, a, b, s, j in pl], kinds(pl)


def refresh(p: np.ndarray, si: int, jm: int) -> None:
    """backwards_step-01.cpp:685-740 in its order: west and east columns, south and north rows
    (corners untouched), then every solid cell with fluid neighbours: the block's face row
    (0 + south), its corner ((0 + east) + south) / 2, its face column (0 + east)."""
    p[1:-1, 0] = p[1:-1, 1]
    p[1:-1, -1] = 0.0
    p[0, 1:-1] = p[1, 1:-1]
    p[-1, 1:-1] = p[-2, 1:-1]
    jb = jm + 1
    p[jb, 1:si] = 0.0 + p[jm, 1:si]
    p[jb, si] = ((0.0 + p[jb, si + 1]) + p[jm, si]) / 2
    p[jb + 1:-1, si] = 0.0 + p[jb + 1:-1, si + 1]


def residual_reference(p: np.ndarray, f: np.ndarray, dx: float, dy: float, si: int, jm: int) -> np.ndarray:
    """backwards_step-01.cpp:916-930 on the cells as stored: 0 in solid cells."""
    idx2, idy2 = 1.0 / (dx * dx), 1.0 / (dy * dy)
    c = p[1:-1, 1:-1]
    lap = ((p[1:-1, 2:] - 2.0 * c) + p[1:-1, :-2]) * idx2 + ((p[2:, 1:-1] - 2.0 * c) + p[:-2, 1:-1]) * idy2
    return np.where(fluid_mask(p.shape[1] - 2, p.shape[0] - 2, si, jm), lap - f[1:-1, 1:-1], 0.0)


def tolerance(f: np.ndarray, tol_factor: float, abs_tol: float, si: int, jm: int) -> float:
    fl = fluid_mask(f.shape[1] - 2, f.shape[0] - 2, si, jm)
    m = float(np.abs(f[1:-1, 1:-1][fl]).max())
    return max(tol_factor * (m if m > 0 else 1.0), abs_tol)


def solve(f, p0, dx, dy, si, jm, tol_factor: float = 1e-7, abs_tol: float = 0.0, nu1: int = 2, nu2: int = 2,
          max_cycles: int = 50, semi: bool = True, couple: bool = True, pair_gs: bool = False):
    """The solve loop (backwards_step-01.cpp:872-939 with a V-cycle for the sweep): a warm start
    from p0, the loop primed with tol + 1, ghosts and solids refreshed after each cycle, the stop
    test on the reference's own residual. Returns (cycles, residual, p, history of max|r|)."""
    ny, nx = f.shape[0] - 2, f.shape[1] - 2
    levels, kd = make_levels(nx, ny, dx, dy, si, jm, semi, couple)
    f = np.ascontiguousarray(f, dtype=np.float64)
    p = np.array(p0, dtype=np.float64, order="C", copy=True)
    tol = tolerance(f, tol_factor, abs_tol, si, jm)
    res, cycles, hist = tol + 1.0, 0, []
    while res > tol and cycles < max_cycles:
        vcycle(levels, kd, 0, p, f, nu1, nu2, pair_gs)
        refresh(p, si, jm)
        res = float(np.abs(residual_reference(p, f, dx, dy, si, jm)).max())
        cycles += 1
        hist.append(res)
    return cycles, res, p, hist


def solve_case(cp, f, p0, **kw):
    """solve() with a CaseParams' spacings, geometry and tolerances."""
    return solve(f, p0, cp.dx, cp.dy, cp.step_i, cp.inlet_jmax, cp.tol_factor, cp.abs_tol, **kw)


def tail(pl) -> int:
    """The first level of the one-launch tail (the cavity plan's rule)."""
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
    prolongation; then the tail, the ghost and solid refresh and the residual pass."""
    per_level = smoothing_launches(nu1, fused) + smoothing_launches(nu2, fused) + 2
    return tail(pl) * per_level + 3


def oracle_step(o, cp, **mg_opts):
    """One timestep of the oracle `o` in the open cases' phase order with solve() in place of
    its SOR loop, warm-started from the oracle's own p: returns (cycles, residual)."""
    o.tentative()
    o.velocity_bc(True)
    o.source()
    cycles, res, p, _ = solve_case(cp, o.field("src"), o.field("p"), **mg_opts)
    o.field("p")[...] = p
    o.correct()
    o.velocity_bc(False)
    return cycles, res


def dense_operator(nx, ny, dx, dy, si, jm) -> np.ndarray:
    """The level-0 operator as a matrix over the fluid cells in row-major order, column by
    column from the pinned residual (residual_reference after refresh) with a zero source:
    not from this file's Level."""
    fl = fluid_mask(nx, ny, si, jm)
    idx = np.argwhere(fl)
    n = len(idx)
    A = np.empty((n, n))
    z = np.zeros((ny + 2, nx + 2))
    for k, (j, i) in enumerate(idx):
        p = np.zeros_like(z)
        p[1 + j, 1 + i] = 1.0
        refresh(p, si, jm)
        A[:, k] = residual_reference(p, z, dx, dy, si, jm)[fl]
    return A


def direct_solve(f, dx, dy, si, jm, refinements: int = 5):
    """A x = f over the fluid cells of level 0 without multigrid: a dense float64 solve refined
    with np.longdouble residuals. Returns (x as a (ny+2, nx+2) field, solid cells zero before the
    refresh, ||A^-1||_inf, max|f - A x| of the refined x in long double)."""
    ny, nx = f.shape[0] - 2, f.shape[1] - 2
    fl = fluid_mask(nx, ny, si, jm)
    A = dense_operator(nx, ny, dx, dy, si, jm)
    Ainv = np.linalg.inv(A)
    b = np.ascontiguousarray(f[1:-1, 1:-1], dtype=np.float64)[fl]
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    x = (Ainv @ b).astype(np.longdouble)
    for _ in range(refinements):
        r = bl - Al @ x
        x = x + (Ainv @ r.astype(np.float64)).astype(np.longdouble)
    rmax = float(np.abs(bl - Al @ x).max())
    out = np.zeros_like(f, dtype=np.float64)
    out[1:-1, 1:-1][fl] = x.astype(np.float64)
    refresh(out, si, jm)
    return out, float(np.abs(Ainv).sum(axis=1).max()), rmax


def yardstick_bound(f, dx, dy, p, res, ainv_norm, si, jm) -> float:
    """mg_reference.yardstick_bound's statement with the step's coefficients, over the fluid cells:
    max|p - x| <= ||A^-1||_inf (res + 48 u max(idx2, idy2) max|p| + u max|f|), u = 2^-53."""
    u = 2.0 ** -53
    c = max(1.0 / (dx * dx), 1.0 / (dy * dy))
    fl = fluid_mask(f.shape[1] - 2, f.shape[0] - 2, si, jm)
    return ainv_norm * (res + 48.0 * u * c * float(np.abs(p[1:-1, 1:-1][fl]).max()) +
                        u * float(np.abs(f[1:-1, 1:-1][fl]).max()))


def random_source(nx, ny, si, jm, seed: int) -> np.ndarray:
    """A random source, zero in the ghosts and the solid, its mean over the fluid cells removed."""
    rng = np.random.default_rng(seed)
    fl = fluid_mask(nx, ny, si, jm)
    f = np.zeros((ny + 2, nx + 2))
    r = rng.standard_normal((ny, nx))
    f[1:-1, 1:-1] = np.where(fl, r - r[fl].mean(), 0.0)
    return f


def random_field(nx: int, ny: int, seed: int) -> np.ndarray:
    """A random p, solid cells and ghosts included."""
    return np.random.default_rng(seed).standard_normal((ny + 2, nx + 2))
