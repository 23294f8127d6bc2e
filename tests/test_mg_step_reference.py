"""The backwards-facing step's multigrid scheme restated in numpy
(tests/mg_step_reference.py) on the CPU: the library's host-only plan
(cfd_mg_step_plan) follows the rule and names the rule it refuses by, the
level-0 operator with the eliminated corner is the reference's loop after the
reference's refresh, the scheme converges within the cycle cap on every GPU
fixture, the corner coupling and the semi-coarsening are what make it converge,
the pair rule is visible in the bits, and a dense solve of the reference's
equations agrees with it."""
from __future__ import annotations

import types

import numpy as np
import pytest

import cfd_amd as C
import mg_step_reference as M
import oracle as O

CYCLE_CAP = 20  # a condition, not a measurement (measured: 6-13)

# (grid, every level) with the reference's geometry (step_x = 2 of 8, h_inlet = 1 of 2)
PLANS = {
    (256, 32): [(256, 32), (128, 32), (64, 16), (32, 8), (16, 4)],
    (8192, 512): [(8192, 512), (4096, 512), (2048, 512), (1024, 256), (512, 128), (256, 64), (128, 32), (64, 16),
                  (32, 8), (16, 4)],
    (48, 16): [(48, 16), (24, 8), (12, 4)],
    (16, 8): [(16, 8), (16, 4)],
    (24, 8): [(24, 8), (12, 4)],
    (480, 112): [(480, 112), (240, 56), (120, 28), (60, 14)],
    (496, 120): [(496, 120), (248, 60), (124, 30)],
    (464, 104): [(464, 104), (232, 52), (116, 26)],
    # the rule gives 250x32 a two-level plan: x once (step_i 62 -> 31), then 125 is odd; 4000 cells <= 4096
    (250, 32): [(250, 32), (125, 32)],
}
# every fixture of tests/test_gpu_multigrid_step.py: (nx, ny, (nu1, nu2))
GPU_FIXTURES = [(16, 8, (2, 2)), (24, 8, (2, 2)), (48, 16, (2, 2)), (64, 32, (2, 2)), (96, 24, (2, 2)),
                (256, 32, (2, 2)), (512, 64, (2, 2)), (480, 112, (2, 2)), (496, 120, (1, 1)), (464, 104, (3, 3)),
                (464, 112, (2, 2)), (496, 112, (2, 2)), (480, 112, (4, 1)), (480, 112, (1, 4))]
YARDSTICK_GRIDS = [(16, 8), (24, 8), (48, 16)]


def step(nx, ny):
    return C.make_params("backwards_step", nx=nx, ny=ny)


def fixture(nx, ny):
    cp = step(nx, ny)
    return cp, M.random_source(nx, ny, cp.step_i, cp.inlet_jmax, seed=nx * 1000 + ny)


def variant(nx, ny, step_x=None, h_inlet=None):
    cp = step(nx, ny)
    if step_x is not None:
        cp.step_x = step_x
    if h_inlet is not None:
        cp.h_inlet = h_inlet
    return cp


@pytest.mark.parametrize("grid", sorted(PLANS))
def test_plan_is_the_rule(grid):
    cp = step(*grid)
    assert (cp.dx, cp.dy) == (8.0 / grid[0], 2.0 / grid[1])
    assert C.mg_step_plan(cp) == PLANS[grid]
    assert M.plan_of(cp) == PLANS[grid]


def test_plan_geometry_per_level():
    lv = M.plan_levels(256, 32, 8.0 / 256, 2.0 / 32, 64, 16)
    assert [(l[4], l[5]) for l in lv] == [(64, 16), (32, 16), (16, 8), (8, 4), (4, 2)]
    assert M.kinds(lv) == [M.X_ONLY, M.FULL, M.FULL, M.FULL]
    cp = step(8192, 512)
    lv = M.plan_levels(cp.nx, cp.ny, cp.dx, cp.dy, cp.step_i, cp.inlet_jmax)
    assert M.kinds(lv) == [M.X_ONLY, M.X_ONLY] + [M.FULL] * 7 and (lv[-1][4], lv[-1][5]) == (4, 2)
    assert M.kinds(M.plan_levels(16, 8, 0.5, 0.25, 4, 4)) == [M.Y_ONLY]
    cp = step(480, 112)
    assert M.plan_levels(cp.nx, cp.ny, cp.dx, cp.dy, cp.step_i, cp.inlet_jmax)[-1][4] == 15


def test_plan_refusals():
    for cp, rule in [(step(472, 108), "grid rule"),  # coarsest 236x54: 12744 cells
                     (step(488, 116), "grid rule"),  # coarsest 244x58
                     (variant(64, 32, step_x=0.2), "geometry rule"),  # step_i = 1
                     (variant(40, 10, h_inlet=1.9), "geometry rule"),  # inlet_jmax = ny - 1
                     (C.make_params("cavity", nx=64, ny=64), "case rule"),
                     (C.make_params("rayleigh_benard", nx=128, ny=32), "case rule"),
                     (C.make_params("channel", nx=96, ny=32), "case rule")]:
        with pytest.raises(C._lib.CfdError, match=rule) as e:
            C.mg_step_plan(cp)
        assert "(-1)" in str(e.value)  # CFD_E_ARG
    assert variant(64, 32, step_x=0.2).step_i == 1
    v = variant(40, 10, h_inlet=1.9)
    assert v.inlet_jmax == v.ny - 1
    assert M.plan_of(step(472, 108)) is None and M.plan_of(step(488, 116)) is None
    assert not M.geometry_ok(32, 1, 16) and not M.geometry_ok(10, 10, 9) and M.geometry_ok(32, 64, 16)
    # the other cases are pointed to their methods
    with pytest.raises(C._lib.CfdError, match="CFD_POISSON_MULTIGRID.*CFD_POISSON_MULTIGRID_OPEN"):
        C.mg_step_plan(C.make_params("cavity", nx=64, ny=64))
    # methods 1 and 2 keep refusing the step, and name the new method
    with pytest.raises(C._lib.CfdError, match="case rule.*CFD_POISSON_MULTIGRID_STEP"):
        C.mg_plan(step(256, 32))
    with pytest.raises(C._lib.CfdError, match="case rule.*CFD_POISSON_MULTIGRID_STEP"):
        C.mg_open_plan(step(256, 32))


def test_plan_null_pointers():
    import ctypes
    cp = C.to_cparams(step(256, 32))
    L = C._lib.lib()
    assert L.cfd_mg_step_plan(ctypes.byref(cp), None, None, None) == 0
    lv = ctypes.c_int()
    assert L.cfd_mg_step_plan(ctypes.byref(cp), ctypes.byref(lv), None, None) == 0 and lv.value == 5
    assert C._lib.POISSON["multigrid-step"] == 3


def oracle_proxy(cp):
    return types.SimpleNamespace(**{k: getattr(cp, k) for k in (
        "case_id", "nx", "ny", "dx", "dy", "nu", "rho", "u_ref", "dt", "tol_factor", "abs_tol", "max_iters",
        "step_i", "inlet_jmax", "length")}, omega=0.0)


@pytest.mark.parametrize("nx,ny", [(48, 16), (64, 32), (24, 8)])
def test_level0_residual_is_the_reference_loop(nx, ny):
    """One oracle iteration with omega = 0 leaves the fluid cells as they are, refreshes the ghosts
    and the solids (backwards_step-01.cpp:685-740) and evaluates 916-930: the restatement's refresh
    and stop residual are those, bit for bit - the stale ghosts beside the face cells included."""
    cp = step(nx, ny)
    si, jm = cp.step_i, cp.inlet_jmax
    rng = np.random.default_rng(nx + 7 * ny)
    p = rng.standard_normal((ny + 2, nx + 2))
    f = rng.standard_normal((ny + 2, nx + 2))
    for ordering in (O.LEX, O.RB):
        o = O.Oracle(oracle_proxy(cp), ordering=ordering)
        o.field("p")[...] = p
        o.field("src")[...] = f
        omax = o.poisson_fixed(1)
        mine = p.copy()
        M.refresh(mine, si, jm)
        assert np.array_equal(o.field("p").view(np.int64), mine.view(np.int64))
        r = M.residual_reference(mine, f, cp.dx, cp.dy, si, jm)
        assert np.array_equal(o.field("res")[1:-1, 1:-1].view(np.int64), r.view(np.int64))
        assert float(np.abs(r).max()) == omax


@pytest.mark.parametrize("nx,ny", [(48, 16), (64, 32)])
def test_level_operator_is_the_reference_operator_at_level_0(nx, ny):
    """The cycle's own residual form - the corner solid eliminated into A's west and B's north
    term - states the same operator as the reference's after its refresh: equal to rounding.
    Without the coupling it does not."""
    cp = step(nx, ny)
    si, jm = cp.step_i, cp.inlet_jmax
    rng = np.random.default_rng(3)
    p, f = rng.standard_normal((ny + 2, nx + 2)), rng.standard_normal((ny + 2, nx + 2))
    L = M.Level(nx, ny, 0, 0, si, jm, cp.dx, cp.dy)
    assert L.cE == L.cx and L.g == 0.0
    a = M.residual(L, p, f)
    a0 = M.residual(M.Level(nx, ny, 0, 0, si, jm, cp.dx, cp.dy, couple=False), p, f)
    M.refresh(p, si, jm)
    b = M.residual_reference(p, f, cp.dx, cp.dy, si, jm)
    scale = 4.0 * (L.cx + L.cy) * np.abs(p).max()
    assert np.abs(a - b).max() <= 16 * 2.0 ** -53 * scale
    assert np.abs(a0 - b).max() > 1e-3 * scale
    assert not a[~L.fluid].any() and not b[~L.fluid].any()


def test_solids_and_ghosts_reach_no_result():
    cp, f = fixture(96, 24)
    si, jm = cp.step_i, cp.inlet_jmax
    fl = M.fluid_mask(96, 24, si, jm)
    p0 = M.random_field(96, 24, 1)
    other = np.random.default_rng(2).standard_normal(p0.shape) * 1e6
    other[1:-1, 1:-1][fl] = p0[1:-1, 1:-1][fl]
    a = M.solve_case(cp, f, p0)
    b = M.solve_case(cp, f, other)
    assert a[:2] == b[:2]
    assert np.array_equal(a[2][1:-1, 1:-1][fl].view(np.int64), b[2][1:-1, 1:-1][fl].view(np.int64))
    interior = ~fl
    interior[jm, :] = False  # the face row (row jm + 1)
    interior[:, si - 1] = False  # the face column
    assert np.array_equal(b[2][1:-1, 1:-1][interior], other[1:-1, 1:-1][interior])  # never written


def converge(nx, ny, nu=(2, 2), warm=False, cap=CYCLE_CAP, **kw):
    cp, f = fixture(nx, ny)
    p0 = M.random_field(nx, ny, nx + ny) if warm else np.zeros_like(f)
    cycles, res, p, hist = M.solve_case(cp, f, p0, nu1=nu[0], nu2=nu[1], max_cycles=cap, **kw)
    tol = M.tolerance(f, cp.tol_factor, cp.abs_tol, cp.step_i, cp.inlet_jmax)
    print(f"{nx}x{ny} V{nu} warm={warm} {kw}: {cycles} cycles, residual / tol {res / tol:.3g}, "
          f"residuals {['%.2e' % h for h in hist]}")
    return cycles, res, tol


@pytest.mark.parametrize("nx,ny,nu", GPU_FIXTURES)
@pytest.mark.parametrize("warm", [False, True])
def test_converges_within_the_cap(nx, ny, nu, warm):
    cycles, res, tol = converge(nx, ny, nu, warm)
    assert res <= tol and cycles <= CYCLE_CAP


def test_custom_geometry_converges():
    cp = variant(128, 32, step_x=4.0, h_inlet=0.75)
    assert (cp.step_i, cp.inlet_jmax) == (64, 12)
    assert M.plan_of(cp) == C.mg_step_plan(cp) == [(128, 32), (64, 16), (32, 8)]  # (jm 12 -> 6 -> 3: odd)
    f = M.random_source(128, 32, 64, 12, 5)
    cycles, res, _, _ = M.solve_case(cp, f, np.zeros_like(f), max_cycles=CYCLE_CAP)
    assert res <= M.tolerance(f, cp.tol_factor, cp.abs_tol, 64, 12) and cycles <= CYCLE_CAP


def test_corner_coupling_matters():
    """Without the coupling in the operator the reference's residual stalls far above the
    tolerance: 256x32 is still above it after 30 cycles."""
    cycles, res, tol = converge(256, 32, cap=30, couple=False)
    assert cycles == 30 and res > 1e3 * tol
    cycles, res, tol = converge(256, 32)
    assert res <= tol


@pytest.mark.parametrize("nx,ny", [(512, 32), (64, 64)])
def test_semi_coarsening_matters(nx, ny):
    """r = (hy / hx)^2 = 16 (x first) and 1/16 (y first): full coarsening alone needs more than twice
    the cycles, or misses 40 (measured 30 against 10 and over 40 against 7)."""
    semi, res, tol = converge(nx, ny)
    assert res <= tol
    full, res, tol = converge(nx, ny, cap=40, semi=False)
    assert full > 2 * semi


def test_pair_rule_is_visible():
    """Gauss-Seidel inside the pair (B from A's new value) gives other bits: the tests see the order."""
    cp, f = fixture(48, 16)
    p0 = M.random_field(48, 16, 64)
    a = M.solve_case(cp, f, p0, max_cycles=1)
    b = M.solve_case(cp, f, p0, max_cycles=1, pair_gs=True)
    assert not np.array_equal(a[2].view(np.int64), b[2].view(np.int64))
    L = M.Level(48, 16, 0, 0, cp.step_i, cp.inlet_jmax, cp.dx, cp.dy)
    assert L.colour[0][L.A] == L.colour[0][L.B]  # one colour
    p, q = p0.copy(), p0.copy()
    M.sweep(L, p, f)
    M.sweep(L, q, f, pair_gs=True)
    d = (p != q)[1:-1, 1:-1]
    assert d[L.B] and not d[L.A]  # A is formed from the old B either way; B is not formed from the old A


@pytest.mark.parametrize("nx,ny", YARDSTICK_GRIDS)
def test_restatement_solves_the_reference_equations(nx, ny):
    """Independent of the scheme: the level-0 operator over the fluid cells assembled from the
    refresh and residual that test_level0_residual_is_the_reference_loop pins, solved densely and
    refined in long double; the restatement's p is within what its reported residual allows."""
    cp, f = fixture(nx, ny)
    si, jm = cp.step_i, cp.inlet_jmax
    fl = M.fluid_mask(nx, ny, si, jm)
    x, ainv, rmax = M.direct_solve(f, cp.dx, cp.dy, si, jm)
    cycles, res, p, _ = M.solve_case(cp, f, np.zeros_like(f))
    err = float(np.abs(p[1:-1, 1:-1] - x[1:-1, 1:-1])[fl].max())
    bound = M.yardstick_bound(f, cp.dx, cp.dy, p, res, ainv, si, jm)
    print(f"{nx}x{ny}: {cycles} cycles residual {res:.3e}; refined residual {rmax:.3e}; ||A^-1|| {ainv:.3e}; "
          f"max|p - x| {err:.3e} <= {bound:.3e}")
    assert res <= M.tolerance(f, cp.tol_factor, cp.abs_tol, si, jm) and cycles <= CYCLE_CAP
    assert rmax <= res * 1e-3  # x is exact against what p is held to
    assert err <= bound


def test_zero_source():
    cp = step(96, 24)
    f = np.zeros((26, 98))
    cycles, res, p, _ = M.solve_case(cp, f, np.zeros_like(f))
    assert (cycles, res) == (1, 0.0) and not p.any()
    p0 = M.random_field(96, 24, 4)
    cycles, res, p, _ = M.solve_case(cp, f, p0, max_cycles=1)
    assert cycles == 1 and res > 0 and not np.array_equal(p, p0)


def test_tail_and_launch_counts():
    pl = PLANS[(8192, 512)]
    assert M.tail(pl) == 6 and pl[6] == (128, 32)
    assert M.launches_per_cycle(pl, 2, 2, True) == 6 * 4 + 3  # the tail, the refresh, the residual pass
    assert M.launches_per_cycle(pl, 2, 2, False) == 6 * 10 + 3
    assert M.tail(M.plan_of(step(512, 64))) == 2
    assert M.tail(PLANS[(16, 8)]) == 1 and M.tail(PLANS[(480, 112)]) == 2


@pytest.mark.parametrize("nx,ny", [(256, 32), (96, 24)])
def test_oracle_step_converges_every_step(nx, ny):
    """The oracle's phases around the restatement's warm-started solve: every step within the cap,
    the ghosts and face cells the corrector reads are the reference's."""
    cp = C.make_params("backwards_step", nx=nx, ny=ny)
    si, jm = cp.step_i, cp.inlet_jmax
    o = O.Oracle(cp, ordering=O.LEX)
    o.velocity_bc(False)  # (the state the solver is created in)
    for k in range(4):
        cycles, res = M.oracle_step(o, cp)
        tol = M.tolerance(o.field("src"), cp.tol_factor, cp.abs_tol, si, jm)
        print(f"step {nx}x{ny} step {k + 1}: {cycles} cycles residual {res:.3e} (tol {tol:.3e})")
        assert res <= tol and cycles <= CYCLE_CAP
        p = o.field("p")
        assert np.array_equal(p[1:jm + 1, 0], p[1:jm + 1, 1]) and not p[1:-1, -1].any()
        assert np.array_equal(p[jm + 1, 1:si], p[jm, 1:si]) and np.array_equal(p[jm + 2:-1, si], p[jm + 2:-1, si + 1])
        assert p[jm + 1, si] == ((0.0 + p[jm + 1, si + 1]) + p[jm, si]) / 2
