"""The channel's multigrid scheme restated in numpy (tests/mg_open_reference.py) on
the CPU: the library's host-only plan (cfd_mg_open_plan) follows the
semi-coarsening rule, the level-0 stop residual is the reference's loop, the
scheme converges within the cycle cap on every fixture, the east-boundary
coefficient and the semi-coarsening are what make it converge that fast, and a
dense solve of the reference's equations agrees with it."""
from __future__ import annotations

import types

import numpy as np
import pytest

import cfd_amd as C
import mg_open_reference as M
import oracle as O

TOL_FACTOR = 1e-7
CYCLE_CAP = 20  # a condition, not a measurement (measured: 5-12, DESIGN.md §8 "The channel")

# (grid, every level) for Lx = 3, Ly = 1: x first at 4096x512 (idx2 / idy2 = 7.1), y first at 64^2
PLANS = {
    (4096, 512): [(4096, 512), (2048, 512), (1024, 256), (512, 128), (256, 64), (128, 32), (64, 16), (32, 8), (16, 4)],
    (512, 64): [(512, 64), (256, 64), (128, 32), (64, 16), (32, 8), (16, 4)],
    (64, 64): [(64, 64), (64, 32), (64, 16), (32, 8), (16, 4)],
    (240, 120): [(240, 120), (240, 60), (120, 30), (60, 15)],
    (96, 32): [(96, 32), (48, 16), (24, 8), (12, 4)],
    (512, 16): [(512, 16), (256, 16), (128, 16), (64, 16), (32, 8), (16, 4)],
    (8, 1024): [(8, 1024), (8, 512), (8, 256), (8, 128), (8, 64), (8, 32), (8, 16), (8, 8), (8, 4)],
    (30, 18): [(30, 18), (30, 9)],
}
# 126x90 (Lx = 3, Ly = 1) is in the fixture lists this scheme's tests were asked to cover, as a two-level plan.
# The rule gives it none: r = (hy / hx)^2 = 0.218 < 1/2 halves y only, 126x45 cannot be halved further (45 is
# odd) and holds 5670 > 4096 cells - a grid rule refusal, which test_plan_refusals pins here and
# test_gpu_multigrid_open.py on the device. 126x60 (-> 126x30, 3780 cells, 504 coarse sweeps) covers the
# two-level plan with a large coarsest level in its place.
CONVERGENCE_GRIDS = [(96, 32), (256, 32), (512, 64), (64, 64), (240, 120), (272, 144), (512, 512), (240, 112),
                     (512, 16), (16, 512), (1024, 8), (8, 1024), (8, 8), (30, 18), (126, 60)]
YARDSTICK_GRIDS = [(16, 16), (48, 16), (16, 48)]


def spacings(nx, ny):
    return 3.0 / nx, 1.0 / ny


def fixture(nx, ny):
    dx, dy = spacings(nx, ny)
    return M.random_source(nx, ny, seed=nx * 1000 + ny), dx, dy


def channel(nx, ny):
    return C.make_params("channel", nx=nx, ny=ny)


@pytest.mark.parametrize("grid", sorted(PLANS))
def test_plan_is_the_rule(grid):
    cp = channel(*grid)
    assert (cp.dx, cp.dy) == spacings(*grid)
    assert C.mg_open_plan(cp) == PLANS[grid]
    assert M.plan(*grid, cp.dx, cp.dy) == PLANS[grid]


def test_plan_kinds():
    X, Y, F = M.X_ONLY, M.Y_ONLY, M.FULL
    kd = lambda nx, ny: M.kinds(M.plan_levels(nx, ny, *spacings(nx, ny)))
    assert kd(4096, 512) == [X] + [F] * 7
    assert kd(512, 64) == [X] + [F] * 4
    assert kd(64, 64) == [Y, Y, F, F]
    assert kd(240, 120) == [Y, F, F]
    assert kd(96, 32) == [F] * 3
    assert kd(512, 16) == [X, X, X, F, F]
    assert kd(8, 1024) == [Y] * 8
    assert kd(30, 18) == [Y]


def test_plan_refusals():
    for cp, rule in [(C.make_params("channel"), "grid rule"),  # the reference's 93x31
                     (channel(126, 90), "grid rule"),  # 126x45: 5670 cells (see CONVERGENCE_GRIDS)
                     (C.make_params("cavity", nx=64, ny=64), "case rule"),
                     (C.make_params("rayleigh_benard", nx=128, ny=32), "case rule"),
                     (C.make_params("backwards_step"), "case rule")]:
        with pytest.raises(C._lib.CfdError, match=rule) as e:
            C.mg_open_plan(cp)
        assert "(-1)" in str(e.value)  # CFD_E_ARG
    with pytest.raises(C._lib.CfdError, match="CFD_POISSON_MULTIGRID"):  # the cavity is pointed to method 1
        C.mg_open_plan(C.make_params("cavity", nx=64, ny=64))
    assert M.plan(93, 31, *spacings(93, 31)) is None
    assert M.plan(126, 90, *spacings(126, 90)) is None
    with pytest.raises(C._lib.CfdError, match="case rule"):  # method 1's plan still refuses the channel
        C.mg_plan(channel(64, 64))


def test_plan_null_pointers():
    import ctypes
    cp = C.to_cparams(channel(96, 32))
    L = C._lib.lib()
    assert L.cfd_mg_open_plan(ctypes.byref(cp), None, None, None) == 0
    lv = ctypes.c_int()
    assert L.cfd_mg_open_plan(ctypes.byref(cp), ctypes.byref(lv), None, None) == 0 and lv.value == 4


@pytest.mark.parametrize("nx,ny", [(48, 16), (16, 48)])
def test_level0_residual_is_the_reference_loop(nx, ny):
    """One oracle iteration with omega = 0 leaves p as it is, refreshes the ghosts
    (channel-01.cpp:531-541) and evaluates channel-01.cpp:672-681: the restatement's
    refresh and stop residual are those, bit for bit."""
    cp = channel(nx, ny)
    proxy = types.SimpleNamespace(**{k: getattr(cp, k) for k in (
        "case_id", "nx", "ny", "dx", "dy", "nu", "rho", "u_ref", "dt", "tol_factor", "abs_tol", "max_iters",
        "step_i", "inlet_jmax", "length")}, omega=0.0)
    rng = np.random.default_rng(nx + 7 * ny)
    p = rng.standard_normal((ny + 2, nx + 2))
    f = rng.standard_normal((ny + 2, nx + 2))
    for ordering in (O.LEX, O.RB):
        o = O.Oracle(proxy, ordering=ordering)
        o.field("p")[...] = p
        o.field("src")[...] = f
        omax = o.poisson_fixed(1)
        mine = p.copy()
        M.refresh_ghosts(mine)
        assert np.array_equal(o.field("p").view(np.int64), mine.view(np.int64))
        r = M.residual_reference(mine, f, cp.dx, cp.dy)
        assert np.array_equal(o.field("res")[1:-1, 1:-1].view(np.int64), r.view(np.int64))
        assert float(np.abs(r).max()) == omax


def test_level_operator_is_the_reference_operator_at_level_0():
    """The cycle's own residual form (sum of coef (nb - c), selects for absent neighbours)
    states the same operator as the reference's on refreshed ghosts: equal to rounding."""
    nx, ny = 48, 16
    dx, dy = spacings(nx, ny)
    rng = np.random.default_rng(3)
    p, f = rng.standard_normal((ny + 2, nx + 2)), rng.standard_normal((ny + 2, nx + 2))
    L = M.Level(nx, ny, 0, 0, dx, dy)
    assert L.cE == L.cx and L.g == 0.0
    a = M.residual(L, p, f)
    M.refresh_ghosts(p)
    b = M.residual_reference(p, f, dx, dy)
    scale = 4.0 * (L.cx + L.cy) * np.abs(p).max()
    assert np.abs(a - b).max() <= 16 * 2.0 ** -53 * scale


def test_ghosts_reach_no_result():
    f, dx, dy = fixture(96, 32)
    p0 = M.random_field(96, 32, 1)
    other = p0.copy()
    g = np.random.default_rng(2).standard_normal(p0.shape) * 1e6
    other[0, :], other[-1, :], other[:, 0], other[:, -1] = g[0, :], g[-1, :], g[:, 0], g[:, -1]
    a = M.solve(f, p0, dx, dy, TOL_FACTOR)
    b = M.solve(f, other, dx, dy, TOL_FACTOR)
    assert a[:2] == b[:2]
    assert np.array_equal(a[2][1:-1, 1:-1].view(np.int64), b[2][1:-1, 1:-1].view(np.int64))


def converge(nx, ny, nu=(2, 2), warm=False, cap=CYCLE_CAP, **kw):
    f, dx, dy = fixture(nx, ny)
    p0 = M.random_field(nx, ny, nx + ny) if warm else np.zeros_like(f)
    cycles, res, p, hist = M.solve(f, p0, dx, dy, TOL_FACTOR, 0.0, nu[0], nu[1], cap, **kw)
    tol = M.tolerance(f, TOL_FACTOR, 0.0)
    print(f"{nx}x{ny} V{nu} warm={warm} {kw}: {cycles} cycles, residual / tol {res / tol:.3g}, "
          f"residuals {['%.2e' % h for h in hist]}")
    return cycles, res, tol


@pytest.mark.parametrize("nx,ny", CONVERGENCE_GRIDS)
def test_converges_within_the_cap(nx, ny):
    cycles, res, tol = converge(nx, ny)
    assert res <= tol and cycles <= CYCLE_CAP


@pytest.mark.parametrize("nx,ny,nu,warm", [(248, 120, (1, 1), False), (232, 104, (3, 3), False),
                                           (240, 120, (4, 1), False), (240, 120, (1, 4), False),
                                           (240, 120, (2, 2), True)])
def test_converges_within_the_cap_options(nx, ny, nu, warm):
    cycles, res, tol = converge(nx, ny, nu, warm)
    assert res <= tol and cycles <= CYCLE_CAP


def test_unit_east_coefficient_misses_the_cap():
    """cE = cx on every level (the coarse levels' zero at their own ghost centre) must
    fail where the scheme passes: the test sees the east boundary's treatment."""
    cycles, res, tol = converge(512, 64, unit_east=True)
    assert cycles == CYCLE_CAP and not res <= tol


@pytest.mark.parametrize("nx,ny", [(512, 64), (64, 64)])
def test_semi_coarsening_matters(nx, ny):
    semi, res, tol = converge(nx, ny)
    assert res <= tol
    full, res, tol = converge(nx, ny, cap=30, semi=False)
    assert res <= tol and full <= 30
    assert full > semi


@pytest.mark.parametrize("nx,ny", YARDSTICK_GRIDS)
def test_restatement_solves_the_reference_equations(nx, ny):
    """Independent of the scheme: the level-0 operator assembled from the residual that
    test_level0_residual_is_the_reference_loop pins, solved densely and refined in long
    double; the restatement's p is within what its reported residual allows."""
    f, dx, dy = fixture(nx, ny)
    x, ainv, rmax = M.direct_solve(f, dx, dy)
    cycles, res, p, _ = M.solve(f, np.zeros_like(f), dx, dy, TOL_FACTOR)
    err = float(np.abs(p[1:-1, 1:-1] - x[1:-1, 1:-1]).max())
    bound = M.yardstick_bound(f, dx, dy, p, res, ainv)
    print(f"{nx}x{ny}: {cycles} cycles residual {res:.3e}; refined residual {rmax:.3e}; ||A^-1|| {ainv:.3e}; "
          f"max|p - x| {err:.3e} <= {bound:.3e}")
    assert res <= M.tolerance(f, TOL_FACTOR, 0.0) and cycles <= CYCLE_CAP
    assert rmax <= res * 1e-3  # x is exact against what p is held to
    assert err <= bound


def test_zero_source():
    """tol = max(tol_factor * 1, abs_tol); the loop is primed with tol + 1, so one cycle
    runs: from a zero field it leaves zeros, from a warm field it smooths it."""
    f = np.zeros((34, 98))
    dx, dy = spacings(96, 32)
    cycles, res, p, _ = M.solve(f, np.zeros_like(f), dx, dy, TOL_FACTOR, 1e-10)
    assert (cycles, res) == (1, 0.0) and not p.any()
    p0 = M.random_field(96, 32, 4)
    cycles, res, p, _ = M.solve(f, p0, dx, dy, TOL_FACTOR, 1e-10, max_cycles=1)
    assert cycles == 1 and res > 0 and not np.array_equal(p, p0)


def test_tail_and_launch_counts():
    pl = M.plan(4096, 512, *spacings(4096, 512))
    assert M.tail(pl) == 5 and pl[5] == (128, 32)
    assert M.launches_per_cycle(pl, 2, 2, True) == 5 * 4 + 3  # the tail, the ghost refresh, the residual pass
    assert M.launches_per_cycle(pl, 2, 2, False) == 5 * 10 + 3
    assert M.tail(M.plan(240, 120, *spacings(240, 120))) == 2
    assert M.tail(M.plan(30, 18, *spacings(30, 18))) == 1


@pytest.mark.parametrize("nx,ny", [(96, 32), (240, 120)])
def test_oracle_step_converges_every_step(nx, ny):
    """The oracle's phases around the restatement's warm-started solve: every step
    within the cap, the ghosts the corrector reads are the reference's."""
    cp = C.make_params("channel", re=100.0, nx=nx, ny=ny)
    o = O.Oracle(cp, ordering=O.LEX)
    o.velocity_bc(False)  # (the state the solver is created in)
    for k in range(4):
        cycles, res = M.oracle_step(o, cp)
        tol = M.tolerance(o.field("src"), cp.tol_factor, cp.abs_tol)
        print(f"channel {nx}x{ny} step {k + 1}: {cycles} cycles residual {res:.3e} (tol {tol:.3e})")
        assert res <= tol and cycles <= CYCLE_CAP
        p = o.field("p")
        assert np.array_equal(p[1:-1, 0], p[1:-1, 1]) and not p[1:-1, -1].any()
        assert np.array_equal(p[0, 1:-1], p[1, 1:-1]) and np.array_equal(p[-1, 1:-1], p[-2, 1:-1])
