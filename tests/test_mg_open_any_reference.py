"""The channel's any-size multigrid scheme's numpy restatement
(tests/mg_open_any_reference.py) on the CPU: its plans and the library's
host-only plan (cfd_mg_open_any_plan, cfd_mg_open_any_level) agree to the bit,
the level widths add up to the finest grid, its level-0 residual is the
reference's on an odd grid, it is mg_open_reference where that has the same
plan, its bits do not depend on the incoming ghost cells, the east coefficient
matters, it converges on odd and other irregular grids in at most one cycle
more than mg_open_reference on the regular grid beside them, and a dense solve
of the reference's equations bounds its p."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import cfd_amd as C
import mg_open_any_reference as A
import mg_open_reference as M

TOL_FACTOR = 1e-7
CYCLE_CAP = 20  # test_mg_open_reference's

PLANS = {
    (93, 31): [(93, 31), (47, 16), (24, 8), (12, 4)],
    (50, 17): [(50, 17), (25, 9), (13, 5)],
    (13, 9): [(13, 9), (13, 5)],
    (17, 40): [(17, 40), (17, 20), (17, 10), (17, 5)],
    (1000, 100): [(1000, 100), (500, 100), (250, 100), (125, 50), (63, 25), (32, 13), (16, 7)],
    (253, 131): [(253, 131), (253, 66), (127, 33), (64, 17), (32, 9), (16, 5)],
}
CONSTANT_GRIDS = [(93, 31), (50, 17), (17, 40), (13, 9), (253, 131), (1000, 100), (4095, 511), (4096, 512),
                  (126, 90), (96, 32), (31, 93)]
SAME_BITS_GRIDS = [(96, 32), (256, 32), (512, 64), (64, 64), (512, 16), (4096, 512)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def channel(nx, ny):
    return C.make_params("channel", nx=nx, ny=ny)


def spacings(nx, ny):
    cp = channel(nx, ny)
    return cp.dx, cp.dy


_FIX = {}


def fixture(nx, ny):
    """(random mean-free source, dx, dy), once per grid."""
    if (nx, ny) not in _FIX:
        _FIX[(nx, ny)] = (M.random_source(nx, ny, seed=nx * 1000 + ny), *spacings(nx, ny))
    return _FIX[(nx, ny)]


@pytest.mark.parametrize("nx,ny", sorted(PLANS))
def test_plans_listed(nx, ny):
    assert A.plan(nx, ny, *spacings(nx, ny)) == PLANS[(nx, ny)]
    assert C.mg_open_any_plan(channel(nx, ny)) == PLANS[(nx, ny)]


def test_plans_of_more_sizes():
    assert C._lib.POISSON["multigrid-open-any"] == 5
    for nx, ny in [(126, 90), (240, 120), (30, 18), (4000, 500), (3000, 1000), (4095, 511), (100, 20), (63, 500),
                   (999, 333), (241, 121)]:
        pl = A.plan(nx, ny, *spacings(nx, ny))
        assert pl is not None and min(pl[-1]) >= 4 and pl[-1][0] * pl[-1][1] <= 4096
        assert C.mg_open_any_plan(channel(nx, ny)) == pl
    assert C.mg_open_any_plan(channel(126, 90))[-1] == (16, 6)
    assert C.mg_open_any_plan(channel(240, 120))[-1] == (15, 4)  # (method 2 stops at 60 x 15)
    assert C.mg_open_any_plan(C.reference_defaults("channel")) == PLANS[(93, 31)]


@pytest.mark.parametrize("nx,ny", SAME_BITS_GRIDS)
def test_same_plan_as_method_2(nx, ny):
    assert C.mg_open_any_plan(channel(nx, ny)) == C.mg_open_plan(channel(nx, ny))
    for L in A.make_levels(nx, ny, *spacings(nx, ny)):  # every level regular in both directions
        assert not L.x.irregular and not L.y.irregular and not L.x.t_irregular and not L.y.t_irregular


@pytest.mark.parametrize("nx,ny", [(240, 120), (30, 18)])
def test_method_2_stops_on_an_odd_size_there(nx, ny):
    assert C.mg_open_any_plan(channel(nx, ny)) != C.mg_open_plan(channel(nx, ny))
    assert C.mg_open_any_plan(channel(nx, ny))[:len(C.mg_open_plan(channel(nx, ny)))] == C.mg_open_plan(channel(nx, ny))


def test_plan_refusals():
    for nx, ny in [(13, 5), (2, 2), (3, 2), (50, 3), (3, 50), (8, 600000)]:
        assert A.plan(nx, ny, *spacings(nx, ny)) is None
    for cp, rule in [(channel(13, 5), "grid rule"),        # one level
                     (channel(2, 2), "grid rule"),
                     (channel(3, 2), "grid rule"),
                     (channel(50, 3), "grid rule"),        # fewer than 4 cells in a direction
                     (channel(3, 50), "grid rule"),
                     (channel(8, 600000), "grid rule"),    # more than 16 levels
                     (C.make_params("cavity", nx=64, ny=64), "case rule"),
                     (C.make_params("cavity", nx=63, ny=63), "case rule"),
                     (C.make_params("rayleigh_benard", nx=128, ny=32), "case rule"),
                     (C.make_params("backwards_step"), "case rule")]:
        with pytest.raises(C._lib.CfdError, match=rule) as e:
            C.mg_open_any_plan(cp)
        assert "(-1)" in str(e.value)  # CFD_E_ARG
    with pytest.raises(C._lib.CfdError, match="CFD_POISSON_MULTIGRID_ANY.*CFD_POISSON_MULTIGRID_STEP"):
        C.mg_open_any_plan(C.make_params("cavity", nx=63, ny=63))  # pointed to methods 1 / 4 and 3
    # method 2's refusals stand
    with pytest.raises(C._lib.CfdError, match="grid rule"):
        C.mg_open_plan(C.make_params("channel"))
    with pytest.raises(C._lib.CfdError, match="grid rule"):
        C.mg_open_plan(channel(126, 90))


def test_plan_null_pointers():
    cp = C.to_cparams(channel(93, 31))
    L = C._lib.lib()
    assert L.cfd_mg_open_any_plan(ctypes.byref(cp), None, None, None) == 0
    lv = ctypes.c_int()
    assert L.cfd_mg_open_any_plan(ctypes.byref(cp), ctypes.byref(lv), None, None) == 0 and lv.value == 4
    out = (ctypes.c_double * 75)()
    assert L.cfd_mg_open_any_level(ctypes.byref(cp), 0, out, 74) == -1  # too little room


@pytest.mark.parametrize("nx,ny", [(93, 31), (253, 131), (1000, 100)])
def test_level_widths_add_up(nx, ny):
    levels = A.make_levels(nx, ny, *spacings(nx, ny))
    for L in levels:
        for D, n0, h in ((L.x, nx, L.a), (L.y, ny, L.b)):
            assert (D.n - 1) * D.W + D.w == n0
            assert 1 <= D.w <= D.W == 2 ** h
            assert D.irregular == (D.w != D.W)
    for L, Lc in zip(levels[:-1], levels[1:]):  # a direction the transfer does not halve is carried over
        for D, Dc in ((L.x, Lc.x), (L.y, Lc.y)):
            assert (Dc.n, Dc.W, Dc.w) == ((D.n, D.W, D.w) if not D.halved else ((D.n + 1) // 2, 2 * D.W, Dc.w))
    assert not levels[0].x.irregular and not levels[0].y.irregular  # level 0 is the reference's grid


def test_plan_of_253x131_has_two_irregular_multi_launch_levels():
    pl = A.plan(253, 131, *spacings(253, 131))
    assert pl[1] == (253, 66) and pl[2] == (127, 33) and 127 * 33 == 4191 and A.tail(pl) == 3
    lv = A.make_levels(253, 131, *spacings(253, 131))
    assert [L.kind for L in lv[:3]] == [A.Y_ONLY, A.FULL, A.FULL]
    assert lv[1].y.irregular and not lv[1].x.irregular and lv[2].x.irregular and lv[2].y.irregular


@pytest.mark.parametrize("nx,ny", CONSTANT_GRIDS)
def test_plan_constants_are_the_restatements(nx, ny):
    """Every field of every level of the C plan, as hexadecimal floats."""
    cp = channel(nx, ny)
    pl = A.plan(nx, ny, cp.dx, cp.dy)
    for l in range(len(pl)):
        got = [float(v).hex() for v in C.mg_open_any_level(cp, l)]
        want = [float(v).hex() for v in A.level_doubles(nx, ny, cp.dx, cp.dy, l)]
        assert len(got) == 75 and got == want, (nx, ny, l, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w])
    with pytest.raises(C._lib.CfdError):
        C.mg_open_any_level(cp, len(pl))


@pytest.mark.parametrize("nx,ny", [(96, 32), (4096, 512), (512, 16)])
def test_regular_levels_hold_method_2s_constants(nx, ny):
    """cE, g, rdiag and omr of a regular level by this module's expressions are mg_open_reference's bits."""
    dx, dy = spacings(nx, ny)
    for L, (n, m, a, b) in zip(A.make_levels(nx, ny, dx, dy), M.plan_levels(nx, ny, dx, dy)):
        R = M.Level(n, m, a, b, dx, dy)
        assert (L.cx.hex(), L.cy.hex(), L.cE.hex(), L.g.hex()) == (R.cx.hex(), R.cy.hex(), R.cE.hex(), R.g.hex())
        assert np.array_equal(bits(L.rdiag), bits(R.rdiag)) and np.array_equal(bits(L.omr), bits(R.omr))
        assert L.x.c_lo == L.x.c_hi == L.cx and L.y.c_lo == L.y.c_hi == L.cy


def test_level0_residual_is_the_reference_residual():
    """Level 0 (w = W = 1) on refreshed ghosts against mg_open_reference.residual_reference
    (channel-01.cpp:672-681, pinned to the oracle in test_mg_open_reference): the same operator,
    equal to the rounding of its other operand order; level 0's coefficients are the reference's."""
    nx, ny = 13, 9
    dx, dy = spacings(nx, ny)
    rng = np.random.default_rng(5)
    p, f = rng.standard_normal((ny + 2, nx + 2)), rng.standard_normal((ny + 2, nx + 2))
    L = A.make_levels(nx, ny, dx, dy)[0]
    assert L.cE == L.cx and L.g == 0.0 and L.x.c_lo == L.x.c_hi == L.cx and L.y.c_lo == L.y.c_hi == L.cy
    got = A.residual(L, p, f)
    M.refresh_ghosts(p)
    want = M.residual_reference(p, f, dx, dy)
    scale = 4.0 * (L.cx + L.cy) * np.abs(p).max()
    assert np.abs(got - want).max() <= 16 * 2.0 ** -53 * scale
    # and bit for bit method 2's level-0 residual, whose level 0 is the reference's too
    assert np.array_equal(bits(got), bits(M.residual(M.Level(nx, ny, 0, 0, dx, dy), p, f)))


@pytest.mark.parametrize("nx,ny", [g for g in SAME_BITS_GRIDS if g != (4096, 512)])
def test_same_plan_gives_method_2s_bits(nx, ny):
    f, dx, dy = fixture(nx, ny)
    assert A.plan(nx, ny, dx, dy) == M.plan(nx, ny, dx, dy)
    p0 = M.random_field(nx, ny, nx + ny)
    a, b = A.solve(f, p0, dx, dy, TOL_FACTOR), M.solve(f, p0, dx, dy, TOL_FACTOR)
    assert (a[0], a[1]) == (b[0], b[1])
    assert np.array_equal(bits(a[2]), bits(b[2]))
    assert a[3] == b[3]
    if (nx, ny) == (96, 32):
        for nu in [(1, 1), (3, 1)]:
            a, b = A.solve(f, p0, dx, dy, TOL_FACTOR, 0.0, *nu), M.solve(f, p0, dx, dy, TOL_FACTOR, 0.0, *nu)
            assert (a[0], a[1]) == (b[0], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))


def test_same_plan_gives_method_2s_bits_at_4096x512():
    """Two cycles (the whole solve takes seconds in numpy): the same residuals and p."""
    nx, ny = 4096, 512
    f, dx, dy = fixture(nx, ny)
    p0 = np.zeros_like(f)
    a, b = A.solve(f, p0, dx, dy, TOL_FACTOR, max_cycles=2), M.solve(f, p0, dx, dy, TOL_FACTOR, max_cycles=2)
    assert a[3] == b[3] and np.array_equal(bits(a[2]), bits(b[2]))


@pytest.mark.parametrize("nx,ny", [(93, 31), (50, 17), (253, 131)])
def test_ghosts_reach_no_result(nx, ny):
    f, dx, dy = fixture(nx, ny)
    p0 = M.random_field(nx, ny, 1)
    other = p0.copy()
    g = np.random.default_rng(2).standard_normal(p0.shape) * 1e6
    other[0, :], other[-1, :], other[:, 0], other[:, -1] = g[0, :], g[-1, :], g[:, 0], g[:, -1]
    a = A.solve(f, p0, dx, dy, TOL_FACTOR)
    b = A.solve(f, other, dx, dy, TOL_FACTOR)
    assert a[:2] == b[:2]
    assert np.array_equal(bits(a[2][1:-1, 1:-1]), bits(b[2][1:-1, 1:-1]))


def converge(nx, ny, cap=CYCLE_CAP, **kw):
    f, dx, dy = fixture(nx, ny)
    cycles, res, p, hist = A.solve(f, np.zeros_like(f), dx, dy, TOL_FACTOR, 0.0, 2, 2, cap, **kw)
    tol = M.tolerance(f, TOL_FACTOR, 0.0)
    print(f"{nx}x{ny} {kw}: {cycles} cycles, residual / tol {res / tol:.3g}, factors "
          f"{['%.3f' % (hist[k + 1] / hist[k]) for k in range(len(hist) - 1)]}")
    return cycles, res, tol


_COMPARISON = {}


def comparison_cycles(nx, ny):
    """mg_open_reference's cycle count on a regular grid, once per grid."""
    if (nx, ny) not in _COMPARISON:
        f, dx, dy = fixture(nx, ny)
        _COMPARISON[(nx, ny)] = M.solve(f, np.zeros_like(f), dx, dy, TOL_FACTOR)[0]
    return _COMPARISON[(nx, ny)]


@pytest.mark.parametrize("grid,beside", [((93, 31), (96, 32)), ((250, 31), (256, 32)), ((241, 121), (240, 120)),
                                         ((500, 63), (512, 64))])
def test_converges_like_the_regular_grid_beside_it(grid, beside):
    """V(2,2) at tol_factor 1e-7 on a random mean-free source from a zero start: converged, in at
    most one cycle more than mg_open_reference on the regular grid beside it (the margin covers the
    operand order and the seed; measured 6 against 6 on all four)."""
    cycles, res, tol = converge(*grid)
    want = comparison_cycles(*beside)
    print(f"mg_open_reference at {beside[0]}x{beside[1]}: {want} cycles")
    assert res <= tol
    assert cycles <= want + 1


@pytest.mark.parametrize("nx,ny", [(50, 17), (17, 40), (13, 9), (100, 20), (126, 90)])
def test_converges_within_the_cap(nx, ny):
    cycles, res, tol = converge(nx, ny)
    assert res <= tol and cycles <= CYCLE_CAP


def test_unit_east_coefficient_misses_the_cap():
    """d = 1 on the coarse levels (cE = cx W / w: their zero one coarse spacing away, not where
    level 0 has it) must fail where the scheme passes: the test sees the east boundary's
    treatment on an odd grid."""
    cycles, res, tol = converge(500, 63)
    assert res <= tol and cycles <= 7
    cycles, res, tol = converge(500, 63, unit_east=True)
    assert cycles == CYCLE_CAP and not res <= tol


@pytest.mark.parametrize("nx,ny", [(13, 9), (17, 9), (9, 17)])
def test_restatement_solves_the_reference_equations(nx, ny):
    """Independent of the scheme: mg_open_reference's dense solve of the level-0 operator, refined
    in long double; the restatement's p is within what its reported residual allows."""
    f, dx, dy = fixture(nx, ny)
    x, ainv, rmax = M.direct_solve(f, dx, dy)
    cycles, res, p, _ = A.solve(f, np.zeros_like(f), dx, dy, TOL_FACTOR)
    err = float(np.abs(p[1:-1, 1:-1] - x[1:-1, 1:-1]).max())
    bound = M.yardstick_bound(f, dx, dy, p, res, ainv)
    print(f"{nx}x{ny}: {cycles} cycles residual {res:.3e}; refined residual {rmax:.3e}; ||A^-1|| {ainv:.3e}; "
          f"max|p - x| {err:.3e} <= {bound:.3e}")
    assert res <= M.tolerance(f, TOL_FACTOR, 0.0) and cycles <= CYCLE_CAP
    assert rmax <= res * 1e-3  # x is exact against what p is held to
    assert err <= bound


def test_tail_and_launch_counts():
    pl = A.plan(253, 131, *spacings(253, 131))
    assert A.tail(pl) == 3 and A.launches_per_cycle(pl, 2, 2, True) == 3 * 4 + 3
    assert A.launches_per_cycle(pl, 4, 1, True) == 3 * 5 + 3 and A.launches_per_cycle(pl, 2, 2, False) == 3 * 10 + 3
    assert A.tail(A.plan(13, 9, *spacings(13, 9))) == 1 and A.tail(A.plan(93, 31, *spacings(93, 31))) == 1
    pl = A.plan(4096, 512, *spacings(4096, 512))
    assert A.tail(pl) == M.tail(M.plan(4096, 512, *spacings(4096, 512))) == 5


def test_zero_source():
    f = np.zeros((33, 95))
    dx, dy = spacings(93, 31)
    cycles, res, p, _ = A.solve(f, np.zeros_like(f), dx, dy, TOL_FACTOR, 1e-10)
    assert (cycles, res) == (1, 0.0) and not bits(p).any()
    p0 = M.random_field(93, 31, 4)
    cycles, res, p, _ = A.solve(f, p0, dx, dy, TOL_FACTOR, 1e-10, max_cycles=1)
    assert cycles == 1 and res > 0 and not np.array_equal(p, p0)
