"""The any-size multigrid scheme's numpy restatement (tests/mg_any_reference.py)
on the CPU: its plans and the library's host-only plan (cfd_mg_any_plan,
cfd_mg_any_level) agree to the bit, the level widths add up to the finest grid,
its level-0 residual is the reference's on an odd grid, it is mg_reference
where that has the same plan, it converges on odd and other irregular grids in
at most one cycle more than mg_reference on the regular grid beside them, and a
dense solve of the reference's equations bounds its p."""
from __future__ import annotations

import numpy as np
import pytest

import cfd_amd as C
import mg_any_reference as A
import mg_reference as M

TOL_FACTOR = 1e-9

PLANS = {
    (63, 63): [(63, 63), (32, 32), (16, 16), (8, 8), (4, 4)],
    (93, 31): [(93, 31), (47, 16), (24, 8), (12, 4)],
    (65, 65): [(65, 65), (33, 33), (17, 17), (9, 9), (5, 5)],
}
CONSTANT_GRIDS = [(63, 63), (93, 31), (65, 65), (253, 131), (1000, 1000), (8200, 8200), (64, 64), (9, 9), (15, 8)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("nx,ny", sorted(PLANS))
def test_plans_listed(nx, ny):
    assert A.plan(nx, ny) == PLANS[(nx, ny)]
    assert C.mg_any_plan(C.make_params("cavity", nx=nx, ny=ny)) == PLANS[(nx, ny)]


def test_plans_of_engineering_sizes():
    pl = A.plan(1000, 1000)
    assert pl is not None and min(pl[-1]) <= 7 and pl[-1] == (4, 4) and len(pl) == 9
    assert C.mg_any_plan(C.make_params("cavity", nx=1000, ny=1000)) == pl
    pl = A.plan(8200, 8200)
    assert pl is not None and pl[-1] == (5, 5)
    assert C.mg_any_plan(C.make_params("cavity", nx=8200, ny=8200)) == pl
    for nx, ny in [(2000, 2000), (4000, 4000), (4095, 4095), (1500, 1000), (4096, 4096), (129, 33)]:
        pl = A.plan(nx, ny)
        assert pl is not None and 4 <= min(pl[-1]) <= 7
        assert C.mg_any_plan(C.make_params("cavity", nx=nx, ny=ny)) == pl
    assert C.mg_any_plan(C.make_params("rayleigh_benard", nx=129, ny=33)) == A.plan(129, 33)
    assert C._lib.POISSON["multigrid-any"] == 4


def test_plan_refusals():
    assert A.plan(7, 40) is None and A.plan(40, 7) is None
    assert A.plan(70000, 8) is None  # 35000 x 4: a coarsest level of over 4096 cells
    for cp, rule in [(C.make_params("cavity", nx=7, ny=40), "grid rule"),
                     (C.make_params("cavity", nx=40, ny=7), "grid rule"),
                     (C.make_params("cavity", nx=70000, ny=8), "grid rule"),
                     (C.make_params("channel"), "case rule"),
                     (C.make_params("channel", nx=64, ny=64), "case rule"),
                     (C.make_params("backwards_step"), "case rule")]:
        with pytest.raises(C._lib.CfdError, match=rule) as e:
            C.mg_any_plan(cp)
        assert "(-1)" in str(e.value)  # CFD_E_ARG
    # method 1's refusals stand
    with pytest.raises(C._lib.CfdError, match="grid rule"):
        C.mg_plan(C.make_params("cavity", nx=63, ny=63))


@pytest.mark.parametrize("nx,ny", [(63, 63), (93, 31), (253, 131), (1000, 1000)])
def test_level_widths_add_up(nx, ny):
    for L in A.make_levels(nx, ny, 1.0 / ny):
        for D, n0 in ((L.x, nx), (L.y, ny)):
            assert (D.n - 1) * D.W + D.w == n0
            assert 1 <= D.w <= D.W == 2 ** L.l
            assert D.irregular == (D.w != D.W)
    L0 = A.make_levels(nx, ny, 1.0 / ny)[0]
    assert not L0.x.irregular and not L0.y.irregular  # level 0 is the reference's grid


def test_plan_of_253x131_has_an_irregular_multi_launch_level():
    pl = A.plan(253, 131)
    assert pl[1] == (127, 66) and 127 * 66 == 8382 and A.tail(pl) == 2
    L1 = A.make_levels(253, 131, 1.0 / 131)[1]
    assert L1.x.irregular and L1.y.irregular and (L1.x.w, L1.y.w) == (1.0, 1.0)


@pytest.mark.parametrize("nx,ny", CONSTANT_GRIDS)
def test_plan_constants_are_the_restatements(nx, ny):
    """Every field of every level of the C plan, as hexadecimal floats."""
    cp = C.make_params("cavity", nx=nx, ny=ny)
    for l in range(len(A.plan(nx, ny))):
        got = [float(v).hex() for v in C.mg_any_level(cp, l)]
        want = [float(v).hex() for v in A.level_doubles(nx, ny, cp.dx, l)]
        assert len(got) == 72 and got == want, (nx, ny, l, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w])
    with pytest.raises(C._lib.CfdError):
        C.mg_any_level(cp, len(A.plan(nx, ny)))


def test_level0_residual_is_the_reference_loop():
    """Bit for bit the plain double loop of cavity-01.cpp:660-673, on an odd grid with a plan."""
    nx, ny = 13, 9
    rng = np.random.default_rng(5)
    p = rng.standard_normal((ny + 2, nx + 2))
    p[0, :] = 0.0  # the ghost row the reference never writes
    f = rng.standard_normal((ny + 2, nx + 2))
    dx = 1.0 / 13
    L = A.make_levels(nx, ny, dx)[0]
    got = A.residual(L, p, f)
    inv = 1.0 / (dx * dx)
    want = np.zeros((ny, nx))
    for j in range(1, ny + 1):
        for i in range(1, nx + 1):
            ew, ee, en, es = int(i > 1), int(i < nx), int(j < ny), 1
            want[j - 1, i - 1] = inv * (
                ee * (p[j][i + 1] - p[j][i]) + ew * (p[j][i - 1] - p[j][i])
                + en * (p[j + 1][i] - p[j][i]) + es * (p[j - 1][i] - p[j][i])) - f[j][i]
    assert np.array_equal(bits(got), bits(want))
    assert L.cS == 1.0 and L.g == 0.0


@pytest.mark.parametrize("nx,ny", [(64, 64), (96, 64), (48, 16)])
def test_regular_grids_are_mg_reference(nx, ny):
    assert A.plan(nx, ny) == M.plan(nx, ny)
    dx = 1.0 / ny
    f = M.random_source(nx, ny, dx, 1e-3, seed=nx * 1000 + ny)
    a, b = A.solve(f, dx, TOL_FACTOR), M.solve(f, dx, TOL_FACTOR)
    assert (a[0], a[1]) == (b[0], b[1])
    assert np.array_equal(bits(a[2]), bits(b[2]))
    assert a[3] == b[3]
    for nu in [(1, 1), (3, 1)]:
        a, b = A.solve(f, dx, TOL_FACTOR, *nu), M.solve(f, dx, TOL_FACTOR, *nu)
        assert (a[0], a[1]) == (b[0], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))


_COMPARISON = {}


def comparison_cycles(nx, ny):
    """mg_reference's cycle count on a regular grid, once per grid."""
    if (nx, ny) not in _COMPARISON:
        dx = 1.0 / ny
        _COMPARISON[(nx, ny)] = M.solve(M.random_source(nx, ny, dx, 1e-3, seed=nx * 1000 + ny), dx, TOL_FACTOR)[0]
    return _COMPARISON[(nx, ny)]


@pytest.mark.parametrize("grid,beside", [((63, 63), (64, 64)), ((65, 65), (64, 64)), ((93, 31), (96, 32)),
                                         ((31, 93), (32, 96)), ((125, 125), (128, 128)), ((241, 121), (240, 120)),
                                         ((250, 250), (256, 256))])
def test_converges_like_the_regular_grid_beside_it(grid, beside):
    """V(2,2) at tol_factor 1e-9 on a random compatible source: converged, in at most one
    cycle more than mg_reference on the regular comparison grid (the margin: the last
    cell's coefficients smooth slightly less well; measured 7 against 7 everywhere,
    factors per cycle 0.036-0.078)."""
    nx, ny = grid
    dx = 1.0 / ny
    f = M.random_source(nx, ny, dx, 1e-3, seed=nx * 1000 + ny)
    cycles, res, p, hist = A.solve(f, dx, TOL_FACTOR)
    want = comparison_cycles(*beside)
    print(f"{nx}x{ny}: {cycles} cycles (mg_reference at {beside[0]}x{beside[1]}: {want}), factors "
          f"{['%.3f' % (hist[k + 1] / hist[k]) for k in range(len(hist) - 1)]}")
    assert res <= TOL_FACTOR * np.abs(f).max()
    assert cycles <= want + 1


@pytest.mark.parametrize("nx,ny", [(9, 9), (15, 9), (17, 31)])
def test_restatement_solves_the_reference_equations(nx, ny):
    """Independent of the scheme: mg_reference's dense solve of the level-0 operator, refined
    in long double; the restatement's p is within what its reported residual allows."""
    dx = 1.0 / nx
    f = M.random_source(nx, ny, dx, 1e-3, seed=nx * 1000 + ny)
    x, ainv, rmax = M.direct_solve(f, dx)
    cycles, res, p, _ = A.solve(f, dx, TOL_FACTOR)
    err = float(np.abs(p - x).max())
    bound = M.yardstick_bound(f, dx, p, res, ainv)
    print(f"{nx}x{ny}: {cycles} cycles residual {res:.3e}; refined residual {rmax:.3e}; ||A^-1|| {ainv:.3e}; "
          f"max|p - x| {err:.3e} <= {bound:.3e}")
    assert res <= TOL_FACTOR * np.abs(f).max() and cycles <= 15
    assert rmax <= res * 1e-3  # x is exact against what p is held to
    assert err <= bound
    assert not p[0].any() and not p[-1].any() and not p[:, 0].any() and not p[:, -1].any()


def test_tail_and_launch_counts():
    pl = A.plan(253, 131)
    assert A.tail(pl) == 2 and A.launches_per_cycle(pl, 2, 2, True) == 10
    assert A.launches_per_cycle(pl, 4, 1, True) == 12 and A.launches_per_cycle(pl, 2, 2, False) == 22
    assert A.tail(A.plan(9, 9)) == 1 and A.tail(A.plan(15, 8)) == 1
    assert A.plan(9, 9) == [(9, 9), (5, 5)] and A.plan(15, 8) == [(15, 8), (8, 4)]
    assert A.tail(A.plan(4096, 4096)) == M.tail(M.plan(4096, 4096)) and A.plan(4096, 4096) == M.plan(4096, 4096)


def test_zero_source_is_one_cycle_of_zeros():
    f = np.zeros((65, 65))
    cycles, res, p, _ = A.solve(f, 1.0 / 63, TOL_FACTOR)
    assert (cycles, res) == (1, 0.0)
    assert not bits(p).any()
