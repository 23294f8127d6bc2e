"""The any-size multigrid pressure solve (CFD_POISSON_MULTIGRID_ANY, csrc/mg.hip's
scheme MgAny) on the GPU: cycle counts, residuals and p bit for bit
the numpy restatement's (tests/mg_any_reference.py) on two-level plans with an odd
coarsest level, the reference's default grids, a grid odd at every level, levels
that are irregular and multi-launch (fused and one launch per colour), grids whose
last smoothing tile holds the last column and row alone, sweep counts that end in
a level's second buffer; the bits of method 1 where the plans agree; whole steps
against the oracle's phases around the restatement; the refusals and the binaries."""
from __future__ import annotations

import io
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import mg_any_reference as A  # noqa: E402
import oracle as O  # noqa: E402
import rb_sums as R  # noqa: E402
from cfd_amd import _lib, logfmt  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_gpu_parity import assert_bits, ofield  # noqa: E402

_REF = {}


def fixture(nx, ny):
    """(params, source, {options: the restatement's solve}) - computed once per grid."""
    if (nx, ny) not in _REF:
        cp = C.make_params("cavity", nx=nx, ny=ny)
        f = A.random_source(nx, ny, cp.dx, cp.dt, seed=nx * 1000 + ny)
        _REF[(nx, ny)] = (cp, f, {})
    return _REF[(nx, ny)]


def reference_solve(nx, ny, nu1=2, nu2=2, max_cycles=50):
    cp, f, cache = fixture(nx, ny)
    key = (nu1, nu2, max_cycles)
    if key not in cache:
        cache[key] = A.solve(f, cp.dx, cp.tol_factor, nu1, nu2, max_cycles)[:3]
    return cp, f, cache[key]


def nu_opts(nu, max_cycles=50):
    return {"pre_sweeps": nu[0], "post_sweeps": nu[1], "max_cycles": max_cycles}


def gpu_solve(cp, f, opts, **kw):
    g = C.CavitySolver(cp, poisson="multigrid-any", mg_options=opts, **kw)
    g.set_field("src", f)
    cycles, res = g.solverPressurePoisson()
    p = g.field("p").copy()
    tm, info = g.timing(), g.mg_info()
    g.close()
    return cycles, res, p, tm, info


def assert_counters(nx, ny, nu, cycles, fused, tm, info):
    """The plan, and the launches, sweeps and cell updates of one solve of `cycles` cycles."""
    pl = A.plan(nx, ny)
    per = A.launches_per_cycle(pl, nu[0], nu[1], fused)
    assert (info.levels, info.coarse_nx, info.coarse_ny) == (len(pl), *pl[-1])
    assert info.coarse_sweeps == 4 * max(pl[-1])
    assert (info.solves, info.cycles) == (1, cycles)
    assert info.launches == cycles * per, (info.launches, cycles, per)
    assert tm.poisson_launches == info.launches and tm.poisson_ms > 0
    assert tm.poisson_sweeps == cycles * (nu[0] + nu[1])
    assert tm.poisson_cell_updates == nx * ny * cycles * (nu[0] + nu[1])
    assert _lib.SOR_KERNEL[tm.sor_kernel] == "multigrid" and tm.sor_kernel == 8


def check_solve(nx, ny, nu=(2, 2), max_cycles=50, fused=True):
    """One GPU solve of the grid's fixture: (cycles, residual), p and the counters are the restatement's."""
    cp, f, (cycles, res, p) = reference_solve(nx, ny, nu[0], nu[1], max_cycles)
    gc, gr, gp, tm, info = gpu_solve(cp, f, nu_opts(nu, max_cycles))
    what = f"{nx}x{ny} V{nu} max_cycles {max_cycles} {'fused' if fused else 'colour launches'}"
    print(f"{what}: gpu {gc} cycles residual {gr!r}; restatement {cycles} cycles residual {res!r}; "
          f"launches {info.launches}")
    assert (gc, gr) == (cycles, res), what
    assert_bits(gp, p, "any-size multigrid p " + what)
    assert_counters(nx, ny, nu, cycles, fused, tm, info)
    return cycles, res, info


# 9x9 -> 5x5 and 15x8 -> 8x4: two levels, the tail is the coarse SOR alone, on an odd coarsest level; the
# reference's default grids 63^2 (cavity), 93x31 and its transpose; 65^2: odd at every level (65, 33, 17, 9, 5)
@pytest.mark.parametrize("nx,ny", [(9, 9), (15, 8), (63, 63), (93, 31), (31, 93), (65, 65)])
def test_solve_is_the_restatement(nx, ny):
    cycles, res, info = check_solve(nx, ny)
    cp, f, _ = fixture(nx, ny)
    assert res <= cp.tol_factor * np.abs(f).max() and cycles <= 15


def test_plans_of_the_fixtures():
    assert A.plan(9, 9) == [(9, 9), (5, 5)] and A.plan(15, 8) == [(15, 8), (8, 4)]
    assert [a for a, _ in A.plan(65, 65)] == [65, 33, 17, 9, 5]
    pl = A.plan(253, 131)
    assert pl[1] == (127, 66) and A.tail(pl) == 2  # an irregular level 1 of 8382 cells: multi-launch
    pl = A.plan(250, 250)
    assert pl[1] == (125, 125) and A.tail(pl) == 2  # regular, but an odd multi-launch level 1
    assert A.plan(241, 113)[1] == (121, 57) and A.tail(A.plan(241, 113)) == 2
    for nx, ny in [(125, 61), (121, 57), (117, 53), (127, 63), (123, 59)]:
        assert A.tail(A.plan(nx, ny)) == 1  # level 0 alone is multi-launch


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("nx,ny", [(253, 131), (250, 250)])
def test_irregular_multi_launch_levels(nx, ny, fused, monkeypatch):
    if not fused:
        monkeypatch.setenv("CFD_MG_FUSED", "0")
    cycles, res, _ = check_solve(nx, ny, fused=fused)
    cp, f, _ = fixture(nx, ny)
    assert res <= cp.tol_factor * np.abs(f).max() and cycles <= 15


# The smoothing tile owns 124x60, 120x56 or 116x52 cells for 1, 2 or 3 sweeps per launch: at 125x61, 121x57 and
# 117x53 the last block owns the last column and the last row alone; 241x113 does the same on level 1 (121x57,
# whose last column and row are 1 of 2 finest cells wide: the irregular coefficients in the last tile and in its
# neighbour's halo); 127x63 and 123x59 are one aligned pair beyond.
@pytest.mark.parametrize("nx,ny,nu", [(125, 61, (1, 1)), (121, 57, (2, 2)), (117, 53, (3, 3)), (241, 113, (2, 2)),
                                      (127, 63, (1, 1)), (123, 59, (2, 2))])
def test_tile_edges(nx, ny, nu):
    cycles, res, _ = check_solve(nx, ny, nu)
    cp, f, _ = fixture(nx, ny)
    assert res <= cp.tol_factor * np.abs(f).max() and cycles <= 15


def test_tile_edge_level_1_colour_launches(monkeypatch):
    monkeypatch.setenv("CFD_MG_FUSED", "0")
    check_solve(241, 113, (2, 2), fused=False)


@pytest.mark.parametrize("max_cycles", [50, 1, 2])
def test_second_buffer_253x131(max_cycles):
    """V(4,1): 3 fused smoothing launches per multi-launch level and cycle - after an odd number of
    cycles level 0's field is in the second buffer (the residual pass reads it there, the solve copies
    it back), and the transfers of level 1 work on its second buffer."""
    pl = A.plan(253, 131)
    assert A.smoothing_launches(4, True) + A.smoothing_launches(1, True) == 3
    assert A.launches_per_cycle(pl, 4, 1, True) == 12
    cycles, _, _ = check_solve(253, 131, (4, 1), max_cycles)
    assert cycles == max_cycles or max_cycles == 50


@pytest.mark.parametrize("nx,ny", [(64, 64), (96, 64)])
def test_same_bits_as_method_1(nx, ny):
    """Where method 1's plan ends on a smaller side below 8 the two methods are one solve."""
    cp, f, _ = fixture(nx, ny)
    g = C.CavitySolver(cp, poisson="multigrid")
    g.set_field("src", f)
    one = g.solverPressurePoisson()
    p1, i1 = g.field("p").copy(), g.mg_info()
    g.set_poisson_method("multigrid-any")
    g.reset_timing()
    four = g.solverPressurePoisson()
    p4, i4 = g.field("p").copy(), g.mg_info()
    g.close()
    print(f"{nx}x{ny}: method 1 {one}, method 4 {four}")
    assert one == four and 0 < one[0] <= 15
    assert_bits(p4, p1, f"method 4 against method 1 at {nx}x{ny}")
    assert (i1.levels, i1.coarse_nx, i1.coarse_ny, i1.launches) == (i4.levels, i4.coarse_nx, i4.coarse_ny, i4.launches)
    rc, rres, rp = reference_solve(nx, ny)[2]
    assert four == (rc, rres)
    assert_bits(p4, rp, f"method 4 against the restatement at {nx}x{ny}")


_ORACLE_STEPS = {}


def oracle_steps(case, nx, ny, steps=4):
    """`steps` steps of the oracle's phases around the restatement's solve, once per case."""
    key = (case, nx, ny)
    if key not in _ORACLE_STEPS:
        cp = C.make_params(case, nx=nx, ny=ny, **({"re": 1000.0} if case == "cavity" else {}))
        o = O.Oracle(cp, ordering=O.RB)  # (the order is the SOR loop's, which these steps do not run)
        rows = [A.oracle_step(o, cp) for _ in range(steps)]
        fields = {n: ofield(o, n, cp).copy() for n in ("u", "v", "p")}
        if case == "rayleigh_benard":
            fields["t"] = o.field("t").copy()
        md, ke = o.stats()  # (and the red-black order's tree sum of the kinetic energy, restated: tests/rb_sums.py)
        _ORACLE_STEPS[key] = (cp, rows, fields, (md, ke, R.oracle_ke(o, R.strips_of(ny, 1))))
    return _ORACLE_STEPS[key]


@pytest.mark.parametrize("case,nx,ny,ordering", [
    ("cavity", 63, 63, "lex"), ("cavity", 63, 63, "rb"), ("cavity", 125, 61, "lex"), ("cavity", 125, 61, "rb"),
    ("rayleigh_benard", 129, 33, "auto")])
def test_four_steps_are_the_oracles(case, nx, ny, ordering):
    cp, rows, want, (omd, oke, oke_rb) = oracle_steps(case, nx, ny)
    cls = C.RayleighBenardSolver if case == "rayleigh_benard" else C.CavitySolver
    g = cls(cp, ordering=ordering, poisson="multigrid-any")
    got = [g.step() for _ in range(4)]
    for k, (a, b) in enumerate(zip(got, rows)):
        print(f"{case} {nx}x{ny} {ordering} step {k + 1}: gpu {a[0]} cycles residual {a[1]!r}; "
              f"oracle {b[0]} cycles residual {b[1]!r}")
    assert got == rows
    assert all(c <= 15 for c, _ in rows)
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), want[n], f"{case} {nx}x{ny} {ordering} after 4 steps: {n}")
    if case == "rayleigh_benard":
        assert_bits(g.field("t")[1:-1, 1:-1], want["t"][1:-1, 1:-1], "T after 4 steps")
    md, ke = g.statistics()
    assert md == omd and ke == (oke if ordering == "lex" else oke_rb)
    info, total = g.mg_info(), sum(c for c, _ in rows)
    assert (info.solves, info.cycles) == (4, total)
    assert info.launches == total * A.launches_per_cycle(A.plan(nx, ny), 2, 2, True)
    assert g.timing().poisson_launches == info.launches
    g.close()


@pytest.mark.parametrize("nx,ny", [(63, 63), (253, 131)])
def test_solve_over_a_dirty_field(nx, ny):
    """p random, ghost cells included, before the solve: each solve starts from zero, ghosts too."""
    cp, f, (cycles, res, p) = reference_solve(nx, ny)
    g = C.CavitySolver(cp, poisson="multigrid-any")
    g.set_field("src", f)
    dirty = np.random.default_rng(nx + ny).standard_normal((ny + 2, nx + 2))
    for k in range(2):  # the second over the buffers the first solve left
        g.set_field("p", dirty)
        assert g.solverPressurePoisson() == (cycles, res)
        assert_bits(g.field("p"), p, f"any-size multigrid p {nx}x{ny} over a dirty field, solve {k + 1}")
    g.close()


def test_reentering_the_mode():
    """method 4 -> sor for two steps -> method 4 V(4,1): the next solve on the current source
    is the restatement's with those options, the plan is back."""
    cp = C.make_params("cavity", re=1000.0, nx=125, ny=61, max_iters=200)
    g = C.CavitySolver(cp, poisson="multigrid-any")
    pl = A.plan(125, 61)
    g.step()
    assert g.mg_info().levels == len(pl) and g.timing().sor_kernel == 8
    g.set_poisson_method("sor")
    assert g.mg_info().levels == 0
    g.step()
    g.step()
    assert g.timing().sor_kernel != 8
    g.set_poisson_method("multigrid-any", {"pre_sweeps": 4, "post_sweeps": 1})
    info = g.mg_info()
    assert (info.levels, info.coarse_nx, info.coarse_ny, info.coarse_sweeps) == (len(pl), *pl[-1], 4 * max(pl[-1]))
    f = g.field("src").copy()
    got = g.solverPressurePoisson()
    cycles, res, p, _ = A.solve(f, cp.dx, cp.tol_factor, 4, 1)
    print(f"re-entered V(4,1): gpu {got}; restatement {(cycles, res)}")
    assert got == (cycles, res) and cycles <= 15
    assert_bits(g.field("p"), p, "any-size multigrid p after re-entering the mode")
    g.close()


def test_zero_source():
    cp = C.make_params("cavity", nx=63, ny=63)
    f = np.zeros((65, 65))
    assert A.solve(f, cp.dx, cp.tol_factor)[:2] == (1, 0.0)
    gc, gr, gp, tm, info = gpu_solve(cp, f, None)
    assert (gc, gr) == (1, 0.0)
    assert not gp.view(np.int64).any()
    assert_counters(63, 63, (2, 2), 1, True, tm, info)


def test_reference_defaults_construct_and_step():
    cp = C.reference_defaults("cavity")
    assert (cp.nx, cp.ny) == (63, 63)
    g = C.CavitySolver(cp, poisson="multigrid-any")
    g.applyBoundaryConditions()
    cycles, res = g.step()
    assert 0 < cycles <= 15 and res <= cp.tol_factor * np.abs(g.field("src")).max()
    assert g.mg_info().levels == 5 and g.timing().sor_kernel == 8
    g.close()


def test_refusals_name_the_rule():
    cav = C.make_params("cavity", nx=63, ny=63)
    with pytest.raises(_lib.CfdError, match="strip rule"):
        C.CavitySolver(cav, n_strips=2, poisson="multigrid-any")
    L = _lib.lib()
    hub = L.cfd_comm_loopback_hub(1)
    comm = L.cfd_comm_init_loopback(hub, 0, 0)
    assert hub and comm
    try:
        with pytest.raises(_lib.CfdError, match="rank rule"):
            C.CavitySolver(cav, ordering="rb", rank_rows=(1, 63), comm=comm, poisson="multigrid-any")
    finally:
        L.cfd_comm_destroy(comm)
        L.cfd_comm_loopback_hub_destroy(hub)
    with pytest.raises(_lib.CfdError, match="case rule"):
        C.ChannelSolver(C.make_params("channel", nx=64, ny=64), poisson="multigrid-any")
    with pytest.raises(_lib.CfdError, match="case rule"):
        C.BackwardsStepSolver(C.reference_defaults("backwards_step"), poisson="multigrid-any")
    with pytest.raises(_lib.CfdError, match="grid rule"):
        C.CavitySolver(C.make_params("cavity", nx=40, ny=7), poisson="multigrid-any")
    with pytest.raises(_lib.CfdError, match="grid rule"):
        C.CavitySolver(cav, poisson="multigrid")  # method 1 still refuses 63^2
    g = C.CavitySolver(cav)  # a refused switch leaves the solver on SOR
    with pytest.raises(_lib.CfdError, match="options"):
        g.set_poisson_method("multigrid-any", {"max_cycles": -1})
    it, _ = g.step()
    assert g.timing().sor_kernel != 8 and it > 15
    g.close()


def test_cycle_cap_in_the_binary(tmp_path):
    """bin/cavity --multigrid-any --mg-cycles 2 at 63^2: the iteration column reads 2 and every
    step warns once, with the lines the Python driver prints."""
    exe = os.path.join(ROOT, "computational-fluid-dynamics_amd", "bin", "cavity")
    r = subprocess.run([exe, "--multigrid-any", "--mg-cycles", "2", "--Nx", "63", "--Ny", "63", "--steps", "2", "--no-vtk",
                        "--print-interval", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ansi = re.compile(r"\x1b\[[0-9;]*m")
    lines = [l for l in ansi.sub("", r.stdout).splitlines() if l.startswith("Step ")]
    warns = [l for l in ansi.sub("", r.stderr).splitlines() if l.startswith("Warning")]
    cp = C.make_params("cavity", nx=63, ny=63)
    cp.print_interval = 1
    out, err = io.StringIO(), io.StringIO()
    g = C.CavitySolver(cp, poisson="multigrid-any", mg_options={"max_cycles": 2})
    g.run(output_directory=None, out=out, err=err, steps=2)
    g.close()
    want = [l for l in out.getvalue().splitlines() if l.startswith("Step ")]
    assert len(want) == 2 and lines == want
    assert all(int(l.rsplit("=", 1)[1]) == 2 for l in lines)
    assert len(warns) == 2 and warns == err.getvalue().splitlines()
    assert all(w.startswith(logfmt.warning_line(cp.case_id, 2, 0.0).split(" Final")[0]) for w in warns)


def test_binaries_refuse_with_the_rule(tmp_path):
    exe = os.path.join(ROOT, "computational-fluid-dynamics_amd", "bin", "channel")
    r = subprocess.run([exe, "--multigrid-any", "--Nx", "64", "--Ny", "64", "--steps", "1", "--no-vtk"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "case rule" in r.stderr and "--multigrid-any" in r.stderr
    exe = os.path.join(ROOT, "computational-fluid-dynamics_amd", "bin", "cavity")
    for other in ("--multigrid", "--multigrid-open", "--multigrid-step"):
        r = subprocess.run([exe, "--multigrid-any", other, "--steps", "1", "--no-vtk"], cwd=tmp_path, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 2 and "excludes" in r.stderr  # (before any device work)
