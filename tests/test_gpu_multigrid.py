"""The multigrid pressure solve (csrc/mg.hip) on the GPU: cycle
counts, residuals and p bit for bit the numpy restatement's
(tests/mg_reference.py) at every size at which the kernels take another path;
whole timesteps that converge where the default solve stops at its cap; the
switch back to SOR; the refusals; Rayleigh-Benard; the drop-in binary. Further:
sweep counts whose fused launches end in a level's second buffer, two-level and
thin plans, grids on a multiple of the smoothing tile, launch counts cycle by
cycle, four whole steps against the oracle's phases around the restatement,
solves over a dirty field and after re-entering the mode, the drivers' cycle
cap, and a dense solve of the reference's equations as a yardstick that does
not depend on the restatement."""
from __future__ import annotations

import io
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import mg_reference as M  # noqa: E402
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
        f = M.random_source(nx, ny, cp.dx, cp.dt, seed=nx * 1000 + ny)
        _REF[(nx, ny)] = (cp, f, {})
    return _REF[(nx, ny)]


def reference_solve(nx, ny, nu1, nu2, max_cycles):
    cp, f, cache = fixture(nx, ny)
    key = (nu1, nu2, max_cycles)
    if key not in cache:
        cache[key] = M.solve(f, cp.dx, cp.tol_factor, nu1, nu2, max_cycles)[:3]
    return cp, f, cache[key]


def nu_opts(nu, max_cycles=50):
    return {"pre_sweeps": nu[0], "post_sweeps": nu[1], "max_cycles": max_cycles}


def assert_counters(nx, ny, nu, cycles, fused, tm, info):
    """Launches, sweeps and cell updates of one solve of `cycles` cycles (mg_reference.launches_per_cycle)."""
    per = M.launches_per_cycle(M.plan(nx, ny), nu[0], nu[1], fused)
    assert (info.solves, info.cycles) == (1, cycles)
    assert info.launches == cycles * per, (info.launches, cycles, per)
    assert tm.poisson_launches == info.launches
    assert tm.poisson_sweeps == cycles * (nu[0] + nu[1])
    assert tm.poisson_cell_updates == nx * ny * cycles * (nu[0] + nu[1])


def check_solve(nx, ny, nu=(2, 2), max_cycles=50, fused=True):
    """One GPU solve of the grid's fixture: (cycles, residual), p and the counters are the restatement's."""
    cp, f, (cycles, res, p) = reference_solve(nx, ny, nu[0], nu[1], max_cycles)
    gc, gr, gp, tm, info = gpu_solve(cp, f, nu_opts(nu, max_cycles))
    what = f"{nx}x{ny} V{nu} max_cycles {max_cycles} {'fused' if fused else 'colour launches'}"
    print(f"{what}: gpu {gc} cycles residual {gr!r}; restatement {cycles} cycles residual {res!r}; "
          f"launches {info.launches}")
    assert (gc, gr) == (cycles, res), what
    assert_bits(gp, p, "multigrid p " + what)
    assert_counters(nx, ny, nu, cycles, fused, tm, info)
    return cycles, res, info


def gpu_solve(cp, f, opts, **kw):
    g = C.CavitySolver(cp, poisson="multigrid", mg_options=opts, **kw)
    g.set_field("src", f)
    cycles, res = g.solverPressurePoisson()
    p = g.field("p").copy()
    tm, info = g.timing(), g.mg_info()
    g.close()
    return cycles, res, p, tm, info


# 16^2: three levels, every cell on a boundary; 48x16 / 16x48: coarsest 12x4 / 4x12 (rows against columns);
# 64^2, 96x64; 240x120: an odd coarsest level (30x15) and a multi-launch level 1; 272x144: past the 128-column
# block and a pitch rounded up; 512^2: levels 0-2 multi-launch hand level 3 (64^2) to the one-launch tail
# two-level plans (the tail is the coarse SOR alone): 8x8, 10x12, 30x18, 126x90, 126x130 (63x65: 4095 cells, 260
# sweeps); strips one tile row or column thin with a coarsest level 4 cells wide: 1024x8, 8x1024, 512x16, 16x512
@pytest.mark.parametrize("nx,ny", [(16, 16), (48, 16), (16, 48), (64, 64), (96, 64), (240, 120), (272, 144),
                                   (512, 512), (8, 8), (10, 12), (30, 18), (126, 130), (126, 90), (1024, 8),
                                   (8, 1024), (512, 16), (16, 512)])
def test_solve_is_the_restatement(nx, ny):
    cp, f, (cycles, res, p) = reference_solve(nx, ny, 2, 2, 50)
    gc, gr, gp, tm, info = gpu_solve(cp, f, None)
    print(f"{nx}x{ny}: gpu {gc} cycles residual {gr!r}; restatement {cycles} cycles residual {res!r}; "
          f"levels {info.levels}, launches {info.launches}")
    assert res <= cp.tol_factor * np.abs(f).max() and cycles <= 15
    assert (gc, gr) == (cycles, res)
    assert_bits(gp, p, f"multigrid p {nx}x{ny}")
    pl = M.plan(nx, ny)
    assert (info.levels, info.coarse_nx, info.coarse_ny) == (len(pl), *pl[-1])
    assert info.coarse_sweeps == 4 * max(pl[-1]) and info.solves == 1 and info.cycles == cycles
    assert _lib.SOR_KERNEL[tm.sor_kernel] == "multigrid" and tm.sor_kernel == 8
    assert tm.poisson_launches == info.launches > 0 and tm.poisson_ms > 0
    assert_counters(nx, ny, (2, 2), cycles, True, tm, info)


@pytest.mark.parametrize("nx,ny", [(48, 16), (240, 120)])
@pytest.mark.parametrize("nu", [(1, 1), (3, 1)])
def test_sweep_counts(nx, ny, nu):
    cp, f, (cycles, res, p) = reference_solve(nx, ny, nu[0], nu[1], 50)
    gc, gr, gp, _, _ = gpu_solve(cp, f, {"pre_sweeps": nu[0], "post_sweeps": nu[1]})
    print(f"{nx}x{ny} V{nu}: {gc} cycles residual {gr!r}")
    assert (gc, gr) == (cycles, res)
    assert_bits(gp, p, f"multigrid p {nx}x{ny} V{nu}")


@pytest.mark.parametrize("nx,ny,nu", [(272, 144, (2, 2)), (240, 120, (3, 1)), (512, 512, (4, 5))])
def test_colour_launches_and_fused_sweeps_agree(nx, ny, nu, monkeypatch):
    """The smoothing as one launch per colour (CFD_MG_FUSED=0) and as fused LDS-tile
    launches (the default; 4 sweeps run as 2 + 2, 5 as 3 + 2) are the same solve."""
    cp, f, (cycles, res, p) = reference_solve(nx, ny, nu[0], nu[1], 50)
    opts = {"pre_sweeps": nu[0], "post_sweeps": nu[1]}
    fused = gpu_solve(cp, f, opts)
    monkeypatch.setenv("CFD_MG_FUSED", "0")
    plain = gpu_solve(cp, f, opts)
    assert fused[:2] == plain[:2] == (cycles, res)
    assert_bits(fused[2], p, f"fused sweeps p {nx}x{ny} V{nu}")
    assert_bits(plain[2], p, f"colour launches p {nx}x{ny} V{nu}")
    assert fused[4].launches < plain[4].launches


def test_max_cycles_stops_unconverged():
    """max_cycles 2: the residual reported is the cycle-2 field's."""
    cp, f, (cycles, res, p) = reference_solve(240, 120, 2, 2, 2)
    assert cycles == 2 and res > cp.tol_factor * np.abs(f).max()
    gc, gr, gp, _, _ = gpu_solve(cp, f, {"max_cycles": 2})
    assert (gc, gr) == (2, res)
    assert_bits(gp, p, "multigrid p after 2 cycles")


# Sweep counts that give 3 fused smoothing launches per multi-launch level and cycle (4 runs as 2 + 2, 5 as
# 3 + 2, 6 as 3 + 3): after an odd number of cycles the field of level 0 is in the second buffer (the residual
# pass reads it there; solve_mg copies it back), and inside every cycle the restriction and the prolongation
# of levels >= 1 work on mg_q[l].
PARITY_NU = [(4, 1), (1, 4), (4, 2), (5, 1), (6, 1)]


@pytest.mark.parametrize("max_cycles", [50, 1, 2])
@pytest.mark.parametrize("nu", PARITY_NU)
def test_second_buffer_240x120(nu, max_cycles):
    """240x120: levels 0 and 1 multi-launch, the tail from 60x30."""
    pl = M.plan(240, 120)
    assert M.tail(pl) == 2
    assert M.smoothing_launches(nu[0], True) + M.smoothing_launches(nu[1], True) == 3
    assert M.launches_per_cycle(pl, nu[0], nu[1], True) == 12
    cycles, _, _ = check_solve(240, 120, nu, max_cycles)
    assert cycles == max_cycles or max_cycles == 50  # 1: ends in the second buffer; 2: in the primary


@pytest.mark.parametrize("nu", [(4, 1), (4, 2)])
def test_second_buffer_512(nu):
    """512^2: levels 0-2 multi-launch."""
    pl = M.plan(512, 512)
    assert M.tail(pl) == 3 and M.launches_per_cycle(pl, nu[0], nu[1], True) == 17
    check_solve(512, 512, nu)


@pytest.mark.parametrize("nx,ny,nu", [(240, 120, (4, 1)), (512, 512, (4, 2))])
def test_second_buffer_colour_launches(nx, ny, nu, monkeypatch):
    """The same fixtures with one in-place launch per colour: the same bits, 2 (nu1 + nu2) smoothing launches."""
    monkeypatch.setenv("CFD_MG_FUSED", "0")
    check_solve(nx, ny, nu, fused=False)


# The smoothing tile owns 124x60, 120x56 or 116x52 cells for 1, 2 or 3 sweeps per launch and the grid is
# n / T + 1 blocks: on a multiple of the tile the last block owns one column or row (level 0 is on a multiple in
# both directions, and so is the multi-launch level 1: 124x60, 120x56, 116x52); the second set is one aligned
# pair past the multiple.
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("nx,ny,nu", [(248, 120, (1, 1)), (240, 112, (2, 2)), (232, 104, (3, 3)),
                                      (252, 124, (1, 1)), (244, 116, (2, 2)), (236, 108, (3, 1))])
def test_tile_edges(nx, ny, nu, fused, monkeypatch):
    if not fused:
        monkeypatch.setenv("CFD_MG_FUSED", "0")
    pl = M.plan(nx, ny)
    assert M.tail(pl) == 2  # level 1 is multi-launch
    cycles, res, _ = check_solve(nx, ny, nu, fused=fused)
    cp, f, _ = fixture(nx, ny)
    assert res <= cp.tol_factor * np.abs(f).max() and cycles <= 15


_ORACLE_STEPS = {}


def oracle_steps(case, nx, ny, nu, steps=4):
    """`steps` steps of the oracle's phases around the restatement's solve, once per case."""
    key = (case, nx, ny, nu)
    if key not in _ORACLE_STEPS:
        cp = C.make_params(case, nx=nx, ny=ny, **({"re": 1000.0} if case == "cavity" else {}))
        o = O.Oracle(cp, ordering=O.RB)  # (the order is the SOR loop's, which these steps do not run)
        rows = [M.oracle_step(o, cp, nu1=nu[0], nu2=nu[1]) for _ in range(steps)]
        fields = {n: ofield(o, n, cp).copy() for n in ("u", "v", "p")}
        if case == "rayleigh_benard":
            fields["t"] = o.field("t").copy()
        md, ke = o.stats()  # (and the red-black order's tree sum of the kinetic energy, restated: tests/rb_sums.py)
        _ORACLE_STEPS[key] = (cp, rows, fields, (md, ke, R.oracle_ke(o, R.strips_of(ny, 1))))
    return _ORACLE_STEPS[key]


@pytest.mark.parametrize("case,nx,ny,ordering,nu", [
    ("cavity", 96, 64, "lex", (2, 2)), ("cavity", 96, 64, "rb", (2, 2)),
    ("cavity", 240, 120, "lex", (2, 2)), ("cavity", 240, 120, "rb", (2, 2)),
    ("cavity", 240, 120, "lex", (4, 1)),  # the second buffer's parity carried from solve to solve
    ("rayleigh_benard", 128, 32, "auto", (2, 2))])
def test_four_steps_are_the_oracles(case, nx, ny, ordering, nu):
    """Every solve of four whole steps, not only the first, against the CPU: per step (cycles,
    residual), then u, v, p (and T) bit for bit, the statistics and the counters."""
    cp, rows, want, (omd, oke, oke_rb) = oracle_steps(case, nx, ny, nu)
    cls = C.RayleighBenardSolver if case == "rayleigh_benard" else C.CavitySolver
    g = cls(cp, ordering=ordering, poisson="multigrid", mg_options=nu_opts(nu))
    got = [g.step() for _ in range(4)]
    for k, (a, b) in enumerate(zip(got, rows)):
        print(f"{case} {nx}x{ny} {ordering} V{nu} step {k + 1}: gpu {a[0]} cycles residual {a[1]!r}; "
              f"oracle {b[0]} cycles residual {b[1]!r}")
    assert got == rows
    assert all(c <= 15 for c, _ in rows)
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), want[n], f"{case} {nx}x{ny} {ordering} V{nu} after 4 steps: {n}")
    if case == "rayleigh_benard":
        assert_bits(g.field("t")[1:-1, 1:-1], want["t"][1:-1, 1:-1], "T after 4 steps")
    md, ke = g.statistics()
    assert md == omd and ke == (oke if ordering == "lex" else oke_rb)
    info, total = g.mg_info(), sum(c for c, _ in rows)
    assert (info.solves, info.cycles) == (4, total)
    assert info.launches == total * M.launches_per_cycle(M.plan(nx, ny), nu[0], nu[1], True)
    assert g.timing().poisson_launches == info.launches
    g.reset_timing()
    info = g.mg_info()
    assert (info.solves, info.cycles, info.launches) == (0, 0, 0)
    assert info.levels == len(M.plan(nx, ny))  # (the plan is no counter)
    g.close()


@pytest.mark.parametrize("nx,ny", [(48, 16), (240, 120)])
def test_solve_over_a_dirty_field(nx, ny):
    """p random, ghost cells included, before the solve: each solve starts from zero, ghosts too."""
    cp, f, (cycles, res, p) = reference_solve(nx, ny, 2, 2, 50)
    g = C.CavitySolver(cp, poisson="multigrid")
    g.set_field("src", f)
    dirty = np.random.default_rng(nx + ny).standard_normal((ny + 2, nx + 2))
    g.set_field("p", dirty)
    assert_bits(g.field("p"), dirty, "the dirty field")
    got = g.solverPressurePoisson()
    assert got == (cycles, res)
    assert_bits(g.field("p"), p, f"multigrid p {nx}x{ny} over a dirty field")
    g.set_field("p", dirty)  # and again, over the buffers the first solve left
    assert g.solverPressurePoisson() == (cycles, res)
    assert_bits(g.field("p"), p, f"multigrid p {nx}x{ny} over a dirty field, second solve")
    g.close()


def test_reentering_the_mode():
    """multigrid -> sor for two steps -> multigrid V(4,1): the next solve on the current
    source is the restatement's with those options, the plan is back."""
    cp = C.make_params("cavity", re=1000.0, nx=240, ny=120, max_iters=200)
    g = C.CavitySolver(cp, poisson="multigrid")
    levels = len(M.plan(240, 120))
    g.step()
    assert g.mg_info().levels == levels and g.timing().sor_kernel == 8
    g.set_poisson_method("sor")
    assert g.mg_info().levels == 0
    g.step()
    g.step()
    assert g.timing().sor_kernel != 8
    g.set_poisson_method("multigrid", {"pre_sweeps": 4, "post_sweeps": 1})
    info = g.mg_info()
    assert (info.levels, info.coarse_nx, info.coarse_ny, info.coarse_sweeps) == (levels, 30, 15, 120)
    f = g.field("src").copy()
    got = g.solverPressurePoisson()
    cycles, res, p, _ = M.solve(f, cp.dx, cp.tol_factor, 4, 1)
    print(f"re-entered V(4,1): gpu {got}; restatement {(cycles, res)}")
    assert got == (cycles, res) and cycles <= 15
    assert_bits(g.field("p"), p, "multigrid p after re-entering the mode")
    assert g.timing().sor_kernel == 8
    g.close()


def test_zero_source():
    cp = C.make_params("cavity", nx=16, ny=16)
    f = np.zeros((18, 18))
    assert M.solve(f, cp.dx, cp.tol_factor)[:2] == (1, 0.0)
    gc, gr, gp, tm, info = gpu_solve(cp, f, None)
    assert (gc, gr) == (1, 0.0)
    assert not gp.view(np.int64).any()
    assert_counters(16, 16, (2, 2), 1, True, tm, info)


@pytest.mark.parametrize("nx,ny", [(16, 16), (48, 16), (16, 48), (30, 18)])
def test_solves_the_reference_equations(nx, ny):
    """The GPU's p against a dense solve of the level-0 operator refined in long double (mg_reference.direct_solve),
    within what its reported residual allows: ||A^-1||_inf (res + 48 u ih2 max|p| + u max|f|)."""
    cp, f, _ = fixture(nx, ny)
    x, ainv, rmax = M.direct_solve(f, cp.dx)
    gc, gr, gp, _, _ = gpu_solve(cp, f, None)
    err = float(np.abs(gp - x).max())
    bound = M.yardstick_bound(f, cp.dx, gp, gr, ainv)
    print(f"{nx}x{ny}: {gc} cycles residual {gr:.3e}; refined residual {rmax:.3e}; max|p - x| {err:.3e} <= {bound:.3e}")
    assert gr <= cp.tol_factor * np.abs(f).max()
    assert rmax <= gr * 1e-3  # x is exact against what p is held to
    assert err <= bound


def run_steps(cp, steps, **kw):
    g = C.CavitySolver(cp, **kw)
    g.applyBoundaryConditions()
    rows = []
    for _ in range(steps):
        it, res = g.step()
        tol = cp.tol_factor * np.abs(g.field("src")).max()
        rows.append((it, res, tol, g.statistics()[0]))
    fields = {n: g.field(n).copy() for n in ("u", "v", "p")}
    tm = g.timing()
    g.close()
    return rows, fields, tm


def test_whole_steps_converge_where_sor_caps():
    cp = C.make_params("cavity", re=1000.0, nx=256, ny=256, max_iters=200)
    capped, _, _ = run_steps(cp, 3)
    mg, f_lex, tm = run_steps(cp, 3, poisson="multigrid", ordering="lex")
    mg_rb, f_rb, _ = run_steps(cp, 3, poisson="multigrid", ordering="rb")
    for k, ((it, res, tol, div), (cyc, mres, mtol, mdiv)) in enumerate(zip(capped, mg)):
        print(f"step {k + 1}: SOR {it} iterations residual {res:.3e} (tol {tol:.3e}) max div {div:.3e}; "
              f"multigrid {cyc} cycles residual {mres:.3e} (tol {mtol:.3e}) max div {mdiv:.3e}")
        assert it == 200 and res > tol
        assert mres <= mtol and cyc <= 15
        assert mdiv < div
    assert tm.sor_kernel == 8
    assert [r[:2] for r in mg] == [r[:2] for r in mg_rb]
    for n in ("u", "v", "p"):
        assert_bits(f_lex[n], f_rb[n], f"multigrid {n}: lex against rb solver")


def test_switching_back_gives_the_sor_bits():
    """A multigrid solve, then CFD_POISSON_SOR: the next steps are those of a
    solver that never switched - the oracle's, bit for bit (as test_gpu_small)."""
    cp = C.make_params("cavity", re=100.0, nx=64, ny=64, dt=1e-3)
    g = C.CavitySolver(cp, ordering="rb", poisson="multigrid")
    g.applyBoundaryConditions()
    g.computeTentativeVelocities()
    g.buildSourceTerm()
    cycles, _ = g.solverPressurePoisson()
    assert 0 < cycles <= 15 and g.timing().sor_kernel == 8 and g.mg_info().levels == 5
    g.set_poisson_method("sor")
    assert g.mg_info().levels == 0
    its = [g.step() for _ in range(5)]
    assert g.timing().sor_kernel != 8
    o = O.Oracle(cp, ordering=O.RB)
    assert its == [o.step() for _ in range(5)]
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), ofield(o, n, cp), f"after switching back: {n}")
    g.close()


def test_refusals_name_the_rule():
    cav = C.make_params("cavity", nx=64, ny=64)
    with pytest.raises(_lib.CfdError, match="strip rule"):
        C.CavitySolver(cav, n_strips=2, poisson="multigrid")
    L = _lib.lib()
    hub = L.cfd_comm_loopback_hub(1)
    comm = L.cfd_comm_init_loopback(hub, 0, 0)
    assert hub and comm
    try:
        with pytest.raises(_lib.CfdError, match="rank rule"):
            C.CavitySolver(cav, ordering="rb", rank_rows=(1, 64), comm=comm, poisson="multigrid")
    finally:
        L.cfd_comm_destroy(comm)
        L.cfd_comm_loopback_hub_destroy(hub)
    with pytest.raises(_lib.CfdError, match="case rule"):
        C.ChannelSolver(C.make_params("channel", nx=64, ny=64), poisson="multigrid")
    with pytest.raises(_lib.CfdError, match="case rule"):
        C.BackwardsStepSolver(C.reference_defaults("backwards_step"), poisson="multigrid")
    with pytest.raises(_lib.CfdError, match="grid rule"):
        C.CavitySolver(C.reference_defaults("cavity"), poisson="multigrid")  # 63^2
    g = C.CavitySolver(cav)  # a refused switch leaves the solver on SOR
    with pytest.raises(_lib.CfdError, match="options"):
        g.set_poisson_method("multigrid", {"max_cycles": -1})
    it, _ = g.step()
    assert g.timing().sor_kernel != 8 and it > 15
    g.close()


def test_rayleigh_benard_step():
    cp = C.make_params("rayleigh_benard", nx=128, ny=32)
    g = C.RayleighBenardSolver(cp, poisson="multigrid")
    g.applyBoundaryConditions()
    cycles, res = g.step()
    f = g.field("src").copy()
    p = g.field("p").copy()
    g.close()
    rc, rres, rp = M.solve(f, cp.dx, cp.tol_factor)[:3]
    print(f"Rayleigh-Benard 128x32: {cycles} cycles residual {res!r}")
    assert res <= cp.tol_factor * np.abs(f).max() and cycles <= 15
    assert (cycles, res) == (rc, rres)
    assert_bits(p, rp, "Rayleigh-Benard multigrid p")


def test_binary_multigrid_flag(tmp_path):
    exe = os.path.join(ROOT, "computational-fluid-dynamics_amd", "bin", "cavity")
    r = subprocess.run([exe, "--multigrid", "--Nx", "64", "--Ny", "64", "--steps", "3", "--no-vtk",
                        "--print-interval", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in re.sub(r"\x1b\[[0-9;]*m", "", r.stdout).splitlines() if l.startswith("Step ")]
    cp = C.make_params("cavity", nx=64, ny=64)
    cp.print_interval = 1
    out, err = io.StringIO(), io.StringIO()
    g = C.CavitySolver(cp, poisson="multigrid")
    g.run(output_directory=None, out=out, err=err, steps=3)
    g.close()
    want = [l for l in out.getvalue().splitlines() if l.startswith("Step ")]
    assert len(want) == 3 and lines == want
    assert all(0 < int(l.rsplit("=", 1)[1]) <= 15 for l in lines)
    assert "Warning" not in r.stderr and err.getvalue() == ""


def test_cycle_cap_in_the_drivers(tmp_path):
    """--mg-cycles 2 / max_cycles 2: every solve stops at the cap, the iteration column
    reads 2, and each step warns with the cap and that step's residual."""
    exe = os.path.join(ROOT, "computational-fluid-dynamics_amd", "bin", "cavity")
    r = subprocess.run([exe, "--multigrid", "--mg-cycles", "2", "--Nx", "64", "--Ny", "64", "--steps", "2", "--no-vtk",
                        "--print-interval", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ansi = re.compile(r"\x1b\[[0-9;]*m")
    lines = [l for l in ansi.sub("", r.stdout).splitlines() if l.startswith("Step ")]
    warns = [l for l in ansi.sub("", r.stderr).splitlines() if l.startswith("Warning")]
    cp = C.make_params("cavity", nx=64, ny=64)
    cp.print_interval = 1
    out, err = io.StringIO(), io.StringIO()
    g = C.CavitySolver(cp, poisson="multigrid", mg_options={"max_cycles": 2})
    g.run(output_directory=None, out=out, err=err, steps=2)
    g.close()
    want = [l for l in out.getvalue().splitlines() if l.startswith("Step ")]
    assert len(want) == 2 and lines == want
    assert all(int(l.rsplit("=", 1)[1]) == 2 for l in lines)
    # the residual each warning carries: the one solverPressurePoisson() returns for that step
    g = C.CavitySolver(cp, poisson="multigrid", mg_options={"max_cycles": 2})
    expect = []
    for _ in range(2):
        g.applyBoundaryConditions()
        g.computeTentativeVelocities()
        g.buildSourceTerm()
        cycles, res = g.solverPressurePoisson()
        g.applyPressureCorrection()
        assert cycles == 2 and res > cp.tol_factor * np.abs(g.field("src")).max()
        expect.append(logfmt.warning_line(cp.case_id, 2, res))
    g.close()
    assert err.getvalue().splitlines() == expect
    assert warns == expect
