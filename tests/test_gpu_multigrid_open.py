"""The channel's multigrid pressure solve (CFD_POISSON_MULTIGRID_OPEN: the mgo_*
kernels of csrc/mg.hip, DESIGN.md §8 "The channel") on the GPU: cycle counts,
residuals and p bit for bit the numpy restatement's (tests/mg_open_reference.py)
from a set source and a set, warm p at every size at which the kernels take
another path - the three transfer kinds, two-level and thin plans, grids on a
multiple of the smoothing tile, sweep counts whose fused launches end in a
level's second buffer, one launch per colour - and with other values in the
ghost cells; the launch counters; whole timesteps against the oracle's phases
around the restatement's solve; the switch to SOR and back; the refusals; the
drop-in binary."""
from __future__ import annotations

import io
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import mg_open_reference as M  # noqa: E402
import oracle as O  # noqa: E402
from cfd_amd import _lib  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_gpu_parity import assert_bits, ofield  # noqa: E402

_REF = {}


def fixture(nx, ny):
    """(params, source, p to start from - ghosts included, {options: the restatement's solve}), once per grid."""
    if (nx, ny) not in _REF:
        cp = C.make_params("channel", nx=nx, ny=ny)
        _REF[(nx, ny)] = (cp, M.random_source(nx, ny, seed=nx * 1000 + ny), M.random_field(nx, ny, nx + ny), {})
    return _REF[(nx, ny)]


def reference_solve(nx, ny, nu=(2, 2), max_cycles=50):
    cp, f, p0, cache = fixture(nx, ny)
    key = (nu, max_cycles)
    if key not in cache:
        cache[key] = M.solve(f, p0, cp.dx, cp.dy, cp.tol_factor, cp.abs_tol, nu[0], nu[1], max_cycles)[:3]
    return cp, f, p0, cache[key]


def nu_opts(nu, max_cycles=50):
    return {"pre_sweeps": nu[0], "post_sweeps": nu[1], "max_cycles": max_cycles}


def gpu_solve(cp, f, p0, opts):
    g = C.ChannelSolver(cp, poisson="multigrid-open", mg_options=opts)
    g.set_field("src", f)
    g.set_field("p", p0)
    cycles, res = g.solverPressurePoisson()
    p = g.field("p").copy()
    tm, info = g.timing(), g.mg_info()
    g.close()
    return cycles, res, p, tm, info


def assert_counters(cp, nu, cycles, fused, tm, info, solves=1):
    """Launches, sweeps and cell updates of `cycles` cycles (mg_open_reference.launches_per_cycle)."""
    pl = M.plan(cp.nx, cp.ny, cp.dx, cp.dy)
    per = M.launches_per_cycle(pl, nu[0], nu[1], fused)
    assert (info.solves, info.cycles) == (solves, cycles)
    assert info.launches == cycles * per, (info.launches, cycles, per)
    assert tm.poisson_launches == info.launches
    assert tm.poisson_sweeps == cycles * (nu[0] + nu[1])
    assert tm.poisson_cell_updates == cp.nx * cp.ny * cycles * (nu[0] + nu[1])
    assert (info.levels, info.coarse_nx, info.coarse_ny) == (len(pl), *pl[-1])
    assert info.coarse_sweeps == 4 * max(pl[-1])
    assert _lib.SOR_KERNEL[tm.sor_kernel] == "multigrid" and tm.sor_kernel == 8


def check_solve(nx, ny, nu=(2, 2), max_cycles=50, fused=True):
    """One GPU solve of the grid's fixture: (cycles, residual), p and the counters are the restatement's."""
    cp, f, p0, (cycles, res, p) = reference_solve(nx, ny, nu, max_cycles)
    gc, gr, gp, tm, info = gpu_solve(cp, f, p0, nu_opts(nu, max_cycles))
    what = f"{nx}x{ny} V{nu} max_cycles {max_cycles} {'fused' if fused else 'colour launches'}"
    print(f"{what}: gpu {gc} cycles residual {gr!r}; restatement {cycles} cycles residual {res!r}; "
          f"levels {info.levels}, launches {info.launches}")
    assert (gc, gr) == (cycles, res), what
    assert_bits(gp, p, "open multigrid p " + what)
    assert_counters(cp, nu, cycles, fused, tm, info)
    if max_cycles == 50:
        assert res <= M.tolerance(f, cp.tol_factor, cp.abs_tol), what
    return cycles, res, info


# 48x16, 96x32, 256x32: full coarsening (256x32 after one x-only level); 16x48, 64x64, 240x120, 272x144, 512x512:
# y-only levels first (272x144: past the 128-column block, a pitch rounded up; 512x512: levels 0-3 multi-launch,
# two of them y-only); 512x64: x-only first. Two-level and thin plans: 8x8, 30x18, 126x60 (a 126x30 coarsest
# level, 504 sweeps; 126x90 has no plan: test_refusals_name_the_rule), 512x16, 16x512, 1024x8, 8x1024.
GRIDS = [(48, 16), (16, 48), (96, 32), (256, 32), (64, 64), (240, 120), (272, 144), (512, 64), (512, 512),
         (8, 8), (30, 18), (126, 60), (512, 16), (16, 512), (1024, 8), (8, 1024)]


@pytest.mark.parametrize("nx,ny", GRIDS)
def test_solve_is_the_restatement(nx, ny):
    check_solve(nx, ny)


# The smoothing tile owns 124x60, 120x56 or 116x52 cells for 1, 2 or 3 sweeps per launch and the grid is
# n / T + 1 blocks: on a multiple of the tile the last block owns one column or row; the second set is one
# aligned pair past the multiple.
TILE_EDGES = [(248, 120, (1, 1)), (240, 112, (2, 2)), (232, 104, (3, 3)),
              (252, 124, (1, 1)), (244, 116, (2, 2)), (236, 108, (3, 3))]


@pytest.mark.parametrize("nx,ny,nu", TILE_EDGES)
def test_tile_edges(nx, ny, nu):
    check_solve(nx, ny, nu)


# Sweep counts that give 3 fused smoothing launches per multi-launch level and cycle (4 runs as 2 + 2, 5 as
# 3 + 2): after an odd number of cycles the field of level 0 is in the second buffer (the refresh and the
# residual pass work on it there; solve_mg_open copies it back, corners excepted).
@pytest.mark.parametrize("max_cycles", [50, 1, 2])
@pytest.mark.parametrize("nu", [(4, 1), (1, 4), (5, 1)])
@pytest.mark.parametrize("nx,ny", [(240, 120), (256, 32)])
def test_second_buffer(nx, ny, nu, max_cycles):
    assert M.smoothing_launches(nu[0], True) + M.smoothing_launches(nu[1], True) == 3
    cycles, _, _ = check_solve(nx, ny, nu, max_cycles)
    assert cycles == max_cycles or max_cycles == 50


# one case per grid class with one in-place launch per colour: the same bits, 2 (nu1 + nu2) smoothing launches
@pytest.mark.parametrize("nx,ny,nu", [(96, 32, (2, 2)), (512, 512, (2, 2)), (30, 18, (2, 2)), (512, 16, (2, 2)),
                                      (8, 1024, (2, 2)), (248, 120, (1, 1)), (240, 120, (4, 1))])
def test_colour_launches(nx, ny, nu, monkeypatch):
    monkeypatch.setenv("CFD_MG_FUSED", "0")
    check_solve(nx, ny, nu, fused=False)


@pytest.mark.parametrize("nx,ny,nu", [(96, 32, (2, 2)), (240, 120, (2, 2)), (240, 120, (4, 1)), (512, 64, (2, 2))])
def test_ghosts_reach_no_result(nx, ny, nu):
    """The same solve with other finite values in p's ghost cells (corners kept): the same bits."""
    cp, f, p0, (cycles, res, p) = reference_solve(nx, ny, nu, 50)
    other = p0.copy()
    g = np.random.default_rng(9).standard_normal(p0.shape) * 1e3
    other[0, 1:-1], other[-1, 1:-1], other[1:-1, 0], other[1:-1, -1] = g[0, 1:-1], g[-1, 1:-1], g[1:-1, 0], g[1:-1, -1]
    gc, gr, gp, _, _ = gpu_solve(cp, f, other, nu_opts(nu))
    assert (gc, gr) == (cycles, res)
    assert_bits(gp, p, f"open multigrid p {nx}x{ny} V{nu} from other ghosts")


def test_max_cycles_stops_unconverged():
    cp, f, p0, (cycles, res, p) = reference_solve(240, 120, (2, 2), 2)
    assert cycles == 2 and res > M.tolerance(f, cp.tol_factor, cp.abs_tol)
    check_solve(240, 120, (2, 2), 2)


def test_zero_source():
    """A zero source: tol = max(tol_factor, abs_tol) and the loop primed with tol + 1 run one cycle -
    zeros from a zero field; from a warm field what the restatement's one cycle gives."""
    cp = C.make_params("channel", nx=96, ny=32)
    f = np.zeros((34, 98))
    for p0 in (np.zeros_like(f), M.random_field(96, 32, 4)):
        cycles, res, p, _ = M.solve(f, p0, cp.dx, cp.dy, cp.tol_factor, cp.abs_tol, max_cycles=1)
        gc, gr, gp, tm, info = gpu_solve(cp, f, p0, {"max_cycles": 1})
        assert (gc, gr) == (cycles, res) and cycles == 1
        assert_bits(gp, p, "open multigrid p, zero source")
        assert_counters(cp, (2, 2), 1, True, tm, info)
        if not p0.any():
            assert res == 0.0 and not gp.view(np.int64).any()
            assert gpu_solve(cp, f, p0, None)[:2] == (1, 0.0)  # (and it stops there)


_ORACLE_STEPS = {}


def oracle_steps(nx, ny, nu, steps=4):
    """`steps` steps of the oracle's phases around the restatement's solve, once per grid."""
    key = (nx, ny, nu)
    if key not in _ORACLE_STEPS:
        cp = C.make_params("channel", re=100.0, nx=nx, ny=ny)
        o = O.Oracle(cp, ordering=O.LEX)
        o.velocity_bc(False)  # (the state the solver is created in)
        rows = [M.oracle_step(o, cp, nu1=nu[0], nu2=nu[1]) for _ in range(steps)]
        fields = {n: ofield(o, n, cp).copy() for n in ("u", "v", "p")}
        _ORACLE_STEPS[key] = (cp, rows, fields, o.stats())
    return _ORACLE_STEPS[key]


@pytest.mark.parametrize("nx,ny,nu", [(96, 32, (2, 2)), (256, 32, (2, 2)), (240, 120, (2, 2)), (240, 120, (4, 1))])
def test_four_steps_are_the_oracles(nx, ny, nu):
    """Channel Re 100, ordering lex: per step (cycles, residual), then u, v, p bit for bit,
    the statistics and the counters."""
    cp, rows, want, (omd, oke) = oracle_steps(nx, ny, nu)
    g = C.ChannelSolver(cp, ordering="lex", poisson="multigrid-open", mg_options=nu_opts(nu))
    got = [g.step() for _ in range(4)]
    for k, (a, b) in enumerate(zip(got, rows)):
        print(f"channel {nx}x{ny} V{nu} step {k + 1}: gpu {a[0]} cycles residual {a[1]!r}; "
              f"oracle {b[0]} cycles residual {b[1]!r}")
    assert got == rows
    assert all(c <= 20 for c, _ in rows)
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), want[n], f"channel {nx}x{ny} V{nu} after 4 steps: {n}")
    md, ke = g.statistics()
    assert md == omd and ke == oke  # (the reference order sums the kinetic energy sequentially, as the oracle)
    assert_counters(cp, nu, sum(c for c, _ in rows), True, g.timing(), g.mg_info(), solves=4)
    g.reset_timing()
    info = g.mg_info()
    assert (info.solves, info.cycles, info.launches) == (0, 0, 0)
    assert info.levels == len(M.plan(nx, ny, cp.dx, cp.dy))  # (the plan is no counter)
    g.close()


def test_red_black_run():
    """ordering rb (the source's mean by a tree sum: no oracle bits): each step's residual meets the
    tolerance, and each step's p is the restatement's solve of the GPU's own source from its own previous p."""
    cp = C.make_params("channel", re=100.0, nx=256, ny=32)
    g = C.ChannelSolver(cp, ordering="rb", poisson="multigrid-open")
    for k in range(4):
        before = g.field("p").copy()
        cycles, res = g.step()
        f = g.field("src").copy()
        tol = M.tolerance(f, cp.tol_factor, cp.abs_tol)
        rc, rres, rp, _ = M.solve(f, before, cp.dx, cp.dy, cp.tol_factor, cp.abs_tol)
        print(f"rb step {k + 1}: gpu {cycles} cycles residual {res!r} (tol {tol:.3e}); restatement {rc} {rres!r}")
        assert res <= tol and cycles <= 20
        assert (cycles, res) == (rc, rres)
        assert_bits(g.field("p"), rp, f"rb step {k + 1}: p")
    g.close()


def test_switching_back_gives_the_oracles_bits():
    """SOR for two steps, multigrid-open for two, then CFD_POISSON_SOR: the steps after switching
    back are the oracle's bits from the field the multigrid steps left."""
    cp = C.make_params("channel", re=100.0, nx=96, ny=32, max_iters=400)
    o = O.Oracle(cp, ordering=O.LEX)
    o.velocity_bc(False)  # (the state the solver is created in)
    g = C.ChannelSolver(cp, ordering="lex")
    assert [g.step() for _ in range(2)] == [o.step() for _ in range(2)]
    assert g.timing().sor_kernel != 8 and g.mg_info().levels == 0
    g.set_poisson_method("multigrid-open")
    assert g.mg_info().levels == 4
    assert [g.step() for _ in range(2)] == [M.oracle_step(o, cp) for _ in range(2)]
    assert g.timing().sor_kernel == 8
    g.set_poisson_method("sor")
    assert g.mg_info().levels == 0
    assert [g.step() for _ in range(3)] == [o.step() for _ in range(3)]
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), ofield(o, n, cp), f"after switching back: {n}")
    assert g.timing().sor_kernel != 8
    g.close()


@pytest.mark.parametrize("ordering", ["lex", "rb"])
def test_switching_back_is_a_solver_that_never_switched(ordering):
    """Either ordering (rb has no oracle bits: its source mean is a tree sum): after multigrid-open
    steps and the switch back, the next steps are those of a fresh SOR solver given the same u, v, p."""
    cp = C.make_params("channel", re=100.0, nx=96, ny=32, max_iters=400)
    g = C.ChannelSolver(cp, ordering=ordering)
    g.step()
    g.set_poisson_method("multigrid-open", {"pre_sweeps": 4, "post_sweeps": 1})  # (ends in the second buffer too)
    g.step()
    g.step()
    g.set_poisson_method("sor")
    h = C.ChannelSolver(cp, ordering=ordering)
    for n in ("u", "v", "p"):
        h.set_field(n, g.field(n))
    assert [g.step() for _ in range(3)] == [h.step() for _ in range(3)]
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), h.field(n), f"after switching back ({ordering}): {n}")
    assert g.timing().sor_kernel != 8
    g.close()
    h.close()


def test_refusals_name_the_rule():
    ch = C.make_params("channel", nx=96, ny=32)
    with pytest.raises(_lib.CfdError, match="case rule.*CFD_POISSON_MULTIGRID|CFD_POISSON_MULTIGRID.*case rule"):
        C.CavitySolver(C.make_params("cavity", nx=64, ny=64), poisson="multigrid-open")
    with pytest.raises(_lib.CfdError, match="case rule"):
        C.RayleighBenardSolver(C.make_params("rayleigh_benard", nx=128, ny=32), poisson="multigrid-open")
    with pytest.raises(_lib.CfdError, match="case rule"):
        C.BackwardsStepSolver(C.reference_defaults("backwards_step"), poisson="multigrid-open")
    with pytest.raises(_lib.CfdError, match="case rule"):  # method 1 keeps refusing the channel
        C.ChannelSolver(ch, poisson="multigrid")
    with pytest.raises(_lib.CfdError, match="grid rule"):
        C.ChannelSolver(C.reference_defaults("channel"), poisson="multigrid-open")  # 93x31
    with pytest.raises(_lib.CfdError, match="grid rule"):
        C.ChannelSolver(C.make_params("channel", nx=126, ny=90), poisson="multigrid-open")  # 126x45: 5670 cells
    with pytest.raises(_lib.CfdError, match="strip rule"):
        C.ChannelSolver(ch, n_strips=2, poisson="multigrid-open")
    L = _lib.lib()
    hub = L.cfd_comm_loopback_hub(1)
    comm = L.cfd_comm_init_loopback(hub, 0, 0)
    assert hub and comm
    try:
        with pytest.raises(_lib.CfdError, match="rank rule"):
            C.ChannelSolver(ch, ordering="rb", rank_rows=(1, 32), comm=comm, poisson="multigrid-open")
    finally:
        L.cfd_comm_destroy(comm)
        L.cfd_comm_loopback_hub_destroy(hub)
    cp = C.make_params("channel", re=100.0, nx=96, ny=32, max_iters=400)
    g = C.ChannelSolver(cp)  # a refused switch leaves the solver on SOR
    with pytest.raises(_lib.CfdError, match="options"):
        g.set_poisson_method("multigrid-open", {"max_cycles": -1})
    with pytest.raises(_lib.CfdError, match="options"):
        g.set_poisson_method("multigrid-open", {"pre_sweeps": -1})
    o = O.Oracle(cp, ordering=O.LEX)
    o.velocity_bc(False)  # (the state the solver is created in)
    assert g.step() == o.step()
    assert g.timing().sor_kernel != 8 and g.mg_info().levels == 0
    g.close()


def ppe_iters(line):
    """The iteration column of the channel's log line (channel-01.cpp:762-768)."""
    return int(re.search(r"PPE iters=\s*(\d+)", line).group(1))


def test_binary_multigrid_open_flag(tmp_path):
    exe = os.path.join(ROOT, "computational-fluid-dynamics_amd", "bin", "channel")
    args = ["--Nx", "96", "--Ny", "32", "--steps", "3", "--no-vtk", "--print-interval", "1"]
    r = subprocess.run([exe, "--multigrid-open"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in re.sub(r"\x1b\[[0-9;]*m", "", r.stdout).splitlines() if l.startswith("Step ")]
    cp = C.make_params("channel", nx=96, ny=32)
    cp.print_interval = 1
    out, err = io.StringIO(), io.StringIO()
    g = C.ChannelSolver(cp, poisson="multigrid-open")
    g.run(output_directory=None, out=out, err=err, steps=3)
    g.close()
    want = [l for l in out.getvalue().splitlines() if l.startswith("Step ")]
    assert len(want) == 3 and lines == want
    assert all(0 < ppe_iters(l) <= 20 for l in lines)
    assert "Warning" not in r.stderr and err.getvalue() == ""
    r = subprocess.run([exe, "--multigrid"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "case rule" in r.stderr  # --multigrid on the channel keeps failing


def test_cycle_cap_in_the_drivers():
    """max_cycles 1: run() reads the cap for both multigrid methods alike - the iteration column is 1
    and each step warns with the cap."""
    cp = C.make_params("channel", nx=96, ny=32)
    cp.print_interval = 1
    out, err = io.StringIO(), io.StringIO()
    g = C.ChannelSolver(cp, poisson="multigrid-open", mg_options={"max_cycles": 1})
    g.run(output_directory=None, out=out, err=err, steps=2)
    g.close()
    lines = [l for l in out.getvalue().splitlines() if l.startswith("Step ")]
    assert len(lines) == 2 and all(ppe_iters(l) == 1 for l in lines)
    warns = [l for l in re.sub(r"\x1b\[[0-9;]*m", "", err.getvalue()).splitlines() if l.startswith("Warning")]
    assert len(warns) == 2
