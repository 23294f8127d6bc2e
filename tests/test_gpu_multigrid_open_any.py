"""The channel's any-size multigrid pressure solve (CFD_POISSON_MULTIGRID_OPEN_ANY:
the scheme MgChannelAny of csrc/mg.hip) on the GPU: cycle counts,
residuals and p bit for bit the numpy restatement's
(tests/mg_open_any_reference.py) from a set source and a set, warm p at every size
at which the kernels take another path - two-level plans with an odd coarse
level, the reference's 93x31 and its transpose, grids with irregular
multi-launch levels and both transfer kinds, the last column and row alone in
the last smoothing tile, sweep counts whose fused launches end in a level's
second buffer, one launch per colour - the launch counters; method 2's bits
where the plans are equal; whole timesteps against the oracle's phases around
the restatement's solve; the switch back to SOR; the refusals; the drop-in
binary at its default grid."""
from __future__ import annotations

import io
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import mg_open_any_reference as A  # noqa: E402
import mg_open_reference as M  # noqa: E402
import oracle as O  # noqa: E402
from cfd_amd import _lib  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_gpu_parity import assert_bits, ofield  # noqa: E402

METHOD = "multigrid-open-any"
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
        cache[key] = A.solve(f, p0, cp.dx, cp.dy, cp.tol_factor, cp.abs_tol, nu[0], nu[1], max_cycles)[:3]
    return cp, f, p0, cache[key]


def nu_opts(nu, max_cycles=50):
    return {"pre_sweeps": nu[0], "post_sweeps": nu[1], "max_cycles": max_cycles}


def gpu_solve(cp, f, p0, opts, method=METHOD, solves=1):
    g = C.ChannelSolver(cp, poisson=method, mg_options=opts)
    out = []
    for _ in range(solves):
        g.set_field("src", f)
        g.set_field("p", p0)
        cycles, res = g.solverPressurePoisson()
        out.append((cycles, res, g.field("p").copy()))
    tm, info = g.timing(), g.mg_info()
    g.close()
    return out if solves > 1 else (*out[0], tm, info)


def assert_counters(cp, nu, cycles, fused, tm, info, solves=1):
    """Launches, sweeps and cell updates of `cycles` cycles (launches_per_cycle: tail (smoothing + 2) + 3)."""
    pl = A.plan(cp.nx, cp.ny, cp.dx, cp.dy)
    per = A.launches_per_cycle(pl, nu[0], nu[1], fused)
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
    assert_bits(gp, p, "any-size open multigrid p " + what)
    assert_counters(cp, nu, cycles, fused, tm, info)
    if max_cycles == 50:
        assert res <= M.tolerance(f, cp.tol_factor, cp.abs_tol), what
    return cycles, res, info


# 13x9 (y only to 13x5) and 9x9 (y only to 9x5): two levels, an odd coarse one; the reference's 93x31 (full, 47x16:
# an odd x, a single child) and 31x93 (y only first); 50x17 (x: a single child on level 1; y: single children on
# levels 0 and 1) and 17x40 (y only three times, the last from 10 to 5); 253x131: y only to 253x66, then full to
# 127x33 - two irregular multi-launch levels (the tail starts at level 3) and both transfer kinds.
GRIDS = [(13, 9), (9, 9), (93, 31), (31, 93), (50, 17), (17, 40), (253, 131)]


@pytest.mark.parametrize("nx,ny", GRIDS)
def test_solve_is_the_restatement(nx, ny):
    check_solve(nx, ny)


def test_plans_are_as_the_cases_say():
    pl = lambda nx, ny: C.mg_open_any_plan(C.make_params("channel", nx=nx, ny=ny))
    assert pl(13, 9) == [(13, 9), (13, 5)] and pl(9, 9) == [(9, 9), (9, 5)]
    assert pl(253, 131)[:4] == [(253, 131), (253, 66), (127, 33), (64, 17)]
    cp = C.make_params("channel", nx=253, ny=131)
    assert A.tail(A.plan(253, 131, cp.dx, cp.dy)) == 3 and 253 * 66 == 16698 and 127 * 33 == 4191


def test_colour_launches_253x131(monkeypatch):
    monkeypatch.setenv("CFD_MG_FUSED", "0")
    check_solve(253, 131, fused=False)


# The smoothing tile owns 124x60, 120x56 or 116x52 cells for 1, 2 or 3 sweeps per launch and the grid is
# n / T + 1 blocks: one past a multiple of the tile the last block owns the last column and row alone - an
# odd size, whose level 1 is irregular; 127x63 is one aligned pair beyond 125x61.
TILE_EDGES = [(125, 61, (1, 1)), (121, 57, (2, 2)), (117, 53, (3, 3)), (127, 63, (1, 1))]


@pytest.mark.parametrize("nx,ny,nu", TILE_EDGES)
def test_tile_edges(nx, ny, nu):
    check_solve(nx, ny, nu)


# V(4,1): 3 fused smoothing launches per multi-launch level and cycle (4 runs as 2 + 2): after an odd number of
# cycles the field of level 0 is in the second buffer (the refresh and the residual pass work on it there; it
# is copied back, corners excepted).
@pytest.mark.parametrize("max_cycles", [50, 1, 2])
def test_second_buffer(max_cycles):
    assert M.smoothing_launches(4, True) + M.smoothing_launches(1, True) == 3
    cycles, _, _ = check_solve(253, 131, (4, 1), max_cycles)
    assert cycles == max_cycles or max_cycles == 50


def test_a_random_start_run_twice():
    """From a random p, ghosts included; the second solve on the same solver (its level buffers used once
    already) gives the same bits."""
    cp, f, p0, (cycles, res, p) = reference_solve(93, 31)
    for gc, gr, gp in gpu_solve(cp, f, p0, None, solves=2):
        assert (gc, gr) == (cycles, res)
        assert_bits(gp, p, "any-size open multigrid p 93x31, run twice")
    other = p0.copy()  # other finite values in the ghost cells (corners kept): the same bits
    g = np.random.default_rng(9).standard_normal(p0.shape) * 1e3
    other[0, 1:-1], other[-1, 1:-1], other[1:-1, 0], other[1:-1, -1] = g[0, 1:-1], g[-1, 1:-1], g[1:-1, 0], g[1:-1, -1]
    gc, gr, gp, _, _ = gpu_solve(cp, f, other, None)
    assert (gc, gr) == (cycles, res)
    assert_bits(gp, p, "any-size open multigrid p 93x31 from other ghosts")


def test_zero_source():
    """A zero source: tol = max(tol_factor, abs_tol) and the loop primed with tol + 1 run one cycle -
    zeros from a zero field; from a warm field what the restatement's one cycle gives."""
    cp = C.make_params("channel", nx=93, ny=31)
    f = np.zeros((33, 95))
    for p0 in (np.zeros_like(f), M.random_field(93, 31, 4)):
        cycles, res, p, _ = A.solve(f, p0, cp.dx, cp.dy, cp.tol_factor, cp.abs_tol, max_cycles=1)
        gc, gr, gp, tm, info = gpu_solve(cp, f, p0, {"max_cycles": 1})
        assert (gc, gr) == (cycles, res) and cycles == 1
        assert_bits(gp, p, "any-size open multigrid p, zero source")
        assert_counters(cp, (2, 2), 1, True, tm, info)
        if not p0.any():
            assert res == 0.0 and not gp.view(np.int64).any()


@pytest.mark.parametrize("nx,ny", [(96, 32), (512, 64)])
def test_method_2s_bits_on_one_solver(nx, ny):
    """Where the two plans are equal: methods 2 and 5 in turn on one solver give the same cycles, residual and p."""
    cp, f, p0, _ = fixture(nx, ny)
    assert C.mg_open_any_plan(cp) == C.mg_open_plan(cp)
    g = C.ChannelSolver(cp)
    got = []
    for method in ("multigrid-open", METHOD, "multigrid-open"):
        g.set_poisson_method(method)
        g.set_field("src", f)
        g.set_field("p", p0)
        got.append((*g.solverPressurePoisson(), g.field("p").copy()))
    g.close()
    want = M.solve(f, p0, cp.dx, cp.dy, cp.tol_factor, cp.abs_tol)
    for c, r, p in got:
        assert (c, r) == (want[0], want[1])
        assert_bits(p, want[2], f"methods 2 and 5 at {nx}x{ny}")


_ORACLE_STEPS = {}


def oracle_steps(nx, ny, steps=4):
    """`steps` steps of the oracle's phases around the restatement's solve, then two of its own SOR
    steps, once per grid."""
    if (nx, ny) not in _ORACLE_STEPS:
        cp = C.make_params("channel", re=100.0, nx=nx, ny=ny, max_iters=400)
        o = O.Oracle(cp, ordering=O.LEX)
        o.velocity_bc(False)  # (the state the solver is created in)
        rows = [A.oracle_step(o, cp) for _ in range(steps)]
        fields = {n: ofield(o, n, cp).copy() for n in ("u", "v", "p")}
        stats = o.stats()
        sor = [o.step() for _ in range(2)]
        after = {n: ofield(o, n, cp).copy() for n in ("u", "v", "p")}
        _ORACLE_STEPS[(nx, ny)] = (cp, rows, fields, stats, sor, after)
    return _ORACLE_STEPS[(nx, ny)]


@pytest.mark.parametrize("nx,ny", [(93, 31), (125, 61)])
def test_four_steps_are_the_oracles_lex(nx, ny):
    """Channel Re 100, ordering lex: per step (cycles, residual), then u, v, p bit for bit, the
    statistics and the counters; the two SOR steps after switching back are the oracle's."""
    cp, rows, want, (omd, oke), sor, after = oracle_steps(nx, ny)
    g = C.ChannelSolver(cp, ordering="lex", poisson=METHOD)
    got = [g.step() for _ in range(4)]
    for k, (a, b) in enumerate(zip(got, rows)):
        print(f"channel {nx}x{ny} step {k + 1}: gpu {a[0]} cycles residual {a[1]!r}; oracle {b[0]} cycles residual {b[1]!r}")
    assert got == rows
    assert all(c <= 20 for c, _ in rows)
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), want[n], f"channel {nx}x{ny} after 4 steps: {n}")
    md, ke = g.statistics()
    assert md == omd and ke == oke  # (the reference order sums the kinetic energy sequentially, as the oracle)
    assert_counters(cp, (2, 2), sum(c for c, _ in rows), True, g.timing(), g.mg_info(), solves=4)
    g.set_poisson_method("sor")
    assert g.mg_info().levels == 0
    assert [g.step() for _ in range(2)] == sor
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), after[n], f"channel {nx}x{ny} after switching back: {n}")
    assert g.timing().sor_kernel != 8
    g.close()


@pytest.mark.parametrize("nx,ny", [(93, 31), (125, 61)])
def test_four_steps_rb(nx, ny):
    """ordering rb (the source's mean by a tree sum: no oracle bits): each step's p is the restatement's
    solve of the GPU's own source from its own previous p; the two SOR steps after switching back are
    those of a fresh SOR solver given the same u, v, p."""
    cp = C.make_params("channel", re=100.0, nx=nx, ny=ny, max_iters=400)
    g = C.ChannelSolver(cp, ordering="rb", poisson=METHOD)
    for k in range(4):
        before = g.field("p").copy()
        cycles, res = g.step()
        f = g.field("src").copy()
        tol = M.tolerance(f, cp.tol_factor, cp.abs_tol)
        rc, rres, rp, _ = A.solve(f, before, cp.dx, cp.dy, cp.tol_factor, cp.abs_tol)
        print(f"rb {nx}x{ny} step {k + 1}: gpu {cycles} cycles residual {res!r} (tol {tol:.3e}); restatement {rc} {rres!r}")
        assert res <= tol and cycles <= 20
        assert (cycles, res) == (rc, rres)
        assert_bits(g.field("p"), rp, f"rb step {k + 1}: p")
    g.set_poisson_method("sor")
    h = C.ChannelSolver(cp, ordering="rb")
    for n in ("u", "v", "p"):
        h.set_field(n, g.field(n))
    assert [g.step() for _ in range(2)] == [h.step() for _ in range(2)]
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), h.field(n), f"rb {nx}x{ny} after switching back: {n}")
    g.close()
    h.close()


def test_refusals_name_the_rule():
    ch = C.make_params("channel", nx=93, ny=31)
    with pytest.raises(_lib.CfdError, match="case rule.*CFD_POISSON_MULTIGRID_ANY"):
        C.CavitySolver(C.make_params("cavity", nx=63, ny=63), poisson=METHOD)
    with pytest.raises(_lib.CfdError, match="case rule"):
        C.RayleighBenardSolver(C.make_params("rayleigh_benard", nx=128, ny=32), poisson=METHOD)
    with pytest.raises(_lib.CfdError, match="case rule.*CFD_POISSON_MULTIGRID_STEP"):
        C.BackwardsStepSolver(C.reference_defaults("backwards_step"), poisson=METHOD)
    with pytest.raises(_lib.CfdError, match="grid rule"):
        C.ChannelSolver(C.make_params("channel", nx=13, ny=5), poisson=METHOD)
    with pytest.raises(_lib.CfdError, match="grid rule"):
        C.ChannelSolver(C.make_params("channel", nx=50, ny=3), poisson=METHOD)
    with pytest.raises(_lib.CfdError, match="grid rule"):  # method 2 keeps refusing the reference's grid
        C.ChannelSolver(C.reference_defaults("channel"), poisson="multigrid-open")
    with pytest.raises(_lib.CfdError, match="strip rule"):
        C.ChannelSolver(ch, n_strips=2, poisson=METHOD)
    L = _lib.lib()
    hub = L.cfd_comm_loopback_hub(1)
    comm = L.cfd_comm_init_loopback(hub, 0, 0)
    assert hub and comm
    try:
        with pytest.raises(_lib.CfdError, match="rank rule"):
            C.ChannelSolver(ch, ordering="rb", rank_rows=(1, 31), comm=comm, poisson=METHOD)
    finally:
        L.cfd_comm_destroy(comm)
        L.cfd_comm_loopback_hub_destroy(hub)
    cp = C.make_params("channel", re=100.0, nx=93, ny=31, max_iters=400)
    g = C.ChannelSolver(cp)  # a refused switch leaves the solver on SOR
    with pytest.raises(_lib.CfdError, match="options"):
        g.set_poisson_method(METHOD, {"max_cycles": -1})
    with pytest.raises(_lib.CfdError, match="options"):
        g.set_poisson_method(METHOD, {"pre_sweeps": -1})
    o = O.Oracle(cp, ordering=O.LEX)
    o.velocity_bc(False)  # (the state the solver is created in)
    assert g.step() == o.step()
    assert g.timing().sor_kernel != 8 and g.mg_info().levels == 0
    g.close()


def ppe_iters(line):
    """The iteration column of the channel's log line (channel-01.cpp:762-768)."""
    return int(re.search(r"PPE iters=\s*(\d+)", line).group(1))


def test_binary_at_its_default_grid(tmp_path):
    """bin/channel --multigrid-open-any with no --Nx / --Ny (93x31): the restatement's cycle counts in the
    iteration column; --multigrid-open there stays an error, and the flags exclude each other."""
    exe = os.path.join(ROOT, "computational-fluid-dynamics_amd", "bin", "channel")
    args = ["--steps", "3", "--no-vtk", "--print-interval", "1"]
    r = subprocess.run([exe, "--multigrid-open-any"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in re.sub(r"\x1b\[[0-9;]*m", "", r.stdout).splitlines() if l.startswith("Step ")]
    cp = C.reference_defaults("channel")
    assert (cp.nx, cp.ny) == (93, 31)
    o = O.Oracle(cp, ordering=O.LEX)
    o.velocity_bc(False)
    want = [A.oracle_step(o, cp)[0] for _ in range(3)]
    assert len(lines) == 3 and [ppe_iters(l) for l in lines] == want
    assert all(0 < c <= 20 for c in want)
    assert "Warning" not in r.stderr
    cp.print_interval = 1
    out, err = io.StringIO(), io.StringIO()
    g = C.ChannelSolver(cp, poisson=METHOD)
    g.run(output_directory=None, out=out, err=err, steps=3)
    g.close()
    assert [l for l in out.getvalue().splitlines() if l.startswith("Step ")] == lines and err.getvalue() == ""
    r = subprocess.run([exe, "--multigrid-open"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "grid rule" in r.stderr
    r = subprocess.run([exe, "--multigrid-open-any", "--multigrid-open"] + args, cwd=tmp_path, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "excludes" in r.stderr
