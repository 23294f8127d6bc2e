"""The backwards-facing step's multigrid pressure solve (CFD_POISSON_MULTIGRID_STEP:
the mgs_* kernels of csrc/mg.hip) on the GPU: cycle counts,
residuals and p bit for bit the numpy restatement's (tests/mg_step_reference.py)
from a set source and a set, warm p - solid cells and ghosts included - at every
size at which the kernels take another path: the three transfer kinds, two-level
plans, the block's corner on and around the smoothing tile's ownership edges,
sweep counts whose fused launches end in the second buffer, one launch per
colour; with other values in the solid and ghost cells; a custom geometry; the
launch counters; whole timesteps against the oracle's phases around the
restatement's solve; the switch to SOR and back; the refusals; the drop-in
binary."""
from __future__ import annotations

import io
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import mg_step_reference as M  # noqa: E402
import oracle as O  # noqa: E402
from cfd_amd import _lib  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_gpu_parity import assert_bits, ofield  # noqa: E402

_REF = {}


def params(nx, ny, geom=None):
    cp = C.make_params("backwards_step", nx=nx, ny=ny)
    if geom:
        cp.step_x, cp.h_inlet = geom
    return cp


def fixture(nx, ny, geom=None):
    """(params, source, p to start from - solids and ghosts included, {options: the restatement's solve}), once per grid."""
    key = (nx, ny, geom)
    if key not in _REF:
        cp = params(nx, ny, geom)
        f = M.random_source(nx, ny, cp.step_i, cp.inlet_jmax, seed=nx * 1000 + ny)
        _REF[key] = (cp, f, M.random_field(nx, ny, nx + ny), {})
    return _REF[key]


def reference_solve(nx, ny, nu=(2, 2), max_cycles=50, geom=None):
    cp, f, p0, cache = fixture(nx, ny, geom)
    key = (nu, max_cycles)
    if key not in cache:
        cache[key] = M.solve_case(cp, f, p0, nu1=nu[0], nu2=nu[1], max_cycles=max_cycles)[:3]
    return cp, f, p0, cache[key]


def nu_opts(nu, max_cycles=50):
    return {"pre_sweeps": nu[0], "post_sweeps": nu[1], "max_cycles": max_cycles}


def gpu_solve(cp, f, p0, opts):
    g = C.BackwardsStepSolver(cp, poisson="multigrid-step", mg_options=opts)
    g.set_field("src", f)
    g.set_field("p", p0)
    cycles, res = g.solverPressurePoisson()
    p = g.field("p").copy()
    tm, info = g.timing(), g.mg_info()
    g.close()
    return cycles, res, p, tm, info


def assert_counters(cp, nu, cycles, fused, tm, info, solves=1):
    """Launches, sweeps and cell updates of `cycles` cycles (mg_step_reference.launches_per_cycle)."""
    pl = M.plan_of(cp)
    per = M.launches_per_cycle(pl, nu[0], nu[1], fused)
    assert (info.solves, info.cycles) == (solves, cycles)
    assert info.launches == cycles * per, (info.launches, cycles, per)
    assert tm.poisson_launches == info.launches
    assert tm.poisson_sweeps == cycles * (nu[0] + nu[1])
    assert tm.poisson_cell_updates == cp.nx * cp.ny * cycles * (nu[0] + nu[1])
    assert (info.levels, info.coarse_nx, info.coarse_ny) == (len(pl), *pl[-1])
    assert info.coarse_sweeps == 4 * max(pl[-1])
    assert _lib.SOR_KERNEL[tm.sor_kernel] == "multigrid" and tm.sor_kernel == 8


def check_solve(nx, ny, nu=(2, 2), max_cycles=50, fused=True, geom=None):
    """One GPU solve of the grid's fixture: (cycles, residual), the whole of p and the counters are the restatement's."""
    cp, f, p0, (cycles, res, p) = reference_solve(nx, ny, nu, max_cycles, geom)
    gc, gr, gp, tm, info = gpu_solve(cp, f, p0, nu_opts(nu, max_cycles))
    what = f"{nx}x{ny} V{nu} max_cycles {max_cycles} {'fused' if fused else 'colour launches'}"
    print(f"{what}: gpu {gc} cycles residual {gr!r}; restatement {cycles} cycles residual {res!r}; "
          f"levels {info.levels}, launches {info.launches}")
    assert (gc, gr) == (cycles, res), what
    assert_bits(gp, p, "step multigrid p " + what)
    assert_counters(cp, nu, cycles, fused, tm, info)
    if max_cycles == 50:
        assert res <= M.tolerance(f, cp.tol_factor, cp.abs_tol, cp.step_i, cp.inlet_jmax), what
    return cycles, res, info


# 16x8 (y only) and 24x8: two levels, the tail alone; 48x16, 64x32 (y only first), 96x24: full and mixed kinds;
# 256x32: the reference's own grid (x only first); 512x64: levels 0 and 1 multi-launch.
GRIDS = [(16, 8), (24, 8), (48, 16), (64, 32), (96, 24), (256, 32), (512, 64)]


@pytest.mark.parametrize("nx,ny", GRIDS)
def test_solve_is_the_restatement(nx, ny):
    check_solve(nx, ny)


# The smoothing tile owns 124x60, 120x56 or 116x52 cells for 1, 2 or 3 sweeps per launch: with the block a
# quarter wide and half high these grids put A = (jm+1, si+1) on the first row and column a tile owns and B
# = (jm, si) on the last of the tile diagonally below; 464x112 and 496x112 put the corner 4 cells inside or
# outside that edge, the V(2,2) halo depth.
TILE_EDGES = [(480, 112, (2, 2)), (496, 120, (1, 1)), (464, 104, (3, 3)), (464, 112, (2, 2)), (496, 112, (2, 2))]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("nx,ny,nu", TILE_EDGES)
def test_corner_on_tile_edges(nx, ny, nu, fused, monkeypatch):
    if not fused:
        monkeypatch.setenv("CFD_MG_FUSED", "0")
    check_solve(nx, ny, nu, fused=fused)


# 3 fused smoothing launches per multi-launch level and cycle: after an odd number of cycles the field of
# level 0 is in the second buffer (the refresh and the residual pass work on it there; the copy back keeps
# p's corner ghosts and interior solid cells).
@pytest.mark.parametrize("max_cycles", [1, 2])
@pytest.mark.parametrize("nu", [(4, 1), (1, 4)])
def test_second_buffer(nu, max_cycles):
    assert M.smoothing_launches(nu[0], True) + M.smoothing_launches(nu[1], True) == 3
    cycles, _, _ = check_solve(480, 112, nu, max_cycles)
    assert cycles == max_cycles


@pytest.mark.parametrize("nx,ny,nu", [(480, 112, (4, 1)), (480, 112, (1, 4))])
def test_second_buffer_to_convergence(nx, ny, nu):
    check_solve(nx, ny, nu)


@pytest.mark.parametrize("nx,ny,nu", [(96, 24, (2, 2)), (480, 112, (2, 2)), (480, 112, (4, 1)), (512, 64, (2, 2))])
def test_solids_and_ghosts_reach_no_result(nx, ny, nu):
    """The same solve with other finite values in p's interior solid cells, face cells and ghosts: the fluid
    cells, cycles and residual keep their bits; the interior solid cells come back as given, the face cells
    and ghosts as the reference's refresh sets them."""
    cp, f, p0, (cycles, res, p) = reference_solve(nx, ny, nu, 50)
    si, jm = cp.step_i, cp.inlet_jmax
    fl = M.fluid_mask(nx, ny, si, jm)
    other = np.random.default_rng(9).standard_normal(p0.shape) * 1e3
    other[1:-1, 1:-1][fl] = p0[1:-1, 1:-1][fl]
    gc, gr, gp, _, _ = gpu_solve(cp, f, other, nu_opts(nu))
    assert (gc, gr) == (cycles, res)
    assert_bits(gp[1:-1, 1:-1][fl], p[1:-1, 1:-1][fl], f"step multigrid fluid p {nx}x{ny} V{nu} from other solids")
    interior = ~fl
    interior[jm, :] = False
    interior[:, si - 1] = False
    assert interior.any()
    assert_bits(gp[1:-1, 1:-1][interior], other[1:-1, 1:-1][interior], "interior solid cells")
    c2, r2, p2, _ = M.solve_case(cp, f, other, nu1=nu[0], nu2=nu[1])  # the whole field: ghosts, face cells, corners
    assert (c2, r2) == (cycles, res)
    assert_bits(gp, p2, "the whole of p from other solids and ghosts")
    assert_bits(gp[jm + 1, 1:si], p[jm + 1, 1:si], "face row")
    assert_bits(gp[jm + 2:-1, si], p[jm + 2:-1, si], "face column")
    assert gp[jm + 1, si] == p[jm + 1, si]


def test_custom_geometry():
    """step_x = 4 of 8 and h_inlet = 0.75 of 2: the block half as wide as the grid and 5/8 high."""
    cp = params(128, 32, (4.0, 0.75))
    assert (cp.step_i, cp.inlet_jmax) == (64, 12) and C.mg_step_plan(cp) == M.plan_of(cp)
    check_solve(128, 32, geom=(4.0, 0.75))


def test_max_cycles_stops_unconverged():
    cp, f, p0, (cycles, res, p) = reference_solve(480, 112, (2, 2), 2)
    assert cycles == 2 and res > M.tolerance(f, cp.tol_factor, cp.abs_tol, cp.step_i, cp.inlet_jmax)
    check_solve(480, 112, (2, 2), 2)


def test_zero_source():
    """A zero source: the loop primed with tol + 1 runs one cycle - zeros from a zero field, residual 0."""
    cp = params(96, 24)
    f = np.zeros((26, 98))
    for p0 in (np.zeros_like(f), M.random_field(96, 24, 4)):
        cycles, res, p, _ = M.solve_case(cp, f, p0, max_cycles=1)
        gc, gr, gp, tm, info = gpu_solve(cp, f, p0, {"max_cycles": 1})
        assert (gc, gr) == (cycles, res) and cycles == 1
        assert_bits(gp, p, "step multigrid p, zero source")
        assert_counters(cp, (2, 2), 1, True, tm, info)
        if not p0.any():
            assert res == 0.0 and not gp.view(np.int64).any()
            assert gpu_solve(cp, f, p0, None)[:2] == (1, 0.0)  # (and it stops there)


_ORACLE_STEPS = {}


def oracle_steps(nx, ny, steps=4):
    """`steps` steps of the oracle's phases around the restatement's solve, once per grid."""
    if (nx, ny) not in _ORACLE_STEPS:
        cp = C.make_params("backwards_step", re=100.0, nx=nx, ny=ny)
        o = O.Oracle(cp, ordering=O.LEX)
        o.velocity_bc(False)  # (the state the solver is created in)
        rows = [M.oracle_step(o, cp) for _ in range(steps)]
        fields = {n: ofield(o, n, cp).copy() for n in ("u", "v", "p")}
        _ORACLE_STEPS[(nx, ny)] = (cp, rows, fields, o.stats())
    return _ORACLE_STEPS[(nx, ny)]


@pytest.mark.parametrize("nx,ny", [(256, 32), (96, 24)])
def test_four_steps_are_the_oracles(nx, ny):
    """The step at Re 100, ordering lex: per step (cycles, residual), then u, v, p bit for bit, the
    statistics and the counters."""
    cp, rows, want, (omd, oke) = oracle_steps(nx, ny)
    g = C.BackwardsStepSolver(cp, ordering="lex", poisson="multigrid-step")
    got = [g.step() for _ in range(4)]
    for k, (a, b) in enumerate(zip(got, rows)):
        print(f"step {nx}x{ny} step {k + 1}: gpu {a[0]} cycles residual {a[1]!r}; oracle {b[0]} cycles residual {b[1]!r}")
    assert got == rows
    assert all(c <= 20 for c, _ in rows)
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), want[n], f"step {nx}x{ny} after 4 steps: {n}")
    md, ke = g.statistics()
    assert md == omd and ke == oke  # (the reference order sums the kinetic energy sequentially, as the oracle)
    assert_counters(cp, (2, 2), sum(c for c, _ in rows), True, g.timing(), g.mg_info(), solves=4)
    g.reset_timing()
    info = g.mg_info()
    assert (info.solves, info.cycles, info.launches) == (0, 0, 0)
    assert info.levels == len(M.plan_of(cp))  # (the plan is no counter)
    g.close()


def test_switching_to_sor_and_back():
    """multigrid-step for two steps, CFD_POISSON_SOR for two - the oracle's own steps from the field the
    multigrid steps left - then multigrid-step again."""
    cp = C.make_params("backwards_step", re=100.0, nx=96, ny=24, max_iters=300)
    o = O.Oracle(cp, ordering=O.LEX)
    o.velocity_bc(False)  # (the state the solver is created in)
    g = C.BackwardsStepSolver(cp, ordering="lex", poisson="multigrid-step")
    assert g.mg_info().levels == 3
    assert [g.step() for _ in range(2)] == [M.oracle_step(o, cp) for _ in range(2)]
    assert g.timing().sor_kernel == 8
    g.set_poisson_method("sor")
    assert g.mg_info().levels == 0
    assert [g.step() for _ in range(2)] == [o.step() for _ in range(2)]
    assert g.timing().sor_kernel != 8
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), ofield(o, n, cp), f"after switching back: {n}")
    g.set_poisson_method("multigrid-step")
    assert [g.step() for _ in range(2)] == [M.oracle_step(o, cp) for _ in range(2)]
    for n in ("u", "v", "p"):
        assert_bits(g.field(n), ofield(o, n, cp), f"after switching on again: {n}")
    g.close()


def test_refusals_name_the_rule():
    sp = params(96, 24)
    with pytest.raises(_lib.CfdError, match="case rule.*CFD_POISSON_MULTIGRID"):
        C.CavitySolver(C.make_params("cavity", nx=64, ny=64), poisson="multigrid-step")
    with pytest.raises(_lib.CfdError, match="case rule.*CFD_POISSON_MULTIGRID_OPEN"):
        C.ChannelSolver(C.make_params("channel", nx=96, ny=32), poisson="multigrid-step")
    with pytest.raises(_lib.CfdError, match="case rule"):  # methods 1 and 2 keep refusing the step
        C.BackwardsStepSolver(sp, poisson="multigrid")
    with pytest.raises(_lib.CfdError, match="case rule"):
        C.BackwardsStepSolver(sp, poisson="multigrid-open")
    with pytest.raises(_lib.CfdError, match="geometry rule"):
        C.BackwardsStepSolver(params(64, 32, (0.2, 1.0)), poisson="multigrid-step")  # step_i = 1
    with pytest.raises(_lib.CfdError, match="geometry rule"):
        C.BackwardsStepSolver(params(40, 10, (2.0, 1.9)), poisson="multigrid-step")  # inlet_jmax = ny - 1
    with pytest.raises(_lib.CfdError, match="grid rule"):
        C.BackwardsStepSolver(params(472, 108), poisson="multigrid-step")  # coarsest 236x54
    with pytest.raises(_lib.CfdError, match="strip rule"):
        C.BackwardsStepSolver(sp, n_strips=2, poisson="multigrid-step")
    L = _lib.lib()
    hub = L.cfd_comm_loopback_hub(1)
    comm = L.cfd_comm_init_loopback(hub, 0, 0)
    assert hub and comm
    try:
        with pytest.raises(_lib.CfdError, match="rank rule"):
            C.BackwardsStepSolver(sp, ordering="rb", rank_rows=(1, 24), comm=comm, poisson="multigrid-step")
    finally:
        L.cfd_comm_destroy(comm)
        L.cfd_comm_loopback_hub_destroy(hub)
    cp = C.make_params("backwards_step", re=100.0, nx=96, ny=24, max_iters=300)
    g = C.BackwardsStepSolver(cp)  # a refused switch leaves the solver on SOR
    with pytest.raises(_lib.CfdError, match="options"):
        g.set_poisson_method("multigrid-step", {"max_cycles": -1})
    with pytest.raises(_lib.CfdError, match="options"):
        g.set_poisson_method("multigrid-step", {"pre_sweeps": -1})
    o = O.Oracle(cp, ordering=O.LEX)
    o.velocity_bc(False)  # (the state the solver is created in)
    assert g.step() == o.step()
    assert g.timing().sor_kernel != 8 and g.mg_info().levels == 0
    g.close()


def ppe_iters(line):
    """The iteration column of the step's log line."""
    return int(re.search(r"PPE iters=\s*(\d+)", line).group(1))


def test_binary_multigrid_step_flag(tmp_path):
    exe = os.path.join(ROOT, "computational-fluid-dynamics_amd", "bin", "backwards_step")
    args = ["--Nx", "256", "--Ny", "32", "--steps", "3", "--no-vtk", "--print-interval", "1"]
    r = subprocess.run([exe, "--multigrid-step"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in re.sub(r"\x1b\[[0-9;]*m", "", r.stdout).splitlines() if l.startswith("Step ")]
    cp, rows, _, _ = oracle_steps(256, 32)
    assert len(lines) == 3 and [ppe_iters(l) for l in lines] == [c for c, _ in rows[:3]]
    cp2 = C.make_params("backwards_step", nx=256, ny=32)
    cp2.print_interval = 1
    out, err = io.StringIO(), io.StringIO()
    g = C.BackwardsStepSolver(cp2, poisson="multigrid-step")
    g.run(output_directory=None, out=out, err=err, steps=3)
    g.close()
    want = [l for l in out.getvalue().splitlines() if l.startswith("Step ")]
    assert lines == want
    assert "Warning" not in r.stderr and err.getvalue() == ""
    for flag in ("--multigrid", "--multigrid-open"):  # the other two methods keep refusing the step
        r = subprocess.run([exe, flag] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "case rule" in r.stderr
        r = subprocess.run([exe, flag, "--multigrid-step"] + args, cwd=tmp_path, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "excludes" in r.stderr  # (before any device work)


def test_cycle_cap_in_the_drivers():
    """max_cycles 1: run() reads the cap for the new method as for the other two - the iteration
    column is 1 and each step warns with the cap."""
    cp = C.make_params("backwards_step", nx=96, ny=24)
    cp.print_interval = 1
    out, err = io.StringIO(), io.StringIO()
    g = C.BackwardsStepSolver(cp, poisson="multigrid-step", mg_options={"max_cycles": 1})
    g.run(output_directory=None, out=out, err=err, steps=2)
    g.close()
    lines = [l for l in out.getvalue().splitlines() if l.startswith("Step ")]
    assert len(lines) == 2 and all(ppe_iters(l) == 1 for l in lines)
    warns = [l for l in re.sub(r"\x1b\[[0-9;]*m", "", err.getvalue()).splitlines() if l.startswith("Warning")]
    assert len(warns) == 2
