"""The multigrid pressure solve (csrc/mg.hip) on the GPU: cycle
counts, residuals and p bit for bit the numpy restatement's
(tests/mg_reference.py) at every size at which the kernels take another path;
whole timesteps that converge where the default solve stops at its cap; the
switch back to SOR; the refusals; Rayleigh-Benard; the drop-in binary."""
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
from cfd_amd import _lib  # noqa: E402
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
@pytest.mark.parametrize("nx,ny", [(16, 16), (48, 16), (16, 48), (64, 64), (96, 64), (240, 120), (272, 144),
                                   (512, 512)])
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
