"""The deep reference-order launches of the cavity (csrc/lexw.hpp): 6 sweeps
per launch (102-column tiles, the source-row ring in LDS), and 4 and 5 sweeps
beside it (5 on the LDS ring too; 4 wherever the build puts it: lexw_lds),
bit for bit against the oracle's restatement of the reference's loop
(oracle/ ORC_LEX) as tests/test_gpu_lexw.py does.

Shapes: widths 204 / 205 put the last column on a 102-column tile edge;
300x130 has several column tiles and bands marching up and down; 129x257 at
K = 2 is all ramp; 257x64 at K = 400 runs steady launches (every cell active,
the unmasked kernel) between the ramps.
"""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import oracle as O  # noqa: E402
from cfd_amd import _lib  # noqa: E402
from test_gpu_lexw import LEXW, random_source  # noqa: E402
from test_gpu_parity import assert_bits, ofield  # noqa: E402

SHAPES = [(40, 24, 37), (204, 41, 29), (205, 41, 30), (300, 130, 25), (129, 257, 2), (257, 64, 400)]
_ORACLE = {}  # (nx, ny, K) -> (source, iterations, residual, p): one reference solve per shape, read only


def reference(nx, ny, K):
    key = (nx, ny, K)
    if key not in _ORACLE:
        cp = C.make_params("cavity", nx=nx, ny=ny, max_iters=K)
        f = random_source(cp)
        o = O.Oracle(cp, ordering=O.LEX)
        o.field("src")[...] = f
        io, ro = o.poisson()
        p = o.field("p").copy()
        f.setflags(write=False)
        p.setflags(write=False)
        _ORACLE[key] = (f, io, ro, p)
    return _ORACLE[key]


@pytest.mark.parametrize("spl", [4, 5, 6])
@pytest.mark.parametrize("nx,ny,K", SHAPES)
def test_deep_capped_solve_bitexact(nx, ny, K, spl):
    f, io, ro, p = reference(nx, ny, K)
    cp = C.make_params("cavity", nx=nx, ny=ny, max_iters=K)
    g = C.CavitySolver(cp, ordering="lex", small_solve="off", sweeps_per_launch=spl, tuning=LEXW)
    g.set_field("src", f)
    ig, rg = g.solverPressurePoisson()
    assert ig == io == K
    assert rg == ro
    assert_bits(g.field("p"), p, f"deep lexw p {nx}x{ny} K={K} spl={spl}")
    tm = g.timing()
    assert tm.poisson_sweeps > (spl - 1) * tm.poisson_launches  # launches of spl sweeps ran
    if (nx, ny, K) == (257, 64, 400):
        assert tm.poisson_steady_launches > 0
    g.close()


def test_deep_converging_solve_stops_at_reference_iteration():
    """The reference's own 63² cavity at 6 sweeps per launch: the stop (found
    late, on sampled rows first) and its replay land on the reference's
    count."""
    cp = C.reference_defaults("cavity")
    g = C.CavitySolver(cp, ordering="lex", small_solve="off", sweeps_per_launch=6, tuning=LEXW)
    o = O.Oracle(cp, ordering=O.LEX)
    g.applyBoundaryConditions()
    g.computeTentativeVelocities()
    g.buildSourceTerm()
    o.velocity_bc(False)
    o.tentative()
    o.source()
    ig, rg = g.solverPressurePoisson()
    io, ro = o.poisson()
    assert 10 < io < cp.max_iters
    assert (ig, rg) == (io, ro)
    assert_bits(g.field("p"), o.field("p"), "converged p, 6 sweeps per launch")


def test_deep_cavity_4096_step_bitexact_capped():
    """The bench size at 6 sweeps per launch: one whole timestep, capped."""
    cp = C.make_params("cavity", re=1000.0, nx=4096, ny=4096, max_iters=24)
    g = C.CavitySolver(cp, ordering="lex", small_solve="off", sweeps_per_launch=6, tuning=LEXW)
    o = O.Oracle(cp, ordering=O.LEX)
    g.applyBoundaryConditions()
    assert g.step() == o.step()
    for name in ("u", "v", "p"):
        assert_bits(g.field(name), ofield(o, name, cp), f"4096 spl=6 {name}")


@pytest.mark.parametrize("case,spl", [("cavity", 7), ("channel", 6)])
def test_deep_sweeps_per_launch_rejected(case, spl):
    """7 nowhere, 6 for the cavity only. (6 on a grid that goes to the
    one-workgroup solve, small_solve auto, is refused too rather than ignored:
    tests/test_host_logic.py; every test above selects the march.)"""
    with pytest.raises(_lib.CfdError) as e:
        C.solver_for(C.make_params(case), ordering="lex", sweeps_per_launch=spl)
    assert "sweeps_per_launch" in str(e.value)
