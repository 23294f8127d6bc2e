"""Parity at BASELINE.json's full sizes (configs[1] cavity 4096², configs[2]
channel 4096x512).

The reference's own loop never converges at these sizes (it hits the
10000-sweep cap every step, ~25 min per step on one core), so a full step is
compared with the CPU oracle at a capped sweep count, and the rest is checked
through size-independent properties:

* one whole timestep (BCs, predictor, source, 30 red-black sweeps, corrector)
  bit-exact against the oracle's red-black restatement (the channel with its
  source mean's tree sum restated, tests/rb_sums.py);
* the residual the solver reports is the true max-norm residual of the field
  it returns (recomputed here in numpy with the reference's formula,
  cavity-01.cpp:659-677), bit for bit;
* homogeneity: the solve of 2f from a zero field is exactly 2x the solve of f
  (scaling by 2 commutes with every IEEE operation in the sweep and in the
  tolerance), with the same iteration count;
* row strips (4 on one device) == one domain, bit for bit.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import oracle as O  # noqa: E402
import rb_sums as R  # noqa: E402
from test_gpu_parity import assert_bits, ofield  # noqa: E402

N = 4096


def cavity(**kw):
    return C.make_params("cavity", nx=N, ny=N, **kw)


def predictor_source(g):
    g.applyBoundaryConditions()
    g.computeTentativeVelocities()
    if not isinstance(g, C.CavitySolver):
        g.applyTentativeBoundaryConditions()
    g.buildSourceTerm()


def cavity_residual(p, f, dx):
    """cavity-01.cpp:659-677 in numpy: the same operand order as the sweep's
    residual, so equal bits are expected."""
    ny, nx = p.shape[0] - 2, p.shape[1] - 2
    ih2 = 1.0 / (dx * dx)
    c = p[1:ny + 1, 1:nx + 1]
    ee = np.ones((1, nx))
    ee[0, -1] = 0.0
    ew = np.ones((1, nx))
    ew[0, 0] = 0.0
    en = np.ones((ny, 1))
    en[-1, 0] = 0.0
    r = ih2 * (ee * (p[1:ny + 1, 2:nx + 2] - c) + ew * (p[1:ny + 1, 0:nx] - c) + en * (p[2:ny + 2, 1:nx + 1] - c) +
               1.0 * (p[0:ny, 1:nx + 1] - c)) - f[1:ny + 1, 1:nx + 1]
    return np.abs(r).max()


def test_cavity_4096_step_bitexact_vs_red_black_oracle():
    cp = cavity(max_iters=30)
    g = C.solver_for(cp, ordering="rb")
    o = O.Oracle(cp, ordering=O.RB)
    ig, rg = g.step()
    io, ro = o.step()
    assert ig == io == 30
    assert rg == ro
    for name in ("u", "v", "p"):
        assert_bits(g.field(name), ofield(o, name, cp), f"4096² step {name}")


def test_channel_4096x512_step_vs_red_black_oracle():
    cp = C.make_params("channel", re=1000.0, nx=4096, ny=512, max_iters=30)
    g = C.solver_for(cp, ordering="rb")
    o = O.Oracle(cp, ordering=O.RB)
    o.velocity_bc(False)
    # source mean: the GPU's tree sum, restated for the oracle
    assert g.step() == o.step(source_total=R.source_hook(o, R.strips_of(cp.ny, 1)))
    for name in ("u", "v", "p", "src"):
        assert_bits(g.field(name), ofield(o, name, cp), f"4096x512 step {name}")


def test_cavity_4096_reported_residual_is_true_residual():
    cp = cavity(max_iters=200)
    g = C.solver_for(cp, ordering="rb")
    predictor_source(g)
    it, res = g.solverPressurePoisson()
    assert it == 200
    r = cavity_residual(g.field("p"), g.field("src"), cp.dx)
    assert res == r, (res, r)


def test_cavity_4096_poisson_homogeneous_in_source():
    cp = cavity(max_iters=10000)
    g = C.solver_for(cp, ordering="rb")
    rng = np.random.default_rng(11)
    f = np.zeros((N + 2, N + 2))
    # smooth source so the solve converges in a few hundred sweeps at 4096²
    y = (np.arange(N) + 0.5) / N
    f[1:N + 1, 1:N + 1] = np.outer(np.sin(np.pi * y), np.sin(np.pi * y)) * 50.0 \
        + rng.standard_normal((N, N)) * 1e-3
    g.set_field("src", f)
    it1, res1 = g.solverPressurePoisson()
    p1 = g.field("p").copy()
    g.set_field("src", 2.0 * f)
    it2, res2 = g.solverPressurePoisson()
    p2 = g.field("p")
    assert it1 == it2
    assert res2 == 2.0 * res1
    assert_bits(p2, 2.0 * p1, "p(2f) vs 2 p(f)")


def test_cavity_4096_strips_equal_single_domain():
    cp = cavity(max_iters=50)
    a = C.solver_for(cp, ordering="rb", n_strips=1)
    b = C.solver_for(cp, ordering="rb", n_strips=4)
    for _ in range(2):
        ia, ra = a.step()
        ib, rb = b.step()
        assert ia == ib and ra == rb
    for name in ("u", "v", "p"):
        assert_bits(b.field(name), a.field(name), f"4096² strips {name}")
