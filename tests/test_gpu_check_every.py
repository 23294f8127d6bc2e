"""check_every's stop rule on every red-black engine, against the oracle.

Seven code paths carry their own copy of "test only multiples of
check_every": the one-workgroup solve (small.hpp), the per-launch window test
(device.hpp window_go_on: wave march, pair / triple march, 4-sweep proof
launches, LDS tiles, open.hip), the host's tail loop and the rank all-reduce
(solver.hip), the resident kernel (resident.hip) and the segmented resident
solve. The rule is stated once, outside the product, by the oracle
(orc_poisson_every: the initial residual, then multiples of check_every
counted from the solve's start, the cap untested); every engine must give its
iteration counts, residuals and fields, bit for bit. No tolerance appears in
this file.

The fixtures (tests/check_every_cases.py) are converging solves on which
check_every decides the stop; tests/test_oracle_check_every.py guards that on
the CPU. Every row asserts which engine ran.
"""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import check_every_cases as F  # noqa: E402
from cfd_amd import _lib  # noqa: E402
from test_gpu_parity import assert_bits  # noqa: E402
from test_gpu_ranks import run_ranks  # noqa: E402

MARCH = {"tile_rounds": 0, "resident": 0}
TILES = {"tile_rounds": 1, "resident": 0}
RESIDENT = {"resident": 1}


def run_fixture(name, ce, **kw):
    """The fixture on the GPU with check_every = ce: ([(iterations, residual)],
    fields, timing)."""
    cp = F.params(name)
    g = C.solver_for(cp, ordering="rb", device=0, check_every=ce, **kw)
    if F.kind(name) == "solve":
        f, p0 = F.solve_inputs(name)
        g.set_field("src", f)
        if p0 is not None:
            g.set_field("p", p0)
        its = [g.solverPressurePoisson()]
        names = ("p",)
    else:
        g.applyBoundaryConditions()
        its = [g.step() for _ in range(F.steps(name))]
        names = ("p", "u", "v")
    out = {n: g.field(n).copy() for n in names}
    tm = g.timing()
    g.close()
    return its, out, tm


def check(name, ce, its, out, what):
    """Iteration counts and residuals equal the oracle's, fields bit for bit."""
    ref = F.oracle_result(name, ce)
    print(f"\n{what}: fixture {name}, check_every {ce}: gpu {[k for k, _ in its]}, oracle {[k for k, _ in ref['its']]}")
    assert its == ref["its"], what
    for f in out:
        assert_bits(out[f], ref[f], f"{what}: {name} check_every {ce} {f}")


def kernel(tm):
    return _lib.SOR_KERNEL[tm.sor_kernel]


CE = [5, 7]
CE_WIDE = [3, 5, 7, 8]


# ---- the one-workgroup solve (small.hpp) ----

@pytest.mark.parametrize("ce", CE)
def test_small_solve(ce):
    its, out, tm = run_fixture("E", ce, small_solve="on")
    assert kernel(tm) == "small" and tm.poisson_launches == len(its)
    check("E", ce, its, out, "one-workgroup solve")


# ---- the wave march, 1 / 2 / 3 sweeps per launch, exact residuals (device.hpp window_go_on, the host's tail) ----

@pytest.mark.parametrize("ce", CE)
@pytest.mark.parametrize("spl", [1, 2, 3])
@pytest.mark.parametrize("name", ["A", "B"])
def test_march_exact(name, spl, ce):
    its, out, tm = run_fixture(name, ce, small_solve="off", tuning=MARCH, proof_test="off", sweeps_per_launch=spl)
    assert kernel(tm) == "march" and tm.proof_fallbacks == 0
    # spl sweeps per launch (the last launch of a solve and its replay may be shorter)
    if spl == 1:
        assert tm.poisson_sweeps == tm.poisson_launches
    else:
        assert (spl - 1) * tm.poisson_launches < tm.poisson_sweeps <= spl * tm.poisson_launches
    check(name, ce, its, out, f"march, {spl} per launch")


@pytest.mark.parametrize("ce", CE)
@pytest.mark.parametrize("spl", [2, 3])
def test_march_exact_on_strips(spl, ce):
    its, out, tm = run_fixture("A", ce, small_solve="off", tuning=MARCH, proof_test="off", sweeps_per_launch=spl,
                               n_strips=3)
    assert kernel(tm) == "march"
    check("A", ce, its, out, f"march on 3 strips, {spl} per launch")


# ---- the 4-sweep proof launches: the stop is an iteration the proof leaves open ----

@pytest.mark.parametrize("ce", CE)
@pytest.mark.parametrize("name", ["A", "A1", "B"])
def test_proof_launches(name, ce):
    its, out, tm = run_fixture(name, ce, small_solve="off", tuning=MARCH, proof_test="on", sweeps_per_launch=0)
    assert kernel(tm) == "march" and tm.proof_fallbacks >= 1
    check(name, ce, its, out, "proof launches")


# ---- the LDS tiles ----

@pytest.mark.parametrize("ce", CE)
@pytest.mark.parametrize("proof", ["on", "off"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_tiles(name, proof, ce):
    its, out, tm = run_fixture(name, ce, small_solve="off", tuning=TILES, proof_test=proof)
    assert kernel(tm) == "tile"
    assert (tm.proof_fallbacks >= 1) == (proof == "on")
    check(name, ce, its, out, f"tiles, proof {proof}")


# ---- the open cases (solve by solve: their whole red-black steps differ from
# the oracle in the source's mean, a tree sum on the GPU) ----

@pytest.mark.parametrize("ce", CE)
@pytest.mark.parametrize("name", ["C", "D"])
def test_open_pair_march(name, ce):
    its, out, tm = run_fixture(name, ce, small_solve="off", tuning=MARCH, sweeps_per_launch=2)
    assert kernel(tm) == "march" and tm.proof_fallbacks == 0
    assert tm.poisson_launches < tm.poisson_sweeps <= 2 * tm.poisson_launches
    check(name, ce, its, out, "open pair march")


@pytest.mark.parametrize("ce", CE)
@pytest.mark.parametrize("name", ["C", "D"])
def test_open_proof_launches(name, ce):
    its, out, tm = run_fixture(name, ce, small_solve="off", tuning=MARCH, proof_test="on", sweeps_per_launch=0)
    assert kernel(tm) == "march" and tm.proof_fallbacks >= 1
    check(name, ce, its, out, "open proof launches")


@pytest.mark.parametrize("ce", CE)
def test_open_tiles(ce):
    its, out, tm = run_fixture("C", ce, small_solve="off", tuning=TILES)
    assert kernel(tm) == "tile"
    check("C", ce, its, out, "open tiles")


# ---- the resident launch ----

@pytest.mark.parametrize("ce", CE_WIDE)
@pytest.mark.parametrize("name", ["A", "A1", "C"])
def test_resident_stop_after_replay(name, ce):
    """The open iteration comes at the stop: the resident launch, a replay to
    the open group's start, then an exact window numbered from that group
    boundary (a multiple of 4, not of check_every)."""
    its, out, tm = run_fixture(name, ce, small_solve="off", tuning=RESIDENT)
    assert kernel(tm) == "resident" and tm.proof_fallbacks >= 1
    check(name, ce, its, out, "resident")


def resident_steps(name, ce):
    """Whole steps of a fixture on the resident path; the timing after the
    first step and after the last."""
    cp = F.params(name)
    g = C.solver_for(cp, ordering="rb", device=0, check_every=ce, small_solve="off", tuning=RESIDENT)
    g.applyBoundaryConditions()
    its = [g.step()]
    tm1 = g.timing()
    its += [g.step() for _ in range(F.steps(name) - 1)]
    out = {n: g.field(n).copy() for n in ("p", "u", "v")}
    tm = g.timing()
    g.close()
    assert kernel(tm1) == "resident" and kernel(tm) == "resident"
    print(f"\nresident, fixture {name}, check_every {ce}: {tm1.resident_segments} segments in step 1, "
          f"{tm.resident_segments} in {len(its)} steps")
    return its, out, tm1, tm


@pytest.mark.parametrize("ce", CE_WIDE)
def test_resident_steps_from_rest(ce):
    """Whole steps from rest at tol_factor 1e-5. Measured on the MI355X: with
    check_every = 1 the first solve's first iterations are open (no proof while
    the residual lives at the lid's corners) and it runs in 2 segments; with
    check_every >= 3 those iterations are not tested ones, nothing has to be
    proven for them, and every solve is one segment ending in a replay and an
    exact window (1 segment in step 1, 3 in three steps, at check_every 3, 5,
    7 and 8). The segmented path is test_resident_segments' (fixture G)."""
    its, out, tm1, tm = resident_steps("B", ce)
    assert tm.proof_fallbacks >= len(its)
    check("B", ce, its, out, "resident, steps from rest")


@pytest.mark.parametrize("ce", CE_WIDE)
def test_resident_segments(ce):
    """Fixture B at the reference's tolerance (1e-9): the proof's margin leaves
    a tested iteration open long before the stop, so each solve - the first,
    from rest, included - takes an exact window (128 iterations from a group
    boundary: its end is no multiple of 3, 5 or 7) and then the resident kernel
    again, whose iterations count from the solve's start, not the segment's."""
    its, out, tm1, tm = resident_steps("G", ce)
    check("G", ce, its, out, "resident, segmented solves")
    assert tm1.resident_segments > 1  # (one solve so far: the resident kernel was relaunched)
    assert tm.resident_segments > len(its)


# ---- loopback ranks: overlapped strips, the all-reduced residuals ----

@pytest.mark.parametrize("ce", CE_WIDE)
def test_ranks(ce):
    cp = F.params("F")
    ref = F.oracle_result("F", ce)
    res = run_ranks(cp, 2, F.steps("F"), check_every=ce)
    for r in res:
        print(f"\nranks: rows {r['rows']}, check_every {ce}: gpu {[k for k, _ in r['its']]}, "
              f"oracle {[k for k, _ in ref['its']]}")
        assert r["overlapped"] > 0, "overlap path not taken"
        assert r["its"] == ref["its"]
        j0, j1 = r["rows"]
        first = 0 if j0 == 1 else j0
        for n in ("u", "v", "p"):
            last = min(j1 + 1 if j1 == cp.ny else j1, ref[n].shape[0] - 1)
            assert_bits(r[n], ref[n][first:last + 1], f"ranks {r['rows']} check_every {ce} {n}")
