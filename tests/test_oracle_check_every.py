"""The check_every stop rule, stated once on the CPU (orc_poisson_every):
the initial residual is tested, then only multiples of check_every counted
from the solve's start, and the cap ends the solve untested.

* check_every = 1 is orc_poisson (the reference's loop, pinned by
  tests/test_oracle_golden.py), bit for bit;
* check_every > 1 equals a plain Python loop over single iterations;
* the fixture guards: on every fixture the GPU engines are compared on
  (tests/check_every_cases.py), every solve stops by the rule before the cap
  and check_every moves at least one stop. A fixture on which check_every
  decides nothing fails here, not silently on the GPU.
"""
from __future__ import annotations

import numpy as np
import pytest

import cfd_amd as C
import oracle as O
import check_every_cases as F


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def first_steps_source(cp, ordering):
    """An oracle of the reference defaults with its first step's source."""
    o = O.Oracle(cp, ordering=ordering)
    if cp.case_id == C.CAVITY:
        o.velocity_bc(False)
        o.tentative()
    else:
        o.velocity_bc(False)  # (the open cases apply their BCs in the constructor)
        o.tentative()
        o.velocity_bc(True)
    o.source()
    return o


@pytest.mark.parametrize("ordering", [O.LEX, O.RB])
@pytest.mark.parametrize("case", ["cavity", "channel", "backwards_step"])
def test_every_1_is_orc_poisson(case, ordering):
    """Two steps of the reference defaults: each solve with orc_poisson and with
    orc_poisson_every(1) from the same state - iterations, residual, p bits."""
    cp = C.reference_defaults(case)
    a = O.Oracle(cp, ordering=ordering)
    b = O.Oracle(cp, ordering=ordering)
    if cp.case_id != C.CAVITY:
        a.velocity_bc(False)
        b.velocity_bc(False)
    for step in range(2):
        ra = a.step()
        rb = b.step_phases(1)
        assert ra == rb, (case, ordering, step)
        assert ra[0] > 0
        for n in ("p", "u", "v"):
            assert np.array_equal(bits(a.field(n)), bits(b.field(n))), (case, ordering, step, n)


@pytest.mark.parametrize("ce", [3, 5, 7, 8])
@pytest.mark.parametrize("ordering", [O.LEX, O.RB])
@pytest.mark.parametrize("case", ["cavity", "channel", "backwards_step"])
def test_every_n_is_the_plain_loop(case, ordering, ce):
    """orc_poisson_every against the rule written out over single iterations
    (poisson_fixed(1)), on the reference defaults' first solve."""
    cp = C.reference_defaults(case)
    a = first_steps_source(cp, ordering)
    b = first_steps_source(cp, ordering)
    p_start = a.field("p").copy()
    ka, ra = a.poisson_every(ce)
    # the plain loop (the cavity's solve starts from a zero field; its tolerance is factor * max|source|)
    if cp.case_id == C.CAVITY:
        b.field("p")[...] = 0.0
        tol = cp.tol_factor * np.abs(b.field("src")[1:-1, 1:-1]).max()
        res = 1.0
    else:
        assert np.array_equal(bits(b.field("p")), bits(p_start))
        src = np.abs(b.field("src")[1:-1, 1:-1])
        m = (src[b.mask()[1:-1, 1:-1] != 0] if cp.case_id == C.BACKSTEP else src).max()
        tol = max(cp.tol_factor * (m if m > 0 else 1.0), cp.abs_tol)
        res = tol + 1.0
    it = 0
    if res > tol:
        while it < cp.max_iters:
            it += 1
            res = b.poisson_fixed(1)
            if it % ce == 0 and not res > tol:
                break
    assert (ka, ra) == (it, res)
    assert ka > 0 and (ka % ce == 0 or ka == cp.max_iters)  # (the channel's first solve in the reference order runs to the cap)
    assert np.array_equal(bits(a.field("p")), bits(b.field("p")))


def test_cap_ends_the_solve_untested():
    """A cap that is no multiple of check_every: the solve runs to the cap."""
    cp = C.reference_defaults("cavity")
    cp.max_iters = 57
    o = first_steps_source(cp, O.RB)
    assert o.poisson_every(4)[0] == 57


PAIRS = [(n, ce) for n, f in F.FIXTURES.items() for ce in f[7]]


@pytest.mark.parametrize("name,ce", PAIRS, ids=[f"{n}-{ce}" for n, ce in PAIRS])
def test_fixture_guard(name, ce):
    """check_every decides this fixture: every solve stops before the cap, on a
    multiple of check_every, and at least one stop is not check_every = 1's."""
    cp = F.params(name)
    k1 = [k for k, _ in F.oracle_result(name, 1)["its"]]
    kn = [k for k, _ in F.oracle_result(name, ce)["its"]]
    print(f"{name}: check_every 1 {k1}, {ce} {kn}")
    assert all(0 < k < cp.max_iters for k in k1 + kn), (k1, kn)
    assert all(k % ce == 0 for k in kn), kn
    if F.kind(name) == "solve":  # (the same source: no tested iteration before check_every = 1's stop meets the tolerance)
        assert kn[0] >= k1[0]
    assert kn != k1, f"check_every = {ce} decides nothing on fixture {name}: {kn}"
