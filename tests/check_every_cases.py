"""Fixtures of the check_every tests: converging red-black solves on which
check_every decides the stop, and their reference - the oracle's statement of
the rule (orc_poisson_every: the initial residual, then multiples of
check_every counted from the solve's start; the cap untested).

Shared by tests/test_oracle_check_every.py (CPU: the rule itself, and the guard
that every fixture here has a stop check_every decides) and
tests/test_gpu_check_every.py (every red-black engine against the rule). The
oracle's results are computed once per (fixture, check_every) and kept.

The stops in the comments were computed with the oracle; the oracle, not the
comment, is the reference.
"""
from __future__ import annotations

import numpy as np

import cfd_amd as C
import oracle as O


def _params(case, nx, ny, cap, tol):
    cp = C.make_params(case, nx=nx, ny=ny, max_iters=cap)
    cp.tol_factor = tol
    return cp


# name -> (kind, case, nx, ny, cap, tol_factor, seed or steps, every check_every a test runs it with)
#   kind "solve": one solverPressurePoisson from a random source (open cases: and a random pressure)
#   kind "steps": whole steps from rest
FIXTURES = {
    # stops for check_every = 1 / 3 / 5 / 7 / 8:           341 / 342 / 345 / 343 / 344
    "A": ("solve", "cavity", 240, 120, 3000, 1e-2, 7, (3, 5, 7, 8)),
    #                                                       713 / 714 / 715 / 714 / 720
    "A1": ("solve", "cavity", 240, 120, 3000, 1e-3, 7, (3, 5, 7, 8)),
    # 1: 794,764,737  4: 796,764,740  5: 795,765,740  7: 798,770,742  8: 800,768,744
    "B": ("steps", "cavity", 240, 120, 4000, 1e-5, 3, (3, 5, 7, 8)),
    #                                                       4213 / 4215 / 4215 / 4214 / 4216
    "C": ("solve", "channel", 240, 120, 6000, 1e-2, 3, (3, 5, 7, 8)),
    #                                                       5081 / 5082 / 5085 / 5082 / 5088
    "D": ("solve", "backwards_step", 256, 64, 6000, 1e-2, 5, (5, 7)),
    # 1: 214,219,221  4: 216,220,220  5: 215,220,220  7: 217,224,224  8: 216,224,224  (fits small.hpp)
    "E": ("steps", "cavity", 48, 40, 4000, 1e-5, 3, (4, 5, 7)),
    # B with the reference's own tolerance: the proof's margin leaves iterations open long before the stop, so a
    # resident solve runs in several segments at every check_every
    # 1: 2070,2078,2082  3: 2070,2079,2082  5: 2070,2080,2085  7: 2072,2079,2086  8: 2072,2080,2088
    "G": ("steps", "cavity", 240, 120, 4000, 1e-9, 3, (3, 5, 7, 8)),
    # 1: 308,314,315  4: 308,316,316  5: 310,315,315  7: 308,315,315  8: 312,320,320  (2 ranks: 64-row strips)
    "F": ("steps", "cavity", 96, 128, 4000, 1e-5, 3, (3, 5, 7, 8)),
}


def params(name):
    _, case, nx, ny, cap, tol, _, _ = FIXTURES[name]
    return _params(case, nx, ny, cap, tol)


def kind(name):
    return FIXTURES[name][0]


def steps(name):
    assert kind(name) == "steps"
    return FIXTURES[name][6]


def solve_inputs(name):
    """(source, initial pressure or None) of a "solve" fixture."""
    k, case, nx, ny, _, _, seed, _ = FIXTURES[name]
    assert k == "solve"
    rng = np.random.default_rng(seed)
    if case == "cavity":  # (every cavity solve starts from a zero field)
        return rng.standard_normal((ny + 2, nx + 2)), None
    f = rng.standard_normal((ny + 2, nx + 2)) * 10.0
    p0 = rng.standard_normal((ny + 2, nx + 2))
    return f, p0


_cache = {}


def oracle_result(name, check_every):
    """{"its": [(iterations, residual), ...], "p", "u", "v"}: the oracle's
    red-black solve(s) of fixture `name`; fields in the reference's shapes.
    Computed once; callers must not write to the arrays."""
    key = (name, check_every)
    if key in _cache:
        return _cache[key]
    cp = params(name)
    o = O.Oracle(cp, ordering=O.RB)
    if kind(name) == "solve":
        f, p0 = solve_inputs(name)
        o.field("src")[...] = f
        if p0 is not None:
            o.field("p")[...] = p0
        its = [o.poisson_every(check_every)]
    else:
        assert cp.case_id == C.CAVITY
        its = [o.step(check_every=check_every) if check_every > 1 else o.step() for _ in range(steps(name))]
    out = {"its": its, "p": o.field("p").copy(), "u": o.field("u")[:, : cp.nx + 1].copy(),
           "v": o.field("v")[: cp.ny + 1, :].copy()}
    for a in (out["p"], out["u"], out["v"]):
        a.setflags(write=False)
    _cache[key] = out
    return out
