#!/usr/bin/env python3
"""Records tests/golden/sor_plans.json: the SOR launch plans (Solver.sor_plan()) the library gives for
the fixtures of tests/test_gpu_tuning.py under the knob settings that file uses, and for the BASELINE
grids in both orders, each with the planner's inputs. tests/plan_check.cpp replays csrc/plan.hpp from
the inputs and must give the recorded outputs; a change that is meant to leave the plans alone records
the file again and finds it byte for byte the same.

Needs the GPU (the wave budgets come from the device's occupancy):  python scripts/record_sor_plans.py [out]

Per case: "in" = [case_id, nx, ny, step_i, inlet_jmax, n_strips, lex, pair_edge_pct, lexw_edge_pct,
march_min_th, lexw_ramp_pct, lexw_left, lexw_updown, march_order], "K" the cap, "iters" what the solve
ran, "plans" = one row of PLAN_FIELDS per cfd_sor_band_plan, "ramp" = RAMP_FIELDS of cfd_sor_plan.
Where iters < K (a stop, its replay) the launch-dependent fields are left out: those rows end at
march_order and "ramp" is null. The overlapped two-rank fixture gives one case per rank (its interior plans)."""
from __future__ import annotations

import copy
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "computational-fluid-dynamics_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))

import cfd_amd as C  # noqa: E402
from cfd_amd import _lib  # noqa: E402
from cfd_amd.solver import to_cparams  # noqa: E402
import test_gpu_tuning as T  # noqa: E402
from test_gpu_lexw import random_field, random_source  # noqa: E402

PLAN_FIELDS = [n for n, _ in _lib.SorBandPlan._fields_ if n != "launches"]
STATIC = PLAN_FIELDS.index("march_order") + 1  # fields that do not depend on which launches ran
RAMP_FIELDS = [n for n, _ in _lib.SorPlan._fields_ if n.startswith("ramp")]
KNOBS = ["pair_edge_pct", "lexw_edge_pct", "march_min_th", "lexw_ramp_pct", "lexw_left", "lexw_updown", "march_order"]

SETTINGS = {  # fixture: the settings its tests in tests/test_gpu_tuning.py run it under
    "lex_cavity": [{}] + T.LEX_ALL + [{"march_min_th": 1000, "lexw_ramp_pct": 100}],
    "lex_converging": [{}] + T.LEX_SOME,
    "lex_channel": [{}] + T.LEX_ALL,
    "lex_step": T.LEX_STEP,
    "lex_tall": T.LEX_TALL,
    "lex_strips": T.LEX_STRIPS,
    "lex_spl5": T.LEX_DEEP,
    "lex_spl6": T.LEX_DEEP,
    "lex_deep5": [{"march_min_th": 1000}],
    "lex_deep6": [{"march_min_th": 1000}],
    "rb_cavity_proof": [{}] + T.RB_PAIR,
    "rb_cavity_exact": [{}] + T.RB_PAIR,
    "rb_converging": [{}] + T.RB_SOME,
    "rb_remainder": T.RB_REMAINDER,
    "rb_wide": T.RB_WIDE,
    "rb_channel_proof": [{}] + T.RB_PAIR,
    "rb_step_proof": [{}] + T.RB_PAIR,
    "rb_channel_exact": T.RB_OPEN_EXACT,
    "rb_step_exact": T.RB_OPEN_EXACT,
}


def baseline_cases():
    """(name, params, source, initial pressure, solver keywords): the BASELINE grids and the benchmark's, in both
    orders; the reference order capped with 2K > nx + ny (steady launches), red-black at 61 (a one-sweep last launch)."""
    grids = [("cavity128", "cavity", dict(re=100.0, nx=128, ny=128, dt=1e-3), 1),
             ("cavity1024", "cavity", dict(re=1000.0, nx=1024, ny=1024), 1),
             ("cavity4096", "cavity", dict(re=1000.0, nx=4096, ny=4096), 1),
             ("channel4096x512", "channel", dict(re=1000.0, nx=4096, ny=512), 1),
             ("step8192x512", "backwards_step", dict(re=400.0, nx=8192, ny=512), 1),
             ("step8192x512_strips4", "backwards_step", dict(re=400.0, nx=8192, ny=512), 4),
             ("rb8192x2048", "rayleigh_benard", dict(ra=1e6, pr=0.71, nx=8192, ny=2048), 1)]
    for name, case, kw, strips in grids:
        for order in ("lex", "rb"):
            K = (kw["nx"] + kw["ny"]) // 2 + 100 if order == "lex" else 61
            cp = C.make_params(case, max_iters=K, **kw)
            f = random_source(cp) if case in ("cavity", "rayleigh_benard") else random_field(cp, 5, 10.0)
            p0 = None if case in ("cavity", "rayleigh_benard") else random_field(cp, 6)
            skw = dict(ordering=order, small_solve="off", n_strips=strips)
            if order == "rb":
                skw.update(proof_test="on")
            yield f"{name}_{order}", cp, f, p0, skw


def knob_values(cp, setting):
    """The device-independent knobs in effect: cfd_tuning_default of the solver's parameters, then the setting."""
    cp = copy.copy(cp)
    if cp.case_id == C.RAYLEIGH_BENARD:
        cp.case_id = C.CAVITY  # (the solver plans it as the cavity it runs)
    out = []
    for k in KNOBS:
        v = ctypes.c_int(0)
        _lib.check(_lib.lib().cfd_tuning_default(ctypes.byref(cp), _lib.TUNING[k], ctypes.byref(v)), k)
        out.append(int(setting.get(k, v.value)))
    return cp, out


def record(name, cp, f, p0, kw, setting):
    engine = T.LEXW if kw["ordering"] == "lex" else T.MARCH
    g = C.solver_for(cp, tuning={**engine, **setting}, **kw)
    try:
        g.set_field("src", f)
        if p0 is not None:
            g.set_field("p", p0)
        iters, _ = g.solverPressurePoisson()
        rep = g.sor_plan()
        c, knobs = knob_values(g._cp, setting)
    finally:
        g.close()
    assert rep.plans_dropped == 0, name
    full = iters == cp.max_iters and kw["ordering"] == "lex"
    plans = [[getattr(rep.plan[q], n) for n in (PLAN_FIELDS if full else PLAN_FIELDS[:STATIC])] for q in range(rep.n_plans)]
    return {"name": name + ("/" + T.ident(setting) if setting else ""),
            "in": [c.case_id, c.nx, c.ny, c.step_i, c.inlet_jmax, kw.get("n_strips", 1), int(kw["ordering"] == "lex")] + knobs,
            "K": cp.max_iters, "iters": iters, "plans": plans,
            "ramp": [getattr(rep, n) for n in RAMP_FIELDS] if full else None}


def record_ranks(setting):
    """The overlapped two-rank fixture: each rank's report (kind CFD_PLAN_INTERIOR), as a red-black case of its own."""
    cp = T.ranks_params()
    c, knobs = knob_values(to_cparams(cp, ordering="rb"), setting)
    for r, res in enumerate(T.run_ranks(cp, 2, 2, small_solve="off", proof_test="on", tuning={**T.MARCH, **setting})):
        rep = res["plan"]
        assert rep.plans_dropped == 0 and res["overlapped"] > 0, setting
        yield {"name": f"rb_ranks_overlapped/rank{r}" + ("/" + T.ident(setting) if setting else ""),
               "in": [c.case_id, c.nx, c.ny, c.step_i, c.inlet_jmax, 1, 0] + knobs, "K": cp.max_iters, "iters": res["its"][-1][0],
               "plans": [[getattr(b, n) for n in PLAN_FIELDS[:STATIC]] for b in rep.plans], "ramp": None}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sor_plans.json")
    cases = []
    for name, settings in SETTINGS.items():
        cp, f, p0, kw = T._fixture(name)
        for s in settings:
            cases.append(record(name, cp, f, p0, kw, s))
    for s in T.RB_RANKS:
        cases.extend(record_ranks(s))
    for name, cp, f, p0, kw in baseline_cases():
        cases.append(record(name, cp, f, p0, kw, {}))
    with open(out, "w") as fh:
        fh.write('{"plan_fields": %s,\n "ramp_fields": %s,\n "cases": [\n' % (json.dumps(PLAN_FIELDS), json.dumps(RAMP_FIELDS)))
        fh.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in cases))
        fh.write("\n]}\n")
    print(f"{len(cases)} cases -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
