"""The launch-planning knobs (cfd_set_tuning) against their contract: "performance only, same bits".

Every case runs one fixture under one knob setting and compares it with the oracle's solve of that
fixture, computed once per module (O.LEX for the reference order, O.RB for red-black) - never with a
default-knob GPU run: iteration count equal, residual ==, p bit for bit (ghosts included, as the
engines' own tests compare it), the intended engine, and the default-knob run's poisson_launches /
poisson_sweeps (knobs move tiles, not launches). There are no tolerances in this file.

The plan report (cfd_sor_plan_info, Solver.sor_plan()) keeps the cases from being vacuous: a case
chosen for a plan shape asserts that shape from the report, and every plan of every case is held to
the planner's invariants (check_plan). The knobs bring the plan regimes of the BASELINE sizes within
reach of grids of ~10^5 cells; the shapes below were read off csrc/plan.hpp (multi_plan, wave_bands,
lexw_launch_plan) for an MI355X (256 CUs: budgets of 2048 tiles) and are asserted, not assumed.

Fixtures (grid, cap; what the report shows there):
  lex cavity 460 x 188, K 420 (2K > nx + ny: steady launches; 5 column tiles of 110 columns, two wall
      and three interior; 190 rows). Default: th 21, 10 interior bands (up bands between down bands),
      ramps at height 1 from the budget. lexw_waves 64: the search loop shortens the plan (th 31) and
      the ramps grow by 10 until their tiles fit. march_min_th 1: one-row bands. march_min_th 1000:
      th clamped to 96 (190 rows need two bands of 95, rounded to 101 > 96), two interior bands, the up
      band the top one. lexw_edge_pct 10 / 100: the 8 / the == th. lexw_ramp_pct 50 / 100: the floor
      rule; with march_min_th 1000 the floor (96, rounded to 101) takes the fallback to the steady height.
  the same grid converging (tol_factor 1.3e-2: the oracle stops at 356, between (nx + ny) / 2 = 324
      and the cap): the late-detected stop and its replay through steady launches.
  lex channel 460 x 152 and step 480 x 160 (step_i 240, inlet_jmax 80: column tile 1 in the left class,
      tile 2 crossing, tile 3 right of it), K 420.
  lex cavity 129 x 300, K 60 (tall: a ramp launch at height 1 has more than 256 bands and grows by the
      band-table rule; march_min_th 1 sends it past the steady height 1 into the fallback, height 2).
  lex cavity 460 x 188 on 3 strips (3 sweeps per launch, a third of the budget per strip).
  lex cavity 460 x 188 with sweeps_per_launch 5 and 6 (LDS source ring, 106- / 102-column tiles, max_th
      90); 240 x 178, K 230 for th clamped to 90 (180 rows: two bands of 90 round to 97 / 93 > 90).
  rb cavity 460 x 188, K 420, proof on (4 sweeps) and off (3 sweeps); march_min_th 1: one-row bands;
      1000: one band per column tile; pair_edge_pct 10: the 8; both march orders.
  rb cavity fixture "A" of tests/check_every_cases.py (240 x 120, natural stop at 341): with the proof
      on, the fallback window.
  rb cavity 460 x 188, K 61 = 15 x 4 + 1: the last launch is poisson_wave_kernel under plan.hpp's wave_bands.
  rb cavity 700 x 150, K 61: 7 column tiles x 152 rows exceed pair_wps 1's budget of 1024 at one-row
      bands - the knob that brings a budget-bound red-black plan within reach at this size.
  rb channel 460 x 152 and step 480 x 160, K 420: proof on (open.hip, the step's left class) and off
      (the 2-sweep pair kernel).
  rb cavity 240 x 128 on two loopback ranks of 64 rows, 2 steps capped at 200: the overlapped path
      (interior plan budget = waves - 2 ctiles).
"""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import oracle as O  # noqa: E402
from cfd_amd import _lib  # noqa: E402
import check_every_cases as CE  # noqa: E402
from test_gpu_lexw import random_field, random_source  # noqa: E402
from test_gpu_parity import assert_bits  # noqa: E402
from test_gpu_ranks import run_ranks  # noqa: E402

LEXW = {"resident": 0}                     # engine lexw (with ordering="lex", small_solve="off")
MARCH = {"tile_rounds": 0, "resident": 0}  # engine march (with ordering="rb", small_solve="off")
PAIR, WAVE, LEXP, INTERIOR = 0, 1, 2, 3    # enum cfd_sor_plan_kind


# ---- fixtures ---------------------------------------------------------------------------------

def _step_params(nx, ny, K):
    cp = C.make_params("backwards_step", nx=nx, ny=ny, max_iters=K)
    cp.step_x = (nx // 2 + 0.5) * cp.dx   # step_i = nx / 2
    cp.h_inlet = (ny // 2 + 0.5) * cp.dy  # inlet_jmax = ny / 2
    assert (cp.step_i, cp.inlet_jmax) == (nx // 2, ny // 2)
    return cp


_fixtures = {}


def _fixture(name):
    """(params, source, initial pressure or None, solver keywords) of a fixture; built once, read only."""
    if name not in _fixtures:
        cp, f, p0, kw = _make_fixture(name)
        for a in (f, p0):
            if a is not None:
                a.setflags(write=False)
        _fixtures[name] = (cp, f, p0, kw)
    return _fixtures[name]


def _make_fixture(name):
    order = "lex" if name.startswith("lex") else "rb"
    kw = dict(ordering=order, small_solve="off")
    p0 = None
    if name in ("lex_cavity", "lex_strips", "lex_spl5", "lex_spl6", "lex_converging"):
        cp = C.make_params("cavity", nx=460, ny=188, max_iters=420)
        f = random_source(cp)
        if name == "lex_converging":
            cp.tol_factor = 1.3e-2
        kw.update(n_strips=3 if name == "lex_strips" else 1,
                  sweeps_per_launch={"lex_spl5": 5, "lex_spl6": 6}.get(name, 0))
    elif name in ("lex_deep5", "lex_deep6"):
        cp = C.make_params("cavity", nx=240, ny=178, max_iters=230)
        f = random_source(cp, seed=6)
        kw.update(sweeps_per_launch=int(name[-1]))
    elif name == "lex_tall":
        cp = C.make_params("cavity", nx=129, ny=300, max_iters=60)
        f = random_source(cp, seed=7)
    elif name in ("lex_channel", "rb_channel_proof", "rb_channel_exact"):
        cp = C.make_params("channel", nx=460, ny=152, max_iters=420)
        f, p0 = random_field(cp, 5, 10.0), random_field(cp, 6)
    elif name in ("lex_step", "rb_step_proof", "rb_step_exact"):
        cp = _step_params(480, 160, 420)
        f, p0 = random_field(cp, 15, 10.0), random_field(cp, 16)
        if order == "rb":
            f[O.Oracle(cp, ordering=O.RB).mask() == 0] = 0.0
    elif name in ("rb_cavity_proof", "rb_cavity_exact", "rb_remainder"):
        cp = C.make_params("cavity", nx=460, ny=188, max_iters=61 if name == "rb_remainder" else 420)
        f = random_source(cp)
    elif name == "rb_wide":
        cp = C.make_params("cavity", nx=700, ny=150, max_iters=61)
        f = random_source(cp, seed=8)
    elif name == "rb_converging":
        cp = CE.params("A")
        f, p0 = CE.solve_inputs("A")
    else:
        raise KeyError(name)
    if order == "rb":
        kw.update(proof_test="off" if name.endswith("_exact") else "on")
    return cp, f, p0, kw


_oracle, _default = {}, {}


def oracle_result(name):
    """((iterations, residual), p) of the oracle's solve of a fixture; computed once, read only."""
    if name not in _oracle:
        cp, f, p0, kw = _fixture(name)
        o = O.Oracle(cp, ordering=O.LEX if kw["ordering"] == "lex" else O.RB)
        o.field("src")[...] = f
        if p0 is not None:
            o.field("p")[...] = p0
        its = o.poisson()
        p = o.field("p").copy()
        p.setflags(write=False)
        _oracle[name] = (its, p)
    return _oracle[name]


def gpu_solve(name, setting):
    """One solverPressurePoisson of a fixture under a knob setting: (result, p, timing, plan report)."""
    cp, f, p0, kw = _fixture(name)
    engine = LEXW if kw["ordering"] == "lex" else MARCH
    g = C.solver_for(cp, tuning={**engine, **setting}, **kw)
    try:
        g.set_field("src", f)
        if p0 is not None:
            g.set_field("p", p0)
        its = g.solverPressurePoisson()
        return its, g.field("p"), g.timing(), g.sor_plan()
    finally:
        g.close()


def default_counts(name):
    """(poisson_launches, poisson_sweeps) of the fixture's default-knob run (once per module)."""
    if name not in _default:
        _, _, t, _ = gpu_solve(name, {})
        _default[name] = (t.poisson_launches, t.poisson_sweeps)
    return _default[name]


def check_plan(b, what):
    """The planner's invariants, for every plan of every case."""
    rows0, rows1 = b.hi0 - b.lo0, max(0, b.hi1 - b.lo1)
    assert b.waves >= 1 and b.ctiles >= 1 and b.th >= 1 and b.the >= 1, what
    # at most one resident round of tiles, unless the plan is down to one band (or clamped: the search stops)
    assert b.tiles <= b.waves or b.nb0 + b.nb1 == 1 or b.clamped == 1, (what, b.tiles, b.waves)
    # interior bands in 10-row groups (the one-sweep kernel has none)
    if b.kind != WAVE and not b.clamped:
        assert (b.th + b.extra) % 10 == 0, (what, b.th, b.extra)
    if b.clamped == 1:
        assert b.th == b.max_th, what
    assert b.th <= b.max_th, what
    # the bands cover their rows, none of them empty
    for th, n0, n1 in ((b.th, b.nb0, b.nb1), (b.the, b.nbe0, b.nbe1)):
        assert (n0 - 1) * th < rows0 <= n0 * th, (what, th, n0, rows0)
        assert (n1 == 0 and rows1 == 0) or (n1 - 1) * th < rows1 <= n1 * th, (what, th, n1, rows1)


def check(name, setting, engine):
    """The contract for one (fixture, setting); returns (timing, report) for the regime assertions."""
    what = f"{name} {setting}"
    (io, ro), po = oracle_result(name)
    (ig, rg), pg, t, rep = gpu_solve(name, setting)
    print(what, "gpu", (ig, rg), "oracle", (io, ro), "launches", t.poisson_launches, "sweeps", t.poisson_sweeps)
    for b in rep.plans:
        print("  plan", {n: getattr(b, n) for n, _ in _lib.SorBandPlan._fields_})
    print("  ramps", {n: getattr(rep, n) for n, _ in _lib.SorPlan._fields_ if n.startswith("ramp")})
    assert ig == io, what
    assert rg == ro, what
    assert_bits(pg, po, what)
    assert _lib.SOR_KERNEL[t.sor_kernel] == engine and _lib.SOR_KERNEL[rep.sor_kernel] == engine, what
    assert (t.poisson_launches, t.poisson_sweeps) == default_counts(name), what
    assert rep.n_plans >= 1 and rep.plans_dropped == 0, what
    for b in rep.plans:
        check_plan(b, what)
    return t, rep


def one(rep, kind, **match):
    """The plans of a kind (and field values) in a report; at least one."""
    out = [b for b in rep.plans if b.kind == kind and all(getattr(b, k) == v for k, v in match.items())]
    assert out, (kind, match, [(b.kind, b.sweeps, b.proof) for b in rep.plans])
    return out


def th_min(b):
    """The shortest interior band of a plan: one row, rounded up so that th + extra is a 10-row group
    (1 at 4 sweeps per launch, where extra is 19; 5 at 3 sweeps, 7 and 3 at 5 and 6)."""
    return (1 + b.extra + 9) // 10 * 10 - b.extra


def ident(setting):
    return "-".join(f"{k}{v}" for k, v in setting.items()) or "default"


# ---- knob settings ----------------------------------------------------------------------------

LEX_SINGLES = [{"lexw_waves": 64}, {"lexw_waves": 256}, {"march_min_th": 1}, {"march_min_th": 7},
               {"march_min_th": 1000}, {"lexw_edge_pct": 10}, {"lexw_edge_pct": 100}, {"lexw_ramp_pct": 0},
               {"lexw_ramp_pct": 50}, {"lexw_ramp_pct": 100}, {"lexw_updown": 0}, {"lexw_updown": 1}]
LEX_COMBOS = [{"lexw_waves": 64, "lexw_ramp_pct": 0}, {"lexw_waves": 64, "lexw_ramp_pct": 100, "lexw_edge_pct": 10},
              {"march_min_th": 1, "lexw_updown": 1, "lexw_edge_pct": 100}]
LEX_ALL = LEX_SINGLES + LEX_COMBOS
LEX_SOME = [{"lexw_waves": 64}, {"march_min_th": 1}, {"march_min_th": 1000}, {"lexw_edge_pct": 10},
            {"lexw_ramp_pct": 100}, {"lexw_updown": 0}] + LEX_COMBOS
RB_SINGLES = [{"pair_wps": 1}, {"pair_wps": 4}, {"wave_wps": 1}, {"wave_wps": 4}, {"pair_edge_pct": 10},
              {"pair_edge_pct": 100}, {"march_min_th": 1}, {"march_min_th": 7}, {"march_min_th": 1000},
              {"march_order": 0}, {"march_order": 1}]
RB_COMBOS = [{"pair_wps": 1, "pair_edge_pct": 10, "march_min_th": 1}, {"pair_wps": 4, "march_order": 1, "march_min_th": 1000}]
RB_ALL = RB_SINGLES + RB_COMBOS
RB_PAIR = [s for s in RB_ALL if "wave_wps" not in s]  # (fixtures without a one-sweep launch)
RB_SOME = [{"pair_wps": 1}, {"pair_edge_pct": 10}, {"march_min_th": 1}, {"march_min_th": 1000}, {"march_order": 1}] + RB_COMBOS
# per test (scripts/record_sor_plans.py records the plans of the same lists)
LEX_STEP = [{}, {"lexw_left": 0}, {"lexw_left": 1}] + LEX_ALL
LEX_TALL = [{}, {"lexw_waves": 64}, {"march_min_th": 1}, {"march_min_th": 7}, {"lexw_ramp_pct": 50}, {"lexw_edge_pct": 10}] + LEX_COMBOS
LEX_STRIPS = [{}, {"lexw_waves": 64}, {"march_min_th": 1}, {"march_min_th": 1000}, {"lexw_edge_pct": 10}, {"lexw_ramp_pct": 100},
              {"lexw_updown": 0}, LEX_COMBOS[2]]
LEX_DEEP = [{}, {"march_min_th": 1}, {"lexw_edge_pct": 10}, {"lexw_waves": 64}, {"lexw_updown": 0}]
RB_REMAINDER = [{}, {"wave_wps": 1}, {"wave_wps": 4}, {"march_min_th": 1}, {"march_min_th": 7}, {"march_min_th": 1000}, {"march_order": 1}]
RB_WIDE = [{"march_min_th": 1}, {"pair_wps": 1, "march_min_th": 1}, RB_COMBOS[0]]
RB_OPEN_EXACT = [{}, {"pair_wps": 1}, {"pair_edge_pct": 10}, {"march_min_th": 1}, {"march_min_th": 1000}, {"march_order": 1}]
RB_RANKS = [{}, {"pair_wps": 1}, {"pair_wps": 4}, {"march_min_th": 1}, {"march_min_th": 1000}, {"pair_edge_pct": 10}, {"march_order": 1},
            RB_COMBOS[0]]


def lex_regimes(setting, b, rep, max_th=96, up_exact=True, ramp_default=0):
    """What a reference-order knob value must show in the steady plan b and the ramp counters.
    ramp_default: the case's default lexw_ramp_pct (cfd_tuning_default: 100 for the step, else 0)."""
    rows = b.hi0 - b.lo0
    if "lexw_waves" in setting:
        assert b.waves == setting["lexw_waves"] // max(1, sum(1 for q in rep.plans if q.kind == LEXP))
    if setting.get("march_min_th") == 1 and b.waves // b.ctiles >= rows:
        assert b.th == th_min(b) and b.nb0 == -(-rows // b.th) and not b.clamped  # (4 sweeps: one-row bands)
    if setting.get("march_min_th") == 7 and b.waves // b.ctiles >= rows and b.sweeps == 4:
        assert 7 <= b.th <= 16  # (bands of at least 7 rows, th + extra rounded up to a 10-row group)
    if setting.get("march_min_th") == 1000:
        assert b.nb0 == -(-rows // b.th) and b.nb0 <= -(-rows // max_th) and b.max_th == max_th
    if setting.get("lexw_edge_pct") == 10:
        assert b.the == 8
    if setting.get("lexw_edge_pct") == 100:
        assert b.the == max(8, b.th)
    pct = setting.get("lexw_ramp_pct", ramp_default)
    if pct == 0:
        assert rep.ramp_by_floor == 0 and rep.ramp_by_budget == rep.ramp_launches > 0
    elif b.th * pct // 100 > 1:
        assert rep.ramp_by_floor > 0 and rep.ramp_th_min >= min(b.th, b.th * pct // 100)
    if setting.get("lexw_updown", 1) == 0:
        assert b.up_bands == 0 and rep.ramp_up == 0
    elif up_exact and b.launches > 0 and b.ctiles > 2:
        assert b.up_bands == (b.nb0 + b.nb1) // 2  # (the cavity's sampled launches: every odd band)


# ---- the reference order (engine lexw) ---------------------------------------------------------

@pytest.mark.parametrize("setting", [{}] + LEX_ALL, ids=ident)
def test_lex_cavity(setting):
    """Cavity 460 x 188, capped at 420 > (nx + ny) / 2: five 110-column tiles, steady launches. Reaches:
    default - 10 interior bands of 21 rows with up bands between down bands, a ramp launch with an up
    band, ramp heights from the budget; lexw_waves 64 - a plan the budget shortened, ramps grown to
    fit their tiles; march_min_th 1 - one-row bands; 1000 - th clamped to 96, two interior bands, the
    up band the top one; lexw_edge_pct 10 / 100 - the 8 / the == th; lexw_ramp_pct 50 / 100 - the
    floor rule; lexw_updown 0 - no band marches up."""
    t, rep = check("lex_cavity", setting, "lexw")
    (b,) = one(rep, LEXP)
    assert (b.sweeps, b.ctiles, b.extra, b.max_th) == (4, 5, 19, 96)
    assert t.poisson_steady_launches > 0 and b.launches == t.poisson_steady_launches
    assert rep.ramp_launches > 0 and rep.ramp_tiles_max < 65536 and rep.ramp_nb_max <= 256
    lex_regimes(setting, b, rep)
    if not setting:
        assert b.nb0 >= 5 and b.up_bands >= 2 and rep.ramp_up == 1  # up bands between down bands
        assert b.the < b.th and not (b.shortened or b.budget_bands or b.clamped)
        assert rep.ramp_th_min == 1  # (a round of 2048 tiles: tot / waves = 1)
    if setting.get("lexw_waves") == 64:
        assert b.shortened or b.budget_bands
        if setting.get("lexw_ramp_pct", 0) == 0:
            assert rep.ramp_grown_tiles > 0 and rep.ramp_tiles_max <= 64
    if setting.get("march_min_th") == 1:
        assert b.th == 1 and b.the == 8
    if setting.get("march_min_th") == 1000:
        assert b.th == 96 and b.clamped == 1 and b.nb0 == 2 and b.up_bands == 1
    if setting.get("lexw_updown") == 1:
        assert b.nb0 >= 3 and b.up_bands >= 1 and rep.ramp_up == 1


def test_lex_cavity_ramp_fallback():
    """The fifth ramp-height rule on the same fixture: under march_min_th 1000 the steady th is clamped to
    96, and lexw_ramp_pct 100 floors the ramps at 96, which the 10-row rounding takes to 101 > 96: every
    ramp launch falls back to the steady height."""
    t, rep = check("lex_cavity", {"march_min_th": 1000, "lexw_ramp_pct": 100}, "lexw")
    (b,) = one(rep, LEXP)
    assert b.th == 96 and b.clamped == 1
    assert rep.ramp_fallback == rep.ramp_by_floor == rep.ramp_launches > 0
    assert rep.ramp_th_min == rep.ramp_th_max == 96


@pytest.mark.parametrize("setting", [{}] + LEX_SOME, ids=ident)
def test_lex_cavity_converging(setting):
    """The same grid with tol_factor 1.3e-2: the oracle stops at 356, strictly between (nx + ny) / 2 = 324
    and the cap 420, so the GPU detects the stop late, in steady launches, and replays the solve to it
    through steady launches again."""
    (io, _), _ = oracle_result("lex_converging")
    assert (460 + 188) // 2 < io < 420
    t, rep = check("lex_converging", setting, "lexw")
    (b,) = one(rep, LEXP)
    assert b.launches > 0
    lex_regimes(setting, b, rep, up_exact=False)  # (a continuation's launches evaluate every row: no up bands)


@pytest.mark.parametrize("setting", [{}] + LEX_ALL, ids=ident)
def test_lex_channel(setting):
    """Channel 460 x 152, capped at 420: ghosts refreshed in the skew, the first and last interior bands
    row-checked (they stay down), the bands between them up and down."""
    t, rep = check("lex_channel", setting, "lexw")
    (b,) = one(rep, LEXP)
    assert (b.sweeps, b.ctiles) == (4, 5)
    assert t.poisson_steady_launches > 0 and b.launches == t.poisson_steady_launches
    lex_regimes(setting, b, rep, up_exact=False)
    if setting.get("lexw_updown", 1) == 1 and b.nb0 >= 4:
        assert b.up_bands >= 1


@pytest.mark.parametrize("setting", LEX_STEP, ids=ident)
def test_lex_step(setting):
    """Backwards step 480 x 160 with the step's column at 240 and the inlet 80 rows high, capped at 420: of
    the five 110-column tiles, tile 1 is in the left class (beside the wall tile), tile 2 crosses the
    step's column (its bands at the block's edge split) and tile 3 lies right of it. lexw_left 0 puts
    tile 1 on the masked march with the crossing ones."""
    t, rep = check("lex_step", setting, "lexw")
    (b,) = one(rep, LEXP)
    assert (b.sweeps, b.ctiles) == (4, 5)
    assert t.poisson_steady_launches > 0 and b.launches == t.poisson_steady_launches
    lex_regimes(setting, b, rep, up_exact=False, ramp_default=100)
    if setting.get("lexw_left", 1):
        assert (b.left_tiles, b.xn) == (1, 1)
    else:
        assert (b.left_tiles, b.xn) == (0, 2)
    assert b.xbn >= 1 and b.ctiles - 2 - b.left_tiles - b.xn == 1  # a split band; a tile right of the step
    assert b.launch_tiles == 2 * b.nbe0 + (b.ctiles - 2) * b.nb0 + b.xn * b.xbn * 2  # (crossing bands in three parts)


@pytest.mark.parametrize("setting", LEX_TALL, ids=ident)
def test_lex_tall(setting):
    """Cavity 129 x 300 capped at 60 (all ramp): a ramp launch at height 1 has more than 256 bands, so the
    band-table rule raises it by 10; with march_min_th 1 the steady height is 1, the raised height lies
    past it and the launch falls back to what 256 bands need (height 2: bands split into halves of 1)."""
    t, rep = check("lex_tall", setting, "lexw")
    (b,) = one(rep, LEXP)
    assert (b.ctiles, b.hi0 - b.lo0) == (2, 302) and t.poisson_steady_launches == 0
    lex_regimes(setting, b, rep)
    if "lexw_waves" not in setting and setting.get("lexw_ramp_pct", 0) == 0:
        assert rep.ramp_grown_bands > 0 and rep.ramp_nb_max > 128
    if setting.get("march_min_th") == 1:
        assert b.th == 1 and rep.ramp_fallback > 0 and rep.ramp_th_max == 2


@pytest.mark.parametrize("setting", LEX_STRIPS, ids=ident)
def test_lex_cavity_strips(setting):
    """The cavity fixture on 3 strips: 3 sweeps per launch (112-column tiles), one plan per strip, each
    for a third of the budget (lexw_waves 64: 21 tiles)."""
    t, rep = check("lex_strips", setting, "lexw")
    plans = one(rep, LEXP)
    assert len(plans) == 3 and len({b.waves for b in plans}) == 1
    for b in plans:
        assert (b.sweeps, b.ctiles, b.extra) == (3, 5, 15) and b.launches > 0
        lex_regimes(setting, b, rep)


@pytest.mark.parametrize("spl", [5, 6])
@pytest.mark.parametrize("setting", LEX_DEEP, ids=ident)
def test_lex_cavity_deep_launches(spl, setting):
    """The cavity fixture at 5 and 6 sweeps per launch: the LDS source ring, 106- / 102-column tiles
    (5 of them), max_th 90."""
    t, rep = check(f"lex_spl{spl}", setting, "lexw")
    (b,) = one(rep, LEXP)
    assert (b.sweeps, b.ctiles, b.extra, b.max_th) == (spl, 5, 4 * spl + 3, 90)
    assert t.poisson_steady_launches > 0 and b.launches == t.poisson_steady_launches
    lex_regimes(setting, b, rep, max_th=90)


@pytest.mark.parametrize("spl", [5, 6])
def test_lex_cavity_deep_launches_clamped(spl):
    """Cavity 240 x 178 capped at 230, 5 and 6 sweeps per launch, march_min_th 1000: 180 rows need two
    bands of 90, which the 10-row rounding takes past max_th 90 - th is clamped to 90."""
    t, rep = check(f"lex_deep{spl}", {"march_min_th": 1000}, "lexw")
    (b,) = one(rep, LEXP)
    assert (b.sweeps, b.th, b.max_th, b.clamped, b.nb0) == (spl, 90, 90, 1, 2)
    assert t.poisson_steady_launches > 0 and b.up_bands == 1


# ---- red-black (engine march) --------------------------------------------------------------------

def rb_regimes(setting, b):
    """What a red-black knob value must show in a fused-launch plan b."""
    rows = b.hi0 - b.lo0
    if "pair_wps" in setting:  # (a whole number of CUs x 4 SIMDs x pair_wps; the overlapped interior: less 2 ctiles)
        assert (b.waves + (2 * b.ctiles if b.kind == INTERIOR else 0)) % (4 * setting["pair_wps"]) == 0
    if setting.get("march_min_th") == 1 and b.waves // b.ctiles >= rows:
        assert b.th == th_min(b) and b.nb0 == -(-rows // b.th)  # (4 sweeps: one-row bands)
    if setting.get("march_min_th") == 1000:
        assert b.nb0 + b.nb1 == 1 and b.th == rows  # one band per column tile
    if setting.get("pair_edge_pct") == 10:
        assert b.the == 8
    if setting.get("pair_edge_pct") == 100 and not b.clamped:
        assert b.the == max(8, b.th)
    assert b.march_order == setting.get("march_order", 0)


@pytest.mark.parametrize("proof", ["proof", "exact"])
@pytest.mark.parametrize("setting", [{}] + RB_PAIR, ids=ident)
def test_rb_cavity(setting, proof):
    """Cavity 460 x 188 capped at 420: 105 proof launches of 4 sweeps, or 140 exact launches of 3. Reaches
    one-row bands (march_min_th 1), one band per column tile (1000), the == 8 (pair_edge_pct 10) and
    both march orders."""
    t, rep = check(f"rb_cavity_{proof}", setting, "march")
    ns = 4 if proof == "proof" else 3
    (b,) = one(rep, PAIR, sweeps=ns)
    assert (b.proof, b.ctiles, b.extra) == (int(proof == "proof"), 5, 4 * ns + 3)
    if t.proof_fallbacks == 0:
        assert b.launches == 420 // ns and rep.n_plans == 1
    rb_regimes(setting, b)
    if setting.get("march_min_th") == 1:
        assert b.th == (1 if ns == 4 else 5) and b.the == 8


@pytest.mark.parametrize("setting", [{}] + RB_SOME, ids=ident)
def test_rb_cavity_converging(setting):
    """Fixture "A" of check_every_cases.py (240 x 120, a natural stop at 341) with the proof on: proof
    launches, then the exact window from the launch that computed the iteration the proof left open."""
    (io, _), _ = oracle_result("rb_converging")
    assert 0 < io < CE.params("A").max_iters
    t, rep = check("rb_converging", setting, "march")
    assert t.proof_fallbacks >= 1
    assert one(rep, PAIR, proof=1) and one(rep, PAIR, proof=0)
    for b in one(rep, PAIR):
        rb_regimes(setting, b)


@pytest.mark.parametrize("setting", RB_REMAINDER, ids=ident)
def test_rb_cavity_one_sweep_last_launch(setting):
    """The cavity fixture capped at 61 = 15 x 4 + 1: the last launch runs one iteration with
    poisson_wave_kernel under plan.hpp's wave_bands (120-column tiles: 4 of them); march_min_th 1 gives it one-row
    bands, 1000 one band per column tile."""
    t, rep = check("rb_remainder", setting, "march")
    (w,) = one(rep, WAVE)
    assert (w.sweeps, w.launches, w.ctiles, w.the, w.nbe0) == (1, 1, 4, w.th, w.nb0)
    (b,) = one(rep, PAIR, sweeps=4, proof=1)
    if t.proof_fallbacks == 0:
        assert b.launches == 15
    rows = w.hi0 - w.lo0
    if "wave_wps" in setting:
        assert w.waves % (4 * setting["wave_wps"]) == 0
    if setting.get("march_min_th") == 1:
        assert w.th == 1 and w.nb0 == rows
    if setting.get("march_min_th") == 1000:
        assert w.nb0 == 1 and w.th == rows


@pytest.mark.parametrize("setting", RB_WIDE, ids=ident)
def test_rb_cavity_wide_budget_bound(setting):
    """Cavity 700 x 150 capped at 61: at one-row bands 7 column tiles x 152 rows are more tiles than
    pair_wps 1's round (1024 on 256 CUs), so the budget, not the floor, sets the band count - the plan
    pair_wps 1 shortens. The default budget (2 waves per SIMD for proof launches) still fits one-row bands."""
    t, rep = check("rb_wide", setting, "march")
    (b,) = one(rep, PAIR, sweeps=4)
    assert b.ctiles == 7
    if setting.get("pair_wps") == 1:
        assert b.budget_bands and b.th > 1 and b.tiles <= b.waves
    else:
        assert not b.budget_bands and b.th == 1


@pytest.mark.parametrize("case", ["channel", "step"])
@pytest.mark.parametrize("setting", [{}] + RB_PAIR, ids=ident)
def test_rb_open_proof(case, setting):
    """Channel 460 x 152 and step 480 x 160 (step column 240) capped at 420, proof on: open.hip's 4-sweep
    launches; the step's plan carries the left class (tile 1 left of the step's column, tile 2 across)."""
    t, rep = check(f"rb_{case}_proof", setting, "march")
    (b,) = one(rep, PAIR, sweeps=4, proof=1)
    assert b.ctiles == 5 and (t.proof_fallbacks > 0 or b.launches == 105)
    assert (b.nl, b.ncx) == ((1, 1) if case == "step" else (0, 0))
    rb_regimes(setting, b)


@pytest.mark.parametrize("case", ["channel", "step"])
@pytest.mark.parametrize("setting", RB_OPEN_EXACT, ids=ident)
def test_rb_open_exact(case, setting):
    """The same fixtures with proof_test off: the 2-sweep pair kernel, 210 launches."""
    t, rep = check(f"rb_{case}_exact", setting, "march")
    (b,) = one(rep, PAIR, sweeps=2, proof=0)
    assert b.launches == 210 and (b.nl, b.ncx) == (0, 0) and b.extra == 15
    rb_regimes(setting, b)


_ranks_oracle = {}


def ranks_params():
    return C.make_params("cavity", nx=240, ny=128, max_iters=200)


@pytest.mark.parametrize("setting", RB_RANKS, ids=ident)
def test_rb_ranks_overlapped(setting):
    """Cavity 240 x 128 on two loopback ranks of 64 rows, two steps capped at 200, against the red-black
    oracle's steps: the overlapped path, whose interior rows (48 of them: 16 go to the boundary launch)
    are planned for the budget less the boundary launches' 2 x 3 tiles."""
    cp = ranks_params()
    if not _ranks_oracle:
        o = O.Oracle(cp, ordering=O.RB)
        _ranks_oracle["its"] = [o.step() for _ in range(2)]
        _ranks_oracle["p"] = o.field("p").copy()
    if "counts" not in _ranks_oracle:
        _ranks_oracle["counts"] = [(r["launches"], r["sweeps"]) for r in
                                   run_ranks(cp, 2, 2, small_solve="off", proof_test="on", tuning=MARCH)]
    res = run_ranks(cp, 2, 2, small_solve="off", proof_test="on", tuning={**MARCH, **setting})
    for r, counts in zip(res, _ranks_oracle["counts"]):
        assert r["its"] == _ranks_oracle["its"], setting
        j0, j1 = r["rows"]
        first, last = (0 if j0 == 1 else j0), (j1 + 1 if j1 == cp.ny else j1)
        assert_bits(r["p"], _ranks_oracle["p"][first:last + 1], f"ranks {setting} rows {j0}..{j1}")
        assert r["overlapped"] > 0 and (r["launches"], r["sweeps"]) == counts
        rep = r["plan"]
        assert _lib.SOR_KERNEL[rep.sor_kernel] == "march" and rep.plans_dropped == 0
        for b in rep.plans:
            check_plan(b, f"ranks {setting}")
        for b in one(rep, INTERIOR):
            assert (b.hi0 - b.lo0, b.ctiles) == (64 + 1 - 16, 3)  # (the wall's ghost row is the rank's too)
            assert (b.waves + 2 * b.ctiles) % (4 * setting.get("pair_wps", 1)) == 0
            rb_regimes(setting, b)
