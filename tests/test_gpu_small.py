"""The one-workgroup LDS solve (small.hpp) used for reference-sized grids:
whole timesteps bit-exact against the oracle's red-black restatement and
against the multi-launch kernels (small_solve="off") on the reference's own grids
(cavity 63², channel 93x31, step 256x32) and BASELINE configs[0] (128²) —
the open cases with the source mean's tree sum restated for the oracle
(tests/rb_sums.py), so bit-exact as well — the
stop rule with check_every > 1, and the size limit (a grid just over it takes
the multi-launch path with the same results)."""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import check_every_cases as F  # noqa: E402
import oracle as O  # noqa: E402
import rb_sums as R  # noqa: E402
from test_gpu_parity import assert_bits, ofield  # noqa: E402


def run_gpu(cp, steps, small=True, cavity=True, **kw):
    g = C.solver_for(cp, ordering="rb", small_solve="on" if small else "off", **kw)
    if cavity:  # cavity-01.cpp:380 (the open cases apply their BCs in the constructor)
        g.applyBoundaryConditions()
    its = [g.step() for _ in range(steps)]
    fields = {n: g.field(n).copy() for n in ("u", "v", "p", "src")}
    tm = g.timing()
    g.close()
    return its, fields, tm


@pytest.mark.parametrize("case,kw,steps", [
    ("cavity", {}, 25),
    ("channel", {}, 25),
    ("backwards_step", {}, 25),
    ("cavity", {"re": 100.0, "nx": 128, "ny": 128, "dt": 1e-3}, 10),
])
def test_small_solve_bitexact_vs_oracle_and_multi_launch(case, kw, steps):
    cp = C.reference_defaults(case) if not kw else C.make_params(case, **kw)
    assert (cp.nx + 2) * (cp.ny + 2) <= 20224
    cav = case == "cavity"
    its_s, f_s, tm = run_gpu(cp, steps, small=True, cavity=cav)
    assert tm.poisson_launches == steps  # one launch per solve: the small path ran
    o = O.Oracle(cp, ordering=O.RB)
    if case != "cavity":
        o.velocity_bc(False)
    # (the open cases' source mean: the GPU's tree sum, restated for one strip)
    hook = None if cav else R.source_hook(o, R.strips_of(cp.ny, 1))
    its_o = [o.step(source_total=hook) for _ in range(steps)]
    assert its_s == its_o
    for n in ("u", "v", "p", "src"):
        assert_bits(f_s[n], ofield(o, n, cp), f"{case} small vs oracle {n}")
    its_m, f_m, tm_m = run_gpu(cp, steps, small=False, cavity=cav)
    assert tm_m.poisson_launches > steps
    assert its_m == its_s
    for n in ("u", "v", "p", "src"):
        assert_bits(f_s[n], f_m[n], f"{case} small vs multi-launch {n}")


def test_small_check_every_and_cap():
    """check_every = 4 on the one-workgroup path. Converging (48x40,
    tol_factor 1e-5, cap 4000: three steps stop at 216, 220, 220 where
    check_every = 1 stops at 214, 219, 221): every stop a multiple of 4, the
    oracle's counts, residuals and fields, and the multi-launch path's. Capped
    (cap 57, no multiple of 4): every solve runs to the cap."""
    cp = F.params("E")
    its_s, f_s, tm = run_gpu(cp, F.steps("E"), small=True, check_every=4)
    its_m, f_m, _ = run_gpu(cp, F.steps("E"), small=False, check_every=4)
    ref = F.oracle_result("E", 4)
    assert tm.poisson_launches == len(its_s)
    assert all(0 < i < cp.max_iters and i % 4 == 0 for i, _ in its_s), its_s
    assert its_s == ref["its"] and its_s == its_m
    for n in ("u", "v", "p"):
        assert_bits(f_s[n], ref[n], f"check_every 4 vs oracle {n}")
        assert_bits(f_s[n], f_m[n], f"check_every 4 vs multi-launch {n}")
    cp = C.make_params("cavity", nx=48, ny=40, max_iters=57)
    its_s, f_s, _ = run_gpu(cp, 6, small=True, check_every=4)
    its_m, f_m, _ = run_gpu(cp, 6, small=False, check_every=4)
    assert its_s == its_m
    assert all(i == 57 for i, _ in its_s)
    assert_bits(f_s["p"], f_m["p"], "check_every 4, capped")


def test_over_the_limit_takes_multi_launch():
    cp = C.make_params("cavity", nx=150, ny=150, max_iters=200)  # 152² > 20224
    its, _, tm = run_gpu(cp, 2, small=True)
    assert tm.poisson_launches > 2
