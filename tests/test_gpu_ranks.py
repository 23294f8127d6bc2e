"""The multi-process (rank) code path on one GPU: ranks run in host threads of
one process and exchange halos / all-reduce through the library's in-process
loopback transport (RCCL refuses two ranks on one device). Everything but the
RCCL calls themselves is the code the 8-GPU run executes: rank strips, halo
row indices, the residual all-reduce feeding each rank's convergence test,
the source-sum and stats reductions, rank-local field transfer.

The open cases' source mean and every case's kinetic energy are tree sums whose
order depends on the layout (each rank sums its own strip, the loopback
all-reduce adds the ranks 0, 1, 2, ..): a rank run and a single-domain run
differ in the last bits, so each is held to the red-black oracle with its own
layout's total restated (tests/rb_sums.py): (iterations, residual) of every
step, u, v, p on the owned rows, max divergence and kinetic energy, bit for
bit. The claim for three or more ranks is the loopback transport's: a real
RCCL all-reduce over more than two devices states no order."""
from __future__ import annotations

import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import oracle as O  # noqa: E402
import rb_sums as R  # noqa: E402
from cfd_amd import _lib  # noqa: E402
from cfd_amd.dist import strip_rows  # noqa: E402


def run_ranks(cp, world, steps, check_every=1, timing=False, **kw):
    L = _lib.lib()
    hub = L.cfd_comm_loopback_hub(world)
    assert hub
    results = [None] * world
    errors = []

    def body(r):
        try:
            comm = L.cfd_comm_init_loopback(hub, r, 0)
            assert comm, L.cfd_last_error()
            s = C.solver_for(cp, ordering="rb", rank_rows=strip_rows(r, world, cp.ny), comm=comm, check_every=check_every, **kw)
            if cp.case_id == C.CAVITY:
                s.applyBoundaryConditions()
            its = [s.step() for _ in range(steps)]
            md, ke = s.statistics()
            results[r] = dict(rows=s.owned_rows(), u=s.field("u"), v=s.field("v"), p=s.field("p"), src=s.field("src"), its=its,
                              stats=(md, ke), overlapped=s.timing().poisson_overlapped,
                              fallbacks=s.timing().proof_fallbacks, launches=s.timing().poisson_launches,
                              sweeps=s.timing().poisson_sweeps, plan=s.sor_plan())
            s.close()
            L.cfd_comm_destroy(comm)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    L.cfd_comm_loopback_hub_destroy(hub)
    assert not errors, errors
    return results


FIELDS = ("u", "v", "p", "src")


def oracle_run(cp, steps, n=1, ranks=False):
    """The red-black oracle's run with the tree sums restated for n strips or n ranks:
    its, fields, (max divergence, kinetic energy)."""
    o = O.Oracle(cp, ordering=O.RB)
    o.velocity_bc(False)  # (the open cases' constructor; the cavity's applyBoundaryConditions)
    layout = R.layout(cp.ny, n, ranks)
    hook = None if cp.case_id == C.CAVITY else R.source_hook(o, layout, ranks)
    its = [o.step(source_total=hook) for _ in range(steps)]
    md, _ = o.stats()
    out = dict(its=its, stats=(md, R.oracle_ke(o, layout, ranks)))
    for n_ in FIELDS:
        a = o.field(n_)
        out[n_] = (a[:, :cp.nx + 1] if n_ == "u" else a[:cp.ny + 1] if n_ == "v" else a).copy()
    return out


def assert_rank_equals(r, ref, cp, stats=True):
    """A rank's result against a whole-domain run (the oracle's): bits on its rows."""
    assert r["its"] == ref["its"], r["rows"]
    j0, j1 = r["rows"]
    first = 0 if j0 == 1 else j0
    for n in FIELDS:
        last = min(j1 + 1 if j1 == cp.ny else j1, ref[n].shape[0] - 1)
        a, b = r[n], ref[n][first:last + 1]
        assert a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)), (n, r["rows"])
    if stats:
        assert r["stats"] == ref["stats"], r["rows"]


def assert_single_equals(s, its, ref):
    """A single-domain solver against the oracle's run with one strip's restated sums."""
    assert its == ref["its"]
    for n in FIELDS:
        a = s.field(n)
        assert np.array_equal(a.view(np.int64), ref[n].view(np.int64)), n
    assert s.statistics() == ref["stats"]


def single(cp, steps, **kw):
    s = C.solver_for(cp, ordering="rb", **kw)
    if cp.case_id == C.CAVITY:
        s.applyBoundaryConditions()
    its = [s.step() for _ in range(steps)]
    return s, its


@pytest.mark.parametrize("case,world,steps", [("cavity", 2, 15), ("cavity", 3, 10), ("channel", 2, 10),
                                               ("backwards_step", 2, 2)])
def test_rank_path_equals_single_domain(case, world, steps):
    cp = C.reference_defaults(case)
    res = run_ranks(cp, world, steps)
    s, its = single(cp, steps)
    ref = {n: s.field(n) for n in FIELDS}
    if case == "cavity":  # no sum feeds the state: the ranks equal one domain
        ref["its"] = its
        for r in res:
            assert_rank_equals(r, ref, cp, stats=False)
    oref = oracle_run(cp, steps, world, ranks=True)
    for r in res:
        assert_rank_equals(r, oref, cp)
    assert_single_equals(s, its, oracle_run(cp, steps))


def test_rank_path_check_every_8():
    """check_every=8 (an option; every GPU count defaults to 1, the reference's
    rule): the solve may run up to 7 sweeps past the reference's stopping
    point, never fewer, and still converges - at the oracle's iteration
    (the stop rule on multiples of 8 counted from the solve's start), with its
    residual and, on the owned rows, its pressure, bit for bit."""
    cp = C.reference_defaults("cavity")
    res = run_ranks(cp, 2, 5, check_every=8)
    _, its = single(cp, 5)
    o = O.Oracle(cp, ordering=O.RB)
    its_o = [o.step(check_every=8) for _ in range(5)]
    assert any(k8 != k1 for (k8, _), (k1, _r) in zip(its_o, its))  # (check_every decides a stop here)
    for r in res:
        for (ig, rg), (i1, _r1) in zip(r["its"], its):
            assert i1 <= ig <= i1 + 7
            assert ig % 8 == 0 or ig == cp.max_iters
        assert r["its"] == its_o
        j0, j1 = r["rows"]
        first = 0 if j0 == 1 else j0
        last = min(j1 + 1 if j1 == cp.ny else j1, cp.ny + 1)
        assert np.array_equal(r["p"].view(np.int64), o.field("p")[first:last + 1].view(np.int64)), r["rows"]


@pytest.mark.parametrize("case,world,ny,steps", [("cavity", 2, 128, 6), ("cavity", 3, 160, 4), ("channel", 2, 128, 4)])
def test_overlapped_halo_exchange_equals_single_domain(case, world, ny, steps):
    """Strips of >= 48 rows split each pair launch: the rows within 16 of a
    neighbour (after the halo exchange) on a second stream, the interior rows
    concurrently on the first. Must equal one domain (cavity bit for bit)."""
    cp = C.make_params(case, ny=ny, nx=96)
    res = run_ranks(cp, world, steps)
    s, its = single(cp, steps)
    if case == "cavity":
        ref = {n: s.field(n) for n in FIELDS}
        ref["its"] = its
    else:  # the channel: each layout against the oracle with its own restated source mean
        ref = oracle_run(cp, steps, world, ranks=True)
        assert_single_equals(s, its, oracle_run(cp, steps))
    for r in res:
        assert r["overlapped"] > 0, "overlap path not taken"
        assert_rank_equals(r, ref, cp, stats=case != "cavity")


@pytest.mark.parametrize("delta", [-2, -1, 0, 1, 2, 3])
def test_overlapped_lagged_stop_and_caps(delta):
    """Overlapped ranks test the residuals one pair late (their all-reduce runs
    beside the next launch) and keep three pressure buffers: a stop at an odd
    or even count, a cap just below / at / above the natural stop K, and the
    host's test of the last untested iterations must all give the
    single-domain iteration count and field."""
    base = C.make_params("cavity", ny=128, nx=96)
    s0, its0 = single(base, 1)
    K = its0[0][0]
    cp = C.make_params("cavity", ny=128, nx=96, max_iters=max(1, K + delta))
    res = run_ranks(cp, 2, 2)
    s, its = single(cp, 2)
    ref = s.field("p")
    for r in res:
        assert r["overlapped"] > 0
        assert r["its"] == its, (K, delta)
        j0, j1 = r["rows"]
        first = 0 if j0 == 1 else j0
        last = min(j1 + 1 if j1 == cp.ny else j1, ref.shape[0] - 1)
        assert np.array_equal(r["p"].view(np.int64), ref[first:last + 1].view(np.int64))


@pytest.mark.parametrize("world,nx,ny,steps,cap", [(2, 256, 256, 3, 0), (3, 300, 240, 2, 0), (2, 512, 512, 2, 61)])
def test_proof_mode_on_ranks(world, nx, ny, steps, cap):
    """The proof-mode convergence test on ranks: interior column
    tiles (nx >= 240), overlapped strips with the lagged test, ratios
    all-reduced (max) like residuals. Iteration counts and fields must equal
    one domain with exact residuals, bit for bit."""
    kw = {"max_iters": cap} if cap else {}
    cp = C.make_params("cavity", nx=nx, ny=ny, **kw)
    s, its = single(cp, steps, small_solve="off", proof_test="off")
    ref = s.field("p")
    res = run_ranks(cp, world, steps, proof_test="on")
    for r in res:
        assert r["overlapped"] > 0
        assert r["its"] == its
        if cap:
            assert r["fallbacks"] == 1  # the first step's corner-only source (tests/test_gpu_proof.py)
        else:
            assert r["fallbacks"] >= sum(1 for k, _ in its if k < cp.max_iters)
        j0, j1 = r["rows"]
        first = 0 if j0 == 1 else j0
        last = min(j1 + 1 if j1 == cp.ny else j1, ref.shape[0] - 1)
        assert np.array_equal(r["p"].view(np.int64), ref[first:last + 1].view(np.int64))


@pytest.mark.parametrize("case,world,nx,ny,steps,cap", [("channel", 2, 300, 160, 3, 0), ("channel", 3, 256, 200, 2, 900),
                                                        ("backwards_step", 2, 400, 160, 2, 0),
                                                        ("backwards_step", 4, 512, 256, 2, 700)])
def test_open_proof_mode_on_ranks(case, world, nx, ny, steps, cap):
    """The open cases' proof-mode launches (open.hip: 4 sweeps for the
    channel, 3 for the step on ranks) on overlapped ranks with the lagged,
    all-reduced test, and one domain with exact residuals: each against the
    red-black oracle with its own layout's source mean restated (summed per
    rank and all-reduced in rank order; one strip's tree sum), bit for bit,
    residuals included; iteration counts equal between the two."""
    kw = {"max_iters": cap} if cap else {}
    cp = C.make_params(case, nx=nx, ny=ny, **kw)
    s, its = single(cp, steps, small_solve="off", proof_test="off", tuning={"tile_rounds": 0, "resident": 0})
    assert_single_equals(s, its, oracle_run(cp, steps))
    res = run_ranks(cp, world, steps, proof_test="on")
    ref = oracle_run(cp, steps, world, ranks=True)
    for r in res:
        assert r["overlapped"] > 0
        assert [i for i, _ in r["its"]] == [i for i, _ in its]
        assert_rank_equals(r, ref, cp)
