"""The red-black order's tree sums on the GPU (source_kernel / centers_stats_kernel
-> block_sum<256> -> sum_partials_kernel, on ranks comm_allreduce_sum) against
their restatement on the host (tests/rb_sums.py), bit for bit.

u*, v* (and u, v) are set from the host with fields whose terms span about
2^+-30 with mixed signs, on which the restated total differs from the
reference's sequential one (tests/test_rb_sums.py asserts that on the CPU): the
source after the mean removal, one capped solve's (iterations, residual) and
pressure, and the kinetic energy equal the oracle's with the restated totals.
Shapes (rb_sums.SHAPES): nx + 2 at 64 and 65, rows no multiple of 4, more than
256 partials, three strips with their part_off, the step's solids inside
blocks, two and three loopback ranks with even and uneven rows; and a zero
source. The claim for three ranks is the loopback transport's (ranks added
0, 1, 2): a real RCCL all-reduce over more than two devices states no order.
"""
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
from test_gpu_parity import assert_bits, ofield  # noqa: E402

CAP = 40


def oracle_side(shape, fields):
    """The oracle's source with the restated total, its capped solve, and the restated KE."""
    case, nx, ny, n, ranks = shape
    cp = C.make_params(case, nx=nx, ny=ny, max_iters=CAP)
    strips = R.layout(ny, n, ranks)
    o = O.Oracle(cp, ordering=O.RB)
    for name in ("us", "vs", "u", "v"):
        ofield(o, name, cp)[...] = fields[name]
    seen = []

    def total(raw_f):
        t = R.source_total(raw_f, np.array(o.mask()), strips, ranks)
        seen.append((t, R.sequential_total(raw_f, np.array(o.mask()))))
        return t

    o.source(total=total)
    src = o.field("src").copy()
    solve = o.poisson()
    omd, _ = o.stats()
    return dict(cp=cp, strips=strips, src=src, solve=solve, p=o.field("p").copy(), md=omd,
                ke=R.oracle_ke(o, strips, ranks), totals=seen)


def gpu_phases(g, fields, rows=None):
    """Source, capped solve, statistics of one solver (rows: the rank-local row slice per field)."""
    cut = (lambda name, a: a) if rows is None else (lambda name, a: a[rows(name, a.shape[0])])
    g.set_field("us", cut("us", fields["us"]))
    g.set_field("vs", cut("vs", fields["vs"]))
    g.buildSourceTerm()
    src = g.field("src")
    solve = g.solverPressurePoisson()
    p = g.field("p")
    g.set_field("u", cut("u", fields["u"]))
    g.set_field("v", cut("v", fields["v"]))
    md, ke = g.statistics()
    return dict(src=src, solve=solve, p=p, md=md, ke=ke)


def check(got, ref, what, rows=None):
    cut = (lambda a: a) if rows is None else (lambda a: a[rows("src", a.shape[0])])
    assert_bits(got["src"], cut(ref["src"]), f"{what}: source")
    assert got["solve"] == ref["solve"], what
    assert_bits(got["p"], cut(ref["p"]), f"{what}: pressure")
    assert got["md"] == ref["md"], what
    assert got["ke"] == ref["ke"], what


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if not s[4]], ids=R.shape_id)
def test_source_mean_and_kinetic_energy_equal_the_restated_sums(shape):
    fields = R.adversarial_fields(shape)
    ref = oracle_side(shape, fields)
    (tree, seq), = ref["totals"]
    assert tree != seq  # (the sequential total would give other bits: tests/test_rb_sums.py)
    g = C.solver_for(ref["cp"], ordering="rb", n_strips=shape[3])
    got = gpu_phases(g, fields)
    g.close()
    assert ref["solve"][0] > 0
    check(got, ref, R.shape_id(shape))


def run_rank_phases(cp, world, fields):
    L = _lib.lib()
    hub = L.cfd_comm_loopback_hub(world)
    assert hub
    results, errors = [None] * world, []

    def body(r):
        try:
            comm = L.cfd_comm_init_loopback(hub, r, 0)
            assert comm, L.cfd_last_error()
            j0, j1 = strip_rows(r, world, cp.ny)
            s = C.solver_for(cp, ordering="rb", rank_rows=(j0, j1), comm=comm)
            assert s.owned_rows() == (j0, j1)

            def rows(name, total_rows):  # the rows a rank solver stores (Solver::owned_field_rows)
                return slice(0 if j0 == 1 else j0, min(j1 + 1 if j1 == cp.ny else j1, total_rows - 1) + 1)

            results[r] = (gpu_phases(s, fields, rows), rows)
            s.close()
            L.cfd_comm_destroy(comm)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    L.cfd_comm_loopback_hub_destroy(hub)
    assert not errors, errors
    return results


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[4]], ids=R.shape_id)
def test_rank_reduction_equals_the_restated_sums(shape):
    """Each rank sums its own strip; the loopback all-reduce adds the ranks 0, 1, 2 in order."""
    fields = R.adversarial_fields(shape)
    ref = oracle_side(shape, fields)
    (tree, seq), = ref["totals"]
    assert tree != seq
    for r, (got, rows) in enumerate(run_rank_phases(ref["cp"], shape[3], fields)):
        check(got, ref, f"{R.shape_id(shape)} rank {r}", rows)


@pytest.mark.parametrize("case,nx,ny,strips", [("channel", 62, 5, 1), ("backwards_step", 64, 16, 2)])
def test_zero_source_keeps_total_zero(case, nx, ny, strips):
    """u* = v* = 0: every partial and the total are +0.0, the mean removal subtracts 0.0,
    the source stays +0.0 in every cell and the solve takes the absolute tolerance."""
    cp = C.make_params(case, nx=nx, ny=ny, max_iters=CAP)
    g = C.solver_for(cp, ordering="rb", n_strips=strips)
    o = O.Oracle(cp, ordering=O.RB)
    g.set_field("us", np.zeros((ny + 2, nx + 1)))
    g.set_field("vs", np.zeros((ny + 1, nx + 2)))
    g.buildSourceTerm()
    called = []
    o.source(total=lambda f: called.append(1) or 0.0)
    assert not called  # (max|f| = 0: the oracle removes no mean; the GPU removes 0.0 / count)
    assert R.source_total(o.field("src"), np.array(o.mask()), R.strips_of(ny, strips)) == 0.0
    src = g.field("src")
    assert not src.view(np.int64).any()  # +0.0 everywhere: no -0.0 from 0.0 - mean
    assert_bits(src, o.field("src"), "zero source")
    assert g.solverPressurePoisson() == o.poisson()
    assert_bits(g.field("p"), o.field("p"), "pressure")
    g.close()
