"""tests/rb_sums.py (the red-black tree sums restated on the host) kept sharp
and not vacuous, on the CPU:

* adversarial inputs: on every shape of tests/test_gpu_rb_sums.py the restated
  total differs from the reference's sequential one, for the source and for the
  kinetic energy (a condition on the inputs: with equal totals the GPU test
  could not tell the two orders apart);
* mutants: each deviation of the stated order (waves added 3..0, butterfly
  offsets 1..32, partials column-major, stride 255, ranks added in reverse,
  ghost row 0 counted) changes, alone, the total on at least one of those
  shapes: a kernel that deviated so would show in the bits;
* exactness: on integer-valued inputs below 2^53 every order gives the exact
  sum, and so must the restatement;
* the oracle hooks: step_phases given the sequential sum as its callable is
  orc_step, bit for bit.
"""
from __future__ import annotations

import numpy as np
import pytest

import cfd_amd as C
import oracle as O
import rb_sums as R


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a: float, b: float) -> bool:
    return bits([a])[0] == bits([b])[0]


_cache: dict = {}


def shape_inputs(shape):
    """(raw f, ke terms, mask, layout) of a shape's adversarial fields, from the oracle's own phases."""
    if shape not in _cache:
        case, nx, ny, n, ranks = shape
        cp = C.make_params(case, nx=nx, ny=ny)
        o = O.Oracle(cp)
        F = R.adversarial_fields(shape)
        o.field("us")[:, :nx + 1] = F["us"]
        o.field("vs")[:ny + 1, :] = F["vs"]
        o.field("u")[:, :nx + 1] = F["u"]
        o.field("v")[:ny + 1, :] = F["v"]
        raw = []
        o.source(total=lambda f: raw.append(np.array(f)) or 0.0)
        o.centers()
        mask = np.array(o.mask())
        _cache[shape] = (raw[0], R.ke_terms(o.field("uc"), o.field("vc"), mask), mask, R.layout(ny, n, ranks))
    return _cache[shape]


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_adversarial_inputs_tell_the_orders_apart(shape):
    raw, ke, mask, strips = shape_inputs(shape)
    ranks = shape[4]
    terms = np.abs(raw[mask != 0])
    assert terms.max() / terms[terms > 0].min() >= 2.0 ** 40  # (the span the inputs are built for)
    assert (raw > 0).any() and (raw < 0).any()
    tree, seq = R.source_total(raw, mask, strips, ranks), R.sequential_total(raw, mask)
    assert not same(tree, seq), (tree, seq)
    assert abs(tree - seq) <= 1e-9 * terms.max()  # (two orders of one sum)
    tree, seq = R.tree_total(ke, strips, ranks), R.sequential_total(ke, mask)
    assert not same(tree, seq), (tree, seq)
    assert abs(tree - seq) <= 1e-9 * ke.max()


def test_sequential_total_is_orc_source():
    """rb_sums.sequential_total is orc_source's own sum: source(total=sequential) leaves
    orc_source's bits."""
    for shape in R.SHAPES[:6]:
        case, nx, ny, _, _ = shape
        cp = C.make_params(case, nx=nx, ny=ny)
        F = R.adversarial_fields(shape)
        a, c = O.Oracle(cp), O.Oracle(cp)
        for o in (a, c):
            o.field("us")[:, :nx + 1] = F["us"]
            o.field("vs")[:ny + 1, :] = F["vs"]
        mask = np.array(a.mask())
        assert a.source() == c.source(total=lambda f: R.sequential_total(f, mask))
        assert np.array_equal(bits(a.field("src")), bits(c.field("src"))), shape


MUTANTS = {
    "waves added 3..0": dict(wave_order=(3, 2, 1, 0)),
    "butterfly offsets 1..32": dict(offsets=(1, 2, 4, 8, 16, 32)),
    "partials column-major": dict(column_major=True),
    "stride 255": dict(stride=255),
    "ranks added in reverse": dict(reverse=True),
    "ghost row 0 counted": dict(ghost_row0=True),
}


def caught_on(mutant: dict) -> list[str]:
    out = []
    for shape in R.SHAPES:
        raw, ke, mask, strips = shape_inputs(shape)
        ranks = shape[4]
        if mutant.get("reverse") and not ranks:
            continue
        vals = np.where(mask != 0, raw, 0.0)
        if mutant.get("ghost_row0"):  # the mutant reads the ghost row: the u* / v* difference a kernel would form there
            vals = vals.copy()
            vals[0, 1:-1] = raw[1, 1:-1][::-1]
        if not same(R.tree_total(vals, strips, ranks, **mutant), R.tree_total(vals, strips, ranks)):
            out.append(R.shape_id(shape))
    return out


@pytest.mark.parametrize("name", list(MUTANTS))
def test_each_deviation_of_the_order_shows_in_the_bits(name):
    shapes = caught_on(MUTANTS[name])
    print(f"mutant '{name}' changes the total on: {', '.join(shapes) or 'no shape'}")
    assert shapes, name


def test_mutants_that_cannot_show_on_a_shape_do_not():
    """The converse, where the order cannot matter: stride 255 with at most 255 partials,
    two ranks in reverse (a + b = b + a), column-major with one block row."""
    raw, _, mask, strips = shape_inputs(R.SHAPES[0])  # 62 x 5: 1 x 2 blocks
    v = np.where(mask != 0, raw, 0.0)
    assert same(R.tree_total(v, strips, stride=255), R.tree_total(v, strips))
    raw, _, mask, strips = shape_inputs(("channel", 96, 48, 2, True))
    v = np.where(mask != 0, raw, 0.0)
    assert same(R.tree_total(v, strips, True, reverse=True), R.tree_total(v, strips, True))


def test_fold_is_the_butterfly():
    """wave_sums' fold a = a[:h] + a[h:2h] is lane 0 of the xor butterfly as device.hpp writes
    it (v[l] + v[l ^ off] in every lane), and every lane ends with the same bits."""
    rng = np.random.default_rng(5)
    v = R.adversarial(rng, (50, 4, 64), 30.0)
    full = R.butterfly(v)
    assert np.array_equal(bits(full[..., 0]), bits(R.wave_sums(v)))
    assert np.array_equal(bits(full), bits(np.broadcast_to(full[..., :1], full.shape)))


def test_block_layout_by_hand():
    """partials() against a direct loop over blocks and threads as source_kernel indexes them."""
    shape = ("channel", 96, 25, 3, False)
    raw, _, mask, strips = shape_inputs(shape)
    nx, ny = 96, 25
    assert strips == [(1, 8), (9, 16), (17, 25)]
    want = []
    for j0, j1 in strips:
        gx, gy = (nx + 2 + 63) // 64, (j1 - j0 + 1 + 3) // 4
        assert (gx, gy) == (2, 3 if j1 == 25 else 2)
        for by in range(gy):
            for bx in range(gx):
                v = np.zeros(256)
                for t in range(256):
                    i, j = bx * 64 + (t & 63), j0 + by * 4 + (t >> 6)
                    if 1 <= i <= nx and 1 <= j <= ny and j <= j1:
                        v[t] = raw[j, i]
                red = []
                for w in range(4):
                    a = v[64 * w:64 * w + 64].copy()
                    for off in (32, 16, 8, 4, 2, 1):
                        a = np.array([a[l] + a[l ^ off] for l in range(64)])
                    red.append(a[0])
                want.append(((red[0] + red[1]) + red[2]) + red[3])
    got = R.partials(raw, strips)
    assert len(got) == 4 + 4 + 6
    assert np.array_equal(bits(got), bits(want))
    # sum_partials: 14 partials, thread t holds 0.0 + p[t]
    s = np.zeros(256)
    s[:14] = 0.0 + got
    red = [R.butterfly(s[64 * w:64 * w + 64])[0] for w in range(4)]
    assert same(R.sum_partials(got), ((red[0] + red[1]) + red[2]) + red[3])


def test_sum_partials_second_round():
    """300 partials: threads 0..43 add p[t] then p[t + 256]."""
    rng = np.random.default_rng(11)
    p = R.adversarial(rng, 300, 30.0)
    s = np.zeros(256)
    for t in range(256):
        for k in range(t, 300, 256):
            s[t] = s[t] + p[k]
    assert same(R.sum_partials(p), float(R.block_sum256(s.reshape(4, 64))))
    assert same(R.sum_partials(np.zeros(0)), 0.0)


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_exact_on_integers(shape):
    """Integer-valued terms whose every partial sum stays below 2^53: no addition rounds,
    in any order. The restatement must return the exact sum."""
    case, nx, ny, n, ranks = shape
    _, _, mask, strips = shape_inputs(shape)
    rng = np.random.default_rng(R.shape_seed(shape) + 1)
    ints = rng.integers(-2 ** 30, 2 ** 30, size=(ny + 2, nx + 2))
    exact = int(ints[1:-1, 1:-1][mask[1:-1, 1:-1] != 0].sum())
    assert R.source_total(ints.astype(np.float64), mask, strips, ranks) == float(exact)
    for mutant in MUTANTS.values():
        if mutant.get("ghost_row0") or (mutant.get("reverse") and not ranks):
            continue
        assert R.source_total(ints.astype(np.float64), mask, strips, ranks, **mutant) == float(exact)
    a = 2 * rng.integers(-2 ** 10, 2 ** 10, size=(ny + 2, nx + 2))
    b = 2 * rng.integers(-2 ** 10, 2 ** 10, size=(ny + 2, nx + 2))
    inner = (slice(1, -1), slice(1, -1))
    exact = int((((a * a + b * b) // 2)[inner])[mask[inner] != 0].sum())
    assert R.ke_total(a.astype(np.float64), b.astype(np.float64), mask, strips, ranks) == float(exact)


def test_strips_of_and_rank_rows():
    assert R.strips_of(25, 3) == [(1, 8), (9, 16), (17, 25)]
    assert R.strips_of(7, 1) == [(1, 7)]
    assert R.layout(50, 3, True) == [(1, 17), (18, 34), (35, 50)]
    assert R.layout(48, 2, True) == [(1, 24), (25, 48)]


@pytest.mark.parametrize("ordering", [O.LEX, O.RB])
@pytest.mark.parametrize("case,steps", [("channel", 4), ("backwards_step", 3)])
def test_step_phases_with_the_sequential_sum_is_orc_step(case, steps, ordering):
    """Oracle.step(source_total=...) runs step_phases with orc_source_raw, the callable's total and
    orc_subtract_mean: given the sequential sum it is orc_step, bit for bit, every step."""
    cp = C.make_params(case)
    a, b = O.Oracle(cp, ordering=ordering), O.Oracle(cp, ordering=ordering)
    a.velocity_bc(False)
    b.velocity_bc(False)
    calls = []

    def total(f):
        calls.append(1)
        return R.sequential_total(f, np.array(b.mask()))

    for step in range(steps):
        ra, rb = a.step(), b.step(source_total=total)
        assert ra == rb, (case, step)
        for n in ("p", "src", "us", "vs", "u", "v"):
            assert np.array_equal(bits(a.field(n)), bits(b.field(n))), (case, step, n)
    assert len(calls) == steps  # (every step's source was non-zero: the callable ran)
    a.stats()
    b.stats()
    mask = np.array(b.mask())
    assert a.stats()[1] == b.kinetic_energy(lambda uc, vc: R.sequential_total(R.ke_terms(uc, vc, mask), mask))
