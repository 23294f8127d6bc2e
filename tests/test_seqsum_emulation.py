"""Host restatement of seqsum.hip's binade-chunked sequential sum, checked bit
for bit against the plain chain (one IEEE rounding per term, the reference's
loop: channel-01.cpp:620-628, backwards_step-01.cpp:843-866) on terms built to
stress it: the open cases' shape (a steady mean plus noise), random signs over
many binades (the running sum crossing zero), exact ties at the running sum's
unit, -0.0 solids, a carried start (strips / ranks), non-finite terms, and the
crafted families of tests/seqsum_cases.py (ties of either sign against sums of
either sign, partial sums landing on a binade's edge, terms too large for a
binade, the kinetic energy's half-integers). It pins the integer-path argument
on the CPU; tests/test_gpu_seqsum.py runs the kernels themselves against the
same plain chain.

FAULTS names one-line faults of the restatement (fault() puts one in): the
fault matrix below asserts that the crafted families tell each faulty version
from the chain, which keeps them from going vacuous."""
from __future__ import annotations

import contextlib
import math

import numpy as np
import pytest

import seqsum_cases as SC
from seqsum_cases import chain

CH = 512           # SQ_CH
L_, H_ = 2 ** 52 + 1, 2 ** 53 - 1

# fault -> the crafted families (tests/seqsum_cases.py) that must notice it
FAULTS = {
    "q_trunc": ("neg_ties", "neg_halves", "neg_mixed_halves", "mixed_halves"),  # q = trunc(y), not floor(y)
    # a tie rounds up, not to even. (neg_odd_const cannot notice: its q = -2^36 - 1 is odd and its sums even, so the
    # even neighbour is always the upper one; tie_down is its fault, and odd_const cannot notice that one.)
    "tie_up": ("neg_ties", "neg_halves", "mixed_halves", "neg_mixed_halves", "odd_const", "ke_halves", "ke_mixed",
               "graze+", "graze-", "hit_up:511", "hit_up:512", "hit_up:767", "hit_up:32767", "hit_up:32768"),
    # a tie rounds down, not to even. (ke_halves' ties all go down, see seqsum_cases.ke_fields: of the faults here it
    # notices tie_up alone, and ke_mixed is the kinetic energy's family for the others.)
    "tie_down": ("neg_odd_const", "neg_ties", "neg_halves", "ke_mixed"),
    "tie_no_p": ("neg_ties", "graze+", "graze-", "ke_mixed"),  # the tie's parity term ignores the incoming parity p
    "combine_no_parity": ("neg_ties", "ke_mixed"),     # meta_combine ignores the parity handed over
    "check_record0": ("neg_ties", "ke_mixed"),         # meta_check always takes record 0
    "low_bound": ("graze+", "graze-"),                 # lower bound 2^52, not 2^52 + 1
    "neg_bound": ("graze-",),                          # the negative sum's bound off by one (hi <= -L + 1)
}
FAULT = None


@contextlib.contextmanager
def fault(name):
    global FAULT
    assert name in FAULTS
    FAULT = name
    try:
        yield
    finally:
        FAULT = None


def chunk_record(block, u):
    """seq_chunk_kernel: per incoming parity (R, min, max) of the integer prefix sums, or None (serial)."""
    y = np.ldexp(block, -u)
    if not np.all(np.abs(y) < 2.0 ** 51):
        return None
    tr = np.trunc(y)
    fr = y - tr
    tie = np.abs(fr) == 0.5
    r = tr.astype(np.int64) + (fr > 0.5) - (fr < -0.5)
    q = (np.trunc(y) if FAULT == "q_trunc" else np.floor(y)).astype(np.int64)
    recs = []
    for par in (0, 1):
        if not tie.any():
            p = np.cumsum(r)
            recs.append((int(p[-1]), min(0, int(p.min())), max(0, int(p.max()))))
            continue
        R = lo = hi = 0
        p_in = 0 if FAULT == "tie_no_p" else par
        for k in range(block.size):
            if tie[k]:
                up = {"tie_up": 1, "tie_down": 0}.get(FAULT, (p_in + R + int(q[k])) & 1)
                R += int(q[k]) + up
            else:
                R += int(r[k])
            lo, hi = min(lo, R), max(hi, R)
        recs.append((R, lo, hi))
    return recs


def combine(a, b):
    """meta_combine: a then b, b's record chosen by the parity a hands over."""
    out = []
    for p in (0, 1):
        R, lo, hi = a[p]
        bR, blo, bhi = b[p if FAULT == "combine_no_parity" else (p + R) & 1]
        out.append((R + bR, min(lo, R + blo), max(hi, R + bhi)))
    return out


def apply(s, recs, u):
    """meta_apply: the exact check, then s + the record by the integer path."""
    if recs is None:
        return None
    S = math.ldexp(s, -u) if math.isfinite(s) else math.inf
    if not (2.0 ** 52 <= abs(S) < 2.0 ** 53):
        return None
    Si = int(S)
    R, lo, hi = recs[0 if FAULT == "check_record0" else Si & 1]
    L = 2 ** 52 if FAULT == "low_bound" else L_
    negL = L - 1 if FAULT == "neg_bound" else L
    ok = (Si + lo >= L and Si + hi <= H_) if Si > 0 else (Si + hi <= -negL and Si + lo >= -H_)
    return math.ldexp(float(Si + R), u) if ok else None


def chunked(x, s0=0.0):
    """seq_approx/units/chunk kernels + seq_walk_kernel (the longest passing prefix of up to 64 chunks)."""
    nch = (x.size + CH - 1) // CH
    blocks = np.concatenate([x, np.full(nch * CH - x.size, -0.0)]).reshape(nch, CH)
    with np.errstate(invalid="ignore", over="ignore"):
        approx = blocks.sum(axis=1)
        pre = np.concatenate([[0.0], np.cumsum(approx)[:-1]]) + s0
    units = [math.frexp(p)[1] - 53 if math.isfinite(p) else 0 for p in pre]
    recs = [chunk_record(blocks[c], units[c]) for c in range(nch)]
    s, k, plain = s0, 0, 0
    while k < nch:
        run = 0
        while run < 64 and k + run < nch and units[k + run] == units[k]:
            run += 1
        acc, take, s_new = None, 0, None
        for c in range(k, k + run):
            if recs[c] is None:
                break
            acc = recs[c] if acc is None else combine(acc, recs[c])
            t = apply(s, acc, units[k])
            if t is None:
                break
            take, s_new = take + 1, t
        if take:
            s, k = s_new, k + take
            continue
        plain += 1
        s, k = chain(blocks[k], s), k + 1
    return s, nch, plain


def same_bits(a, b):
    return np.float64(a).view(np.int64) == np.float64(b).view(np.int64) or (math.isnan(a) and math.isnan(b))


def _terms(kind, rng, n):
    if kind == "drift":
        return -9900.0 + rng.normal(0.0, 50.0, n)
    if kind == "signs":
        return rng.choice([-1.0, 1.0], n) * np.exp(rng.normal(0.0, 8.0, n))
    if kind == "ties":
        return 1024.0 * rng.integers(2 ** 39, 2 ** 41, n).astype(np.float64)
    if kind == "halves":
        return rng.integers(1, 2 ** 20, n) + 0.5
    if kind == "solids":
        return np.where(rng.random(n) < 0.3, -0.0, rng.normal(-5.0, 1.0, n))
    raise ValueError(kind)


@pytest.mark.parametrize("kind,s0", [("drift", 0.0), ("signs", 0.0), ("ties", 0.0), ("halves", 2.0 ** 52),
                                     ("solids", 0.0), ("drift", -1.0e6), ("signs", 3.5e12)])
def test_chunked_equals_plain_chain(kind, s0):
    rng = np.random.default_rng([len(kind), ord(kind[0]), int(abs(s0)) % 100003])
    x = _terms(kind, rng, 150_000)
    want = chain(x, s0)
    got, nch, plain = chunked(x, s0)
    assert same_bits(want, got), (want, got)
    if kind in ("drift", "ties", "halves", "solids"):
        assert plain <= nch // 4, (plain, nch)


def test_chunked_non_finite_and_empty():
    x = np.full(10_000, 1.25)
    x[3000], x[7000] = np.inf, -np.inf
    got, _, _ = chunked(x)
    assert math.isnan(got) and math.isnan(chain(x))
    assert chunked(np.zeros(0), 2.5)[0] == 2.5


# ---- the crafted families (tests/seqsum_cases.py) --------------------------------------------------------------

_want = {}


def _chain_of(name):
    if name not in _want:
        _want[name] = chain(SC.terms(name))
    return _want[name]


@pytest.mark.parametrize("name", SC.NAMES + SC.KE_NAMES)
def test_crafted_family_equals_plain_chain(name):
    """Same bits as the chain, on the path the family was built for: the
    integer path for all but big:2^51, whose every chunk runs as the chain."""
    x = SC.terms(name)
    got, nch, plain = chunked(x)
    assert same_bits(_chain_of(name), got), (_chain_of(name), got)
    assert nch == (x.size + CH - 1) // CH
    if name == SC.BIG_SERIAL:
        assert plain == nch, (plain, nch)
    else:
        assert plain <= nch // 4, (plain, nch)


@pytest.mark.parametrize("name", sorted(FAULTS))
def test_each_fault_is_noticed_by_its_families(name):
    """The fault matrix: the restatement with one fault put in gives another
    sum than the chain on every family named for that fault, and another
    mean: the GPU tests see a sum through sum / count only. (Each fault runs
    on its noticing families only: the file stays under its half minute.)"""
    missed = []
    with fault(name):
        for fam in FAULTS[name]:
            x = SC.terms(fam)
            got, _, _ = chunked(x)
            if same_bits(_chain_of(fam), got) or same_bits(_chain_of(fam) / x.size, got / x.size):
                missed.append(fam)
    assert not missed, f"fault {name} goes unnoticed on {missed}"


def test_graze_lands_where_it_was_built():
    """The grazes' landing stands where the chunk is still guessed in the
    upper binade: the chunk of the landing is refused by the exact check (and
    runs as the chain), not by a guess of the lower binade's unit."""
    for fam, sign in (("graze+", 1.0), ("graze-", -1.0)):
        x = SC.terms(fam)
        pos = SC.graze_position()
        assert chain(x[:pos]) == sign * SC.SCALE * (2.0 ** 52 + SC.GRAZE_M)
        c = pos // CH
        approx = float(x[:c * CH].sum())
        assert math.frexp(approx)[1] - 53 == 10, approx  # unit 2^10: the binade [2^62, 2^63) of SCALE * 2^52
