"""Term families of the sequential-sum tests: sums built to meet seqsum.hip's
integer path at its edges (ties of either sign against sums of either sign,
partial sums landing on a binade's edge, terms too large for a binade, the
kinetic energy's half-integers), held once as plain numpy.

Shared by tests/test_seqsum_emulation.py (CPU: the restatement against the
plain chain, and the fault matrix that keeps these families from going vacuous)
and tests/test_gpu_seqsum.py (the kernels against the same chain).

A mode-0 family is kept in "d-scale": the per-cell u* differences d, ny x nx.
source_kernel forms the term (rho / dt) * (d / dx); with rho / dt a power of
two and dx = 1 (params() below, checked by assert_scaling) the term is
SCALE * d exactly. rows_from_terms() turns d into u* rows whose cumulative sums
restart every row: that keeps a fractional term representable next to a 2^52
running sum, and assert_exact() checks that the row differences give d back
bit for bit. In the comments below "unit" is the running sum's unit in d-scale
(1 while the d-scale sum is in [2^52, 2^53)).
"""
from __future__ import annotations

import math

import numpy as np

import cfd_amd as C

NY, NX = 96, 2048  # 196 608 terms: the smallest size at which terms of 2^36..2^38 carry a sum from zero up
#                    through the 2^52- and 2^53-unit binades (where ties start)
DT = 2.0 ** -10
SCALE = 1024.0     # rho / dt of params()
GRAZE_M = 2 ** 29 + 12345


def chain(x, s=0.0):
    """The reference's loop: one IEEE rounding per term."""
    for v in np.asarray(x, dtype=np.float64).ravel().tolist():
        s = s + v
    return s


def params(case, nx, ny):
    """dx = 1 and rho / dt = 2^10: a u* difference d becomes the term 1024 d exactly."""
    cp = C.make_params(case, nx=nx, ny=ny, dt=DT)
    cp.length = float(nx)
    if case == "backwards_step":  # the block keeps its quarter of the length
        cp.step_x = float(nx // 4)
    assert_scaling(cp)
    return cp


def assert_scaling(cp):
    scale = cp.rho / cp.dt
    assert math.frexp(scale)[0] == 0.5 and scale == SCALE, scale  # a power of two
    assert 1.0 / cp.dx == 1.0, cp.dx


def rows_from_terms(d):
    """u* rows (ny x (nx + 1), column 0 zero) whose differences are the per-cell values d."""
    d = np.asarray(d, dtype=np.float64)
    return np.concatenate([np.zeros((d.shape[0], 1)), np.cumsum(d, axis=1)], axis=1)


def assert_exact(d):
    """The terms survive the trip through the fields: the row differences of
    rows_from_terms(d) are d bit for bit, and SCALE * d is finite."""
    us = rows_from_terms(d)
    back = us[:, 1:] - us[:, :-1]
    assert np.array_equal(back.view(np.int64), d.view(np.int64)), "row cumulative sums are not exact"
    assert np.all(np.isfinite(SCALE * d))
    return us


def _ties(ny, nx):  # (test_gpu_seqsum.py's "ties": integer terms, ties at unit 2 and up)
    return np.random.default_rng(3).integers(2 ** 36, 2 ** 38, ny * nx).astype(np.float64)


def _halves(ny, nx):  # (its "halves": ties from unit 1 on)
    return np.random.default_rng(4).integers(2 ** 36, 2 ** 38, ny * nx) + 0.5


def _mixed_halves(ny, nx):  # +-(k + 1/2), one sign three times in four: ties of either sign
    rng = np.random.default_rng(7)
    return rng.choice([-1.0, 1.0, 1.0, 1.0], ny * nx) * (rng.integers(2 ** 36, 2 ** 38, ny * nx) + 0.5)


def _odd_const(ny, nx):  # once the sum's unit doubles, every term is a tie
    return np.full(ny * nx, float(2 ** 37 + 1))


def _hit_up(t, ny, nx):
    """The sum lands exactly on 2^53 after index t; every later term (odd, unit 2) is a tie."""
    m = 2 ** 37 + 1
    d = np.full(ny * nx, float(m))
    d[0] = float(2 ** 53 - m * t)
    assert chain(d[:t + 1]) == 2.0 ** 53
    return d


def _hit_down(t, ny, nx):
    """The sum descends onto exactly 2^52 after index t, and on into the binade below."""
    m = 2 ** 30 + 1
    d = np.full(ny * nx, -float(m))
    d[0] = float(2 ** 52 + m * t)
    assert chain(d[:t + 1]) == 2.0 ** 52
    return d


def graze_position(nx=NX):
    """Flat index of the graze's landing term (the second term of row 41)."""
    return 41 * nx + 1


def _graze(sign, ny, nx):
    """A partial sum on a binade's lower edge. 40 rows of integers climb to
    exactly 2^52 + 2^41; row 40 descends by -(k + f); the first term of row 41
    is tuned so the chain stands at exactly 2^52 + m; the next term -(m + 3/8)
    takes the chain to 2^52 - 1/2 where the integer path would say 2^52; the
    term after that, (2^29 + 77) + 3/4, turns the half unit into a different
    rounded sum. All later terms are positive. Row 41 is the last chunk still
    guessed in the upper binade at 96 x 2048 (ten rows later the chunk is guessed
    in the lower binade and the lower bound is never asked)."""
    assert (ny, nx) == (NY, NX)
    n = ny * nx
    rng = np.random.default_rng(11)
    d = np.empty(n)
    up = 40 * nx
    d[:up] = rng.integers(2 ** 35, 2 ** 36, up).astype(np.float64)
    d[up:] = -(rng.integers(2 ** 29, 2 ** 30, n - up) + rng.choice([0.25, 0.375, 0.5, 0.625, 0.75], n - up))
    d[39 * nx] = float(2 ** 52 + 2 ** 41) - chain(np.delete(d[:up], 39 * nx))
    assert 0 < d[39 * nx] < 2 ** 50, d[39 * nx]
    assert chain(d[:up]) == float(2 ** 52 + 2 ** 41)
    pos = graze_position(nx)
    d[pos - 1] = (2.0 ** 52 + GRAZE_M) - chain(d[:pos - 1])
    d[pos] = -(GRAZE_M + 0.375)
    assert chain(d[:pos]) == 2.0 ** 52 + GRAZE_M
    assert chain(d[:pos + 1]) == 2.0 ** 52 - 0.5
    d[pos + 1:] = np.abs(d[pos + 1:])
    d[pos + 1] = float(2 ** 29 + 77) + 0.75
    return sign * d


def _big(y, ny, nx):
    """Alternating +-y units around S = 2^52 + 2^50."""
    d = np.empty(ny * nx)
    d[0] = float(2 ** 52 + 2 ** 50)
    d[1::2] = float(y)
    d[2::2] = -float(y)
    return d


BIG_SERIAL = "big:%d" % 2 ** 51  # an oversize term in every chunk: all of them run as the chain

# name -> (builder(ny, nx) of the flat d-scale terms, ny, nx). The hit_up landings at 511, 512 and 767 need rows
# shorter than the landing index: in the row that holds the first term the u* cumulative sum passes 2^53 otherwise,
# where the odd terms are no longer representable.
_SHAPE_HIT = (768, 256)
FAMILIES = {
    "neg_ties": (lambda ny, nx: -_ties(ny, nx), NY, NX),
    "neg_halves": (lambda ny, nx: -_halves(ny, nx), NY, NX),
    "mixed_halves": (_mixed_halves, NY, NX),
    "neg_mixed_halves": (lambda ny, nx: -_mixed_halves(ny, nx), NY, NX),
    "odd_const": (_odd_const, NY, NX),
    "neg_odd_const": (lambda ny, nx: -_odd_const(ny, nx), NY, NX),
    "graze+": (lambda ny, nx: _graze(1.0, ny, nx), NY, NX),
    "graze-": (lambda ny, nx: _graze(-1.0, ny, nx), NY, NX),
}
for _t in (511, 512, 767, 32767, 32768):  # a chunk's last term, a chunk's first, mid-chunk, the 64-chunk scan's end
    FAMILIES["hit_up:%d" % _t] = ((lambda ny, nx, t=_t: _hit_up(t, ny, nx)),) + _SHAPE_HIT
for _t in (511, 512, 700, 32767):
    FAMILIES["hit_down:%d" % _t] = ((lambda ny, nx, t=_t: _hit_down(t, ny, nx)), NY, NX)
for _y in (2 ** 51 - 1, 2 ** 51, 2 ** 50):
    FAMILIES["big:%d" % _y] = ((lambda ny, nx, y=_y: _big(y, ny, nx)), NY, NX)
NAMES = tuple(FAMILIES)
KE_NAMES = ("ke_halves", "ke_mixed")

_cache = {}


def family(name):
    """The d-scale terms of a mode-0 family, ny x nx, checked by assert_exact; read only."""
    if name not in _cache:
        build, ny, nx = FAMILIES[name]
        d = np.ascontiguousarray(build(ny, nx).reshape(ny, nx), dtype=np.float64)
        assert_exact(d)
        d.setflags(write=False)
        _cache[name] = d
    return _cache[name]


def terms(name):
    """What the sum sees, in loop order: SCALE * d (mode 0) or 0.5 (a^2 + b^2) (mode 1)."""
    if name in KE_NAMES:
        a, b, _, _ = ke_fields(name)
        return (0.5 * (a * a + b * b)).ravel()
    return (SCALE * family(name)).ravel()


def ke_fields(name, ny=NY, nx=NX):
    """Mode 1. ke_halves: cell-centre values a = 2k + 1, k in 2^17..2^18, with
    v = 0. The terms a^2 / 2 are exact half-integers, ties for the ~65 000
    terms the sum spends in [2^52, 2^53). Their floor (a^2 - 1) / 2 is a
    multiple of 4, so from the first tie on the sum is even and every tie goes
    down. ke_mixed: one cell in three also has an odd b, its term (a^2 + b^2) / 2
    an odd integer, which flips the sum's parity: the ties then go either way.
    Returns (a, b, u, v): the face fields with u_0 = 0, u_i = 2 a_i - u_{i-1}
    along the rows and v likewise up the columns: integers, so
    0.5 (u_{i-1} + u_i) = a_i exactly."""
    key = (name, ny, nx)
    if key not in _cache:
        rng = np.random.default_rng(3)
        a = (2 * rng.integers(2 ** 17, 2 ** 18, (ny, nx)) + 1).astype(np.float64)
        b = np.zeros((ny, nx))
        if name == "ke_mixed":
            b = np.where(rng.integers(0, 3, (ny, nx)) == 0, 2.0 * rng.integers(2 ** 16, 2 ** 17, (ny, nx)) + 1.0, 0.0)
        else:
            assert name == "ke_halves"
        u = np.zeros((ny, nx + 1))
        for i in range(1, nx + 1):
            u[:, i] = 2.0 * a[:, i - 1] - u[:, i - 1]
        v = np.zeros((ny + 1, nx))
        for j in range(1, ny + 1):
            v[j] = 2.0 * b[j - 1] - v[j - 1]
        for c, f in ((a, 0.5 * (u[:, :-1] + u[:, 1:])), (b, 0.5 * (v[:-1] + v[1:]))):
            assert np.array_equal(f.view(np.int64), c.view(np.int64)), "face field is not exact"
        t = 0.5 * (a * a + b * b)
        assert np.all((t - np.floor(t) == 0.5) == (b == 0.0)) and np.all(np.floor(t[b != 0.0]) % 2 == 1)
        for f in (a, b, u, v):
            f.setflags(write=False)
        _cache[key] = (a, b, u, v)
    return _cache[key]


def strip_chunks(ny, nx, n_strips=1, chunk=512):
    """seqsum_chunks of one sum: per strip (rows 1 + ny k / n .. ny (k + 1) / n) its terms in chunks of 512."""
    rows = [ny * (k + 1) // n_strips - ny * k // n_strips for k in range(n_strips)]
    return sum((r * nx + chunk - 1) // chunk for r in rows)


def sees_one_ulp(total, count):
    """Whether total / count tells total from both of its neighbours (the tests see a sum through its mean)."""
    q = total / count
    return np.nextafter(total, np.inf) / count != q and np.nextafter(total, -np.inf) / count != q
