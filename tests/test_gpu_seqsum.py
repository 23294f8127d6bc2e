"""The reference order's sequential sums (seqsum.hip, binade-chunked) against
the plain chain of adds, bit for bit, on crafted terms.

The reference removes the source mean with one running sum in loop order
(channel-01.cpp:620-628, backwards_step-01.cpp:843-866) and sums the kinetic
energy the same way (cavity-01.cpp:750-755): every partial sum rounded before
the next term. seqsum.hip evaluates chunks of 512 terms as exact integer sums
where the running sum provably stays in one binade and as the plain chain
elsewhere. These tests reach the kernels in both of their modes:
 * mode 0: u* / v* are set so that source_kernel forms chosen terms (wide
   magnitudes, sign changes, exact ties of either sign at the running sum's
   unit, partial sums landing on a binade's edge, terms too large for a binade,
   solids, a carried start on strips and ranks, rows and term counts at the
   chunk geometry's edges), buildSourceTerm runs, and the mean-removed source is
   compared with numpy: the same per-cell operations, the sum as a Python loop
   of float adds (one IEEE rounding per term, the reference's loop);
 * mode 1: u / v are set, statistics() runs, and the average kinetic energy
   is compared with the same loop over 0.5 (a^2 + b^2) of the cell-centre
   fields read back.
The crafted families live in tests/seqsum_cases.py; tests/test_seqsum_emulation.py
shows on the CPU which one-line faults of the algorithm each of them notices.
Every test also holds cfd_timing.seqsum_chunks to the chunk count of its grid.
Reference-sized whole runs and the BASELINE digests cover the real sources
(test_gpu_parity.py, test_gpu_lex_digests.py, test_gpu_lex_ranks.py)."""
from __future__ import annotations

import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import seqsum_cases as SC  # noqa: E402
from cfd_amd import _lib  # noqa: E402
from cfd_amd.dist import strip_rows  # noqa: E402

SOLVERS = {"channel": C.ChannelSolver, "backwards_step": C.BackwardsStepSolver, "cavity": C.CavitySolver}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def expected_source(g, cp, us, vs):
    """source_kernel + the sequential sum + subtract_mean_kernel, on the host."""
    ny, nx = cp.ny, cp.nx
    with np.errstate(invalid="ignore"):
        du = us[1:ny + 1, 1:nx + 1] - us[1:ny + 1, 0:nx]
    dv = vs[1:ny + 1, 1:nx + 1] - vs[0:ny, 1:nx + 1]
    f = (cp.rho / cp.dt) * (du * (1.0 / cp.dx) + dv * (1.0 / cp.dy))
    J, I = np.meshgrid(np.arange(1, ny + 1), np.arange(1, nx + 1), indexing="ij")
    fluid = (I > cp.step_i) | (J <= cp.inlet_jmax) if cp.case_id == 2 else np.ones_like(f, dtype=bool)
    f = np.where(fluid, f, 0.0)
    s = 0.0
    for v in f[fluid].tolist():  # loop order: j outer, i inner (row-major), solids skipped
        s = s + v
    mean = s / float(fluid.sum())
    return np.where(fluid, f - mean, 0.0), fluid, s


def run_source(cp, us_rows, n_strips=1, vs=None, label=None):
    """buildSourceTerm on u* rows; the chunk count is held to the grid's."""
    nx, ny = cp.nx, cp.ny
    g = SOLVERS[C.CASE_NAMES[cp.case_id]](cp, ordering="lex", n_strips=n_strips)
    us = np.zeros(g.field_shape("us"))
    us[1:ny + 1, :] = us_rows
    vsf = np.zeros(g.field_shape("vs")) if vs is None else vs
    g.set_field("us", us)
    g.set_field("vs", vsf)
    g.reset_timing()
    g.buildSourceTerm()
    got = g.field("src")[1:ny + 1, 1:nx + 1]
    t = g.timing()
    want, fluid, total = expected_source(g, cp, g.field("us"), g.field("vs"))
    g.close()
    bad = np.count_nonzero(bits(got[fluid]) != bits(want[fluid]))
    print(f"seqsum {label or ''} {C.CASE_NAMES[cp.case_id]} {ny}x{nx} strips={n_strips}: chunks {t.seqsum_chunks} "
          f"plain {t.seqsum_serial_chunks} sum {total!r} differing cells {bad}")
    assert t.seqsum_chunks == SC.strip_chunks(ny, nx, n_strips), (t.seqsum_chunks, SC.strip_chunks(ny, nx, n_strips))
    return bad, t, total, fluid


def run(case, nx, ny, us_rows, n_strips=1, vs=None):
    cp = C.make_params(case, nx=nx, ny=ny, dt=2.0 ** -10)
    if case == "channel":
        cp.length = float(nx)  # dx = 1: integer u* differences give terms (rho / dt) * du exactly
    bad, t, total, _ = run_source(cp, us_rows, n_strips, vs)
    return bad, t, total


def rows_from_terms(d, ny, nx):
    """u* rows whose differences are the given per-cell values (as floats)."""
    return SC.rows_from_terms(np.asarray(d, dtype=np.float64).reshape(ny, nx))


@pytest.mark.parametrize("kind", ["drift", "signs", "ties", "halves"])
def test_chunked_sum_equals_plain_chain(kind):
    rng = np.random.default_rng({"drift": 1, "signs": 2, "ties": 3, "halves": 4}[kind])
    ny, nx = 96, 2048
    n = ny * nx
    if kind == "drift":  # the open cases' shape: a steady mean plus noise
        d = -9.7 + rng.normal(0.0, 0.05, n)
    elif kind == "signs":  # sign changes, magnitudes over ~20 binades: many crossings of zero
        d = rng.choice([-1.0, 1.0], n) * np.exp(rng.normal(0.0, 7.0, n))
    elif kind == "ties":  # terms 1024 k: as the sum passes 2^63, 2^64, ... exact ties at its unit
        d = rng.integers(2 ** 36, 2 ** 38, n).astype(np.float64)
    else:  # terms 1024 (k + 1/2): ties once the sum passes 2^62
        d = rng.integers(2 ** 36, 2 ** 38, n) + 0.5
    bad, t, total = run("channel", nx, ny, rows_from_terms(d, ny, nx))
    assert bad == 0, f"{bad} cells differ (sum {total!r})"
    assert t.seqsum_chunks == (n + 511) // 512  # (chunks of 512 terms)
    if kind in ("drift", "ties"):  # the integer path carries most chunks
        assert t.seqsum_serial_chunks <= t.seqsum_chunks // 4, (t.seqsum_serial_chunks, t.seqsum_chunks)


@pytest.mark.parametrize("n_strips", [1, 3])
def test_chunked_sum_backwards_step_solids_and_strips(n_strips):
    """Solid cells (-0.0 terms) and strips continuing the previous strip's sum."""
    rng = np.random.default_rng(5)
    ny, nx = 64, 1000  # 64000 terms: a partial last chunk
    d = -3.3 + rng.normal(0.0, 0.5, ny * nx)
    bad, t, total = run("backwards_step", nx, ny, rows_from_terms(d, ny, nx), n_strips=n_strips)
    assert bad == 0, f"{bad} cells differ (sum {total!r})"
    assert t.seqsum_chunks == SC.strip_chunks(ny, nx, n_strips)


def test_chunked_sum_carries_non_finite_terms():
    """An infinite term: the chain's own result (inf, then NaN past -inf)."""
    ny, nx = 16, 512
    d = np.full(ny * nx, 1.25)
    d[3000] = np.inf
    d[5000] = -np.inf
    us = rows_from_terms(d, ny, nx)
    cp = C.make_params("channel", nx=nx, ny=ny, dt=2.0 ** -10)
    g = C.ChannelSolver(cp, ordering="lex")
    u = np.zeros(g.field_shape("us"))
    u[1:ny + 1, :] = us
    g.set_field("us", u)
    g.set_field("vs", np.zeros(g.field_shape("vs")))
    g.reset_timing()
    g.buildSourceTerm()
    got = g.field("src")[1:ny + 1, 1:nx + 1]
    assert g.timing().seqsum_chunks == ny * nx // 512
    want, fluid, total = expected_source(g, cp, g.field("us"), g.field("vs"))
    assert np.isnan(total) or np.isinf(total)
    assert np.array_equal(np.isnan(got), np.isnan(want))


# ---- mode 0: the crafted families through buildSourceTerm --------------------------------------------------------


def run_family(name, case="channel", n_strips=1):
    d = SC.family(name)
    ny, nx = d.shape
    cp = SC.params(case, nx, ny)
    bad, t, total, fluid = run_source(cp, SC.assert_exact(d), n_strips, label=name)
    if fluid.all():  # the kernels summed the family's own terms
        assert bits(total) == bits(SC.chain(SC.terms(name))), total
    return bad, t, total


def assert_path(name, t):
    """The path the family was built for: the integer path carries most chunks,
    but every chunk of big:2^51 (an oversize term in each) runs as the chain."""
    if name == SC.BIG_SERIAL:
        assert t.seqsum_serial_chunks == t.seqsum_chunks, (t.seqsum_serial_chunks, t.seqsum_chunks)
    else:
        assert t.seqsum_serial_chunks <= t.seqsum_chunks // 4, (t.seqsum_serial_chunks, t.seqsum_chunks)


@pytest.mark.parametrize("name", SC.NAMES)
def test_crafted_family_source_equals_plain_chain(name):
    bad, t, total = run_family(name)
    if name.startswith("graze"):  # (the graze moves the sum by one unit: the mean must show that much)
        assert SC.sees_one_ulp(total, SC.family(name).size)
    assert bad == 0, f"{bad} cells differ (sum {total!r})"
    assert_path(name, t)


@pytest.mark.parametrize("name,case", [("neg_ties", "backwards_step"), ("mixed_halves", "channel"),
                                       ("graze+", "channel")])
def test_crafted_family_on_strips_carried_start(name, case):
    """Three strips: the second and third start from a carried integer, odd
    or even, and guess their unit from it. (The graze's landing, row 41, lies
    in the second strip; the strips begin on chunk edges of the whole sum. The
    step's solids drop terms: its sum is the chain over the fluid cells.)"""
    bad, t, total = run_family(name, case, n_strips=3)
    assert bad == 0, f"{bad} cells differ (sum {total!r})"
    assert_path(name, t)


# ---- mode 1: the kinetic energy through statistics() -------------------------------------------------------------


def ke_expected(cp, uc, vc):
    """chain(0.5 (a a + b b)) / fluid cells, from the cell-centre fields."""
    ny, nx = cp.ny, cp.nx
    a, b = uc[1:ny + 1, 1:nx + 1], vc[1:ny + 1, 1:nx + 1]
    J, I = np.meshgrid(np.arange(1, ny + 1), np.arange(1, nx + 1), indexing="ij")
    fluid = (I > cp.step_i) | (J <= cp.inlet_jmax) if cp.case_id == 2 else np.ones(a.shape, dtype=bool)
    assert not np.any(a[~fluid]) and not np.any(b[~fluid])  # uc, vc are zeroed in the solids
    total = SC.chain((0.5 * (a * a + b * b))[fluid])
    return total / float(fluid.sum()), total


def run_ke(case, ny, nx, u_rows, v_rows=None, n_strips=1, label=""):
    cp = C.make_params(case, nx=nx, ny=ny)
    g = SOLVERS[case](cp, ordering="lex", n_strips=n_strips)
    u = np.zeros(g.field_shape("u"))
    u[1:ny + 1, :] = u_rows
    v = np.zeros(g.field_shape("v"))
    if v_rows is not None:
        v[:, 1:nx + 1] = v_rows
    g.set_field("u", u)
    g.set_field("v", v)
    g.reset_timing()
    _, ke = g.statistics()
    t = g.timing()
    uc, vc = g.field("uc"), g.field("vc")
    g.close()
    want, total = ke_expected(cp, uc, vc)
    print(f"seqsum ke {label} {case} {ny}x{nx} strips={n_strips}: chunks {t.seqsum_chunks} plain "
          f"{t.seqsum_serial_chunks} sum {total!r} ke {ke!r} want {want!r}")
    assert t.seqsum_chunks == SC.strip_chunks(ny, nx, n_strips), (t.seqsum_chunks, SC.strip_chunks(ny, nx, n_strips))
    return ke, want, t, uc


@pytest.mark.parametrize("name,case,n_strips", [("ke_halves", "cavity", 1), ("ke_halves", "cavity", 3),
                                                ("ke_halves", "channel", 1), ("ke_mixed", "cavity", 1),
                                                ("ke_mixed", "channel", 3)])
def test_kinetic_energy_half_integer_ties(name, case, n_strips):
    """Terms a^2 / 2 that are exact half-integers, ties while the sum is in
    [2^52, 2^53): all of them going down (ke_halves) or either way (ke_mixed)."""
    a, b, u_rows, v_rows = SC.ke_fields(name)
    ny, nx = a.shape
    ke, want, t, uc = run_ke(case, ny, nx, u_rows, v_rows, n_strips=n_strips, label=name)
    assert np.array_equal(bits(uc[1:ny + 1, 1:nx + 1]), bits(a))  # the kernels summed the family's own terms
    assert bits(want) == bits(SC.chain(SC.terms(name)) / a.size)
    assert bits(ke) == bits(want), (ke, want)
    assert t.seqsum_serial_chunks <= t.seqsum_chunks // 4, (t.seqsum_serial_chunks, t.seqsum_chunks)


@pytest.mark.parametrize("n_strips", [1, 3])
def test_kinetic_energy_backwards_step_random_fields(n_strips):
    """Random signs, magnitudes over many binades, solids (uc, vc zeroed there), a partial last chunk."""
    rng = np.random.default_rng(6)
    ny, nx = 64, 1000
    u_rows = rng.choice([-1.0, 1.0], (ny, nx + 1)) * np.exp(rng.normal(0.0, 4.0, (ny, nx + 1)))
    v_rows = rng.choice([-1.0, 1.0], (ny + 1, nx)) * np.exp(rng.normal(0.0, 4.0, (ny + 1, nx)))
    ke, want, t, _ = run_ke("backwards_step", ny, nx, u_rows, v_rows, n_strips=n_strips, label="random")
    assert bits(ke) == bits(want), (ke, want)


# ---- ranks: the chain handed from rank to rank --------------------------------------------------------------------


def on_ranks(cp, world, body):
    """body(solver, rank) on `world` loopback ranks (host threads sharing the
    GPU, as tests/test_gpu_lex_ranks.py runs them); the ranks' results."""
    L = _lib.lib()
    hub = L.cfd_comm_loopback_hub(world)
    assert hub
    results = [None] * world
    errors = []

    def thread(r):
        try:
            comm = L.cfd_comm_init_loopback(hub, r, 0)
            assert comm, L.cfd_last_error()
            s = C.solver_for(cp, ordering="lex", rank_rows=strip_rows(r, world, cp.ny), comm=comm)
            results[r] = body(s, r)
            s.close()
            L.cfd_comm_destroy(comm)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=thread, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    L.cfd_comm_loopback_hub_destroy(hub)
    assert not errors, errors
    return results


def set_owned_rows(s, name, whole):
    """A rank's rows of the global field `whole` (rank 0 holds ghost row 0, the last rank the top ghost row)."""
    j0, _ = s.owned_rows()
    first = 0 if j0 == 1 else j0
    rows, _ = s.field_shape(name)
    s.set_field(name, whole[first:first + rows])


def rank_chunks(s, nx):
    j0, j1 = s.owned_rows()
    return ((j1 - j0 + 1) * nx + 511) // 512


def test_neg_ties_source_on_three_ranks():
    """neg_ties through the source on 3 ranks: each rank sets its rows, the
    sum goes rank to rank, and the mean-removed source equals one chain's."""
    d = SC.family("neg_ties")
    ny, nx = d.shape
    cp = SC.params("channel", nx, ny)
    us = np.zeros((ny + 2, nx + 1))
    us[1:ny + 1, :] = SC.assert_exact(d)

    def body(s, r):
        set_owned_rows(s, "us", us)
        s.reset_timing()
        s.buildSourceTerm()
        t = s.timing()
        return dict(src=s.field("src"), chunks=t.seqsum_chunks, plain=t.seqsum_serial_chunks, want=rank_chunks(s, nx))

    res = on_ranks(cp, 3, body)
    want, fluid, total = expected_source(None, cp, us, np.zeros((ny + 1, nx + 2)))
    assert bits(total) == bits(SC.chain(SC.terms("neg_ties")))
    got = np.concatenate([r["src"] for r in res], axis=0)[1:ny + 1, 1:nx + 1]
    print("seqsum neg_ties 3 ranks: chunks", [r["chunks"] for r in res], "plain", [r["plain"] for r in res])
    assert [r["chunks"] for r in res] == [r["want"] for r in res]
    assert np.count_nonzero(bits(got) != bits(want)) == 0
    assert sum(r["plain"] for r in res) <= sum(r["chunks"] for r in res) // 4


def test_ke_halves_statistics_on_three_ranks():
    a, _, u_rows, _ = SC.ke_fields("ke_halves")
    ny, nx = a.shape
    cp = C.make_params("cavity", nx=nx, ny=ny)
    u = np.zeros((ny + 2, nx + 1))
    u[1:ny + 1, :] = u_rows

    def body(s, r):
        set_owned_rows(s, "u", u)
        s.reset_timing()
        _, ke = s.statistics()
        t = s.timing()
        return dict(ke=ke, uc=s.field("uc"), chunks=t.seqsum_chunks, plain=t.seqsum_serial_chunks,
                    want=rank_chunks(s, nx))

    res = on_ranks(cp, 3, body)
    uc = np.concatenate([r["uc"] for r in res], axis=0)[1:ny + 1, 1:nx + 1]
    assert np.array_equal(bits(uc), bits(a))
    want = SC.chain(SC.terms("ke_halves")) / a.size
    print("seqsum ke_halves 3 ranks: chunks", [r["chunks"] for r in res], "plain", [r["plain"] for r in res])
    assert [r["chunks"] for r in res] == [r["want"] for r in res]
    for r in res:  # the last rank's total goes back to every rank
        assert bits(r["ke"]) == bits(want), (r["ke"], want)
    assert sum(r["plain"] for r in res) <= sum(r["chunks"] for r in res) // 4


# ---- chunk geometry ----------------------------------------------------------------------------------------------

# (ny, nx, strips, chunks, terms): drift plus noise; "halves" (ties, terms of 2^36..2^38) only at 96 x 2048 and
# larger, below that the sum never reaches a tie
GEOMETRY = [
    (4000, 3, 1, 24, "drift"),    # rows shorter than a lane's 8 terms: a lane's terms span 3 rows
    (4000, 5, 1, 40, "drift"),    # ... 2 or 3 rows
    (4000, 7, 1, 55, "drift"),    # ... 2 rows
    (73, 7, 1, 1, "drift"),       # 511 terms: one chunk, one term short
    # ... as strips of 168, 168, 175 terms, short chunks from a carried start. With terms of -13 * 1024 the third
    # strip's sum runs from 336 * 13312 = 4.47e6 to 511 * 13312 = 6.80e6, inside [2^22, 2^23): the integer path
    (73, 7, 3, 3, "drift13"),
    (171, 3, 1, 2, "drift"),      # 513 terms: one term in the last chunk
    (256, 2, 1, 1, "drift"),      # 512 terms: exactly one chunk
    (64, 512, 1, 64, "drift"),    # exactly one walk scan of 64 chunks
    (64, 513, 1, 65, "drift"),    # one chunk past the scan; 4 k + 1 chunks: a workgroup with one live wave
    (256, 512, 1, 256, "drift"),  # exactly one batch of 256 chunk records
    (256, 513, 1, 257, "drift"),  # one record past the batch (a run of equal-unit chunks across it); 4 k + 1
    (96, 2051, 1, 385, "halves"),  # ties, rows and chunks out of step, a run across the batch, 4 k + 1 chunks
]


@pytest.mark.parametrize("ny,nx,n_strips,chunks,kind", GEOMETRY)
def test_chunk_geometry_edges(ny, nx, n_strips, chunks, kind):
    rng = np.random.default_rng([ny, nx])
    if kind.startswith("drift"):
        d = {"drift": -9.7, "drift13": -13.0}[kind] + rng.normal(0.0, 0.05, (ny, nx))
    else:
        d = rng.integers(2 ** 36, 2 ** 38, (ny, nx)) + 0.5
    cp = SC.params("channel", nx, ny)
    us_rows = SC.assert_exact(d) if kind == "halves" else SC.rows_from_terms(d)
    bad, t, total, _ = run_source(cp, us_rows, n_strips, label=kind)
    assert t.seqsum_chunks == chunks, (t.seqsum_chunks, chunks)
    assert bad == 0, f"{bad} cells differ (sum {total!r})"
    if kind == "drift13":
        assert t.seqsum_serial_chunks <= 2, t.seqsum_serial_chunks
