"""GPU parity: libcfd_amd.so (HIP kernels) against the CPU oracle.

Bars:
  * stencil phases (BCs, predictor, source, corrector): bit-exact;
  * SOR solve: bit-exact against the oracle's red-black restatement (same
    iteration count, same field); against the reference's lexicographic
    ordering the converged fields agree to the solver tolerance;
  * whole runs: centerline u/v within 1e-6 relative L2 of the reference
    algorithm (north_star), bit-exact against the red-black oracle (the open
    cases' source mean and the kinetic energy are tree sums on the GPU: the
    oracle takes them restated for the solver's strips, tests/rb_sums.py);
  * strip decomposition: the cavity identical to one domain; the open cases'
    mean-removal sum depends on the strips, so each layout is held to the
    oracle with its own restated total, bit for bit.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

import cfd_amd as C  # noqa: E402
import oracle as O  # noqa: E402
import rb_sums as R  # noqa: E402

CASES = ["cavity", "channel", "backwards_step"]


def small_params(case: str, **kw):
    if case == "cavity":
        return C.make_params(case, **kw)
    if case == "channel":
        return C.make_params(case, **kw)
    return C.make_params(case, **kw)


def ofield(o, name, cp):
    """Oracle field cut to the reference shape of `name`."""
    a = o.field(name)
    if name in ("u", "us"):
        return a[:, : cp.nx + 1]
    if name in ("v", "vs"):
        return a[: cp.ny + 1, :]
    return a


def set_both(g, o, name, value, cp):
    g.set_field(name, value)
    ofield(o, name, cp)[...] = value


def assert_bits(a, b, what):
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, what
    bad = np.argwhere(a.view(np.int64) != b.view(np.int64))
    if bad.size:
        j, i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} cells differ, first at (j={j}, i={i}): gpu={a[j, i]!r} "
                             f"oracle={b[j, i]!r}")


def centerlines(u_c, v_c, cp):
    """u along the vertical centreline, v along the horizontal one (cell centres)."""
    ic = (cp.nx + 1) // 2
    jc = (cp.ny + 1) // 2
    return u_c[1:cp.ny + 1, ic], v_c[jc, 1:cp.nx + 1]


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def stencil_phases(cp, ordering, strips, tuning=None, seed=1234):
    """Every stencil phase once on random fields, GPU against the oracle, bit for bit.
    The two sums the red-black order re-associates (the open cases' source mean,
    the kinetic energy: tree sums there, the reference's sequential loop in the
    reference order) are held to the oracle's sequential sums in the reference order
    and to the tree sums restated for these strips (tests/rb_sums.py) in red-black."""
    case = C.CASE_NAMES[cp.case_id]
    closed = case in ("cavity", "rayleigh_benard")
    g = C.solver_for(cp, ordering=ordering, n_strips=strips, tuning=tuning)
    o = O.Oracle(cp)
    rng = np.random.default_rng(seed)
    nx, ny = cp.nx, cp.ny
    set_both(g, o, "u", rng.standard_normal((ny + 2, nx + 1)), cp)
    set_both(g, o, "v", rng.standard_normal((ny + 1, nx + 2)), cp)

    g.applyBoundaryConditions()
    o.velocity_bc(False)
    assert_bits(g.field("u"), ofield(o, "u", cp), "BC u")
    assert_bits(g.field("v"), ofield(o, "v", cp), "BC v")

    g.computeTentativeVelocities()
    o.tentative()
    assert_bits(g.field("us"), ofield(o, "us", cp), "tentative u*")
    assert_bits(g.field("vs"), ofield(o, "vs", cp), "tentative v*")

    if case == "rayleigh_benard":  # bc_temperature_kernel + thermal_kernel (buoyancy into v*, T advanced)
        set_both(g, o, "t", rng.standard_normal((ny + 2, nx + 2)), cp)
        g.advanceTemperature()
        o.temperature_bc()
        o.thermal()
        assert_bits(g.field("vs"), ofield(o, "vs", cp), "v* with buoyancy")
        assert_bits(g.field("t")[1:-1, 1:-1], o.field("t")[1:-1, 1:-1], "T after one update")

    if not closed:
        g.applyTentativeBoundaryConditions()
        o.velocity_bc(True)
        assert_bits(g.field("us"), ofield(o, "us", cp), "BC u*")
        assert_bits(g.field("vs"), ofield(o, "vs", cp), "BC v*")

    layout = R.strips_of(ny, strips)
    g.buildSourceTerm()
    o.source(total=None if ordering == "lex" else R.source_hook(o, layout))  # (red-black: the tree sum, restated)
    assert_bits(g.field("src")[1:-1, 1:-1], o.field("src")[1:-1, 1:-1], "source")
    if case != "rayleigh_benard":
        assert_bits(g.field("src"), o.field("src"), "source")

    pr = rng.standard_normal((ny + 2, nx + 2))
    set_both(g, o, "p", pr, cp)
    set_both(g, o, "us", rng.standard_normal((ny + 2, nx + 1)), cp)
    set_both(g, o, "vs", rng.standard_normal((ny + 1, nx + 2)), cp)
    g.applyPressureCorrection()
    o.correct()
    assert_bits(g.field("u"), ofield(o, "u", cp), "corrected u")
    assert_bits(g.field("v"), ofield(o, "v", cp), "corrected v")

    md, ke = g.statistics()
    omd, oke = o.stats()
    assert md == omd
    assert ke == (oke if ordering == "lex" else R.oracle_ke(o, layout))
    assert_bits(g.field("uc"), o.field("uc"), "u_center")
    assert_bits(g.field("vc"), o.field("vc"), "v_center")
    g.close()


@pytest.mark.parametrize("strips", [1, 3])
@pytest.mark.parametrize("case", CASES)
def test_stencil_phases_bitexact(case, strips):
    stencil_phases(small_params(case), "rb", strips)


# Shapes at the launch-geometry edges of the stencil kernels (solver.hip):
#  * the predictor's column tiles of 112 (ct = nx/112 + 1): nx = 111, 112, 113, 223, 224, 225;
#  * its row bands (tent_th rows; the knob set to 5 keeps the grids small): ny = 9, 10, 11;
#  * the 64-column x 4-row blocks of grid2d and the cavity's 128-column pair_grid passes:
#    nx = 62, 63, 64, 127, 128, 129, and 3, 4, 5 rows;
#  * the row pitch (nx + 3 rounded up to 16): nx = 13 (pitch nx + 3 exactly), 14, 29;
#  * two and three strips of 8 rows, and 8 + 9;
#  * the tiny grids of test_gpu_shapes.py.
# (nx, ny, tent_th or 0)
EDGE_SHAPES = [(111, 9, 0), (112, 9, 0), (113, 9, 0), (223, 9, 0), (224, 9, 0), (225, 9, 0),
               (13, 9, 5), (14, 10, 5), (29, 11, 5), (113, 11, 5),
               (62, 3, 0), (63, 4, 0), (64, 5, 0), (127, 5, 0), (128, 3, 0), (129, 4, 0),
               (64, 16, 0), (129, 17, 5), (113, 24, 5)]
TINY_SHAPES = {"cavity": [(2, 2), (2, 5), (5, 2), (3, 3), (7, 4), (13, 9)],
               "channel": [(2, 2), (3, 2), (2, 7), (6, 3), (13, 5)],
               "backwards_step": [(4, 2), (4, 4), (8, 4), (5, 3), (9, 2), (16, 4)],
               "rayleigh_benard": [(2, 2), (4, 2), (5, 3)]}
# the step's block column on the predictor's tile edge (step_i = nx/4 = 111, 112, 113)
STEP_EDGE = [(444, 8, 0), (448, 8, 0), (452, 8, 0), (444, 16, 5)]


def edge_cases():
    out = []
    for case in CASES + ["rayleigh_benard"]:
        shapes = EDGE_SHAPES + [(nx, ny, 0) for nx, ny in TINY_SHAPES[case]]
        if case == "backwards_step":
            shapes = shapes + STEP_EDGE
        out += [(case, nx, ny, th) for nx, ny, th in shapes]
    return out


def edge_params(case, nx, ny):
    if case == "rayleigh_benard":
        return C.make_params(case, nx=nx, ny=ny, ra=2e4)
    return C.make_params(case, nx=nx, ny=ny)


@pytest.mark.parametrize("ordering", ["rb", "lex"])
@pytest.mark.parametrize("case,nx,ny,tent_th", edge_cases(), ids=lambda v: str(v))
def test_stencil_phases_at_launch_edges(case, nx, ny, tent_th, ordering):
    """test_stencil_phases_bitexact's body at the shapes above, in both orders,
    on one strip and on the most strips the rows allow (8 each), up to 3."""
    cp = edge_params(case, nx, ny)
    tuning = {"tent_th": tent_th} if tent_th else None
    for strips in sorted({1, max(1, min(3, ny // 8))}):
        stencil_phases(cp, ordering, strips, tuning, seed=1000 * nx + ny)


@pytest.mark.parametrize("ordering", ["rb", "lex"])
@pytest.mark.parametrize("step_x,h_inlet", [(0.2, 1.0), (2.0, 1.9)])
def test_stencil_phases_degenerate_blocks(step_x, h_inlet, ordering):
    """The step's block one cell wide (64x32, step_i = 1) and one cell high
    (40x10, inlet_jmax = ny-1 = 9), as the reference variants have them."""
    nx, ny = (64, 32) if step_x == 0.2 else (40, 10)
    cp = C.make_params("backwards_step", nx=nx, ny=ny)
    cp.step_x, cp.h_inlet = step_x, h_inlet
    assert (cp.step_i == 1) != (cp.inlet_jmax == ny - 1)
    stencil_phases(cp, ordering, 1)
    if ordering == "rb":  # (the reference order keeps such a block on one strip)
        stencil_phases(cp, ordering, min(3, ny // 8))


@pytest.mark.parametrize("ordering", ["rb", "lex"])
@pytest.mark.parametrize("case,nx,ny", [("cavity", 2, 2), ("cavity", 129, 5), ("channel", 2, 7), ("channel", 113, 9),
                                        ("backwards_step", 4, 2), ("backwards_step", 448, 8)])
def test_source_maximum_sets_the_tolerance(case, nx, ny, ordering):
    """srcmax_kernel on its own: a source set from the host, then one capped
    solve. The tolerance comes from max|f| over the interior, so the iteration
    count and the residual equal the oracle's with the same source."""
    cp = C.make_params(case, nx=nx, ny=ny, max_iters=200)
    cp.tol_factor = 1e-3
    g = C.solver_for(cp, ordering=ordering)
    o = O.Oracle(cp, ordering=O.LEX if ordering == "lex" else O.RB)
    rng = np.random.default_rng(nx * 100 + ny)
    f = np.zeros((ny + 2, nx + 2))
    f[1:ny + 1, 1:nx + 1] = rng.standard_normal((ny, nx)) * (0.05 if case == "cavity" else 10.0)
    f[o.mask() == 0] = 0.0
    # the largest value in the last interior cell: a maximum that skips it changes the stop
    f[ny, nx] = 3.0 * np.abs(f).max()
    set_both(g, o, "src", f, cp)
    assert g.solverPressurePoisson() == o.poisson()
    assert_bits(g.field("p"), o.field("p"), "pressure")
    g.close()


@pytest.mark.parametrize("strips", [1, 2])
@pytest.mark.parametrize("case", CASES)
def test_poisson_rb_bitexact(case, strips):
    """The fused red-black kernel == the oracle's red-black restatement, bit for bit."""
    cp = small_params(case, max_iters=3000)
    g = C.solver_for(cp, ordering="rb", n_strips=strips)
    o = O.Oracle(cp, ordering=O.RB)
    rng = np.random.default_rng(7)
    nx, ny = cp.nx, cp.ny
    f = np.zeros((ny + 2, nx + 2))
    f[1:ny + 1, 1:nx + 1] = rng.standard_normal((ny, nx)) * 10.0
    if case == "backwards_step":
        f[o.mask() == 0] = 0.0
    f[1:ny + 1, 1:nx + 1] -= f[1:ny + 1, 1:nx + 1].mean() if case == "channel" else 0.0
    set_both(g, o, "src", f, cp)
    if case != "cavity":
        set_both(g, o, "p", rng.standard_normal((ny + 2, nx + 2)) * 0.1, cp)
    it_g, res_g = g.solverPressurePoisson()
    it_o, res_o = o.poisson()
    assert it_g == it_o
    assert res_g == res_o
    assert_bits(g.field("p"), o.field("p"), "pressure")


@pytest.mark.parametrize("case", ["cavity", "channel"])
def test_poisson_converges_to_reference_solution(case):
    """Red-black vs the reference's lexicographic SOR: same fixed point to tolerance
    (cases whose reference solve converges; see test_oracle_golden for the step)."""
    cp = small_params(case, max_iters=10000)
    g = C.solver_for(cp, ordering="rb")
    o = O.Oracle(cp, ordering=O.LEX)
    if case != "cavity":
        g.applyBoundaryConditions()
    # a realistic source: one predictor step from the initial state
    for s in (g,):
        if case == "cavity":
            s.applyBoundaryConditions()
        s.computeTentativeVelocities()
        if case != "cavity":
            s.applyTentativeBoundaryConditions()
        s.buildSourceTerm()
    o.velocity_bc(False)  # cavity: step's BC; open cases: the constructor's BC
    o.tentative()
    if case != "cavity":
        o.velocity_bc(True)
    o.source()
    it_g, res_g = g.solverPressurePoisson()
    it_o, res_o = o.poisson()
    pg, po = g.field("p"), o.field("p")
    inner = (slice(1, cp.ny + 1), slice(1, cp.nx + 1))
    scale = np.abs(po[inner]).max()
    assert np.abs(pg[inner] - po[inner]).max() <= 1e-6 * scale, (it_g, it_o)


@pytest.mark.parametrize("case,steps", [("cavity", 60), ("channel", 40)])
def test_run_matches_reference_algorithm(case, steps):
    """North-star bar: centerline u/v within 1e-6 rel-L2 of the reference algorithm.

    Norm: ||gpu - ref|| / ||u_ref|| on each centerline, i.e. relative to the
    centerline velocity scale (the channel's horizontal-centerline v is ~0 by
    symmetry, so normalising by ||v_ref|| would measure round-off)."""
    cp = small_params(case)
    g = C.solver_for(cp, ordering="rb")
    olex = O.Oracle(cp, ordering=O.LEX)
    orb = O.Oracle(cp, ordering=O.RB)
    if case != "cavity":
        olex.velocity_bc(False)
        orb.velocity_bc(False)
    hook = None if case == "cavity" else R.source_hook(orb, R.strips_of(cp.ny, 1))
    for _ in range(steps):
        olex.step()
        assert g.step() == orb.step(source_total=hook)
    g.statistics()
    olex.centers()
    orb.centers()
    ug, vg = centerlines(g.field("uc"), g.field("vc"), cp)
    ul, vl = centerlines(olex.field("uc"), olex.field("vc"), cp)
    scale = np.linalg.norm(ul)
    assert np.linalg.norm(ug - ul) / scale <= 1e-6
    assert np.linalg.norm(vg - vl) / max(scale, np.linalg.norm(vl)) <= 1e-6
    for name in ("u", "v", "p", "src"):
        assert_bits(g.field(name), ofield(orb, name, cp), f"{case} run {name} vs red-black oracle")


def run_vs_red_black_oracle(cp, steps, n_strips=1):
    """Whole steps of an open case against the red-black oracle whose source mean is the
    tree sum restated for this strip layout: (iterations, residual) of every step, then
    u, v, p, src and the kinetic energy, bit for bit."""
    g = C.solver_for(cp, ordering="rb", n_strips=n_strips)
    orb = O.Oracle(cp, ordering=O.RB)
    orb.velocity_bc(False)
    layout = R.strips_of(cp.ny, n_strips)
    hook = R.source_hook(orb, layout)
    for k in range(steps):
        assert g.step() == orb.step(source_total=hook), (k, n_strips)
    for name in ("u", "v", "p", "src"):
        assert_bits(g.field(name), ofield(orb, name, cp), f"{n_strips} strips, {name} vs red-black oracle")
    md, ke = g.statistics()
    omd, _ = orb.stats()
    assert (md, ke) == (omd, R.oracle_ke(orb, layout))
    g.close()


def test_backstep_run_matches_red_black_oracle():
    """The step's reference solve never converges, so the red-black path is held
    to its own CPU restatement (same ordering, the source mean's tree sum
    restated): residuals, iteration counts and fields, bit for bit."""
    run_vs_red_black_oracle(small_params("backwards_step"), 3)


def test_channel_run_matches_red_black_oracle_at_reference_default():
    """40 steps of the reference's own channel (its default grid), bit for bit."""
    run_vs_red_black_oracle(C.reference_defaults("channel"), 40)


@pytest.mark.parametrize("case", CASES)
def test_strips_equal_single_domain(case):
    """The cavity: strips equal one domain, bit for bit. The open cases' source mean is a
    tree sum over the strips' blocks, so the two layouts differ in the last bits: each is
    held to the oracle with its own layout's restated total, bit for bit."""
    cp = small_params(case)
    steps = 3 if case == "backwards_step" else 20
    n = min(4, cp.ny // 8)  # each strip owns >= HALO (8) rows
    assert n > 1
    if case != "cavity":
        run_vs_red_black_oracle(cp, steps, 1)
        run_vs_red_black_oracle(cp, steps, n)
        return
    a = C.solver_for(cp, ordering="rb", n_strips=1)
    b = C.solver_for(cp, ordering="rb", n_strips=n)
    for _ in range(steps):
        assert a.step() == b.step()
    for name in ("u", "v", "p"):
        assert_bits(b.field(name), a.field(name), f"strips {name}")


def test_cavity_final_frame_matches_reference_output():
    """Full reference run (63^2, Re 1000, 2520 steps) against its own VTK output."""
    cp = C.reference_defaults("cavity")
    g = C.CavitySolver(cp, ordering="rb")
    g.applyBoundaryConditions()
    g.run_steps(cp.total_steps)
    g.statistics()
    F = np.load(os.path.join(GOLDEN, "ref_fields.npz"))
    inner = (slice(1, cp.ny + 1), slice(1, cp.nx + 1))
    for name, key in (("uc", "u_velocity"), ("vc", "v_velocity"), ("p", "pressure")):
        ref = F[f"cavity/{cp.total_steps}/{key}"]
        mine = g.field(name)[inner]
        # reference prints 6 decimals (|rounding| <= 5e-7) + converged-SOR ordering difference
        assert np.abs(mine - ref).max() <= 2e-6, (name, np.abs(mine - ref).max())
    ug, vg = centerlines(g.field("uc"), g.field("vc"), cp)
    uref = F[f"cavity/{cp.total_steps}/u_velocity"][:, (cp.nx + 1) // 2 - 1]
    vref = F[f"cavity/{cp.total_steps}/v_velocity"][(cp.ny + 1) // 2 - 1, :]
    assert rel_l2(ug, uref) <= 5e-6
    assert rel_l2(vg, vref) <= 5e-6


def test_log_lines_match_reference_format():
    """run() prints the reference's log lines; iteration counts differ only by ordering."""
    import io
    cp = C.reference_defaults("channel")
    g = C.ChannelSolver(cp, ordering="rb")
    out, err = io.StringIO(), io.StringIO()
    g.run(output_directory=None, out=out, err=err, steps=200)
    lines = out.getvalue().splitlines()
    logs = json.load(open(os.path.join(GOLDEN, "ref_logs.json")))["channel"]["steps"][:2]
    assert len(lines) == 2
    for a, b in zip(lines, logs):
        # same fields, same formatting; avg_KE agrees to within one unit of the
        # 6th printed decimal (red-black vs lexicographic SOR, tolerance 1e-7)
        fa, fb = a.split("|"), b.split("|")
        assert len(fa) == len(fb) and fa[0] == fb[0] and fa[1] == fb[1]
        ka, kb = float(fa[3].split("=")[1]), float(fb[3].split("=")[1])
        assert abs(ka - kb) <= 1.5e-6


@pytest.mark.parametrize("strips", [1, 2])
@pytest.mark.parametrize("nx", [111, 112, 113, 126, 127, 128, 129, 224, 254, 255, 256, 300])
def test_cavity_column_tile_widths(nx, strips):
    """The cavity's column-tiled passes (tentative_kernel: 128-column tiles
    whose outer neighbours come from extra edge loads;
    cavity_source_kernel + max|f|: 128-column pairs) at widths on and next to
    a tile edge, bit-exact vs the oracle. ny = 190 keeps the grid off the
    one-workgroup path; a capped solve in each ordering checks the tolerance
    (from max|f|) and the reported residual."""
    ny = 190
    for ordering, oo in (("rb", O.RB), ("lex", O.LEX)):
        cp = C.make_params("cavity", re=100.0, nx=nx, ny=ny, dt=1e-3, max_iters=40)
        g = C.solver_for(cp, n_strips=strips, ordering=ordering)
        o = O.Oracle(cp, ordering=oo)
        rng = np.random.default_rng(nx * 10 + strips)
        set_both(g, o, "u", rng.standard_normal((ny + 2, nx + 1)), cp)
        set_both(g, o, "v", rng.standard_normal((ny + 1, nx + 2)), cp)
        g.applyBoundaryConditions()
        o.velocity_bc(False)
        g.computeTentativeVelocities()
        o.tentative()
        assert_bits(g.field("us"), ofield(o, "us", cp), "tentative u*")
        assert_bits(g.field("vs"), ofield(o, "vs", cp), "tentative v*")
        g.buildSourceTerm()
        o.source()
        assert_bits(g.field("src"), o.field("src"), "source")
        it_g, res_g = g.solverPressurePoisson()
        it_o, res_o = o.poisson()
        assert (it_g, res_g) == (it_o, res_o), ordering
        assert_bits(g.field("p"), o.field("p"), f"pressure ({ordering})")
        g.close()
