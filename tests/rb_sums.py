"""The red-black order's tree sums, restated on the host (numpy, no GPU).

In ordering="rb" the open cases remove the source's mean, and every case sums
the kinetic energy, with a tree sum whose order the code fixes:

  * device.hpp wave_sum: an xor butterfly over the 64 lanes, offsets 32, 16,
    .., 1 (lane 0 ends with ((v[l] + v[l^32]) + ..), every lane the same bits);
  * device.hpp block_sum<256>: lane 0 of each wave stores its sum, thread 0
    adds red[0] + red[1] + red[2] + red[3] left to right;
  * kernels.hpp source_kernel / centers_stats_kernel: blocks of 64 columns x 4
    rows (thread t: column t & 63, row t >> 6) from column 0 and the strip's
    first row j0, grid ((nx + 2 + 63) / 64, (j1 - j0 + 1 + 3) / 4) per strip
    (solver.hip grid2d); a thread outside 1 <= i <= nx, 1 <= j <= min(ny, j1)
    or on a solid cell contributes +0.0; the block's sum goes to
    partials[part_off + blockIdx.y * gridDim.x + blockIdx.x], part_off the
    blocks of the strips before (solver.hip);
  * kernels.hpp sum_partials_kernel: one block, thread t adds partials[t],
    partials[t + 256], .. onto 0.0 in order, then block_sum<256>;
  * comm.hip loop_reduce_kernel (ranks, the loopback transport): v = total of
    rank 0, then v = v + total of rank r for r = 1, 2, ... A rank solver has
    one strip of its own rows. (A real RCCL all-reduce over more than two
    devices states no order: the bit claim for three or more ranks is the
    loopback transport's.)

Written from that code; never adjusted to a GPU output. Fed to the oracle
(Oracle.source(total=...), Oracle.step(source_total=...), Oracle.kinetic_energy)
it makes every red-black open-case comparison against ORC_RB a comparison of
bits. tests/test_rb_sums.py keeps it sharp (each deviation from the order above
changes the bits on some shape); tests/test_gpu_rb_sums.py holds the kernels to it.

`order` arguments name deviations of the stated order, for the mutant tests only.
"""
from __future__ import annotations

import numpy as np

OFFSETS = (32, 16, 8, 4, 2, 1)


def strips_of(ny: int, n_strips: int) -> list[tuple[int, int]]:
    """The (j0, j1) rows of cfd_create's strips (solver.hip cfd_create)."""
    return [(1 + ny * k // n_strips, ny * (k + 1) // n_strips) for k in range(n_strips)]


def butterfly(v: np.ndarray, offsets=OFFSETS) -> np.ndarray:
    """wave_sum as written: every lane l takes v[l] + v[l ^ off] for each offset in turn. All 64 lanes."""
    a = np.asarray(v, dtype=np.float64)
    lanes = np.arange(64)
    for off in offsets:
        a = a + a[..., lanes ^ off]
    return a


def wave_sums(v: np.ndarray, offsets=OFFSETS) -> np.ndarray:
    """wave_sum over the last axis (64 lanes), lane 0's value. In the stated order lane 0
    depends on lanes below 2 * off only, so the butterfly folds: a = a[:h] + a[h:2h]."""
    a = np.asarray(v, dtype=np.float64)
    assert a.shape[-1] == 64
    if tuple(offsets) != OFFSETS:
        return butterfly(a, offsets)[..., 0]
    for h in OFFSETS:
        a = a[..., :h] + a[..., h:2 * h]
    return a[..., 0]


def block_sum256(v: np.ndarray, wave_order=(0, 1, 2, 3), offsets=OFFSETS) -> np.ndarray:
    """block_sum<256> of v[..., 4, 64] (wave, lane): thread 0's value."""
    red = wave_sums(v, offsets)
    s = red[..., wave_order[0]]
    for k in wave_order[1:]:
        s = s + red[..., k]
    return s


def partials(values: np.ndarray, strips, *, column_major=False, ghost_row0=False, wave_order=(0, 1, 2, 3),
             offsets=OFFSETS) -> np.ndarray:
    """The partial-sum buffer after source_kernel / centers_stats_kernel.
    values: (ny + 2, nx + 2), the cell's contribution (only rows 1..ny and columns
    1..nx are read; solids already zero). strips: [(j0, j1), ..] as the solver has them."""
    values = np.asarray(values, dtype=np.float64)
    ny, nx = values.shape[0] - 2, values.shape[1] - 2
    gx = (nx + 2 + 63) // 64
    out = []
    for j0, j1 in strips:
        if ghost_row0 and j0 == 1:  # (deviation: the bottom strip's blocks begin at the ghost row and count it)
            j0 = 0
        gy = (j1 - j0 + 1 + 3) // 4
        blk = np.zeros((gy * 4, gx * 64))
        ja, jb = (j0 if ghost_row0 else max(j0, 1)), min(ny, j1)  # contributing rows
        if jb >= ja:
            blk[ja - j0:jb - j0 + 1, 1:nx + 1] = values[ja:jb + 1, 1:nx + 1]
        # (by, wave, bx, lane) -> (by, bx, wave, lane)
        b = blk.reshape(gy, 4, gx, 64).transpose(0, 2, 1, 3)
        s = block_sum256(b, wave_order, offsets)  # (gy, gx)
        out.append((s.T if column_major else s).reshape(-1))
    return np.concatenate(out) if out else np.zeros(0)


def sum_partials(p: np.ndarray, *, stride=256, wave_order=(0, 1, 2, 3), offsets=OFFSETS) -> float:
    """sum_partials_kernel: thread t adds p[t], p[t + 256], .. onto 0.0, then block_sum<256>."""
    p = np.asarray(p, dtype=np.float64)
    rounds = (len(p) + stride - 1) // stride if len(p) else 0
    pad = np.zeros(max(rounds, 1) * stride)
    pad[:len(p)] = p
    s = np.zeros(256)
    for r in range(rounds):  # (absent terms are not added on the GPU; + 0.0 changes no sum begun at +0.0)
        s[:stride] = s[:stride] + pad[r * stride:(r + 1) * stride]
    return float(block_sum256(s.reshape(4, 64), wave_order, offsets))


def allreduce_loopback(totals, *, reverse=False) -> float:
    """loop_reduce_kernel (op sum): ranks added 0, 1, 2, .. in order."""
    t = [float(x) for x in totals]
    if reverse:
        t = t[::-1]
    v = np.float64(t[0])
    for x in t[1:]:
        v = v + np.float64(x)
    return float(v)


def tree_total(values: np.ndarray, strips, ranks=False, **order) -> float:
    """The device total of `values`: strips of one solver (one partial buffer, one
    sum_partials), or with ranks=True one solver per strip, all-reduced."""
    reverse = order.pop("reverse", False)
    stride = order.pop("stride", 256)
    wo = dict(wave_order=order.get("wave_order", (0, 1, 2, 3)), offsets=order.get("offsets", OFFSETS))
    if not ranks:
        return sum_partials(partials(values, strips, **order), stride=stride, **wo)
    return allreduce_loopback([sum_partials(partials(values, [s], **order), stride=stride, **wo) for s in strips],
                              reverse=reverse)


def source_total(raw_f: np.ndarray, mask: np.ndarray, strips, ranks=False, **order) -> float:
    """The total build_source divides by the fluid count: raw_f is f before the mean
    removal ((ny + 2, nx + 2)), mask the oracle's fluid mask (non-zero = fluid)."""
    vals = np.where(np.asarray(mask) != 0, np.asarray(raw_f, dtype=np.float64), 0.0)
    return tree_total(vals, strips, ranks, **order)


def ke_terms(uc: np.ndarray, vc: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """centers_stats_kernel's term 0.5 * (a*a + b*b), each operation rounded; +0.0 on solids."""
    a, b = np.asarray(uc, dtype=np.float64), np.asarray(vc, dtype=np.float64)
    return np.where(np.asarray(mask) != 0, 0.5 * (a * a + b * b), 0.0)


def ke_total(uc: np.ndarray, vc: np.ndarray, mask: np.ndarray, strips, ranks=False, **order) -> float:
    """The kinetic-energy sum of Solver::stats (before the division by the fluid count)."""
    return tree_total(ke_terms(uc, vc, mask), strips, ranks, **order)


def sequential_total(values: np.ndarray, mask: np.ndarray) -> float:
    """The reference's sum: the fluid cells row by row onto 0.0."""
    inner = (slice(1, values.shape[0] - 1), slice(1, values.shape[1] - 1))
    t = 0.0
    for x in np.asarray(values, dtype=np.float64)[inner][np.asarray(mask)[inner] != 0].tolist():
        t += x
    return t


# ---- shapes and inputs shared by tests/test_rb_sums.py and tests/test_gpu_rb_sums.py ----

# (case, nx, ny, strips or ranks, ranks?): the smallest shapes at which the layout can go wrong
SHAPES = [
    ("channel", 62, 5, 1, False),    # nx + 2 = 64: one block column; 5 rows: a block row of one row
    ("channel", 63, 7, 1, False),    # nx + 2 = 65: two block columns, the second one column wide
    ("channel", 200, 300, 1, False),  # 4 x 75 = 300 partials: threads 0..43 add two terms
    ("channel", 96, 25, 3, False),   # strips of 8 + 8 + 9 rows: 2, 2 and 3 block rows, part_off per strip
    ("backwards_step", 64, 16, 1, False),   # solids inside blocks
    ("backwards_step", 448, 8, 1, False),   # step_i = 112: block column 0 solid above the inlet, the edge inside column 1
    ("channel", 96, 48, 2, True), ("channel", 96, 48, 3, True), ("channel", 96, 50, 3, True),
    ("backwards_step", 96, 48, 2, True), ("backwards_step", 96, 48, 3, True), ("backwards_step", 96, 50, 3, True),
]


# (the base seed of this shape gives fields on which the two orders round to the same total)
SEED_BUMP = {("backwards_step", 64, 16, 1, False): 1}


def shape_id(shape) -> str:
    case, nx, ny, n, ranks = shape
    return f"{case}-{nx}x{ny}-{n}{'ranks' if ranks else 'strips'}"


def layout(ny: int, n: int, ranks: bool) -> list[tuple[int, int]]:
    """The strips of a solver of n strips, or the rows of n ranks (cfd_amd.dist.strip_rows)."""
    if not ranks:
        return strips_of(ny, n)
    from cfd_amd.dist import strip_rows
    return [strip_rows(r, n, ny) for r in range(n)]


def shape_seed(shape) -> int:
    """The seed of a shape's adversarial fields (tests/test_rb_sums.py asserts that with it
    the restated totals differ from the sequential ones: a condition on the inputs)."""
    _, nx, ny, n, ranks = shape
    return 100000 * nx + 100 * ny + 10 * n + int(ranks) + SEED_BUMP.get(tuple(shape), 0)


def adversarial(rng, shape, span: float) -> np.ndarray:
    """Mixed signs, magnitudes 2^-span .. 2^span: every re-association of their sum moves its last bits."""
    return rng.choice([-1.0, 1.0], size=shape) * np.exp2(rng.uniform(-span, span, size=shape))


def adversarial_fields(shape) -> dict[str, np.ndarray]:
    """us, vs (magnitudes 2^+-30, so source terms of both signs spanning as much) and u, v in
    the reference's array shapes. The kinetic-energy terms are all positive: spread as wide, a
    few of them would carry the whole sum in any order, so the velocities span 2^+-6 (terms
    2^+-12), where every addition of either order rounds."""
    _, nx, ny, _, _ = shape
    rng = np.random.default_rng(shape_seed(shape))
    return {"us": adversarial(rng, (ny + 2, nx + 1), 30.0), "vs": adversarial(rng, (ny + 1, nx + 2), 30.0),
            "u": adversarial(rng, (ny + 2, nx + 1), 6.0), "v": adversarial(rng, (ny + 1, nx + 2), 6.0)}


# ---- for the tests that feed the oracle ------------------------------------

def source_hook(o, strips, ranks=False):
    """Oracle.source(total=...) / Oracle.step(source_total=...) for a solver with these strips."""
    mask = np.array(o.mask())
    return lambda raw_f: source_total(raw_f, mask, strips, ranks)


def oracle_ke(o, strips, ranks=False) -> float:
    """The average kinetic energy Solver::stats returns, from the oracle's fields
    (after o.stats() or o.centers())."""
    mask = np.array(o.mask())
    return o.kinetic_energy(lambda uc, vc: ke_total(uc, vc, mask, strips, ranks))
