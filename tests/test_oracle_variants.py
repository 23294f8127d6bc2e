"""Pin the CPU oracle, and the parameter derivation of params.py, to the
reference at grids and geometries other than its three compiled-in ones.

tests/golden/ref_variants.json holds runs of reference binaries built with
other values of their named constants (oracle/build_ref_variants.sh,
tests/golden/make_ref_variants.py): tiny grids down to 2x2, nx < ny, both dt
limits, a block geometry whose truncations (int)(step_x/dx) and
(int)(h_inlet/dy) are not exact, and the degenerate blocks step_i = 1 and
inlet_jmax = ny-1. For every variant the oracle in the reference's order must
reproduce the header values (dt, steps, omega, nu, fluid-cell count, step_i,
inlet_jmax), every Step line and capped-solve warning string for string, the
stored fields at the file's 6 decimals, and - through the product's VTK
writer - both frame files byte for byte.

test_gpu_shapes.py holds the GPU engines to the same fixture and imports
VARIANTS / params_of / expected_header from here.
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import cfd_amd as C
from cfd_amd.logfmt import step_line, warning_line
import oracle as O

VARIANTS = json.load(open(os.path.join(GOLDEN, "ref_variants.json")))

# reference constant -> CaseParams field(s)
CONSTANT_FIELDS = {
    "n_interior": ("nx", "ny"), "NX_INT": ("nx",), "NY_INT": ("ny",),
    "reynolds_number": ("re",), "REYNOLDS_NUMBER": ("re",),
    "final_time": ("final_time",),
    "print_interval": ("print_interval",), "PRINT_INTERVAL": ("print_interval",),
    "save_data_interval": ("save_interval",), "SAVE_DATA_INTERVAL": ("save_interval",),
    "STEP_LOCATION": ("step_x",), "HEIGHT_INLET": ("h_inlet",),
}


def params_of(name: str) -> C.CaseParams:
    """The reference defaults of the variant's case with its substituted
    constants applied; everything else is derived by params.py."""
    v = VARIANTS[name]
    cp = C.reference_defaults(v["case"])
    for const, text in v["constants"].items():
        for field in CONSTANT_FIELDS[const]:
            setattr(cp, field, type(getattr(cp, field))(float(text)))
    return cp


def expected_header(cp: C.CaseParams, fluid_count: int) -> list[str]:
    """The header lines the fixture keeps, formatted from cp as the reference
    prints them (the geometry lines come before its stream turns fixed)."""
    lines = []
    if cp.case_id == C.params.BACKSTEP:
        lines += [f"  Step location: x = {cp.step_x:g} (i = {cp.step_i})",
                  f"  Inlet height: {cp.h_inlet:g} (j = 1 to {cp.inlet_jmax})",
                  f"Geometry setup complete. Fluid cells: {fluid_count}/{cp.nx * cp.ny}"]
    if cp.case_id == C.params.CAVITY:
        lines.append(f"Grid: {cp.nx}x{cp.ny} (spacing={cp.dx:.6f})")
    else:
        lines.append(f"Grid: {cp.nx}x{cp.ny} (dx={cp.dx:.6f}, dy={cp.dy:.6f})")
    lines += [f"Time: dt={cp.dt:.6f}, steps={cp.total_steps}, final_time={cp.final_time:.6f}",
              f"Reynolds={cp.re:.6f}, kinematic viscosity={cp.nu:.6f}, CFL={cp.cfl:.6f}",
              f"Relaxation factor={cp.omega:.6f}"]
    return lines


def fmt6(a):
    return ["%.6f" % x for x in np.asarray(a).ravel()]


def fresh_oracle(cp, ordering=O.LEX):
    o = O.Oracle(cp, ordering=ordering)
    o.velocity_bc(False)  # cavity run() / the open cases' constructors, before frame 0
    return o


def test_variant_set_covers_the_named_rules():
    """The set this file pins: the rules each variant is there for."""
    p = {n: params_of(n) for n in VARIANTS}
    assert {(c.nx, c.ny) for c in p.values() if c.case_id == 0} >= {(2, 2), (3, 3), (20, 20)}
    diffusive = [c for c in p.values() if c.case_id == 0 and 0.25 * c.dx * c.dx / c.nu < c.dx / c.u_ref]
    convective = [c for c in p.values() if c.case_id == 0 and 0.25 * c.dx * c.dx / c.nu > c.dx / c.u_ref]
    assert diffusive and convective
    assert {(c.nx, c.ny) for c in p.values() if c.case_id == 1} >= {(2, 2), (3, 2), (2, 7), (13, 5), (17, 40), (50, 17)}
    steps = {(c.nx, c.ny): c for c in p.values() if c.case_id == 2}
    assert set(steps) >= {(4, 2), (5, 3), (9, 2), (12, 6), (60, 12), (100, 20), (448, 8), (64, 32), (40, 10)}
    assert (steps[4, 2].step_i, steps[4, 2].inlet_jmax) == (1, 1)
    assert steps[64, 32].step_i == 1 and steps[40, 10].inlet_jmax == 9
    assert steps[448, 8].step_i == 112
    # dx = 8/12 and 8/60 are rounded; the reference's i = 3 and 15 hold only if step_x/dx rounds up to them
    assert (steps[12, 6].step_i, steps[60, 12].step_i) == (3, 15)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_header_values(name):
    """dt (both limits), steps (the truncation of final_time/dt), omega (also for
    nx != ny), nu, the fluid-cell count, step_i and inlet_jmax, as the variant
    binary printed them."""
    cp = params_of(name)
    assert expected_header(cp, O.Oracle(cp).fluid_count()) == VARIANTS[name]["header"]
    assert cp.total_steps == VARIANTS[name]["last_frame"] == len(VARIANTS[name]["steps"])


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_oracle_reproduces_variant_run(name, tmp_path):
    ref = VARIANTS[name]
    cp = params_of(name)
    o = fresh_oracle(cp)
    o.centers()
    f0 = tmp_path / "f0.vtk"
    C.write_vtk_arrays(cp, str(f0), 0.0, o.field("uc"), o.field("vc"), o.field("p"))
    assert hashlib.sha256(f0.read_bytes()).hexdigest() == ref["vtk_sha256"]["0"]

    lines, warns = [], []
    for k in range(1, cp.total_steps + 1):
        it, res = o.step()
        if it >= cp.max_iters:
            warns.append(warning_line(cp.case_id, cp.max_iters, res))
        if k % cp.print_interval == 0 or k == cp.total_steps:
            md, ke = o.stats()
            lines.append(step_line(cp.case_id, k, cp.total_steps, k * cp.dt, md, ke, it, res))
    assert lines == ref["steps"]
    assert warns == ref["warnings"]

    o.centers()
    if "fields" in ref:
        inner = (slice(1, cp.ny + 1), slice(1, cp.nx + 1))
        fluid = o.mask()[inner] > 0
        for mine, key in (("uc", "u_velocity"), ("vc", "v_velocity"), ("p", "pressure")):
            a = o.field(mine)[inner]
            if cp.case_id == C.params.BACKSTEP:
                a = np.where(fluid, a, 0.0)  # the reference writes 0 in the block
            assert fmt6(a) == ref["fields"][key], (name, key)
    fl = tmp_path / "last.vtk"
    C.write_vtk_arrays(cp, str(fl), cp.total_steps * cp.dt, o.field("uc"), o.field("vc"), o.field("p"))
    assert hashlib.sha256(fl.read_bytes()).hexdigest() == ref["vtk_sha256"][str(ref["last_frame"])]
