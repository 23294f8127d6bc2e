#!/usr/bin/env python3
"""Generate tests/golden/ref_variants.json from variants of the reference.

oracle/build_ref_variants.sh compiles the reference solvers with other values
of their named constants (grid, block geometry, Reynolds number, run length)
into oracle/_ref/variants/. This script runs each one in
oracle/_ref/runs/variants/<name>/ and extracts DATA only, per variant:

  case          cavity | channel | backwards_step
  constants     the substituted constants, {name: value text}
  header        the Grid:/Time:/Relaxation/Reynolds=/Geometry setup lines and
                the step's "Step location" / "Inlet height" lines
  steps         every Step line (print interval 1)
  warnings      every capped-solve warning line (stderr)
  vtk_sha256    {"0": ..., "<last>": ...} of the first and last frame files
  last_frame    the last frame's step number
  fields        grids of at most 400 cells: the last frame's u_velocity,
                v_velocity and pressure, as the file's 6-decimal text

A variant is kept only if its binary's own "Grid:" line shows the intended
size, so a substitution that silently changed nothing cannot pass. No variant
had to be dropped: every one of them, the 4x2 step included, runs to the end
with exit status 0 and finite output.

Run from the repo root:  python tests/golden/make_ref_variants.py
"""
from __future__ import annotations

import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF_DIR = os.environ.get("CFD_REFERENCE_DIR", "/root/reference")
BUILD = os.path.join(ROOT, "oracle", "build_ref_variants.sh")
BIN = os.path.join(ROOT, "oracle", "_ref", "variants")
RUNS = os.path.join(ROOT, "oracle", "_ref", "runs", "variants")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_variants.json")

VTK_BASE = {"cavity": "cavity_flow", "channel": "channel_flow", "backwards_step": "backwards_step"}
FIELDS = ("u_velocity", "v_velocity", "pressure")
FIELD_CELLS = 400
ANSI = re.compile(r"\x1b\[[0-9;]*m")
HEADER = ("Grid:", "Time:", "Relaxation", "Reynolds=", "Geometry setup", "  Step location", "  Inlet height")


def table() -> list[tuple[str, str, dict[str, str]]]:
    rows = []
    for line in subprocess.check_output([BUILD, "--list"], text=True).splitlines():
        name, case, subs = line.split("|")
        rows.append((name, case, dict(kv.split("=", 1) for kv in subs.split())))
    return rows


def grid_of(case: str, constants: dict[str, str]) -> tuple[int, int]:
    if case == "cavity":
        return int(constants["n_interior"]), int(constants["n_interior"])
    return int(constants["NX_INT"]), int(constants["NY_INT"])


def vtk_text_fields(path: str, nx: int, ny: int) -> dict[str, list[str]]:
    with open(path) as f:
        lines = f.read().split("\n")
    assert f"DIMENSIONS {nx} {ny} 1" in lines, path
    out = {}
    for k, line in enumerate(lines):
        parts = line.split()
        if len(parts) >= 2 and parts[0] == "SCALARS" and parts[1] in FIELDS:
            out[parts[1]] = lines[k + 2: k + 2 + nx * ny]
    assert sorted(out) == sorted(FIELDS), path
    return out


def run_variant(name: str, case: str, constants: dict[str, str]) -> dict:
    wd = os.path.join(RUNS, name)
    shutil.rmtree(wd, ignore_errors=True)
    os.makedirs(wd)
    r = subprocess.run([os.path.join(BIN, name)], cwd=wd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-400:])
    out = [ANSI.sub("", l) for l in r.stdout.splitlines()]
    err = [ANSI.sub("", l) for l in r.stderr.splitlines()]
    nx, ny = grid_of(case, constants)
    grid = [l for l in out if l.startswith("Grid:")]
    assert len(grid) == 1 and grid[0].startswith(f"Grid: {nx}x{ny} "), (name, grid)
    steps = [l for l in out if l.startswith("Step ")]
    total = int(steps[-1].split()[1].split("/")[1])
    assert len(steps) == total > 0, (name, len(steps), total)
    assert "nan" not in r.stdout.lower() and "inf" not in "".join(steps).lower(), name
    rec = {
        "case": case,
        "constants": constants,
        "header": [l for l in out if l.startswith(HEADER)],
        "steps": steps,
        "warnings": [l for l in err if "Warning" in l],
        "last_frame": total,
        "vtk_sha256": {},
    }
    for fr in (0, total):
        path = os.path.join(wd, "vtk_output", f"{VTK_BASE[case]}_{fr:06d}.vtk")
        with open(path, "rb") as fh:
            rec["vtk_sha256"][str(fr)] = hashlib.sha256(fh.read()).hexdigest()
    if nx * ny <= FIELD_CELLS:
        rec["fields"] = vtk_text_fields(path, nx, ny)
    return rec


def main() -> int:
    if not os.path.isdir(REF_DIR):
        print(f"reference tree {REF_DIR} absent; the fixture is committed, nothing to do")
        return 0
    subprocess.check_call([BUILD, REF_DIR])
    golden = {name: run_variant(name, case, constants) for name, case, constants in table()}
    with open(OUT, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(golden)} variants, {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
