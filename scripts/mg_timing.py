#!/usr/bin/env python3
"""Timing of the multigrid pressure solve beside the default (SOR) solve.

For each grid (--case cavity, channel or step, Re = 1000 unless --re; the step: 400,
BASELINE configs[3]) in one process on one device (the channel: --method
multigrid-open, the step: multigrid-step, their defaults):
  * the default solve (the reference's SOR, which stops at its 10000-sweep cap
    at these sizes): HIP-event ms per solve, sweeps, final residual, tolerance;
  * the multigrid solve V(2,2): ms per solve, cycles, launches, ms per cycle
    split into the level-0 launches (cfd_mg_info.fine_ms) and the rest;
  * the rate of the level-0 launches from the bytes they have to move (24 B per
    cell and smoothing pass: p read, f read, p written; 16 each for the
    restriction and the prolongation) as a fraction of the HBM peak (a grid
    that fits the 256 MiB Infinity Cache, such as 1024^2, can exceed it);
  * V(2,2) with the smoothing as one launch per colour (CFD_MG_FUSED=0), where
    every sweep moves its 24 B per cell;
Every time is device time from HIP events as cfd_timing / cfd_mg_info report
it, over `--steps` whole timesteps after `--warmup` untimed ones. Writes one
JSON file per grid under --out.

  python scripts/mg_timing.py --sizes 1024x1024 4096x4096 992x992 --out profiles/mg --commit <hash>
  python scripts/mg_timing.py --case channel --sizes 4096x512 1024x128 --out profiles/mg --commit <hash>
  python scripts/mg_timing.py --case step --sizes 256x32 1024x128 8192x512 --out profiles/mg --commit <hash>
  python scripts/mg_timing.py --method multigrid-any --sizes 1000x1000 4095x4095 --out profiles/mg --commit <hash>

  python scripts/mg_timing.py --case channel --method multigrid-open-any --sizes 4000x500 4095x511 4096x512 --out profiles/mg --commit <hash>

--method multigrid-any (the cavity at any grid size) writes mg_timing_cavity_any_<size>.json,
--method multigrid-open-any (the channel at any grid size) mg_timing_channel_open_any_<size>.json.

The channel's and the step's run fails (exit 1) if a multigrid solve ends above its tolerance.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "computational-fluid-dynamics_amd"))

import numpy as np  # noqa: E402

import cfd_amd as C  # noqa: E402

HBM_PEAK = 8.0e12       # B/s, MI355X specification
# What the level-0 launches of one V(2,2) cycle have to move per level-0 cell: a smoothing pass reads p and f and
# writes p (24 B) - once per smoothing step when its sweeps are fused, once per sweep otherwise; the restriction
# reads p and f (16 B), the prolongation reads and writes p (16 B); coarse-level traffic (a quarter) left out.
FUSED_BYTES_PER_CELL = 2 * 24.0 + 16.0 + 16.0
COLOUR_BYTES_PER_CELL = 4 * 24.0 + 16.0 + 16.0


def level0_rate(fine_ms_per_cycle, bytes_per_cell, cells):
    rate = bytes_per_cell * cells / (fine_ms_per_cycle * 1e-3)
    return dict(ms_per_cycle=fine_ms_per_cycle, bytes_per_cell=bytes_per_cell, bytes_per_s=rate,
                fraction_of_hbm_peak=rate / HBM_PEAK)


def tolerance(cp, src):
    a = np.abs(src[1:-1, 1:-1])
    if cp.case_id == C.BACKSTEP:  # over the fluid cells (backwards_step-01.cpp:879-888)
        i, j = np.arange(1, cp.nx + 1)[None, :], np.arange(1, cp.ny + 1)[:, None]
        a = a[(i > cp.step_i) | (j <= cp.inlet_jmax)]
    m = float(a.max())
    if cp.case_id == C.CAVITY:
        return cp.tol_factor * m
    return max(cp.tol_factor * (m if m > 0 else 1.0), cp.abs_tol)  # channel-01.cpp:642-649


def run(cp, steps, warmup, **kw):
    g = C.solver_for(cp, **kw)
    if cp.case_id == C.CAVITY:
        g.applyBoundaryConditions()
    for _ in range(warmup):
        g.step()
    g.reset_timing()
    its, ress, tols = [], [], []
    for _ in range(steps):
        it, res = g.step()
        its.append(it)
        ress.append(res)
        tols.append(tolerance(cp, g.field("src")))
    tm, info = g.timing(), g.mg_info()
    out = dict(iterations=its, residual=ress, tolerance=tols, converged=[r <= t for r, t in zip(ress, tols)],
               poisson_ms_per_solve=tm.poisson_ms / steps, step_ms=tm.step_ms / max(1, tm.steps),
               kernel=C._lib.SOR_KERNEL[tm.sor_kernel])
    if info.solves:
        out.update(levels=info.levels, coarsest=[info.coarse_nx, info.coarse_ny], coarse_sweeps=info.coarse_sweeps,
                   cycles_per_solve=info.cycles / info.solves, launches_per_solve=info.launches / info.solves,
                   ms_per_solve=info.solve_ms / info.solves, ms_per_cycle=info.solve_ms / info.cycles,
                   fine_ms_per_cycle=info.fine_ms / info.cycles,
                   rest_ms_per_cycle=(info.solve_ms - info.fine_ms) / info.cycles)
    g.close()
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=["cavity", "channel", "step"], default="cavity")
    ap.add_argument("--method", choices=["multigrid", "multigrid-open", "multigrid-step", "multigrid-any", "multigrid-open-any"],
                    default=None,
                    help="default: multigrid for the cavity, multigrid-open for the channel, multigrid-step for the step;\n"
                         "multigrid-any: the cavity at any grid size; multigrid-open-any: the channel at any grid size")
    ap.add_argument("--re", type=float, default=None, help="default: 1000; the step: 400")
    ap.add_argument("--sizes", nargs="+", default=None, help="default: 1024x1024 4096x4096 992x992 (cavity), "
                    "4096x512 1024x128 (channel), 256x32 1024x128 8192x512 (step)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mg"))
    ap.add_argument("--commit", default="unknown", help="commit of the tree being measured (recorded)")
    ap.add_argument("--skip-default", action="store_true", help="leave the default (SOR) solve out")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    method = a.method or {"cavity": "multigrid", "channel": "multigrid-open", "step": "multigrid-step"}[a.case]
    sizes = a.sizes or {"cavity": ["1024x1024", "4096x4096", "992x992"], "channel": ["4096x512", "1024x128"],
                        "step": ["256x32", "1024x128", "8192x512"]}[a.case]
    if a.re is None:
        a.re = 400.0 if a.case == "step" else 1000.0
    ok = True
    for size in sizes:
        nx, ny = (int(v) for v in size.split("x"))
        cp = C.make_params("backwards_step" if a.case == "step" else a.case, re=a.re, nx=nx, ny=ny)
        rec = dict(case=a.case, method=method, re=a.re, nx=nx, ny=ny, steps=a.steps, warmup=a.warmup, commit=a.commit,
                   timer="HIP events (cfd_timing.poisson_ms, cfd_mg_info.solve_ms / fine_ms)")
        rec["multigrid_v22"] = v22 = run(cp, a.steps, a.warmup, poisson=method)
        cells = float(nx) * ny
        rec["level0_fused"] = f0 = level0_rate(v22["fine_ms_per_cycle"], FUSED_BYTES_PER_CELL, cells)
        os.environ["CFD_MG_FUSED"] = "0"  # the smoothing as one launch per colour, in place (the same bits)
        rec["multigrid_v22_colour_launches"] = c22 = run(cp, a.steps, a.warmup, poisson=method)
        del os.environ["CFD_MG_FUSED"]
        rec["level0_colour_launches"] = f1 = level0_rate(c22["fine_ms_per_cycle"], COLOUR_BYTES_PER_CELL, cells)
        if not a.skip_default:
            rec["default_sor"] = run(cp, a.steps, a.warmup)
        if a.case != "cavity" and not (all(v22["converged"]) and all(c22["converged"])):
            ok = False
            print(f"{nx}x{ny}: a multigrid solve ended above its tolerance", file=sys.stderr)
        tag = a.case + {"multigrid-any": "_any", "multigrid-open-any": "_open_any"}.get(method, "")
        path = os.path.join(a.out, f"mg_timing_{tag}_{nx}x{ny}.json")
        with open(path, "w") as fh:
            json.dump(rec, fh, indent=1)
        d = rec.get("default_sor")
        print(f"{nx}x{ny}: multigrid {v22['ms_per_solve']:.3f} ms/solve, {v22['cycles_per_solve']:.1f} cycles, "
              f"{v22['launches_per_solve']:.0f} launches, {v22['ms_per_cycle']:.3f} ms/cycle "
              f"(level 0 {v22['fine_ms_per_cycle']:.3f}, rest {v22['rest_ms_per_cycle']:.3f}), "
              f"residual {v22['residual'][-1]:.3e} <= tol {v22['tolerance'][-1]:.3e}: {v22['converged'][-1]}; "
              f"colour launches {c22['ms_per_solve']:.3f} ms/solve (level 0 {c22['fine_ms_per_cycle']:.3f} ms/cycle); "
              f"level 0 moves {f0['bytes_per_s'] / 1e12:.2f} TB/s ({100 * f0['fraction_of_hbm_peak']:.0f} % of the HBM peak; "
              f"colour launches {f1['bytes_per_s'] / 1e12:.2f} TB/s)"
              + (f"; default {d['kernel']} {d['poisson_ms_per_solve']:.2f} ms/solve, {d['iterations'][-1]} sweeps, "
                 f"residual {d['residual'][-1]:.3e} (tol {d['tolerance'][-1]:.3e})" if d else ""), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
