"""The SOR launch planner (csrc/plan.hpp) on the CPU: tests/plan_check.cpp, a stand-alone program,
holds the planner to its invariants and to what the kernels' tile decode relies on over a sweep of
shapes (the smallest that can go wrong, and the BASELINE sizes), and replays the plans recorded from
the library on an MI355X (tests/golden/sor_plans.json, written by scripts/record_sor_plans.py) from
their recorded inputs: every recorded field must come out again. Built with g++ alone - once plain,
once with the address and undefined-behaviour sanitizers - and run directly."""
from __future__ import annotations

import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "plan_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sor_plans.json")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_planner_invariants_and_recorded_plans(tmp_path, flags):
    exe = tmp_path / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", SRC, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe), GOLDEN], capture_output=True, text=True)
    print(run.stdout[-4000:], run.stderr[-4000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert " 0 failed" in run.stdout and "replayed" in run.stdout
