"""CPU test of the scheduling rules of the ICP loop (icp-symm_amd/csrc/loop_plan.h): the feedback of a pass and the codec of the two record
slots that carry it, the grid sizes, the plan of a TREE pass, when a device-driven run may start and how it is cut into chunks.
tests/cpp/loop_plan.cpp holds the cases (expected values as literals); here it is built with g++ and run, and once more under
-fsanitize=address,undefined where the toolchain links it.  No GPU, nothing preloaded."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

GROUPS = ["feedback", "codec", "walk grid", "optimistic", "compact", "make_hood", "budget_walk", "grids", "batch_eligible", "chunks"]


def test_loop_plan_on_the_host(tmp_path):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the loop-plan driver")
    src = os.path.join(ROOT, "tests", "cpp", "loop_plan.cpp")
    base = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "icp-symm_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), src]
    exe = str(tmp_path / "loop_plan")
    subprocess.check_call(base + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "loop_plan: ok" in out.stdout, out.stdout + out.stderr
    assert out.stdout.splitlines() == [g + " ok" for g in GROUPS] + ["loop_plan: ok"]
    # the same program under the sanitizers (a stand-alone program with its own main), where the toolchain can link them
    san = str(tmp_path / "loop_plan_san")
    r = subprocess.run(base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san], capture_output=True, text=True)
    if r.returncode == 0:
        out = subprocess.run([san], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "loop_plan: ok" in out.stdout, out.stdout + out.stderr
    else:
        print("no sanitizer runtime to link against: the plain build only")
