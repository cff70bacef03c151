"""The plan of adjust_shift_variance and its two scratch layouts (csrc/asv_plan.hpp) on the host, under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/host/asv_plan_host.cpp is a stand-alone program that makes no HIP call and includes no
HIP header.  What it prints is compared with tests/golden/asv_plan_parent.json: the plans, and the offsets the host driver and
the kernels each spelled out by hand, while all of it was still part of csrc/legacy.hip (the file's "source" field says which
lines of which commit)."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_and_layouts_match_the_recorded_ones(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "asv_plan_host")
    # (the sanitizers' runtimes are linked statically: the program stands alone)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "batchelor_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "asv_plan_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # (non-zero: an invariant is broken, or a sanitizer spoke)
    assert "plan checks ok" in run.stdout
    got = [json.loads(line) for line in run.stdout.splitlines() if line.startswith("{")]
    with open(os.path.join(ROOT, "tests", "golden", "asv_plan_parent.json")) as f:
        want = json.load(f)["rows"]
    assert len(want) >= 58
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    forms = {(w["plan"]["exact"], w["plan"]["wide"]) for w in want}
    assert forms == {(1, 0), (0, 1), (0, 0)}  # every form is among the recorded calls
