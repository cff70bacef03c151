"""The plan of a kNN candidate pass (csrc/knn_plan.hpp) on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/knn_plan_host.cpp is a stand-alone program that makes no HIP call and includes no HIP header.  What it prints is
compared with tests/golden/knn_plan_parent.json, the plans the rules gave while they were still part of candidate_pass (the
file's "source" field says which lines of which commit)."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_matches_the_recorded_plans(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "knn_plan_host")
    # (the sanitizers' runtimes are linked statically: the program stands alone)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "batchelor_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "knn_plan_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # (non-zero: an invariant is broken, or a sanitizer spoke)
    assert "plan checks ok" in run.stdout
    got = [json.loads(line) for line in run.stdout.splitlines() if line.startswith("{")]
    with open(os.path.join(ROOT, "tests", "golden", "knn_plan_parent.json")) as f:
        want = json.load(f)["rows"]
    assert len(want) >= 19
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
