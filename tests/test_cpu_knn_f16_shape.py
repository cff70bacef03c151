"""The workgroup shape of the fp16 candidate pass (csrc/knn_f16_shape.hpp) on the host, under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/host/knn_f16_shape_host.cpp is a stand-alone program that makes no HIP call and includes no
HIP header.  What it prints -- one row per instantiation f16_launch can reach: KS = 32 with NS = 1..8, KS = 48 with NS = 1..4 --
is compared with tests/golden/knn_f16_shape_parent.json, the shapes the four sizing functions gave while they stood in
knn_f16.hip and the kernel and its launcher each combined them by hand (the file's "source" field says which lines of which
commit)."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shape_matches_the_recorded_shapes(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "knn_f16_shape_host")
    # (the sanitizers' runtimes are linked statically: the program stands alone)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "batchelor_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "knn_f16_shape_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # (non-zero: an invariant is broken, or a sanitizer spoke)
    assert "shape checks ok" in run.stdout
    got = [json.loads(line) for line in run.stdout.splitlines() if line.startswith("{")]
    with open(os.path.join(ROOT, "tests", "golden", "knn_f16_shape_parent.json")) as f:
        want = json.load(f)["rows"]
    assert [(w["KS"], w["NS"]) for w in want] == [(32, ns) for ns in range(1, 9)] + [(48, ns) for ns in range(1, 5)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
        # the invariants the kernel relies on, on the recorded numbers themselves
        assert g["lds_bytes"] <= 160 * 1024 and g["NSLOT"] >= 2 and g["KS"] < g["LCAP"] <= 64 and g["KEEP_MAX"] >= g["KS"]
        assert 8 % g["NSERV"] == 0 and (8 // g["NSERV"]) % 2 == 0
        assert g["TP"] != 2 or g["NSLOT"] >= 3
