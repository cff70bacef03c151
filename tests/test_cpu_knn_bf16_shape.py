"""The workgroup shape of the split-bf16 candidate pass (csrc/knn_bf16_shape.hpp) on the host, under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/host/knn_bf16_shape_host.cpp is a stand-alone program that makes no HIP call and includes
no HIP header.  What it prints -- one row per instantiation bf16_launch can reach: KS = 24 with NS in 1, 2, 3, 4, 6, 8, 10,
13, 16, 19, 24, KS = 40 with the same up to 16 -- is compared with tests/golden/knn_bf16_shape_parent.json, the shapes
ring_shape, ring_slots and list_pitch gave while the kernel, ring_slots and launch() each stated the LDS budget by hand (the
file's "source" field says which lines of which commit)."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NS_ALL = [1, 2, 3, 4, 6, 8, 10, 13, 16, 19, 24]


def test_shape_matches_the_recorded_shapes(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "knn_bf16_shape_host")
    # (the sanitizers' runtimes are linked statically: the program stands alone)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "batchelor_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "knn_bf16_shape_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # (non-zero: an invariant is broken, or a sanitizer spoke)
    assert "shape checks ok" in run.stdout
    got = [json.loads(line) for line in run.stdout.splitlines() if line.startswith("{")]
    with open(os.path.join(ROOT, "tests", "golden", "knn_bf16_shape_parent.json")) as f:
        want = json.load(f)["rows"]
    assert [(w["KS"], w["NS"]) for w in want] == [(24, ns) for ns in NS_ALL] + [(40, ns) for ns in NS_ALL if ns <= 16]
    assert len(got) == len(want) == 20
    for g, w in zip(got, want):
        assert g == w
        # what the kernel's static_asserts and its ring rely on, on the recorded numbers themselves
        assert g["lds_bytes"] <= 160 * 1024      # the LDS of a CU
        assert g["NSLOT"] >= 2                   # a tile is staged while another is read
        assert g["KS"] + 2 * g["PLN"] <= 64      # one list entry per lane during compaction
