"""The argument checks, the block bookkeeping (dense and CSC) and the cutting of output blocks of
csrc/resident_batches.hpp on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/resident_batches_host.cpp is a stand-alone program that makes no HIP call."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_program_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "resident_batches_host")
    # (the sanitizers' runtimes are linked statically: the program stands alone)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + os.path.join(ROOT, "batchelor_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "resident_batches_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "csc_output_blocks_parent.json")], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "host checks ok" in run.stdout
