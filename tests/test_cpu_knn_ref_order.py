"""The pure part of the ordered references of the fp16 kNN tier (csrc/knn_order.hpp) on the host, under AddressSanitizer
and UndefinedBehaviorSanitizer: tests/host/knn_ref_order_host.cpp is a stand-alone program that makes no HIP call and
includes no HIP header.  The permutation it writes is compared with numpy: 256 equal-width buckets between the smallest and
the largest key (f32 arithmetic, as in the header), a stable sort by bucket, padding rows last."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 128  # rows of a ring slot: what a reference image is padded to a multiple of


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    out = str(tmp_path_factory.mktemp("ref_order") / "knn_ref_order_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "batchelor_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "knn_ref_order_host.cpp"), "-o", out], check=True)
    return out


def _numpy_buckets(key):
    key = key.astype(np.float32)
    lo, hi = key.min(), key.max()
    w = np.float32(hi - lo)
    if not w > 0:
        return np.zeros(key.size, dtype=np.int64)
    scale = np.float32(256.0) / w
    t = (key - lo) * scale  # f32 throughout
    return np.clip(np.floor(t), 0, 255).astype(np.int64)


def _keys(kind, nr):
    rng = np.random.Generator(np.random.PCG64(7 + nr))
    if kind == "random":
        return (rng.standard_normal((nr, 8)) ** 2).sum(axis=1).astype(np.float32)  # chi-square: uneven buckets
    if kind == "equal":
        return np.full(nr, 3.25, dtype=np.float32)
    if kind == "two":
        return np.where(rng.random(nr) < 0.3, np.float32(1.5), np.float32(9.0)).astype(np.float32)
    raise AssertionError(kind)


@pytest.mark.parametrize("nr", [4096, 4100, 8229])
@pytest.mark.parametrize("kind", ["random", "equal", "two"])
def test_permutation(exe, tmp_path, kind, nr):
    nr_pad = -(-nr // SLOT) * SLOT
    key = _keys(kind, nr)
    kf, of = str(tmp_path / "k.f32"), str(tmp_path / "o.i32")
    key.tofile(kf)
    run = subprocess.run([exe, kf, str(nr), str(nr_pad), of], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr  # (non-zero: a check failed, or a sanitizer spoke)
    pos = np.fromfile(of, dtype=np.int32)
    assert pos.size == nr_pad
    # padding comes last and stays where it is
    assert np.array_equal(pos[nr:], np.arange(nr, nr_pad))
    # a bijection of [0, nr)
    assert np.array_equal(np.sort(pos[:nr]), np.arange(nr))
    b = _numpy_buckets(key)
    bi = b[pos[:nr]]
    # buckets ascending
    assert (np.diff(bi) >= 0).all()
    # stable inside a bucket
    same = np.diff(bi) == 0
    assert (np.diff(pos[:nr])[same] > 0).all()
    # ... which together is numpy's stable sort by bucket
    assert np.array_equal(pos[:nr], np.argsort(b, kind="stable"))
    used = int(run.stdout.split()[1])
    assert used == np.unique(b).size
    if kind == "equal":
        assert used == 1 and np.array_equal(pos[:nr], np.arange(nr))  # the degenerate case: one bucket, identity
    if kind == "two":
        assert used == 2 and set(np.unique(b)) == {0, 255}
    if kind == "random":
        assert used > 100
