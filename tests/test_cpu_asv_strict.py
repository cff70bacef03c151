"""Strict mode of adjust_shift_variance (var_adj_strict) as far as no device is needed: the new symbols and the knob, the
argument checks of the C entry points and of the Python functions, the parameter structs of callers built against the
earlier header, and the strict pass's scratch plan (tests/host/asv_strict_plan_host.cpp, a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer)."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "batchelor_mi355x.h")) as f:
        return f.read()


def test_symbols_and_knob_are_in_header_and_library():
    from batchelor_amd import _lib
    h = _header()
    for sym in ("bmx_adjust_shift_variance_ex", "bmx_engine_var_adj_strict_cells", "bmx_mnn_result_strict_cells"):
        assert sym + "(" in h, sym
        assert hasattr(_lib.lib(), sym), sym
    assert h.count("int32_t var_adj_strict;") == 2 and '"asv_strict"' in h
    try:
        _lib.dev_set("asv_strict", 1)
        _lib.dev_set("asv_strict", -1)
    finally:
        _lib.dev_set("reset", 0)
    assert _lib.lib().bmx_dev_set(b"asv_stricter", ctypes.c_int32(1)) != 0


def _asv_ex(d1, d2, v, r1, r2, strict=1):
    from batchelor_amd import _lib
    d1, d2, v = (np.asfortranarray(x, dtype=np.float64) for x in (d1, d2, v))
    r1, r2 = np.asarray(r1, dtype=np.int32), np.asarray(r2, dtype=np.int32)
    out = np.zeros(d2.shape[1])
    counts = np.zeros(4, dtype=np.int64)
    rc = _lib.lib().bmx_adjust_shift_variance_ex(_lib.f64p(d1), d1.shape[0], d1.shape[1], _lib.f64p(d2), d2.shape[0], d2.shape[1],
                                                 _lib.f64p(v), v.shape[0], v.shape[1], ctypes.c_double(1.0), _lib.i32p(r1),
                                                 r1.size, _lib.i32p(r2), r2.size, _lib.f64p(out), strict,
                                                 counts.ctypes.data_as(_lib.c_i64p))
    return rc, _lib.lib().bmx_last_error().decode(), counts


@pytest.mark.parametrize("shapes,msg", [
    (((3, 4), (2, 5), (5, 3), [0], [0]), "number of genes do not match up between matrices"),
    (((3, 4), (3, 5), (4, 3), [0], [0]), "number of cells do not match up between matrices"),
    (((3, 4), (3, 5), (5, 3), [4], [0]), "subset indices out of range"),
    (((3, 4), (3, 5), (5, 3), [0], [-1]), "subset indices out of range"),
])
def test_ex_refuses_bad_shapes_with_the_legacy_messages(shapes, msg):
    s1, s2, sv, r1, r2 = shapes
    rc, err, counts = _asv_ex(np.zeros(s1), np.zeros(s2), np.zeros(sv), r1, r2)
    assert rc != 0 and err == msg
    assert counts.tolist() == [-1, -1, -1, -1]


class _OldParams(ctypes.Structure):  # bmx_params_t as the header before var_adj_strict has it
    _fields_ = [("struct_size", ctypes.c_int32), ("k", ctypes.c_int32), ("prop_k", ctypes.c_double), ("ndist", ctypes.c_double),
                ("min_batch_skip", ctypes.c_double), ("auto_merge", ctypes.c_int32), ("var_adj", ctypes.c_int32),
                ("sigma", ctypes.c_double)]


class _OldMnnParams(ctypes.Structure):  # bmx_mnn_params_t likewise
    _fields_ = [("struct_size", ctypes.c_int32), ("k", ctypes.c_int32), ("prop_k", ctypes.c_double),
                ("sigma", ctypes.c_double), ("cos_norm_in", ctypes.c_int32), ("cos_norm_out", ctypes.c_int32),
                ("var_adj", ctypes.c_int32), ("correct_all", ctypes.c_int32), ("svd_dim", ctypes.c_int32),
                ("auto_merge", ctypes.c_int32), ("subset_row", ctypes.c_void_p), ("n_subset_row", ctypes.c_int32),
                ("tree", ctypes.c_void_p), ("tree_len", ctypes.c_int32)]


def _fast_mnn_rc(params):
    """bmx_fast_mnn with no batches: the parameter struct is read first, whatever comes after fails for another reason."""
    from batchelor_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    rc = L.bmx_fast_mnn(0, 0, None, None, None, None, ctypes.byref(params), None, 0, None, None, None, None, None, None, None,
                        ctypes.byref(h))
    err = L.bmx_last_error().decode()
    if h:
        L.bmx_engine_destroy(h)
    return rc, err


def test_params_struct_versions():
    from batchelor_amd.reduced_mnn import BmxParams
    assert ctypes.sizeof(BmxParams) > ctypes.sizeof(_OldParams)
    assert BmxParams.var_adj_strict.offset == ctypes.sizeof(_OldParams)
    # strict without var_adj: refused while the struct is read
    rc, err = _fast_mnn_rc(BmxParams(ctypes.sizeof(BmxParams), 20, float("nan"), 3.0, 0.0, 0, 0, 0.1, 1))
    assert rc != 0 and "var_adj_strict needs var_adj" in err
    # the earlier header's struct, and today's with the field set properly: read without complaint
    for p in (_OldParams(ctypes.sizeof(_OldParams), 20, float("nan"), 3.0, 0.0, 0, 1, 0.1),
              BmxParams(ctypes.sizeof(BmxParams), 20, float("nan"), 3.0, 0.0, 0, 1, 0.1, 1)):
        rc, err = _fast_mnn_rc(p)
        assert rc != 0 and "var_adj_strict" not in err and "struct_size" not in err and "does not know" not in err, err


def test_mnn_params_struct_versions():
    """var_adj_strict lies BEHIND the 80 bytes of the earlier bmx_mnn_params_t, whose last four are padding that such a
    caller leaves unspecified: it is read only where struct_size covers it, and the padding (now `reserved`) never."""
    from batchelor_amd import _lib
    from batchelor_amd.mnn_correct import BmxMnnParams
    L = _lib.lib()
    old_size = ctypes.sizeof(_OldMnnParams)
    assert _OldMnnParams.tree_len.offset + 4 == BmxMnnParams.reserved.offset == old_size - 4
    assert BmxMnnParams.var_adj_strict.offset == old_size and ctypes.sizeof(BmxMnnParams) == old_size + 8
    x = np.asfortranarray(np.ones((4, 3)))
    data = (ctypes.c_void_p * 1)(x.ctypes.data)
    n = np.array([3], dtype=np.int32)
    tree = np.array([1], dtype=np.int32)
    h = ctypes.c_void_p()
    first_real_check = b"at least two batches must be specified"   # (what a struct that was read without complaint meets next)

    def call(p):
        rc = L.bmx_mnn_correct(1, 4, data, _lib.i32p(n), None, None, p, ctypes.byref(h))
        return rc, L.bmx_last_error()

    for var_adj in (1, 0):
        old = _OldMnnParams(old_size, 20, float("nan"), 0.1, 1, 1, var_adj, 0, 0, 0, None, 0, tree.ctypes.data, 1)
        rc, err = call(ctypes.byref(old))
        assert rc != 0 and err == first_real_check
        # the same caller with its padding full of whatever the stack held -- and with bytes behind the struct that say
        # "strict" if anybody read them
        buf = (ctypes.c_ubyte * (old_size + 8))(*([0xFF] * (old_size + 8)))
        ctypes.memmove(buf, ctypes.byref(old), old_size - 4)
        assert bytes(buf[old_size - 4:]) == b"\xff" * 12
        rc, err = call(ctypes.cast(buf, ctypes.c_void_p))
        assert rc != 0 and err == first_real_check, err
    short = _OldMnnParams(_OldMnnParams.tree_len.offset + 4, 20, float("nan"), 0.1, 1, 1, 1, 0, 0, 0, None, 0, tree.ctypes.data, 1)
    rc, err = call(ctypes.byref(short))
    assert rc != 0 and err == first_real_check
    # today's struct: `reserved` is ignored whatever it holds, the field is read
    new = BmxMnnParams(ctypes.sizeof(BmxMnnParams), 20, float("nan"), 0.1, 1, 1, 1, 0, 0, 0, None, 0, tree.ctypes.data, 1, -1, 1)
    rc, err = call(ctypes.byref(new))
    assert rc != 0 and err == first_real_check
    bad = BmxMnnParams(ctypes.sizeof(BmxMnnParams), 20, float("nan"), 0.1, 1, 1, 0, 0, 0, 0, None, 0, tree.ctypes.data, 1, 0, 1)
    rc, err = call(ctypes.byref(bad))
    assert rc != 0 and b"var_adj_strict needs var_adj" in err


def test_python_refuses_strict_without_var_adj_before_any_device():
    import batchelor_amd as bx
    from batchelor_amd import reduced_mnn
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((30, 5)), rng.standard_normal((20, 5))
    with pytest.raises(ValueError, match="var_adj_strict"):
        bx.reducedMNN(a, b, var_adj_strict=True)
    with pytest.raises(ValueError, match="var_adj_strict"):
        reduced_mnn.fast_mnn_one_shot([a, b], var_adj_strict=True)
    with pytest.raises(ValueError, match="var_adj_strict"):
        bx.mnnCorrect(a.T, b.T, var_adj=False, var_adj_strict=True)
    eng = bx.MnnEngine.__new__(bx.MnnEngine)   # (no device: run() refuses before it touches the handle)
    eng._h = ctypes.c_void_p()
    with pytest.raises(ValueError, match="var_adj_strict"):
        eng.run(var_adj_strict=True)


def test_param_classes():
    from batchelor_amd.batch_correct import ClassicMnnParam, FastMnnParam
    assert ClassicMnnParam(var_adj_strict=True) is not None
    with pytest.raises((ValueError, TypeError)):
        FastMnnParam(var_adj_strict=True)


def test_strict_scratch_plan(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "asv_strict_plan_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "batchelor_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "asv_strict_plan_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "strict plan checks ok" in run.stdout
    got = [json.loads(line) for line in run.stdout.splitlines() if line.startswith("{")]
    assert len(got) >= 20
    # the call's own plan is what it was: every row that asv_plan_host.cpp lists too is the recorded one
    with open(os.path.join(ROOT, "tests", "golden", "asv_plan_parent.json")) as f:
        want = json.load(f)["rows"]
    keys = ("g", "n2", "nr1", "nr2", "vect_row_major", "asv_fast", "asv_wide", "asv_chunk", "asv_cap")
    recorded = {tuple(w[k] for k in keys): w["plan"] for w in want}
    shared = [r for r in got if tuple(r[k] for k in keys) in recorded]
    assert len(shared) >= 18
    for r in shared:
        assert r["plan"] == recorded[tuple(r[k] for k in keys)], r
    for r in got:
        s = r["strict"]
        per_cell = 2 * r["nr2"] + 2 * s["npad"] + r["g"] + 2     # AsvLiteralLayout::wide_per_cell
        cells = max(r["n2"], 1)
        assert s["chunk"] >= 1
        assert s["doubles"] >= per_cell * s["chunk"] + (cells + 1) // 2 + (cells + 7) // 8 + 1
        if r["asv_chunk"] > 0:
            assert s["chunk"] <= r["asv_chunk"]
