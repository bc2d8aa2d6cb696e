"""The C-ABI library (include/vaeb_hip.h -> vaeb_amd/libvaeb_hip.so) loads without a GPU
and exports every function the header declares; the ctypes binding covers all of them."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vaeb_hip.h")
DIAG_HEADER = os.path.join(ROOT, "include", "vaeb_diag.h")
LIB = os.path.join(ROOT, "vaeb_amd", "libvaeb_hip.so")


def header_functions(path=HEADER):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vaeb_[a-z0-9_]+)\s*\(", src)))


def all_functions():
    return sorted(set(header_functions()) | set(header_functions(DIAG_HEADER)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(LIB)


def test_header_declares_expected_surface():
    fns = header_functions()
    for must in ["vaeb_create", "vaeb_update", "vaeb_validate", "vaeb_comm_init", "vaeb_set_params"]:
        assert must in fns


def test_library_exports_every_declared_symbol(lib):
    missing = [f for f in all_functions() if not hasattr(lib, f)]
    assert not missing, missing


def test_binding_covers_header():
    from vaeb_amd import _lib
    assert sorted(_lib.EXPORTS) == header_functions()
    assert sorted(_lib.DIAG_EXPORTS) == header_functions(DIAG_HEADER)


def test_diagnostics_are_not_in_the_dropin_header():
    """The drop-in boundary (vaeb_hip.h) holds only the reference's operations and their
    state transfers; timing / GEMM test hooks live in vaeb_diag.h."""
    pub = header_functions()
    for f in ("vaeb_debug_timeline", "vaeb_test_gemm_bf16", "vaeb_bench_gemm_bf16", "vaeb_profile_steps", "vaeb_get_h16",
              "vaeb_get_h16_f32"):
        assert f not in pub and f in header_functions(DIAG_HEADER)


def test_exports_are_c_linkage():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    for f in all_functions():
        assert re.search(r"\bT %s$" % f, out, re.M), f


def test_error_reporting_without_gpu(lib):
    """Argument validation happens before any device call: a bad config fails cleanly."""
    from vaeb_amd import _lib
    L = _lib.load()
    cfg = _lib.VaebConfig()
    cfg.D, cfg.H, cfg.Z, cfg.B, cfg.L = 0, 5, 2, 10, 1
    h = ctypes.c_void_p()
    rc = L.vaeb_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == -1
    assert b"dimensions" in L.vaeb_last_error()
    cfg.D, cfg.estimator, cfg.L = 5, 2, 2   # FV with L > 1 is rejected (VAEB.py:361 shadowing bug)
    assert L.vaeb_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    # the 16-bit engines keep the LA estimator's per-sample terms in eight registers
    # (step_bf16.hpp la[8]): L = 9 is VAEB_ERR_ARG, checked before the device is touched
    for dtype in (_lib.DTYPE_BF16, _lib.DTYPE_F16):
        cfg = _lib.VaebConfig()
        cfg.D, cfg.H, cfg.Z, cfg.B, cfg.L = 128, 64, 16, 40, 9
        cfg.estimator, cfg.dtype = _lib.EST_LA, dtype
        h = ctypes.c_void_p()
        assert L.vaeb_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
        assert b"L <= 8" in L.vaeb_last_error()
        assert not h.value
        # LB has no such limit: the same config passes the argument checks (and then needs a GPU)
        cfg.estimator = _lib.EST_LB
        rc = L.vaeb_create(ctypes.byref(cfg), ctypes.byref(h))
        assert rc != -1 and (rc == 0 or b"L <= 8" not in L.vaeb_last_error()), (rc, L.vaeb_last_error())
        if rc == 0:
            assert L.vaeb_destroy(h) == 0
    major, minor = ctypes.c_int32(), ctypes.c_int32()
    assert L.vaeb_version(ctypes.byref(major), ctypes.byref(minor)) == 0


def test_config_struct_layout_matches_header():
    from vaeb_amd import _lib
    # 17 int32/float fields (dtype included) + 5 reserved = 22 * 4 bytes
    assert ctypes.sizeof(_lib.VaebConfig) == 22 * 4
    assert _lib.VaebConfig.dtype.offset == 16 * 4
