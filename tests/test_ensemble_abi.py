"""Ensemble entry points of the C ABI (no device needed): exported, declared, and argument checks that answer before any device work."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("geoac_upload_atmo_1d_ensemble", "geoac_get_members")


def _lib():
    import geoac_amd
    return geoac_amd.load_library(), geoac_amd.library_path()


def test_symbols_exported():
    _, path = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in SYMS:
        assert s in names, s


def test_header_declares():
    hdr = open(os.path.join(ROOT, "include", "geoac_hip.h")).read()
    for s in SYMS:
        assert f"{s}(" in hdr, s
    assert "#define GEOAC_MAX_MEMBERS 64" in hdr


def test_null_context_and_bad_k_are_invalid():
    lib, _ = _lib()
    x = (ctypes.c_double * 8)(*range(8))
    f = lib.geoac_upload_atmo_1d_ensemble
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
    assert f(None, 2, 8, x, x, x, x, x, x) == -1
    k = ctypes.c_int(0)
    assert lib.geoac_get_members(None, ctypes.byref(k)) == -1
    # a fake, zero-filled context is never dereferenced past the argument checks
    assert f(None, 0, 8, x, x, x, x, x, x) == -1
    assert f(None, 65, 8, x, x, x, x, x, x) == -1
