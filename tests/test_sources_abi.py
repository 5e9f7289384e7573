"""Source-set entry points of the C ABI (no device needed): exported, declared, and argument checks that answer before any device work."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("geoac_set_sources", "geoac_get_sources")


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


def test_null_context_and_bad_n_src_are_invalid():
    lib, _ = _lib()
    src = (ctypes.c_double * (3 * 65))()
    f = lib.geoac_set_sources
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert f(None, 2, src) == -1
    n = ctypes.c_int(0)
    assert lib.geoac_get_sources(None, ctypes.byref(n)) == -1
    assert f(None, 0, src) == -1
    assert f(None, 65, src) == -1
