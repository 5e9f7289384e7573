"""Frequency-set entry points of the C ABI (no device needed): exported, declared, mirrored in Python, and argument checks that answer
before any device work."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("geoac_set_frequencies", "geoac_get_frequencies", "geoac_fan_fetch_atten", "geoac_fan_atten_dev")


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
    m = re.search(r"#define\s+GEOAC_MAX_FREQS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 16


def test_python_mirror_has_the_three_members():
    import geoac_amd
    C = geoac_amd.FanContext
    assert callable(C.set_frequencies) and callable(C.fetch_atten)
    assert isinstance(C.n_frequencies, property)


def test_strerror_is_unchanged():
    lib, _ = _lib()
    want = {0: "ok", -1: "invalid argument or call order", -2: "no usable HIP device (this library has no CPU fallback)", -3: "HIP runtime error",
            -4: "equation set or mode not implemented", -5: "capacity exceeded (step_limit or buffer)", -6: "out of memory", -7: "unknown error"}
    lib.geoac_strerror.restype = ctypes.c_char_p
    for code, text in want.items():
        assert lib.geoac_strerror(code).decode() == text


def test_null_context_and_null_arguments_are_invalid():
    lib, _ = _lib()
    fr = (ctypes.c_double * 17)(*([0.1] * 17))
    f = lib.geoac_set_frequencies
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    for n in (2, 0, 17, -3):
        assert f(None, n, fr) == -1
    assert f(None, 2, None) == -1
    n = ctypes.c_int(0)
    assert lib.geoac_get_frequencies(None, ctypes.byref(n)) == -1
    lib.geoac_fan_fetch_atten.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.geoac_fan_fetch_atten(None, fr) == -1
    lib.geoac_fan_atten_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.geoac_fan_atten_dev(None, None, None) == -1
