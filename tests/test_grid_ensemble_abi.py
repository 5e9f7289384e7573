"""Grid-ensemble entry point of the C ABI (no device needed): exported, declared, and argument checks that answer before any device work."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "geoac_upload_atmo_3d_ensemble"


def _lib():
    import geoac_amd
    return geoac_amd.load_library(), geoac_amd.library_path()


def test_symbol_exported():
    _, path = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert SYM in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_declares():
    hdr = open(os.path.join(ROOT, "include", "geoac_hip.h")).read()
    assert f"{SYM}(geoac_ctx* ctx, int n_members, int nx, int ny, int nz," in hdr
    assert "#define GEOAC_MAX_MEMBERS 64" in hdr


def test_python_mirror_exists():
    import geoac_amd
    assert callable(geoac_amd.FanContext.upload_atmo_3d_ensemble) and callable(geoac_amd.FanContext.load_grid_ensemble)


def test_null_context_and_bad_k_are_invalid():
    lib, _ = _lib()
    x = (ctypes.c_double * 64)(*range(64))
    f = getattr(lib, SYM)
    f.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 7
    # no context: nothing is dereferenced, no device is touched
    assert f(None, 2, 2, 2, 4, x, x, x, x, x, x, x) == -1
    assert f(None, 0, 2, 2, 4, x, x, x, x, x, x, x) == -1
    assert f(None, 65, 2, 2, 4, x, x, x, x, x, x, x) == -1
