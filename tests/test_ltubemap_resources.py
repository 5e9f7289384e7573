"""No kernel of geoac_ltubemap.hip may touch scratch memory or LDS, or spill a register: read from the compiler's own resource report of the
shipped build (geoac_amd/csrc/build/geoac_ltubemap.hip.resource_usage.txt, written by the Makefile with -Rpass-analysis=kernel-resource-usage;
hipcc cross-compiles for gfx950 without a GPU), as tests/test_lstations_resources.py does for the level stations."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "geoac_amd", "csrc", "build", "geoac_ltubemap.hip.resource_usage.txt")
KERNELS = {"k_ltube_args": 1, "k_ltube_raster": 2, "k_ltube_finish": 1}          # (the raster kernel has an instance per pass)


def test_level_tube_map_kernels_use_no_scratch_no_lds_and_spill_nothing():
    if not os.path.exists(REPORT):
        subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(ROOT, "geoac_amd", "csrc"), "ARCH=gfx950"])
    rows, cur = [], None
    for line in open(REPORT):
        m = re.search(r"remark: .*?(Function Name|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    names = " ".join(r["name"] for r in rows)
    assert len(rows) == sum(KERNELS.values()), names                              # every kernel of the file is one of these
    for k, n in KERNELS.items():
        mine = [r for r in rows if k in r["name"]]
        assert len(mine) == n, (k, names)
        for r in mine:
            print(f'{r["name"]}: scratch {r["ScratchSize"]} B/lane, spilled VGPRs {r["VGPRs Spill"]}, spilled SGPRs {r["SGPRs Spill"]}, LDS {r["LDS Size"]} B/block')
            assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, r
