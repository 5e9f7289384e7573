"""No kernel of geoac_lstations.hip may touch scratch memory or LDS: read from the compiler's own resource report of the shipped build
(geoac_amd/csrc/build/geoac_lstations.hip.resource_usage.txt, written by the Makefile with -Rpass-analysis=kernel-resource-usage; hipcc
cross-compiles for gfx950 without a GPU), as tests/test_stations_resources.py does for the ground stations."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "geoac_amd", "csrc", "build", "geoac_lstations.hip.resource_usage.txt")
KERNELS = ("k_lsta_prep", "k_lsta_count", "k_lsta_rows")


def test_level_station_kernels_use_no_scratch_and_no_lds():
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
    assert all(k in names for k in KERNELS), names
    for k in KERNELS:
        mine = [r for r in rows if k in r["name"]]
        assert len(mine) == 1, (k, names)
        r = mine[0]
        print(f'{r["name"]}: scratch {r["ScratchSize"]} B/lane, spilled VGPRs {r["VGPRs Spill"]}, spilled SGPRs {r["SGPRs Spill"]}, LDS {r["LDS Size"]} B/block')
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["LDS Size"] == 0, r
