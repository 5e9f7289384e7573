"""No kernel of geoac_tubemap.hip may touch scratch memory or spill a register: read from the compiler's own resource report of the shipped build
(geoac_amd/csrc/build/geoac_tubemap.hip.resource_usage.txt, written by the Makefile with -Rpass-analysis=kernel-resource-usage; hipcc
cross-compiles for gfx950 without a GPU), as tests/test_stations_resources.py does for the station file."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "geoac_amd", "csrc", "build", "geoac_tubemap.hip.resource_usage.txt")
FIELDS = "Function Name|SGPRs Spill|VGPRs Spill|ScratchSize \\[bytes/lane\\]|LDS Size \\[bytes/block\\]"


def test_tube_map_kernels_use_no_scratch_no_spills_no_lds():
    if not os.path.exists(REPORT):
        subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(ROOT, "geoac_amd", "csrc"), "ARCH=gfx950"])
    rows, cur = [], None
    for line in open(REPORT):
        m = re.search(r"remark: .*?(" + FIELDS + r"): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    names = {n for r in rows for n in re.findall(r"k_tube_[a-z]+", r["name"])}
    assert names == {"k_tube_args", "k_tube_raster"}, names                        # (the layers' kernels: geoac_map.hip; the landing table's: geoac_stations.hip)
    assert sum("k_tube_raster" in r["name"] for r in rows) == 2                     # the reducing walk and the BEST walk
    assert all(k in r for r in rows for k in ("ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size"))
    offenders = [f'{r["name"]}: {r["ScratchSize"]} B/lane scratch, {r["VGPRs Spill"]} + {r["SGPRs Spill"]} spilled VGPRs + SGPRs, {r["LDS Size"]} B LDS' for r in rows
                 if r["ScratchSize"] or r["VGPRs Spill"] or r["SGPRs Spill"] or r["LDS Size"]]
    assert not offenders, "\n".join(offenders)
