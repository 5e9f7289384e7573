"""No kernel of geoac_stations.hip may touch scratch memory: read from the compiler's own resource report of the shipped build
(geoac_amd/csrc/build/geoac_stations.hip.resource_usage.txt, written by the Makefile with -Rpass-analysis=kernel-resource-usage; hipcc
cross-compiles for gfx950 without a GPU), as tests/test_kernel_resources.py does for the launch plan's files."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "geoac_amd", "csrc", "build", "geoac_stations.hip.resource_usage.txt")


def test_station_kernels_use_no_scratch():
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
    assert all(k in names for k in ("k_sta_prep", "k_sta_count", "k_sta_rows")), names
    assert all("ScratchSize" in r for r in rows)
    offenders = [f'{r["name"]}: {r["ScratchSize"]} B/lane scratch, {r.get("VGPRs Spill", 0)} spilled VGPRs' for r in rows if r["ScratchSize"] != 0 or r.get("VGPRs Spill", 0) != 0]
    assert not offenders, "\n".join(offenders)
    prep = [r for r in rows if "k_sta_prep" in r["name"]]                          # the landing table's kernel, which serves the tube map as well
    assert len(prep) == 1 and prep[0]["SGPRs Spill"] == 0 and prep[0]["LDS Size"] == 0, prep
