#!/usr/bin/env python3
"""Per-kernel VGPR / SGPR / scratch / LDS / occupancy (hipcc -Rpass-analysis=kernel-resource-usage) of every csrc/*.hip, or of the
.hip sources named; an argument that is no .hip file is a regular expression the kernel names are filtered by."""
import glob
import re
import subprocess
import sys
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
srcs = [a for a in sys.argv[1:] if a.endswith(".hip")] or sorted(glob.glob(os.path.join(ROOT, "rust-renderer_amd/csrc/*.hip")))
pat = ([a for a in sys.argv[1:] if not a.endswith(".hip")] or ["."])[0]
rows = {}
for src in srcs:
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "rust-renderer_amd/csrc"), "--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True).stderr
    cur = None
    for line in out.splitlines():
        m = re.search(r"remark: (?:\s*)(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip().split("(")[0]
            rows[cur] = {"file": os.path.basename(src)}
        elif cur:
            rows[cur][k.split(" ")[0].replace("Total", "")] = v
print("%-70s %5s %5s %8s %4s %7s  %s" % ("kernel", "VGPR", "SGPR", "scratch", "occ", "LDS", "file"))
for k, r in rows.items():
    if re.search(pat, k):
        print("%-70s %5s %5s %8s %4s %7s  %s" % (k[:70], r.get("VGPRs"), r.get("SGPRs"), r.get("ScratchSize"), r.get("Occupancy"), r.get("LDS"), r["file"]))
