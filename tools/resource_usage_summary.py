#!/usr/bin/env python3
"""`make -C bronko_amd/csrc resource-usage 2>&1 | python tools/resource_usage_summary.py > profiles/NAME.txt`: the compiler's
kernel-resource-usage remarks as one line per kernel of the project's sources (source line, mangled name cut at 72 characters and then
tagged with the crc32 of the whole, the figures), and one last line for the library kernels that rocprim's sorts instantiate: how
many, and a sha256 of their name-and-figure lines.  Two such files diff line by line."""
import hashlib
import re
import sys
import zlib

SHORT = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "Dynamic Stack": "dynstack",
         "Occupancy [waves/SIMD]": "waves", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds"}
rows = []
for ln in sys.stdin:
    m = re.match(r"(\S+?):(\d+):\d+: remark:\s+(.*?): (.*?)(?: \[-Rpass-analysis=kernel-resource-usage\])?$", ln.rstrip("\n"))
    if not m:
        continue
    src, line, key, val = m.groups()
    if key == "Function Name":
        name = val if len(val) <= 72 else val[:72] + "~%08x" % zlib.crc32(val.encode())
        rows.append([src, "%s:%s" % (src, line), name])
    elif key in SHORT:
        rows[-1].append("%s=%s" % (SHORT[key], val))
own = [" ".join(r[1:]) for r in rows if "rocprim" not in r[0]]
lib = [" ".join(r[2:]) for r in rows if "rocprim" in r[0]]
print("# make -C bronko_amd/csrc resource-usage 2>&1 | python tools/resource_usage_summary.py: one line per kernel (source line, "
      "mangled name, the figures the compiler reports)")
print("\n".join(own))
field = lambda k: "/".join(sorted({x.split(k + "=")[1].split()[0] for x in lib}, key=int))   # noqa: E731
print("# rocprim kernels instantiated by the sorts of bk_build.hip and bk_kmer_dump.hip (library code): %d kernels, scratch %s, "
      "waves/SIMD %s; sha256 of their lines (name and figures, in the compiler's order): %s" %
      (len(lib), field("scratch"), field("waves"), hashlib.sha256(("\n".join(lib) + "\n").encode()).hexdigest()))
