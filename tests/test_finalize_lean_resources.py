"""finalize_vbin_kernel (bk_finalize_lean.hip) is built for two workgroups of 1024 threads per CU: eight waves per SIMD.  What the
compiler reports for both instantiations pins that -- a few more scalar registers (more than 96 cost a wave per SIMD, and with it
the second workgroup), a 65th vector register or any scratch would undo it without a test of results noticing.  No GPU needed:
the file is compiled for gfx950 with -Rpass-analysis=kernel-resource-usage and the remarks are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bronko_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not (os.path.isfile(HIPCC) and os.access(HIPCC, os.X_OK)), reason="no hipcc")


@pytest.fixture(scope="module")
def usage():
    """{kernel's mangled name: {field: value}} of bk_finalize_lean.hip, from one compilation with the library's flags."""
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", "bk_finalize_lean.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    out, cur = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"remark: (?:\S+: )?\s*([A-Za-z][A-Za-z /\[\]]*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None and val.isdigit():
            cur[key] = int(val)
    return out


@pytest.mark.parametrize("fused", ["Lb1E", "Lb0E"])
def test_two_workgroups_per_cu(usage, fused):
    names = [n for n in usage if "finalize_vbin_kernel" in n and fused in n]
    assert len(names) == 1, sorted(usage)
    u = usage[names[0]]
    print(names[0], u)
    assert u["Occupancy [waves/SIMD]"] == 8
    assert u["VGPRs"] <= 64
    assert u["ScratchSize [bytes/lane]"] == 0


def test_both_instantiations_are_the_only_kernels(usage):
    assert sorted("fused" if "Lb1E" in n else "plane" for n in usage if "finalize_vbin_kernel" in n) == ["fused", "plane"]
