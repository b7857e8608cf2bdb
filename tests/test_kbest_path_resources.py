"""Register budget of the K-best decode kernels (kbest_path.hip): every
instantiated capacity of the decode kernel keeps its candidate lists in
registers -- no VGPR spill, no scratch memory (a dynamically indexed candidate
array would show up there), at most 128 VGPRs -- by the compiler's own
resource report, checked on the CPU (hipcc cross-compiles gfx950), as
test_best_path_resources.py does for best_path.hip."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "w-fsa_amd", "csrc")
# the compiler the library's Makefile uses, when none is on the PATH
HIPCC = shutil.which("hipcc") or shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_kbest_path_kernels_keep_their_lists_in_registers(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "-c", os.path.join(CSRC, "kbest_path.hip"), "-o", str(tmp_path / "kb.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels = {}
    name = None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    print(kernels)
    # the old decoder's kernel names stay its own (test_best_path_resources.py counts them)
    assert not [k for k in kernels if "best_path_kernel" in k or "best_edge_weight_kernel" in k], sorted(kernels)
    wanted = ["kbest_kernelILi%dE" % kc for kc in (2, 4, 8, 16)] + ["kbest_edge_lw_kernel"]
    for want in wanted:
        hit = [k for k in kernels if want in k]
        assert len(hit) == 1, (want, sorted(kernels))
        v = kernels[hit[0]]
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        # 256-thread blocks, 16 waves per CU wanted: at most 128 VGPRs; no LDS (the scratch is global)
        assert 0 < v["VGPRs"] <= 128 and v["LDS Size [bytes/block]"] == 0, (want, v)
    assert len(kernels) == len(wanted), sorted(kernels)
