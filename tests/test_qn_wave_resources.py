"""Register budget of the two-kernel step's QN update (qn_kernel.hip
qn_wave_kernel, a wave per constraint): no VGPR spill, no scratch, at most
128 VGPRs under its 256-thread launch bounds, and no more LDS than the four
waves' private rows -- the compiler's own resource report, checked on the CPU
(hipcc cross-compiles gfx950)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "w-fsa_amd", "csrc")
# the compiler the library's Makefile uses, when none is on the PATH
HIPCC = shutil.which("hipcc") or shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))

# a wave's rows: 256 chunk sums, 64 exp(x), 64 gradients, 8 bytes each; four waves a block
WAVE_LDS = (256 + 2 * 64) * 8 * 4


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_qn_wave_kernel_has_no_spill_and_no_scratch(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "-c", os.path.join(CSRC, "qn_kernel.hip"), "-o", str(tmp_path / "qn.o"),
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
        m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)",
                      line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    hit = [k for k in kernels if re.search(r"qn_wave_kernelENS_6QnArgsE$", k)]
    assert len(hit) == 1, sorted(k for k in kernels if "qn_" in k)
    v = kernels[hit[0]]
    print(hit[0], v)
    assert "VGPRs" in v, v
    assert v.get("VGPRs Spill", 0) == 0, v
    assert v.get("SGPRs Spill", 0) == 0, v
    assert v.get("ScratchSize [bytes/lane]", 0) == 0, v
    assert v["VGPRs"] <= 128, v
    assert v.get("LDS Size [bytes/block]", 0) <= WAVE_LDS, v
