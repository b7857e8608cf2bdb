"""Register budget of the bubble-grid step launch (fb_kernels.hip
step_grid_kernel): no scratch and at most 128 VGPRs -- the compiler's own
resource report, checked on the CPU (hipcc cross-compiles gfx950), as
test_ll_dot_resources.py checks step_dot_kernel's variants."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "w-fsa_amd", "csrc")
HIPCC = shutil.which("hipcc") or shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_step_grid_kernel_does_not_spill(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "-c", os.path.join(CSRC, "fb_kernels.hip"), "-o", str(tmp_path / "fb.o"),
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
        m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    hit = [k for k in kernels if "step_grid_kernel" in k]
    assert len(hit) == 1, sorted(kernels)
    v = kernels[hit[0]]
    print(hit[0], v)
    assert v.get("ScratchSize [bytes/lane]", 0) == 0, v
    assert v.get("VGPRs Spill", 0) == 0, v
    assert 0 < v.get("VGPRs", 0) <= 128, v
