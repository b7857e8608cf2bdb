"""Register and LDS budget of the dense path's sampler kernels
(dense_sample.hip): the exp kernel and the backward walk keep their state in
registers -- no VGPR spill, no scratch memory -- and stay under 64 KB of LDS,
by the compiler's own resource report, checked on the CPU (hipcc
cross-compiles gfx950), as test_dense_decode_resources.py does for
dense_decode.hip."""
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
def test_dense_sample_kernels_keep_their_state_in_registers(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "-c", os.path.join(CSRC, "dense_sample.hip"), "-o", str(tmp_path / "dense_sample.o"),
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
        m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    print(kernels)
    wanted = ["dense_sample_exp_kernel", "dense_sample_walk_kernel"]
    for want in wanted:
        hit = [k for k in kernels if want in k]
        assert len(hit) == 1, (want, sorted(kernels))
        v = kernels[hit[0]]
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        assert 0 < v["VGPRs"] <= 256, (want, v)
        assert v["LDS Size [bytes/block]"] < 64 * 1024, (want, v)
    assert len(kernels) == len(wanted), sorted(kernels)
