"""Register and LDS budget of the dense path's byte-marginal and MEA kernels
(dense_marginals.hip): the exp, mask, count, fill and back-track kernels and
the two reward (max, +) steps keep their state in registers -- no VGPR spill,
no scratch memory; only the (max, +) steps use LDS, and no more than
dense_maxplus_kernel's tile (16 x 129 + 16 x 128 doubles) -- by the compiler's
own resource report, checked on the CPU (hipcc cross-compiles gfx950), as
test_dense_sample_resources.py does for dense_sample.hip."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "w-fsa_amd", "csrc")
# the compiler the library's Makefile uses, when none is on the PATH
HIPCC = shutil.which("hipcc") or shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
TILE_LDS = (16 * 129 + 16 * 128) * 8   # the (max, +) tile: 32 KB and its padding column


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_dense_marginal_kernels_keep_their_state_in_registers(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "-c", os.path.join(CSRC, "dense_marginals.hip"), "-o", str(tmp_path / "dense_marginals.o"),
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
    # (kernel, instantiations, LDS bytes allowed)
    wanted = [("dense_bm_exp_kernel", 1, 0), ("dense_bm_mask_kernel", 1, 0), ("dense_bm_rows_kernel", 2, 0),
              ("dense_bm_maxplus_kernel", 2, TILE_LDS), ("dense_bm_backtrack_kernel", 1, 0)]
    for want, count, lds in wanted:
        hit = [k for k in kernels if want in k]
        assert len(hit) == count, (want, sorted(kernels))
        for k in hit:
            v = kernels[k]
            assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
            assert 0 < v["VGPRs"] <= 256, (k, v)
            assert v["LDS Size [bytes/block]"] <= lds, (k, v)
    assert len(kernels) == sum(c for _, c, _ in wanted), sorted(kernels)
