"""Register budget of the decode kernels (decode.hip): the Viterbi kernel,
every instantiated capacity of the K-best kernel and the edge-weight kernel
they share keep their state in registers -- no VGPR spill, no scratch memory (a
dynamically indexed candidate array would show up there), at most 128 VGPRs --
by the compiler's own resource report, checked on the CPU (hipcc cross-compiles
gfx950), as test_kernel_resources.py does for fb_kernels.hip."""
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
def test_decode_kernels_keep_their_state_in_registers(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "-c", os.path.join(CSRC, "decode.hip"), "-o", str(tmp_path / "decode.o"),
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
    # one Viterbi kernel, four K-best capacities, and ONE edge-weight kernel for both
    wanted = ["best_path_kernel"] + ["kbest_kernelILi%dE" % kc for kc in (2, 4, 8, 16)] + ["decode_edge_weight_kernel"]
    for want in wanted:
        hit = [k for k in kernels if want in k]
        assert len(hit) == 1, (want, sorted(kernels))
        v = kernels[hit[0]]
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        # 256-thread blocks, 16 waves per CU wanted: at most 128 VGPRs; no LDS (the scratch is global)
        assert 0 < v["VGPRs"] <= 128 and v["LDS Size [bytes/block]"] == 0, (want, v)
    assert len(kernels) == 6, sorted(kernels)
