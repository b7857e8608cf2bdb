"""Register budget of the byte-marginal kernels (marginals.hip): they keep
their state in registers -- no VGPR spill, no scratch memory, at most 128 VGPRs
-- and use the LDS DESIGN §3k states (none: the rows are global scratch), by the
compiler's own resource report, checked on the CPU (hipcc cross-compiles
gfx950), as test_posterior_resources.py does for posterior.hip."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "w-fsa_amd", "csrc")
# the compiler the library's Makefile uses, when none is on the PATH
HIPCC = shutil.which("hipcc") or shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))

# the kernels of marginals.hip and the LDS bytes per block of each
KERNELS = {"marginal_rows_kernel": 0, "marginal_decode_kernel": 0}


def _design_section():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    m = re.search(r"^### 3k\..*?(?=^##+ )", text, re.S | re.M)
    assert m, "DESIGN.md has no section 3k"
    return m.group(0)


def test_design_names_the_kernels_and_their_lds():
    sec = _design_section()
    for name in KERNELS:
        assert "`%s`" % name in sec, name
    assert set(re.findall(r"`(marginal_\w+_kernel)`", sec)) == set(KERNELS)
    m = re.search(r"LDS: (\d+) bytes", sec)
    assert m and int(m.group(1)) == 0


def test_makefile_builds_the_translation_unit():
    text = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    m = re.search(r"^HIP_SRC := (.*)$", text, re.M)
    assert m and "marginals.hip" in m.group(1).split()


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_marginal_kernels_keep_their_state_in_registers(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "-c", os.path.join(CSRC, "marginals.hip"), "-o", str(tmp_path / "marginals.o"),
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
    for want, lds in KERNELS.items():
        hit = [k for k in kernels if want in k]
        assert len(hit) == 1, (want, sorted(kernels))
        v = kernels[hit[0]]
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        # 256-thread blocks, 16 waves per CU wanted: at most 128 VGPRs
        assert 0 < v["VGPRs"] <= 128 and v["LDS Size [bytes/block]"] == lds, (want, v)
    assert len(kernels) == len(KERNELS), sorted(kernels)
