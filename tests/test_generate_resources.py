"""Register budget of the generation kernels (generate.hip): the running sums,
the walk (both passes) and the scan keep their state in registers -- no VGPR
spill, no scratch memory, at most 128 VGPRs -- and use the LDS DESIGN §3l
states, by the compiler's own resource report, checked on the CPU (hipcc
cross-compiles gfx950), as test_sample_resources.py does for sample.hip."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "w-fsa_amd", "csrc")
# the compiler the library's Makefile uses, when none is on the PATH
HIPCC = shutil.which("hipcc") or shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))

# the kernels of generate.hip, their instantiations and the LDS bytes per block of each
KERNELS = {"generate_cdf_kernel": (1, 0), "generate_walk_kernel": (2, 0), "generate_scan_kernel": (3, 32)}


def _design_section():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    m = re.search(r"^### 3l\..*?(?=^##+ )", text, re.S | re.M)
    assert m, "DESIGN.md has no section 3l"
    return m.group(0)


def test_design_names_the_kernels_and_their_lds():
    sec = _design_section()
    assert set(re.findall(r"`(generate_\w+_kernel)(?:<[^>`]*>)?`", sec)) == set(KERNELS)
    for name, (_, lds) in KERNELS.items():
        # the first "LDS: N bytes" after the kernel's first mention is its own
        m = re.search(r"`%s(?:<[^>`]*>)?`.*?LDS:\s+(\d+)\s+bytes" % name, sec, re.S)
        assert m and int(m.group(1)) == lds, name


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_generate_kernels_keep_their_state_in_registers(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "-c", os.path.join(CSRC, "generate.hip"), "-o", str(tmp_path / "generate.o"),
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
    for want, (count, lds) in KERNELS.items():
        hit = [k for k in kernels if want in k]
        assert len(hit) == count, (want, sorted(kernels))
        for k in hit:
            v = kernels[k]
            assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
            # 256-thread blocks, 16 waves per CU wanted: at most 128 VGPRs
            assert 0 < v["VGPRs"] <= 128 and v["LDS Size [bytes/block]"] == lds, (k, v)
    assert len(kernels) == sum(c for c, _ in KERNELS.values()), sorted(kernels)
