"""Register budget of the stream-less step launch (fb_kernels.hip
step_dot_kernel<RMIN, QN, PX>): every release variant must fit its VGPR
budget without spilling, within the bounds test_kernel_resources.py allows
the stream kernel's counterparts -- the compiler's own resource report,
checked on the CPU (hipcc cross-compiles gfx950)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "w-fsa_amd", "csrc")
# the compiler the library's Makefile uses, when none is on the PATH
HIPCC = shutil.which("hipcc") or shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))

# <RMIN, QN, PX> as the mangled template arguments: what launch_step_dot launches
VARIANTS = {
    "plain": "Lb0ELb0ELb0E", "rmin": "Lb1ELb0ELb0E", "qn": "Lb0ELb1ELb0E", "qn_rmin": "Lb1ELb1ELb0E",
    "qn_px": "Lb0ELb1ELb1E", "qn_rmin_px": "Lb1ELb1ELb1E",
}


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_step_dot_kernel_variants_do_not_spill(tmp_path):
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
        m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    dot = {k: v for k, v in kernels.items() if "step_dot_kernel" in k}
    found = {}
    for label, args in VARIANTS.items():
        hit = [k for k in dot if re.search(r"step_dot_kernelI" + args + r"EEvNS_12CompiledArgsE", k)]
        assert len(hit) == 1, (label, sorted(dot))
        found[label] = dot[hit[0]]
    print(found)
    for label, v in found.items():
        px = label.endswith("_px")
        # the stream kernel's bounds: no spill in the one-rank variants; the
        # multi-rank ones at most 2 VGPRs and 16 bytes of scratch
        assert v.get("VGPRs Spill", 0) <= (2 if px else 0), (label, v)
        if px:
            assert v.get("ScratchSize [bytes/lane]", 0) <= 16, (label, v)
        # 1024-thread launch bounds: four waves per SIMD
        assert v.get("VGPRs", 0) <= 128, (label, v)
    # the headline variants (no rmin column): at most the small private
    # segment the stream kernel's are allowed
    for label in ("plain", "qn"):
        assert found[label].get("ScratchSize [bytes/lane]", 0) <= 64, (label, found[label])
