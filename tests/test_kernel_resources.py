"""Register budget of the stream kernel (fb_kernels.hip fbs_kernel): every
variant the device QN loop launches must fit 128 VGPRs without spilling.
A spill put the in-kernel QN variant's scratch at 1,184 bytes per lane and
the c3 step from 29 to 116 us (round 5), with every parity test still green
-- so the compiler's own resource report is checked here, on the CPU
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


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_stream_kernel_variants_do_not_spill(tmp_path):
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
        m = re.search(r"remark:\s+(VGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    # fbs_kernel<WIDE, W_LDS, MULTI, DBG=0, RMIN, DELTA, QN>: the release variants
    fbs = {k: v for k, v in kernels.items() if "fbs_kernel" in k and "Li0E" in k}
    assert len(fbs) >= 8, sorted(kernels)
    # (the multi-rank variants, PX = the trailing template flag, may spill a
    # couple of registers at their exchange: the rmin + exchange variant keeps
    # 2 VGPRs, 12 bytes, in scratch; the one-rank variants none)
    px = {k for k in fbs if re.search(r"Lb1EEEvNS_12CompiledArgsE", k) and re.search(r"Li0ELb[01]ELb1ELb1ELb1E", k)}
    bad = {k: v for k, v in fbs.items()
           if v.get("VGPRs Spill", 0) > (2 if k in px else 0) or (k in px and v.get("ScratchSize [bytes/lane]", 0) > 16)}
    assert not bad, f"stream kernel variants spilling VGPRs: {bad}"
    # the delta-format variants without the rmin column (the c3 headline, with and without the QN
    # waves): at most a small private segment (the compiler reserves ~20 bytes there that no
    # instruction touches; the spilling build above had 1,184)
    delta = {k: v for k, v in fbs.items() if re.search(r"Li0ELb0ELb1ELb[01]E", k)}
    assert delta, sorted(fbs)
    assert all(v.get("ScratchSize [bytes/lane]", 0) <= 64 for v in delta.values()), delta
