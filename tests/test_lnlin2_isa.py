"""csrc/lnlin2.hip: the code object of the two-workgroups-per-CU LayerNorm + projection kernel fits half a CU (at most 256 registers per
lane, VGPR + AGPR together, no scratch), and its read-ahead of weight fragments is safe: the generated gfx950 code never touches a fragment
register between the inline-asm ds_read_b128 that fills it and the s_waitcnt lgkmcnt(0) that retires it.  Runs on the build machine: hipcc
cross-compiles to assembly without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _regs(text):
    """register numbers named by the operands of one instruction: v12, v[12:15]"""
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", text):
        if m.group(3) is not None:
            out.add(int(m.group(3)))
        else:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


@pytest.mark.skipif(not (shutil.which(HIPCC) or os.path.exists(HIPCC)), reason="hipcc not available")
def test_code_object_fits_half_a_cu_and_fragments_are_left_alone(tmp_path):
    src = os.path.join(ROOT, "scp_amd", "csrc", "lnlin2.hip")
    asm = tmp_path / "lnlin2.s"
    r = subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src, "-o", str(asm)],
                       capture_output=True, text=True, cwd=os.path.join(ROOT, "scp_amd", "csrc"))
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    kernels = re.findall(r"^(_Z\w*ln2_proj_kernel\w*):", text, re.M)
    assert len(kernels) == 2, kernels
    meta = re.findall(r"\.agpr_count:\s+(\d+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", text, re.S)
    assert len(meta) == 2, meta
    for agpr, scratch, vgpr, spills in meta:
        assert int(vgpr) + int(agpr) <= 256 and int(scratch) == 0 and int(spills) == 0, meta
    lines = text.splitlines()
    for k in kernels:
        start = next(i for i, l in enumerate(lines) if l.startswith(k + ":"))
        end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
        pending, ahead, checked, in_asm = set(), 0, 0, False
        for l in lines[start:end]:
            if "#ASMSTART" in l or "#ASMEND" in l:
                in_asm = "#ASMSTART" in l
                continue
            ins = l.split(";")[0].strip()
            if not ins or ins.endswith(":"):
                continue
            if in_asm and ins.startswith("ds_read_b128"):       # (the compiler counts and waits for its own LDS reads)
                ops = ins.split(None, 1)[1].split(",")
                assert not (_regs(ops[0]) & pending), (k, ins)
                pending |= _regs(ops[0])
                assert not (_regs(ops[1]) & pending), (k, ins)
                ahead += 1
            elif ins.startswith("s_waitcnt") and "lgkmcnt(0)" in ins:
                pending = set()
            elif pending:
                assert not ins.startswith(("s_cbranch", "s_branch")), (k, "branch with fragment reads in flight")
                assert not (_regs(ins) & pending), (k, ins, sorted(pending))
                checked += 1
        assert not pending
        # the reads the scan is about are there, with the MFMAs of a k-step between them and their wait
        assert ahead >= 4 * 16 and checked >= 4 * 3 * 6, (k, ahead, checked)
