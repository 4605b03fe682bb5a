"""Compile-time checks (no GPU) of the key-tiled attention kernels (attention_tiled.hip), cross-compiled for gfx950 as
test_kernel_resources.py does: no scratch, and every kernel's registers and LDS within the occupancy its file header states."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "theia_amd", "csrc", "attention_tiled.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 * 1024
# kernel -> waves per SIMD it is designed for (4-wave workgroups: one wave per SIMD each)
DESIGN = {
    "attn_tiled_fwd_bf16_kernel": 4,
    "attn_tiled_dq_bf16_kernel": 4,
    "attn_tiled_dkv_bf16_kernel": 4,
    "attn_tiled_fwd_f32_kernel": 3,
    "attn_tiled_dq_f32_kernel": 2,
    "attn_tiled_dkv_f32_kernel": 2,
    "attn_tiled_delta_kernel": 8,
}


def _vgpr_budget(waves):
    """512 registers per SIMD lane (arch + accumulation registers, allocated in granules of 8)"""
    return (512 // waves) // 8 * 8


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_tiled_attention_kernels_fit_their_stated_occupancy(tmp_path):
    out = str(tmp_path / "attention_tiled.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", SRC, "-o", out], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    scratch = [int(x) for x in re.findall(r"^; ScratchSize:\s+(\d+)", text, re.M)]
    vgprs = [int(x) for x in re.findall(r"^; TotalNumVgprs:\s+(\d+)", text, re.M)]
    lds = [int(x) for x in re.findall(r"^; LDSByteSize:\s+(\d+)", text, re.M)]
    assert len(names) == len(scratch) == len(vgprs) == len(lds) and names
    seen = set()
    for name, s, v, l in zip(names, scratch, vgprs, lds):
        key = [k for k in DESIGN if k in name]
        assert len(key) == 1, name
        waves = DESIGN[key[0]]
        seen.add(key[0])
        assert s == 0, (name, s)
        assert v <= _vgpr_budget(waves), (name, v, waves)
        # a 4-wave workgroup per `waves` on every CU: their LDS together within the CU's
        assert l * waves <= LDS_PER_CU, (name, l, waves)
    assert seen == set(DESIGN)
    # the tuned kernels' regex checks (test_kernel_resources.py) must keep finding only the kernels they mean
    assert not any(re.search(r"attn_fwd_mfma_kernel|attn_bwd_", n) for n in names)
