"""Register / scratch budget of the projection kernel (csrc/k1p_kernels.hip), checked at compile time like the other decoder kernels
(tests/test_kernel_resources.py): the rule's state rides through the whole MFMA stream of the gradient form, which itself sits at
256 + 229 registers - a spill between MFMAs would cost whole percents and no parity test sees it."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alignsdf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MANGLED = "_ZN4asdf22sdf_mlp_project_kernelENS_12DecodeParamsENS_13ProjectParamsE"


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "k1p.s"
    from alignsdf_amd.build_native import FLAGS, SOURCES, TU_FLAGS
    assert "k1p_kernels.hip" in SOURCES
    flags = [f for f in FLAGS if f != "-fPIC"]
    proc = subprocess.run([HIPCC, *flags, *TU_FLAGS.get("k1p_kernels.hip", []), "-S", "--cuda-device-only", "k1p_kernels.hip", "-o", str(out),
                           "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return proc.stderr, out.read_text()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_projection_kernel_fits_the_register_file_without_scratch(compiled):
    block = [b for b in re.split(r"remark: Function Name: ", compiled[0])[1:] if b.split()[0] == MANGLED]
    assert len(block) == 1
    get = lambda key: int(re.search(key + r": (\d+)", block[0]).group(1))
    assert get("VGPRs") + get("AGPRs") <= 512 and get(r"ScratchSize \[bytes/lane\]") == 0 and get("VGPRs Spill") == 0
    assert get(r"Occupancy \[waves/SIMD\]") == 1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_projection_kernel_is_the_gradient_chain_in_a_loop(compiled):
    body = compiled[1][compiled[1].index(MANGLED + ":"):]
    body = [l.strip() for l in body[:body.index("s_endpgm")].splitlines()]
    ins = [l.split()[0] for l in body if l and not l.startswith((";", ".", "_")) and not l.endswith(":")]
    # ONE copy of the fp32 chain, not one per iteration, and nothing rolled: K-steps of v_mfma_f32_32x32x2_f32 per 32-row output tile -
    # layer 0: 2 (point features) x 16 tiles; layer 1: 512 / 2 x 8; layer 2: 256 / 2 + 2 x 16; layer 3: 512 / 2 x 16
    mfma = [i for i in ins if i.startswith("v_mfma_")]
    assert set(mfma) == {"v_mfma_f32_32x32x2_f32"} and len(mfma) == 2 * 16 + 256 * 8 + (128 + 2) * 16 + 256 * 16, len(mfma)
    assert "s_set_gpr_idx_on" not in ins and not [i for i in ins if i.startswith("v_movrel") or i.startswith("scratch_")]
    # the rule: a correctly rounded division, no fused multiply-add outside the last layer's dot product (16 x 16 x 2 lane halves... per
    # output tile: 256 v_fma_f32 / v_fmac_f32 of dot_w4 at most, plus those of tanhf and of the division's refinement)
    assert any(i.startswith("v_div_fixup_f32") for i in ins) and any(i.startswith("v_div_fmas_f32") for i in ins)
    # the vote goes through LDS behind a barrier, not through a per-wave ballot alone; quad permutes carry f and g
    assert any(i.startswith("ds_write_b32") or i.startswith("ds_store_b32") for i in ins) and "s_barrier" in ins
    assert len([l for l in body if "quad_perm:[1,1,1,1]" in l]) >= 1 and len([l for l in body if "quad_perm:[3,3,3,3]" in l]) >= 1
