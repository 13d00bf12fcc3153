"""Compile-time budget of the interaction kernels (csrc/interaction.hip), checked like the other units (tests/test_kernel_resources.py):
both are bandwidth kernels - full occupancy, no scratch, no spills, no LDS beyond the per-workgroup reduction - and the lattice kernel
reads its aligned body with 16-byte loads."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alignsdf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("interaction_lattice_kernel", "interaction_points_kernel")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "interaction.s"
    from alignsdf_amd.build_native import FLAGS, SOURCES, TU_FLAGS
    assert "interaction.hip" in SOURCES
    flags = [f for f in FLAGS if f != "-fPIC"]
    proc = subprocess.run([HIPCC, *flags, *TU_FLAGS.get("interaction.hip", []), "-S", "--cuda-device-only", "interaction.hip", "-o", str(out),
                           "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return proc.stderr, out.read_text()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("kernel", KERNELS)
def test_interaction_kernels_have_no_scratch_and_full_occupancy(compiled, kernel):
    block = [b for b in re.split(r"remark: Function Name: ", compiled[0])[1:] if kernel in b.split()[0]]
    assert len(block) == 1
    get = lambda key: int(re.search(key + r": (\d+)", block[0]).group(1))
    assert get(r"ScratchSize \[bytes/lane\]") == 0 and get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0
    assert get(r"Occupancy \[waves/SIMD\]") == 8 and get("VGPRs") <= 64 and get("AGPRs") == 0
    assert get(r"LDS Size \[bytes/block\]") <= 256          # the per-workgroup reduction, nothing else


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_lattice_kernel_streams_with_16_byte_loads_and_counts_on_the_scalar_unit(compiled):
    text = compiled[1]
    name = re.search(r"^(_Z\w*%s\w*):" % KERNELS[0], text, flags=re.M).group(1)
    body = text[text.index("\n" + name + ":"):]
    ins = [l.split()[0] for l in (l.strip() for l in body[:body.index("s_endpgm")].splitlines()) if l and not l.startswith((";", ".")) and not l.endswith(":")]
    assert len([i for i in ins if i == "global_load_dwordx4"]) >= 2          # one per volume on the aligned body
    assert any(i.startswith("s_bcnt1_i32_b64") for i in ins)                 # ballot + popcount: the counts never touch a vector register
    assert not [i for i in ins if i.startswith("scratch_") or i.startswith("v_movrel")]
