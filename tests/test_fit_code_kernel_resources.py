"""Compile-time budget of the fit's kernels (csrc/k1v_kernels.hip), from the compiler's resource remarks only, checked like the other
units (tests/test_interaction_kernel_resources.py): the loss form of the reverse-mode kernel and the Adam step have no scratch and
spill no vector register, and the shipped weight form comes out of the compiler with the figures it had before the loss form existed.

The scalar spills of the two reverse-mode instantiations cannot be bounded at zero: the shipped weight form has always kept 39 scalar
values in lanes of a vector register (no memory involved - its ScratchSize is 0), and the loss form is the same body.  Both are
held where they are: the weight form at the parent's 39, the loss form at no more than the 53 it was written with."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alignsdf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
WEIGHT_FORM, LOSS_FORM, ADAM = "18sdf_mlp_vjp_kernelE", "23sdf_mlp_vjp_loss_kernelE", "16adam_step_kernelE"
# the weight form as the parent commit builds it (the same flags, the same compiler): recorded from a build of the parent
PARENT_WEIGHT_FORM = {"VGPRs": 256, "AGPRs": 242, r"LDS Size \[bytes/block\]": 0, r"ScratchSize \[bytes/lane\]": 0, "VGPRs Spill": 0,
                      "SGPRs Spill": 39}
LOSS_FORM_SGPR_SPILLS = 53


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "k1v.s"
    from alignsdf_amd.build_native import FLAGS, SOURCES, TU_FLAGS
    assert "k1v_kernels.hip" in SOURCES
    flags = [f for f in FLAGS if f != "-fPIC"]
    proc = subprocess.run([HIPCC, *flags, *TU_FLAGS.get("k1v_kernels.hip", []), "-S", "--cuda-device-only", "k1v_kernels.hip", "-o", str(out),
                           "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", proc.stderr)[1:]

    def get(kernel, key):
        block = [b for b in blocks if kernel in b.split()[0]]
        assert len(block) == 1, kernel
        return int(re.search(key + r": (\d+)", block[0]).group(1))
    return get


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("kernel", [LOSS_FORM, ADAM])
def test_new_kernels_have_no_scratch_and_no_vector_spills(remarks, kernel):
    print("FITCODE resources %s: VGPRs %d AGPRs %d scratch %d spills VGPR %d SGPR %d" % (
        kernel, remarks(kernel, "VGPRs"), remarks(kernel, "AGPRs"), remarks(kernel, r"ScratchSize \[bytes/lane\]"),
        remarks(kernel, "VGPRs Spill"), remarks(kernel, "SGPRs Spill")))
    assert remarks(kernel, r"ScratchSize \[bytes/lane\]") == 0 and remarks(kernel, "VGPRs Spill") == 0
    assert remarks(kernel, "VGPRs") + remarks(kernel, "AGPRs") <= 512
    if kernel == ADAM:
        assert remarks(kernel, "SGPRs Spill") == 0 and remarks(kernel, "VGPRs") <= 64 and remarks(kernel, r"LDS Size \[bytes/block\]") == 0
    else:
        assert remarks(kernel, r"Occupancy \[waves/SIMD\]") == 1 and remarks(kernel, "SGPRs Spill") <= LOSS_FORM_SGPR_SPILLS


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_weight_form_is_built_as_before(remarks):
    for key, want in PARENT_WEIGHT_FORM.items():
        assert remarks(WEIGHT_FORM, key) == want, (key, remarks(WEIGHT_FORM, key), want)
