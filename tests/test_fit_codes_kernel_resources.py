"""Compile-time budget of the fit's kernels (csrc/k1vb_kernels.hip), from the compiler's resource remarks only, after the pattern of
tests/test_fit_code_kernel_resources.py: the loss form of the reverse-mode kernel has no scratch, spills no vector register,
fits the 512 registers of one wave per SIMD, and the small per-sample kernels around it have no scratch and no spills at all.

The loss form is the one-list body behind a descriptor lookup, so like that body it keeps scalar values in lanes of a vector
register (no memory involved - its ScratchSize is 0; tests/test_fit_code_kernel_resources.py explains).  Their number is held at no more than the 58
it was first built with (the weight form: 39; the loss term's words and the descriptor's - the sample's workgroup index and grid, its
point count and its pointers - are the difference)."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alignsdf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BATCH_FORM = "29sdf_mlp_vjp_loss_batch_kernelE"
SMALL = ("19fit_describe_kernelE", "19fit_cst_init_kernelE", "19fold_samples_kernelE", "23vjp_reduce_batch_kernelE", "24vjp_adjoint_batch_kernelE",
         "28vjp_loss_reduce_batch_kernelE", "22adam_init_batch_kernelE", "22adam_step_batch_kernelE")
BATCH_FORM_SGPR_SPILLS = 58
SCRATCH, LDS = r"ScratchSize \[bytes/lane\]", r"LDS Size \[bytes/block\]"


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "k1vb.s"
    from alignsdf_amd.build_native import FLAGS, SOURCES, TU_FLAGS
    assert "k1vb_kernels.hip" in SOURCES and TU_FLAGS["k1vb_kernels.hip"] == TU_FLAGS["k1v_kernels.hip"]
    flags = [f for f in FLAGS if f != "-fPIC"]
    proc = subprocess.run([HIPCC, *flags, *TU_FLAGS["k1vb_kernels.hip"], "-S", "--cuda-device-only", "k1vb_kernels.hip", "-o", str(out),
                           "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", proc.stderr)[1:]

    def get(kernel, key):
        block = [b for b in blocks if kernel in b.split()[0]]
        assert len(block) == 1, kernel
        return int(re.search(key + r": (\d+)", block[0]).group(1))
    get.kernels = [b.split()[0] for b in blocks]
    return get


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_batched_loss_form_fits_one_wave_without_scratch(remarks):
    k = BATCH_FORM
    print("FITCODES resources %s: VGPRs %d AGPRs %d scratch %d spills VGPR %d SGPR %d occupancy %d" % (
        k, remarks(k, "VGPRs"), remarks(k, "AGPRs"), remarks(k, SCRATCH), remarks(k, "VGPRs Spill"), remarks(k, "SGPRs Spill"),
        remarks(k, r"Occupancy \[waves/SIMD\]")))
    assert remarks(k, SCRATCH) == 0 and remarks(k, "VGPRs Spill") == 0
    assert remarks(k, "VGPRs") + remarks(k, "AGPRs") <= 512
    assert remarks(k, r"Occupancy \[waves/SIMD\]") == 1
    assert remarks(k, "SGPRs Spill") <= BATCH_FORM_SGPR_SPILLS


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("kernel", SMALL)
def test_small_kernels_have_no_scratch_and_no_spills(remarks, kernel):
    assert remarks(kernel, SCRATCH) == 0 and remarks(kernel, "VGPRs Spill") == 0 and remarks(kernel, "SGPRs Spill") == 0
    assert remarks(kernel, "VGPRs") <= 64 and remarks(kernel, "AGPRs") == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_unit_holds_these_kernels_only(remarks):
    """The one-list kernels of the shared bodies stay in k1v_kernels.hip: this unit has its own forms and nothing else."""
    assert len(remarks.kernels) == 1 + len(SMALL), remarks.kernels
