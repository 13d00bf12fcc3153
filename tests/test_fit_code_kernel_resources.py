"""Compile-time budget of the reverse-mode unit (csrc/k1v_kernels.hip), from the compiler's resource remarks only, checked like the other
units (tests/test_interaction_kernel_resources.py): the shipped weight form comes out of the compiler with the figures it had before
the loss form existed, and the unit holds nothing but it and its two finishing kernels.  (The loss form and the fit's small kernels:
csrc/k1vb_kernels.hip, tests/test_fit_codes_kernel_resources.py.)

The scalar spills of the reverse-mode body cannot be bounded at zero: the shipped weight form has always kept 39 scalar values in
lanes of a vector register (no memory involved - its ScratchSize is 0).  It is held where it is, at the parent's 39."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alignsdf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
WEIGHT_FORM = "18sdf_mlp_vjp_kernelE"
FINISH = ("17vjp_reduce_kernelE", "18vjp_adjoint_kernelE")
# the weight form as the parent commit builds it (the same flags, the same compiler): recorded from a build of the parent
PARENT_WEIGHT_FORM = {"VGPRs": 256, "AGPRs": 242, r"LDS Size \[bytes/block\]": 0, r"ScratchSize \[bytes/lane\]": 0, "VGPRs Spill": 0,
                      "SGPRs Spill": 39}


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
    get.kernels = [b.split()[0] for b in blocks]
    return get


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_weight_form_is_built_as_before(remarks):
    for key, want in PARENT_WEIGHT_FORM.items():
        assert remarks(WEIGHT_FORM, key) == want, (key, remarks(WEIGHT_FORM, key), want)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_unit_holds_these_kernels_only(remarks):
    """The loss form, the loss reduce and the Adam kernels exist once, in k1vb_kernels.hip: this unit emits the weight form, its reduce
    and its adjoint, and nothing else."""
    assert len(remarks.kernels) == 1 + len(FINISH), remarks.kernels
    for kernel in (WEIGHT_FORM,) + FINISH:
        remarks(kernel, "VGPRs")
