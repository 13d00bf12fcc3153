"""Compile-time budget of the MANO kernels (csrc/mano.hip), from the compiler's resource remarks like the other units
(tests/test_interaction_kernel_resources.py): no scratch, no spills - every intermediate that is indexed at run time lives in LDS -
and the LDS of a workgroup below the 64 KB a workgroup may declare statically (the device has 160 KB per compute unit)."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alignsdf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("mano_prepare_kernel", "mano_forward_kernel", "mano_backward_kernel")
LDS_LIMIT = 64 * 1024


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "mano.s"
    from alignsdf_amd.build_native import FLAGS, SOURCES, TU_FLAGS
    assert "mano.hip" in SOURCES
    flags = [f for f in FLAGS if f != "-fPIC"]
    proc = subprocess.run([HIPCC, *flags, *TU_FLAGS.get("mano.hip", []), "-S", "--cuda-device-only", "mano.hip", "-o", str(out),
                           "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return proc.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("kernel", KERNELS)
def test_mano_kernels_have_no_scratch_no_spills_and_fit_lds(remarks, kernel):
    block = [b for b in re.split(r"remark: Function Name: ", remarks)[1:] if kernel in b.split()[0]]
    assert len(block) == 1
    get = lambda key: int(re.search(key + r": (\d+)", block[0]).group(1))
    assert get(r"ScratchSize \[bytes/lane\]") == 0 and get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0
    assert get(r"LDS Size \[bytes/block\]") <= LDS_LIMIT
    if kernel != "mano_prepare_kernel":
        assert get(r"LDS Size \[bytes/block\]") > 0          # the sample's intermediates
