"""CPU side of the SDF-gradient feature: the fp64 forward-mode truth the GPU tests are held to (tests/sdf_grad_cases.grad_truth)
against torch autograd and against the reference's own gradients, the conditions of the GPU tests' point sets, grad_refusal, the PLY
layout with normals, and the compile-time budget of the gradient kernel (csrc/k1g_kernels.hip)."""
import os
import re
import subprocess

import numpy as np
import pytest

from alignsdf_amd import synthetic as syn
from tests import sdf_grad_cases as gc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sdf_grad.npz")
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alignsdf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEADS = ("hand", "obj")


@pytest.mark.parametrize("tag", ["nerf3", "both9", "hand6", "obj6", "grasp9", "bothcls9"])
def test_truth_equals_fp64_autograd_through_the_module(tag):
    """Forward mode by hand = reverse mode by torch, through alignsdf_amd.networks.model.SeparateDecoder in fp64, to 1e-12 on the clear
    points (on the others the two agree as well unless a unit sits at exactly 0)."""
    pts = gc.points(512, 31)
    t, a = gc.grad_truth(tag, gc.SAMPLE, pts), gc.module_autograd(tag, gc.SAMPLE, pts)
    for name in HEADS:
        clear = gc.clear_mask(t[name])
        assert clear.any()
        assert np.abs(t[name]["sdf"] - a[name]["sdf"]).max() <= 1e-12
        assert np.abs(t[name]["grad"] - a[name]["grad"])[clear].max() <= 1e-12
        assert np.abs(t[name]["grad"]).max() > 1e-2          # (not a flat decoder)


def test_point_sets_of_the_gpu_tests_are_clear_enough():
    """The condition of tests/test_gpu_sdf_grad.py, on the truth alone: at least 85 % of every head of every set with more than 256
    points is clear at 1e-5 (measured: 98-99 % on nerf3 / both9 / bothcls9, 92-96 % on the trained grasp decoders), and at least one
    point per head of the shorter sets."""
    for label, tag, sample, pts in gc.point_sets():
        t = gc.grad_truth(tag, sample, pts)
        for name in HEADS:
            share = gc.clear_mask(t[name]).mean()
            assert share > 0 and (len(pts) <= 256 or share >= gc.MIN_CLEAR_SHARE), (label, name, share)


def test_truth_matches_the_reference_gradients():
    """tests/golden/ref_sdf_grad.npz (tests/golden/make_grad_goldens.py): the reference's SeparateDecoder in fp32 and its autograd
    gradients, 257 points each of nerf3 and both9.  On the clear points the fp64 truth is within the fp32 autograd's own error of
    them: measured here 2.2e-7 (nerf3) and 2.0e-7 (both9) at max |grad| 0.47 / 0.35; the bound is the largest fp32-autograd error
    measured on any clear point of the 4096-point sets, 1.2e-6 (grasp9, max |grad| 3.3).  The values: within the 1e-6 the fp32
    oracle is pinned to the reference's decoder outputs with (oracle/sdf_oracle.py); measured 2.1e-7."""
    with np.load(GOLDEN) as z:
        for tag in ("nerf3", "both9"):
            pts = z[tag + ".pts"]
            assert pts.shape == (257, 3) and np.array_equal(pts, gc.list_points(257))
            t = gc.grad_truth(tag, gc.SAMPLE, pts)
            for name in HEADS:
                clear = gc.clear_mask(t[name])
                e = np.abs(t[name]["grad"] - z["%s.grad_%s" % (tag, name)])[clear].max()
                s = np.abs(t[name]["sdf"] - z["%s.sdf_%s" % (tag, name)]).max()
                print("SDFGRAD golden %s %s: clear %.1f%% grad %.2e sdf %.2e" % (tag, name, 100 * clear.mean(), e, s))
                assert clear.mean() >= gc.MIN_CLEAR_SHARE and e <= 1.2e-6 and s <= 1e-6, (tag, name, e, s)


def test_grad_refusal():
    from alignsdf_amd.hip_decoder import grad_refusal
    for tag in ("nerf3", "both9", "hand6", "obj6", "grasp3", "grasp9", "bothcls9"):
        specs = syn.specs_for(tag)
        assert grad_refusal(False, specs["PointFeatSize"], specs["EncodeStyle"], False) is None, tag
    for tag in ("nerf9", "nerf15"):
        specs = syn.specs_for(tag)
        assert isinstance(grad_refusal(False, specs["PointFeatSize"], specs["EncodeStyle"], False), str), tag
    assert isinstance(grad_refusal(True, 3, "nerf", False), str)          # comb3
    assert isinstance(grad_refusal(False, 3, "nerf", True), str)          # pixel-aligned


NOT_DIFFERENTIATED = "pixel-aligned latent (the bicubic gather is not differentiated)"
NERF9 = "NeRF encoding with PointFeatSize 9 (only point features affine in xyz are built)"
NERF15 = "NeRF encoding with PointFeatSize 15 (only point features affine in xyz are built)"
# (combined, 3, "nerf", no pixel), (separate, 3, "nerf", pixel), (separate, 9, "nerf", no pixel), (separate, 15, "nerf", no pixel)
REFUSAL_SENTENCES = {
    "grad_refusal": ("CombinedDecoder (the gradient kernel is built for SeparateDecoder)", NOT_DIFFERENTIATED, NERF9, NERF15),
    "vjp_refusal": ("CombinedDecoder (the reverse-mode kernel is built for SeparateDecoder)", NOT_DIFFERENTIATED, NERF9, NERF15),
    "trace_refusal": ("CombinedDecoder (the ray-tracing kernel is built for SeparateDecoder)",
                      "pixel-aligned latent (the ray-tracing kernel has no bicubic gather)", NERF9, NERF15),
    "project_refusal": ("CombinedDecoder (the projection kernel is built for SeparateDecoder)", NOT_DIFFERENTIATED, NERF9, NERF15),
}


@pytest.mark.parametrize("name", sorted(REFUSAL_SENTENCES))
def test_every_refusal_sentence_is_pinned(name):
    """The four coverage rules of the fp32 chain's point and ray forms, sentence by sentence: callers show them to the user
    (NotImplementedError) and tests look for words in them."""
    from alignsdf_amd import hip_decoder
    refusal = getattr(hip_decoder, name)
    combined, pixel, nerf9, nerf15 = REFUSAL_SENTENCES[name]
    assert refusal(True, 3, "nerf", False) == combined
    assert refusal(False, 3, "nerf", True) == pixel
    assert refusal(False, 9, "nerf", False) == nerf9
    assert refusal(False, 15, "nerf", False) == nerf15
    assert refusal(False, 3, "nerf", False) is None
    for size in (3, 6, 9, 15):
        assert refusal(False, size, "both", False) is None
    # (the signature: the same four names, by keyword as by position)
    assert refusal(combined=True, point_feat_size=3, encode_style="nerf", pixel_align=False) == combined


TWO_TRIANGLES = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], np.float32), np.array([[0, 1, 2], [2, 1, 3]]))
# what write_ply wrote for them before it knew normals
TWO_TRIANGLES_FILE = (
    b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 2\n"
    b"property list uchar int vertex_indices\nend_header\n"
    b"\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x80?\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x80?"
    b"\x00\x00\x00\x00\x00\x00\x80?\x00\x00\x80?\x00\x00\x00?"
    b"\x03\x00\x00\x00\x00\x01\x00\x00\x00\x02\x00\x00\x00\x03\x02\x00\x00\x00\x01\x00\x00\x00\x03\x00\x00\x00")


def test_ply_with_and_without_normals(tmp_path):
    from alignsdf_amd.deep_sdf.metrics.chamfer import load_mesh
    from alignsdf_amd.ply import read_ply, write_ply
    v, f = TWO_TRIANGLES
    plain, withn = str(tmp_path / "plain.ply"), str(tmp_path / "normals.ply")
    write_ply(plain, v, f)
    with open(plain, "rb") as fh:
        assert fh.read() == TWO_TRIANGLES_FILE
    n = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 0, 0], [-1, 0, 0]], np.float32)
    write_ply(withn, v, f, n)
    with open(withn, "rb") as fh:
        data = fh.read()
    assert b"property float z\nproperty float nx\nproperty float ny\nproperty float nz\nelement face" in data
    assert len(data) == len(TWO_TRIANGLES_FILE) + len(b"property float nx\nproperty float ny\nproperty float nz\n") + 4 * 12
    rv, rf = read_ply(withn)
    assert np.array_equal(rv, v) and np.array_equal(rf, f) and rv.dtype == np.float32
    rv, rf, rn = read_ply(withn, with_normals=True)
    assert np.array_equal(rv, v) and np.array_equal(rf, f) and np.array_equal(rn, n)
    rv, rf, rn = read_ply(plain, with_normals=True)
    assert np.array_equal(rv, v) and np.array_equal(rf, f) and rn is None
    lv, lf = load_mesh(withn)
    assert lv.dtype == np.float64 and np.array_equal(lv, v) and np.array_equal(lf, f)
    with pytest.raises(ValueError):
        write_ply(withn, v, f, n[:3])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_gradient_kernel_budget(tmp_path):
    """The budget of its siblings (tests/test_kernel_resources.py): __launch_bounds__(256, 1), at most 512 registers, one wave per
    SIMD, no scratch access between the first and the last MFMA of the tile body - with the per-unit flags of the shipped build."""
    from alignsdf_amd.build_native import FLAGS, SOURCES, TU_FLAGS
    assert "k1g_kernels.hip" in SOURCES
    out = str(tmp_path / "k1g.s")
    proc = subprocess.run([HIPCC, *[f for f in FLAGS if f != "-fPIC"], "-fPIC", *TU_FLAGS.get("k1g_kernels.hip", []), "-S", "--cuda-device-only",
                           "k1g_kernels.hip", "-o", out, "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True,
                          text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    block = [b for b in re.split(r"remark: Function Name: ", proc.stderr)[1:] if "19sdf_mlp_grad_kernelE" in b.split()[0]]
    assert len(block) == 1
    get = lambda key: int(re.search(key + r": (\d+)", block[0]).group(1))
    print("K1G resources: VGPRs %d AGPRs %d scratch %d occupancy %d" % (get("VGPRs"), get("AGPRs"), get(r"ScratchSize \[bytes/lane\]"),
                                                                       get(r"Occupancy \[waves/SIMD\]")))
    assert get("VGPRs") + get("AGPRs") <= 512 and get(r"Occupancy \[waves/SIMD\]") == 1
    with open(out) as fh:
        text = fh.read()
    mangled = "_ZN4asdf19sdf_mlp_grad_kernelENS_12DecodeParamsENS_10GradParamsE"
    body = text[text.index(mangled + ":"):]
    body = [l.strip() for l in body[:body.index("s_endpgm")].splitlines()]
    ins = [l.split()[0] for l in body if l and not l.startswith((";", ".", "_")) and not l.endswith(":")]
    mfma = [k for k, i in enumerate(ins) if i.startswith("v_mfma_")]
    # the fp32 chain's MFMAs, all of them: 8192 of the three hidden layers + 64 of the point features, nothing rolled up
    assert {ins[k] for k in mfma} == {"v_mfma_f32_32x32x2_f32"} and len(mfma) == 8192 + 64
    scratch = [k for k, i in enumerate(ins) if i.startswith("scratch_")]
    assert not [k for k in scratch if mfma[0] < k < mfma[-1]], "scratch access inside the MFMA stream"
    assert [i for i in ins if i.endswith("_dpp")], "the quad permute that hands the value column's mask to the tangent columns"
    meta = text[text.index(".amdhsa_kernel " + mangled):]
    assert re.search(r"\.max_flat_workgroup_size:\s+256", text[text.index("amdhsa.kernels"):]), "__launch_bounds__(256, 1)"
    assert ".amdhsa_next_free_vgpr" in meta
