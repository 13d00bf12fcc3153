"""CPU side of the reverse-mode decoder feature: the fp64 truth the GPU tests are held to (tests/sdf_vjp_cases.vjp_truth) against torch
autograd through the oracle, the differentiable kinematic embedding and the shifted embedding of alignsdf_amd.fit, the compile-time
budget of the reverse-mode kernel (csrc/k1v_kernels.hip) and the C ABI's bookkeeping."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from alignsdf_amd import synthetic as syn
from tests import sdf_vjp_cases as vc

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alignsdf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
POSED = ("both9", "hand6", "obj6", "grasp9", "bothcls9")


def _random_w(M, seed=3):
    rng = np.random.default_rng(seed)
    return {name: rng.standard_normal(M) for name in vc.HEADS}


@pytest.mark.parametrize("tag", ["both9", "grasp9"])
def test_truth_equals_fp64_autograd_through_the_oracle(tag):
    """(a) d_latent of the manual reverse chain = autograd through oracle.sdf_oracle in fp64, to 1e-12 max |entry| (300 random points,
    random weights; no point is excluded: in fp64 the two take the same masks) - and d_embed, d_fold's column sums with it."""
    pts = vc.points(300, 9)
    w = _random_w(300)
    t, a = vc.vjp_truth(tag, 3, pts, w), vc.oracle_autograd_vjp(tag, 3, pts, w, torch.float64)
    top = np.abs(a["d_latent"]).max()
    assert top > 1e-3 and np.abs(t["d_latent"] - a["d_latent"]).max() <= 1e-12 * top
    for h in range(2):
        scale = np.abs(a["d_embed"][h]).max()
        assert t["d_embed"][h].shape == a["d_embed"][h].shape and np.abs(t["d_embed"][h] - a["d_embed"][h]).max() <= 1e-12 * max(1.0, scale)
    # one head alone: the other head's blocks are zero, and the two d_latent add up
    th = vc.vjp_truth(tag, 3, pts, {"hand": w["hand"]})
    to = vc.vjp_truth(tag, 3, pts, {"obj": w["obj"]})
    assert not th["d_fold"][1].any() and not to["d_fold"][0].any() and not th["d_embed"][1].any()
    assert np.abs(th["d_latent"] + to["d_latent"] - t["d_latent"]).max() <= 1e-12 * top
    assert np.array_equal(th["d_fold"][0], t["d_fold"][0]) and np.array_equal(to["d_fold"][1], t["d_fold"][1])


@pytest.mark.parametrize("tag", ["both9", "grasp9"])
def test_embedding_gradient_pulled_back_to_the_pose(tag):
    """(b) d_embed pulled through fit.kinematic_affine_torch = fp64 autograd with respect to obj_trans and rot_center through
    oracle.kinematic_embedding, to 1e-10 relative.  obj_trans is compared on its rows 0..2, the rotation and the translation: the
    affine form (hip_decoder.kinematic_affine, by its own statement) takes the homogeneous divisor of a rigid transform as the constant
    it is, so along the bottom row (0, 0, 0, 1) - directions that leave the rigid transforms - it is a different function of the
    matrix than the reference's division per point."""
    from alignsdf_amd.fit import kinematic_affine_torch
    specs = syn.specs_for(tag)
    pts = vc.points(300, 9)
    w = _random_w(300)
    t = vc.vjp_truth(tag, 3, pts, w)
    want = vc.oracle_autograd_vjp(tag, 3, pts, w, torch.float64, pose_grads=True)
    _, mano, obj = vc._pose(tag, 3, torch.float64)
    mano["rot_center"].requires_grad_()
    obj["obj_trans"].requires_grad_()
    E = kinematic_affine_torch(specs["PointFeatSize"], specs["EncodeStyle"], specs["SdfScaleFactor"], mano, obj)
    pulled = sum((e * torch.from_numpy(d)).sum() for e, d in zip(E, t["d_embed"]))
    g_rc, g_ot = torch.autograd.grad(pulled, (mano["rot_center"], obj["obj_trans"]))
    for got, ref in ((g_rc.numpy(), want["rot_center"]), (g_ot.numpy().reshape(4, 4)[:3], want["obj_trans"].reshape(4, 4)[:3])):
        top = np.abs(ref).max()
        assert top > 0 and np.abs(got - ref).max() <= 1e-10 * top, (tag, np.abs(got - ref).max(), top)


@pytest.mark.parametrize("tag", POSED)
def test_kinematic_affine_torch_equals_the_numpy_one(tag):
    """(c) on every synthetic configuration with a pose, every sample of the GPU tests."""
    from alignsdf_amd.fit import kinematic_affine_torch
    from alignsdf_amd.hip_decoder import kinematic_affine
    specs = syn.specs_for(tag)
    for sample in (1, 2, 3):
        _, mano, obj = vc._pose(tag, sample, torch.float64)
        assert mano is not None
        args = (specs["PointFeatSize"], specs["EncodeStyle"], specs["SdfScaleFactor"], mano, obj)
        for combined in (False, True):
            a, b = kinematic_affine(*args, combined), kinematic_affine_torch(*args, combined)
            assert len(a) == len(b)
            for x, y in zip(a, b):
                assert x.shape == tuple(y.shape) and np.abs(x - y.numpy()).max() <= 1e-12


def test_shift_embed_moves_the_field():
    """(d) the oracle under shift_embed(E, t) at x = the oracle under E at x - t."""
    from alignsdf_amd.fit import kinematic_affine_torch, shift_embed
    from oracle import sdf_oracle as orc
    from tests import sdf_grad_cases as gc
    tag = "grasp9"
    specs, sd = syn.specs_for(tag), gc.state_dict(tag)
    latent, mano, obj = vc._pose(tag, 3, torch.float64)
    E = kinematic_affine_torch(specs["PointFeatSize"], specs["EncodeStyle"], specs["SdfScaleFactor"], mano, obj)
    x = torch.from_numpy(vc.points(200, 4)).double()
    shifts = (torch.tensor([0.03, -0.01, 0.02], dtype=torch.float64), torch.tensor([-0.02, 0.04, 0.01], dtype=torch.float64))
    L = latent.numel()
    for letter, e, t, cols in zip("ho", E, shifts, gc._head_slices(specs["EncodeStyle"], L, specs["PointFeatSize"])):
        params = orc.effective_head_params(sd, letter, torch.float64)
        lat = latent.reshape(1, -1).expand(x.shape[0], -1)
        es = shift_embed(e, t)
        moved = vc._forward_head(params, torch.cat([lat, x @ es[:, :3].t() + es[:, 3]], 1), torch.float64)[0]
        inputs = torch.cat([lat, orc.point_features(x - t, specs, mano, obj)], 1)[:, cols]
        assert np.abs(moved.numpy() - vc._forward_head(params, inputs, torch.float64)[0].numpy()).max() <= 1e-12
        assert np.array_equal(es[:, :3].numpy(), e[:, :3].numpy())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_reverse_mode_kernel_budget(tmp_path):
    """(e) with the per-unit flags of the shipped build: at most 512 registers, no scratch, at most 160 KiB of LDS (the kernel's
    LDS is dynamic: the launch size is the header's kVjpLdsBytes), one wave per SIMD, the MFMAs of both passes unrolled."""
    from alignsdf_amd.build_native import FLAGS, SOURCES, TU_FLAGS
    assert "k1v_kernels.hip" in SOURCES
    out = str(tmp_path / "k1v.s")
    proc = subprocess.run([HIPCC, *[f for f in FLAGS if f != "-fPIC"], "-fPIC", *TU_FLAGS.get("k1v_kernels.hip", []), "-S", "--cuda-device-only",
                           "k1v_kernels.hip", "-o", out, "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True,
                          text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    block = [b for b in re.split(r"remark: Function Name: ", proc.stderr)[1:] if "18sdf_mlp_vjp_kernelE" in b.split()[0]]
    assert len(block) == 1
    get = lambda key: int(re.search(key + r": (\d+)", block[0]).group(1))
    regs, scratch = get("VGPRs") + get("AGPRs"), get(r"ScratchSize \[bytes/lane\]")
    with open(os.path.join(CSRC, "sdf_mlp_vjp_kernel.h")) as fh:
        header = fh.read()
    assert "kVjpLdsBytes = kLdsBytes + kWaves * kVjpHeadFloats * 4" in header
    lds = get(r"LDS Size \[bytes/block\]") + (4 * 4096 + 6920) * 4 + 4 * 4096 * 4      # static + ring + constants + the four waves' sums
    print("K1V resources: VGPRs %d AGPRs %d scratch %d LDS %d occupancy %d" % (get("VGPRs"), get("AGPRs"), scratch, lds,
                                                                              get(r"Occupancy \[waves/SIMD\]")))
    assert regs <= 512 and scratch == 0 and lds <= 160 * 1024 and get(r"Occupancy \[waves/SIMD\]") == 1
    with open(out) as fh:
        text = fh.read()
    mangled = "_ZN4asdf18sdf_mlp_vjp_kernelENS_12DecodeParamsENS_9VjpParamsE"
    body = text[text.index(mangled + ":"):]
    ins = [l.split()[0] for l in (s.strip() for s in body[:body.index("s_endpgm")].splitlines()) if l and not l.startswith((";", ".", "_")) and not l.endswith(":")]
    mfma = [i for i in ins if i.startswith("v_mfma_")]
    # forward 8192 + 64 point-feature MFMAs, reverse 8192: nothing rolled up
    assert set(mfma) == {"v_mfma_f32_32x32x2_f32"} and len(mfma) == 2 * 8192 + 64
    assert not [i for i in ins if i.startswith("scratch_")]
    assert not [i for i in ins if "atomic" in i], "the sums are taken without atomics"
    assert [i for i in ins if i.endswith("_dpp")], "the cross-lane sums"


def test_abi_bookkeeping():
    """(f) the new entry point is looked up by name; the ABI version stays where three earlier test files pin it."""
    from alignsdf_amd import _native
    assert "asdf_decode_points_vjp" in _native.EXPORTS and _native.ABI_VERSION == 132
    with open(os.path.join(CSRC, "..", "..", "include", "alignsdf_hip.h")) as fh:
        assert "int asdf_decode_points_vjp(" in fh.read()


def test_vjp_refusal():
    from alignsdf_amd.hip_decoder import vjp_refusal
    for tag in ("nerf3", "both9", "hand6", "obj6", "grasp3", "grasp9", "bothcls9"):
        specs = syn.specs_for(tag)
        assert vjp_refusal(False, specs["PointFeatSize"], specs["EncodeStyle"], False) is None, tag
    for tag in ("nerf9", "nerf15"):
        specs = syn.specs_for(tag)
        assert isinstance(vjp_refusal(False, specs["PointFeatSize"], specs["EncodeStyle"], False), str), tag
    assert isinstance(vjp_refusal(True, 3, "nerf", False), str) and isinstance(vjp_refusal(False, 3, "nerf", True), str)
