"""The fp64 truth of pixel-aligned decoding (oracle/sdf_oracle.py decode_points_pixel): the number the native PixelAlign kernel is held
to in tests/test_gpu_pixel_align_fp64.py.  It must be the reference's function - pinned here to the reference's own run
(tests/golden/ref_variant_pixelalign.npz), to the module path's pixel_alignment + the nn.Module in fp64 and in fp32 - and its `inside`
argument must change the in / out decision and nothing else."""
import numpy as np
import pytest
import torch

from alignsdf_amd import synthetic as syn
from oracle import sdf_oracle as orc
from tests import pixel_align_cases as pc

SPECS, _, SD, MANO, _, CAM, LATENT = syn.variant_config("pixelalign")


def _module():
    from alignsdf_amd.networks import model as arch
    dec = arch.SeparateDecoder(SPECS["LatentSize"], SPECS["PointFeatSize"], SPECS["EncodeStyle"], **SPECS["NetworkSpecs"]).eval()
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in SD.items()})
    return dec


def _module_eval(dec, feat, pts, cam, mano, specs, dtype):
    from alignsdf_amd.torch_decoder import pixel_alignment
    x = torch.from_numpy(pts).to(dtype)
    dec = dec.to(dtype)
    try:
        lat = pixel_alignment(torch.from_numpy(feat).to(dtype), x, torch.from_numpy(cam).to(dtype),
                              {"joints": torch.from_numpy(mano["joints"]).to(dtype)}, specs["ImageSize"][0], specs["SdfScaleFactor"])
        with torch.no_grad():
            h, o, _ = dec(torch.cat([lat, x], 1))
    finally:
        dec.float()
    return h[:, 0].numpy(), o[:, 0].numpy()


def _cases():
    """(name, feature map, points, camera, mano, specs): the variant's own sample, the 64 x 64 sample under its inexact camera, the
    edge points on a 63 x 17 map."""
    pts = syn.uniform((600, 3), 93, -1.0, 1.0).astype(np.float32)
    feat, mano, cam = syn.pixel_align_sample(0)
    especs = dict(SPECS, SdfScaleFactor=pc.EDGE_SCALE, ImageSize=[pc.EDGE_IMAGE] * 2)
    emano = {"joints": np.tile(pc.EDGE_ROOT.reshape(1, 1, 3), (1, 21, 1))}
    return [("variant", LATENT, pts, CAM, MANO, SPECS), ("sample64", feat, pts, cam, mano, SPECS),
            ("edge", syn.pixel_align_sample(1, 63, 17)[0], pc.edge_points(17), pc.EDGE_CAM, emano, especs)]


def test_the_reference_golden(golden_dir):
    g = np.load("%s/ref_variant_pixelalign.npz" % golden_dir)
    for dtype in (torch.float32, torch.float64):
        h, o = orc.decode_points_pixel(SD, LATENT, g["rand_pts"], SPECS, MANO, CAM, dtype=dtype)
        assert h.dtype == dtype and o.dtype == dtype
        d = max(np.abs(h.numpy() - g["rand_hand"]).max(), np.abs(o.numpy() - g["rand_obj"]).max())
        assert d <= (1e-6 if dtype == torch.float32 else 1e-5), (dtype, d)


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_fp64_truth_is_the_module_in_fp64_and_close_to_fp32(case):
    name, feat, pts, cam, mano, specs = case
    root = mano["joints"][0, 0]
    in32 = pc.project(pts, cam, root, specs["ImageSize"][0], specs["SdfScaleFactor"], np.float32)[1]
    in64 = pc.project(pts, cam, root, specs["ImageSize"][0], specs["SdfScaleFactor"], np.float64)[1]
    agree = in32 == in64
    assert agree.mean() >= 0.99 and 0 < in64.sum() < len(pts)
    dec = _module()
    t = [x.numpy() for x in orc.decode_points_pixel(SD, feat, pts, specs, mano, cam, dtype=torch.float64)]
    m64 = _module_eval(dec, feat, pts, cam, mano, specs, torch.float64)
    d64 = max(np.abs(t[k] - m64[k]).max() for k in (0, 1))
    assert d64 <= 1e-12, (name, d64)
    # the fp32 decision handed in: equal where the decisions agree, and the mask of torch's own fp64 projection is project's
    t32 = [x.numpy() for x in orc.decode_points_pixel(SD, feat, pts, specs, mano, cam, dtype=torch.float64, inside=in32)]
    assert all(np.array_equal(t32[k][agree], t[k][agree]) for k in (0, 1))
    same = [x.numpy() for x in orc.decode_points_pixel(SD, feat, pts, specs, mano, cam, dtype=torch.float64, inside=in64)]
    assert all(np.array_equal(same[k], t[k]) for k in (0, 1))                    # bit for bit
    # against the fp32 module path and the fp32 oracle: a real fp64 evaluation, not fp32 values widened
    m32 = _module_eval(dec, feat, pts, cam, mano, specs, torch.float32)
    f = [x.numpy() for x in orc.decode_points_pixel(SD, feat, pts, specs, mano, cam)]
    for other in (m32, f):
        d = max(np.abs(t[k] - other[k])[agree].max() for k in (0, 1))
        assert 0.0 < d <= 1e-6, (name, d)


def test_the_handed_in_decision_is_used():
    """Forcing a point to the other side moves the truth by the size of the map's features, and the sample of a point the mask calls
    inside is taken at the fp64 uv even when that lies an ulp beyond the border (the cubic kernel is continuous there)."""
    feat, mano, cam = syn.pixel_align_sample(0)
    pts = syn.uniform((300, 3), 94, -1.0, 1.0).astype(np.float32)
    kw = dict(dtype=torch.float64)
    t = orc.decode_points_pixel(SD, feat, pts, SPECS, mano, cam, **kw)[0].numpy()
    flipped = ~pc.project(pts, cam, mano["joints"][0, 0], 256, SPECS["SdfScaleFactor"], np.float64)[1]
    u = orc.decode_points_pixel(SD, feat, pts, SPECS, mano, cam, inside=flipped, **kw)[0].numpy()
    assert np.median(np.abs(t - u)) >= 1e-3
    bp, kind = pc.border_points(cam, mano["joints"][0, 0], 256, SPECS["SdfScaleFactor"], 8)
    pair = np.stack([bp[kind == 0], bp[kind == 1]], 1)                           # adjacent floats either side of the border
    a = orc.decode_points_pixel(SD, feat, pair[:, 0], SPECS, mano, cam, inside=np.ones(len(pair), bool), **kw)[0].numpy()
    b = orc.decode_points_pixel(SD, feat, pair[:, 1], SPECS, mano, cam, inside=np.ones(len(pair), bool), **kw)[0].numpy()
    assert np.abs(a - b).max() <= 1e-6


def test_z_cam_zero_is_outside_under_either_mask():
    especs = dict(SPECS, SdfScaleFactor=pc.EDGE_SCALE, ImageSize=[pc.EDGE_IMAGE] * 2)
    emano = {"joints": np.tile(pc.EDGE_ROOT.reshape(1, 1, 3), (1, 21, 1))}
    pts = pc.edge_points()
    z0 = pts[:, 2] == -1.0
    F = pc.signed_wide(8, 8)
    in32 = pc.project(pts, pc.EDGE_CAM, pc.EDGE_ROOT, pc.EDGE_IMAGE, pc.EDGE_SCALE)[1]
    h, o = orc.decode_points_pixel(SD, F, pts, especs, emano, pc.EDGE_CAM, dtype=torch.float64, inside=in32)
    assert torch.isfinite(h).all() and torch.isfinite(o).all()
    mean_only = orc.decode_points_pixel(SD, F, pts[z0], especs, emano, pc.EDGE_CAM, dtype=torch.float64,
                                        inside=np.zeros(int(z0.sum()), bool))
    assert (h[torch.from_numpy(z0)] - mean_only[0]).abs().max().item() <= 1e-12


@pytest.mark.parametrize("name", ["impulse 9x5", "impulse 5x9", "signed_wide 5x3", "signed_wide 1x9", "ramp 8x8"])
def test_the_bicubic_sample_is_not_only_grid_samples_word(name):
    """pixel_latent (torch grid_sample, fp64) against the hand-written cubic convolution of tests/pixel_align_cases.fold_gather
    (identity weights: its output is the latent itself), on maps where one wrong tap costs a pixel's value.  fold_gather's tap
    weights are fp32 (relative error ~1e-7 each, 16 taps), its sums fp64: the two agree to 1e-5 of the map's largest value."""
    kind, size = name.split()
    H, W = (int(v) for v in size.split("x"))
    root = torch.from_numpy(pc.EDGE_ROOT).double()
    if kind == "impulse":
        maps = [pc.impulse(H, W, p) for p in ((0, 0), (H - 1, W - 1), (H // 2, 0), (1, 1), (H // 2, W // 2))]
    else:
        maps = [pc.signed_wide(H, W) if kind == "signed_wide" else pc.ramp(H, W)]
    for F in maps:
        pts = np.concatenate([pc.edge_points(W, H=H), pc.pixel_centre_points(H, W)]
                             + ([pc.impulse_probe_points(H, W, (H // 2, W // 2))] if min(H, W) > 1 else []), 0)
        emu, inside = pc.fold_gather(F[0], np.eye(256, dtype=np.float32), np.zeros(256, np.float32), pts, pc.EDGE_CAM, pc.EDGE_ROOT,
                                     pc.EDGE_IMAGE, pc.EDGE_SCALE)
        lat = orc.pixel_latent(torch.from_numpy(F).double(), torch.from_numpy(pts).double(), torch.from_numpy(pc.EDGE_CAM).double(),
                               root, pc.EDGE_IMAGE, pc.EDGE_SCALE, inside=inside).numpy()
        assert 0 < inside.sum() < len(pts)
        d = np.abs(lat - emu).max()
        assert d <= 1e-5 * np.abs(F).max(), (name, d)
