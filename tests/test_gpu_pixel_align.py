"""The native PixelAlign path (opt-in: decoder_for(..., pixel_align="native") / ASDF_PIXEL_ALIGN=native): the pixel-aligned form of
the fp32 chain (csrc/k1pa_kernels.hip) against the reference's own run, the module path, and an fp64 truth at the image edges; the
routing and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from alignsdf_amd import synthetic as syn
from tests.pixel_align_cases import EDGE_CAM, EDGE_IMAGE, EDGE_ROOT, EDGE_SCALE, edge_points, project

pytestmark = pytest.mark.gpu
EINVAL = -1         # ASDF_EINVAL (include/alignsdf_hip.h)


def _module(name="pixelalign"):
    from alignsdf_amd.networks import model as arch
    specs, cls, sd, mano, obj, cam, latent = syn.variant_config(name)
    dec = getattr(arch, cls)(specs["LatentSize"], specs["PointFeatSize"], specs["EncodeStyle"], **specs["NetworkSpecs"]).eval()
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    t = lambda d: None if d is None else {k: torch.from_numpy(v) for k, v in d.items()}
    return specs, dec, t(mano), t(obj), None if cam is None else torch.from_numpy(cam), torch.from_numpy(latent)


def _sample64():
    feat, mano, cam = syn.pixel_align_sample(0)
    return torch.from_numpy(feat), {k: torch.from_numpy(v) for k, v in mano.items()}, torch.from_numpy(cam)


def test_reference_golden_on_the_native_path(golden_dir, monkeypatch):
    """tests/golden/ref_variant_pixelalign.npz through the drop-in functions with ASDF_PIXEL_ALIGN=native: the bar of
    test_module_path.py (values 1e-5, boxes / zoom cube bit-equal)."""
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.utils.mesh import decode_two_pass
    from alignsdf_amd.utils.utils import decode_sdf_multi_output, decoder_for
    monkeypatch.setenv("ASDF_PIXEL_ALIGN", "native")
    g = np.load("%s/ref_variant_pixelalign.npz" % golden_dir)
    specs, dec, mano, obj, cam, latent = _module()
    hip = decoder_for(dec, specs, mano)
    assert isinstance(hip, HipSdfDecoder) and hip.pixel_align and hip.math == "f32"
    h, o, _ = decode_sdf_multi_output(dec, latent.cuda(), torch.from_numpy(g["rand_pts"]).cuda(), mano, cam, specs, obj_results=obj)
    assert np.abs(h[:, 0].cpu().numpy() - g["rand_hand"]).max() <= 1e-5 and np.abs(o[:, 0].cpu().numpy() - g["rand_obj"]).max() <= 1e-5
    r = decode_two_pass(True, True, dec, latent.cuda(), mano, obj, specs, 32, cam_intr=cam)
    assert np.array_equal(np.stack([r["bbox"][0:6], r["bbox"][8:14]]), g["bbox_32"])
    assert np.array_equal(r["voxel_size"].numpy().reshape(1), g["new_voxel_size_32"])
    assert np.array_equal(np.array(r["origin"], dtype=np.float32), g["new_origin_32"])
    assert np.abs(r["vol_hand"].cpu().numpy() - g["vol2_hand_32"]).max() <= 1e-5
    assert np.abs(r["vol_obj"].cpu().numpy() - g["vol2_obj_32"]).max() <= 1e-5


@pytest.mark.parametrize("N", [64, 128])
def test_native_against_the_module_path(N, tmp_path):
    """A realistic 64 x 64 map with part of the lattice outside the image: both passes within 1e-5 of the module path, the same
    boxes, signs equal except where the module path itself is within 2e-6 of the level; equal meshes at N = 64."""
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    from alignsdf_amd.utils.mesh import create_mesh_combined_decoder, decode_two_pass
    from alignsdf_amd.utils.utils import decoder_for
    specs, dec, _, _, _, _ = _module()
    feat, mano, cam = _sample64()
    native, module = decoder_for(dec, specs, mano, pixel_align="native"), decoder_for(dec, specs, mano, pixel_align="module")
    assert isinstance(native, HipSdfDecoder) and isinstance(module, TorchModuleDecoder)
    rn = decode_two_pass(True, True, native, feat.cuda(), mano, None, specs, N, cam_intr=cam)
    rm = decode_two_pass(True, True, module, feat.cuda(), mano, None, specs, N, cam_intr=cam)
    assert np.array_equal(rn["bbox"], rm["bbox"]) and rn["origin"] == rm["origin"]
    for k in ("vol_hand", "vol_obj"):
        a, b = rn[k].cpu().numpy(), rm[k].cpu().numpy()
        assert np.abs(a - b).max() <= 1e-5, (k, np.abs(a - b).max())
        differ = (a < 0) != (b < 0)
        assert np.all(np.abs(b[differ]) <= 2e-6), (k, int(differ.sum()))
        assert (b < 0).any() and (b >= 0).any()
    if N == 64:
        sn = create_mesh_combined_decoder(True, True, False, native, feat.cuda(), mano, None, cam, specs, str(tmp_path / "n"), N=N,
                                          return_stats=True)
        sm = create_mesh_combined_decoder(True, True, False, module, feat.cuda(), mano, None, cam, specs, str(tmp_path / "m"), N=N,
                                          return_stats=True)
        assert sn["hand"] == sm["hand"] and sn["obj"] == sm["obj"] and sn["hand"][1] > 100 and sn["obj"][1] > 100
        assert (tmp_path / "n_hand.ply").exists() and (tmp_path / "n_obj.ply").exists()


@pytest.mark.parametrize("H,W", [(64, 64), (63, 17), (8, 8)])
def test_decode_points_against_an_fp64_truth_at_the_image_edges(H, W):
    """decode_points at points inside, on the border taps, exactly at u / v = +-1, one fp32 step outside, at z = 0 and behind the
    camera, against the module evaluated in fp64 with pixel_alignment in fp64: within 1e-5.  These points decide in / out alike in
    fp32 and fp64 (exact projections), so a wrong decision would show as an error of the size of the map's features."""
    from alignsdf_amd.torch_decoder import pixel_alignment
    from alignsdf_amd.utils.utils import bind_sample, decoder_for
    specs, dec, _, _, _, _ = _module()
    specs = dict(specs, SdfScaleFactor=EDGE_SCALE, ImageSize=[EDGE_IMAGE, EDGE_IMAGE])
    feat = torch.from_numpy(syn.pixel_align_sample(1, H, W)[0])
    mano = {"joints": torch.from_numpy(np.tile(EDGE_ROOT.reshape(1, 1, 3), (1, 21, 1)))}
    cam = torch.from_numpy(EDGE_CAM)
    pts = edge_points(W)
    _, in32 = project(pts, EDGE_CAM, EDGE_ROOT, EDGE_IMAGE, EDGE_SCALE, np.float32)
    _, in64 = project(pts, EDGE_CAM, EDGE_ROOT, EDGE_IMAGE, EDGE_SCALE, np.float64)
    assert np.array_equal(in32, in64) and 0 < in32.sum() < len(pts)
    hip = decoder_for(dec, specs, mano, pixel_align="native")
    bind_sample(hip, specs, feat.cuda(), mano, None, cam)
    h, o = hip.decode_points(torch.from_numpy(pts).cuda())
    d64 = dec.double()
    try:
        x = torch.from_numpy(pts).double()
        lat = pixel_alignment(feat.double(), x, cam.double(), {"joints": mano["joints"].double()}, EDGE_IMAGE, EDGE_SCALE)
        with torch.no_grad():
            th, to, _ = d64(torch.cat([lat, x], 1))
    finally:
        dec.float()
    assert np.abs(h.cpu().numpy() - th[:, 0].numpy()).max() <= 1e-5
    assert np.abs(o.cpu().numpy() - to[:, 0].numpy()).max() <= 1e-5


def test_routing_and_refusals(monkeypatch):
    """Default routing unchanged; the opt-in selects the native path; every combination it does not cover keeps the module path or
    raises with the reason."""
    from alignsdf_amd import _native
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.networks.model import build_decoder
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    from alignsdf_amd.utils.utils import bind_sample, decoder_for
    monkeypatch.delenv("ASDF_PIXEL_ALIGN", raising=False)
    specs, dec, mano, _, cam, latent = _module()
    assert isinstance(decoder_for(dec, specs, mano), TorchModuleDecoder)
    monkeypatch.setenv("ASDF_PIXEL_ALIGN", "module")
    assert isinstance(decoder_for(dec, specs, mano), TorchModuleDecoder)
    monkeypatch.setenv("ASDF_PIXEL_ALIGN", "native")
    hip = decoder_for(dec, specs, mano)
    assert isinstance(hip, HipSdfDecoder) and hip.pixel_align
    assert decoder_for(dec, specs, mano, pixel_align="module") is not hip
    monkeypatch.setenv("ASDF_PIXEL_ALIGN", "bogus")
    with pytest.raises(ValueError):
        decoder_for(dec, specs, mano)
    monkeypatch.delenv("ASDF_PIXEL_ALIGN")
    # the arithmetic and the sweeps it does not take
    with pytest.raises(ValueError, match="fp32"):
        hip.set_math("f16x3")
    with pytest.raises(ValueError, match="ordinary"):
        hip.set_fast(True)
    with pytest.raises(ValueError, match="set_sample_pixel"):
        hip.set_sample(torch.zeros(256))
    assert hip.math == "f32" and hip.coarse_mode == hip.fine_mode == "exact"
    # refused decoders / samples keep the module path
    refused = []
    for tag in ("comb3", "nerf9", "both9"):
        s = dict(syn.specs_for(tag), PixelAlign=True)
        d = build_decoder(s, {k: torch.from_numpy(v) for k, v in syn.full_state_dict(tag).items()})
        m, _ = syn.pose_inputs(0)
        m = {k: torch.from_numpy(np.asarray(v)) for k, v in m.items()}
        m["joints"] = mano["joints"]
        refused.append(decoder_for(d, s, m, pixel_align="native"))
    s = dict(specs, ClassifierBranch=True)
    refused.append(decoder_for(dec, s, mano, pixel_align="native"))
    refused.append(decoder_for(dec, specs, None, pixel_align="native"))
    assert all(isinstance(r, TorchModuleDecoder) for r in refused)
    with pytest.raises(NotImplementedError, match="CombinedDecoder"):
        HipSdfDecoder({k: torch.from_numpy(v) for k, v in syn.full_state_dict("comb3").items()}, 256, 3, "nerf", pixel_align=True)
    # the C ABI: bad C / H / W, and what a pixel-aligned sample refuses
    bind_sample(hip, specs, latent.cuda(), mano, None, cam)
    L = _native.lib()
    f = torch.zeros((1, 256, 300, 4), device="cuda")
    c12, r3 = (ctypes.c_float * 12)(*cam.reshape(-1).tolist()), (ctypes.c_float * 3)(0.0, 0.0, 0.5)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for C, H, W in ((128, 8, 8), (256, 0, 8), (256, 8, 0), (256, 257, 8), (256, 8, 300)):
        assert L.asdf_decoder_set_sample_pixel(hip._h, f.data_ptr(), C, H, W, c12, r3, ctypes.c_float(256.0), ctypes.c_float(2.0),
                                               stream) == EINVAL
    assert L.asdf_decoder_set_math(hip._h, _native.MATH_F16X3) == EINVAL
    rec = torch.zeros(64, dtype=torch.int32, device="cuda")
    vol = torch.empty(16 ** 3, device="cuda")
    org = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    assert L.asdf_decode_grid_box(hip._h, 16, org, ctypes.c_float(2.0 / 15), _native.GRID_REFERENCE, ctypes.c_float(1e-3),
                                  vol.data_ptr(), None, rec.data_ptr(), stream) == EINVAL
    rep = hip.sweep_report()
    assert "not applied" in rep["pixel_align"]["fast_sweeps"]


def test_fast_settings_are_not_applied(monkeypatch):
    """ASDF_FAST=1 / ASDF_MATH=f16x3 do not reach a pixel-aligned decoder, and its sweep report says so."""
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    monkeypatch.setenv("ASDF_FAST", "1")
    monkeypatch.setenv("ASDF_MATH", "f16x3")
    specs, dec, *_ = _module()
    hip = HipSdfDecoder(dec, pixel_align=True)
    try:
        assert hip.math == "f32" and hip.coarse_mode == hip.fine_mode == "exact"
        rep = hip.sweep_report()["pixel_align"]
        assert rep["ignored_settings"] == {"ASDF_FAST": "1", "ASDF_MATH": "f16x3"}
    finally:
        hip.close()
