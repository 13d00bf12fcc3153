"""CPU side of the native PixelAlign path: the fold-then-gather arithmetic (P = W_lat . F once per sample, then per point b + the
16 bicubic taps of P, or the fold of the channel mean outside the image) reproduces grid_sample-then-Linear, and the new
translation unit compiles for gfx950 without scratch."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from alignsdf_amd import synthetic as syn
from tests import pixel_align_cases as pc
from tests.pixel_align_cases import EDGE_CAM, EDGE_IMAGE, EDGE_ROOT, EDGE_SCALE, edge_points, fold_gather, project

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alignsdf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _layer0_latent_columns():
    from alignsdf_amd.hip_decoder import _effective
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in syn.full_state_dict("nerf3").items()}
    return _effective(sd, "linh0").numpy()[:, :256].copy(), sd["linh0.bias"].numpy().copy()


@pytest.mark.parametrize("H,W", [(8, 8), (64, 64), (63, 17)])
@pytest.mark.parametrize("camera", ["edge", "variant"])
def test_fold_then_gather_matches_grid_sample_then_linear_cpu(H, W, camera):
    """Random maps; points inside, on the border taps, exactly at u / v = +-1, one fp32 step outside, at z = 0 and behind the camera
    (edge camera), and a lattice under the PixelAlign variant's camera.  Bar: 1e-6 of the largest pre-activation - the fp32
    reference's own rounding (256-term sums) is of that size."""
    from alignsdf_amd.torch_decoder import pixel_alignment
    w_lat, b = _layer0_latent_columns()
    F = np.random.default_rng(H * 100 + W).standard_normal((1, 256, H, W)).astype(np.float32)
    if camera == "edge":
        pts, cam, root, isz, sc = edge_points(W), EDGE_CAM, EDGE_ROOT, EDGE_IMAGE, EDGE_SCALE
    else:
        specs, _, _, mano, _, cam, _ = syn.variant_config("pixelalign")
        v = np.linspace(-1.0, 1.0, 11, dtype=np.float32)
        pts = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
        root, isz, sc = mano["joints"][0, 0], specs["ImageSize"][0], specs["SdfScaleFactor"]
    emu, inside = fold_gather(F[0], w_lat, b, pts, cam, root, isz, sc)
    assert 0 < inside.sum() < len(pts)
    lat = pixel_alignment(torch.from_numpy(F), torch.from_numpy(pts), torch.from_numpy(cam),
                          {"joints": torch.from_numpy(np.asarray(root, np.float32)).reshape(1, 1, 3)}, isz, sc)
    ref = torch.nn.functional.linear(lat, torch.from_numpy(w_lat), torch.from_numpy(b)).numpy()
    assert np.abs(emu - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())


def test_edge_points_decide_alike_in_fp32_and_fp64_cpu():
    """The edge cases are exact: the fp32 and fp64 projections agree on every in / out decision - u = +-1 inside, one step beyond
    outside, z = 0 outside (NaN / inf), some points behind the camera inside as in the reference."""
    pts = edge_points()
    uv32, in32 = project(pts, EDGE_CAM, EDGE_ROOT, EDGE_IMAGE, EDGE_SCALE, np.float32)
    uv64, in64 = project(pts, EDGE_CAM, EDGE_ROOT, EDGE_IMAGE, EDGE_SCALE, np.float64)
    assert np.array_equal(in32, in64)
    on_edge = np.isin(np.abs(uv32), [1.0]).any(1)
    assert on_edge.sum() >= 20 and in32[on_edge].all()
    z0 = pts[:, 2] == -1.0
    assert z0.sum() == 3 and not in32[z0].any()
    behind = pts[:, 2] < -1.0
    assert in32[behind].any() and not in32[behind].all()


# ---- the conditions of the cases of tests/test_gpu_pixel_align_fp64.py ----------------------------------------------------------------
def _inexact_cameras():
    _, mano, cam = syn.pixel_align_sample(0)
    return {"sample": (cam, mano["joints"][0, 0]), "skew": (pc.SKEW_CAM, pc.SKEW_ROOT)}


def _forced_gap(F, pts, cam, root, image, scale):
    """|truth with every point decided inside - truth with every point decided outside|, the larger of the two heads, per point."""
    from oracle import sdf_oracle as orc
    specs, _, sd, _, _, _, _ = syn.variant_config("pixelalign")
    specs = dict(specs, SdfScaleFactor=scale, ImageSize=[image, image])
    mano = {"joints": np.tile(np.asarray(root, np.float32).reshape(1, 1, 3), (1, 21, 1))}
    a, b = (orc.decode_points_pixel(sd, F, pts, specs, mano, cam, dtype=torch.float64, inside=np.full(len(pts), side))
            for side in (True, False))
    return np.maximum((a[0] - b[0]).abs().numpy(), (a[1] - b[1]).abs().numpy())


@pytest.mark.parametrize("camera", ["sample", "skew"])
def test_border_points_straddle_the_border_cpu(camera):
    """Adjacent fp32 neighbours on either side of u, v = +-1 under an inexact camera; on the maps the GPU test uses a wrong decision
    costs 1e-3 or more at every one of them.  How often fp32 and fp64 decide differently is printed - it is not zero, which is why
    the truth takes the fp32 decision."""
    cam, root = _inexact_cameras()[camera]
    scale = syn.variant_config("pixelalign")[0]["SdfScaleFactor"]
    pts, kind = pc.border_points(cam, root, 256, scale, 16)
    assert (kind == 0).sum() == (kind == 1).sum() == 64 and (kind == 2).sum() >= 8
    uv, in32 = project(pts, cam, root, 256, scale, np.float32)
    _, in64 = project(pts, cam, root, 256, scale, np.float64)
    last, first = pts[kind == 0], pts[kind == 1]
    moved = last != first
    assert (moved.sum(1) == 1).all()                                    # one coordinate, one fp32 step apart
    step = np.abs(first[moved].view(np.int32).astype(np.int64) - last[moved].view(np.int32).astype(np.int64))
    assert (step == 1).all()
    assert in32[kind == 0].all() and not in32[kind == 1].any()
    on = uv[kind == 2]
    assert in32[kind == 2].all() and (np.abs(on) == 1.0).any(1).all()
    for b in range(4):                                                  # u = 1, u = -1, v = 1, v = -1: 16 pairs each, in order
        edge = uv[kind == 0][16 * b:16 * b + 16, b // 2]
        assert (np.abs(edge - (1.0 if b % 2 == 0 else -1.0)) <= 1e-5).all()
    print("%s camera: fp32 and fp64 decide differently at %d of %d border points" % (camera, int((in32 != in64).sum()), len(pts)))
    for seed, H, W in ((0, 64, 64), (1, 63, 17)):
        assert _forced_gap(syn.pixel_align_sample(seed, H, W)[0], pts, cam, root, 256, scale).min() >= 1e-3


RAMP_SIZES = [(8, 8), (5, 9), (63, 17), (64, 64)]        # tests/test_gpu_pixel_align_fp64.py test_ramp_map_at_the_border_taps


@pytest.mark.parametrize("name,H,W", [("signed_wide", H, W) for H, W in pc.SIZES] + [("ramp", H, W) for H, W in RAMP_SIZES])
def test_exact_edge_points_cannot_hide_a_wrong_decision_cpu(name, H, W):
    """edge_points on every map the GPU tests run them on (signed_wide of every size, the ramp maps): at the points on the border
    and one step beyond it, inside and outside differ by 1e-3 or more - except on the 1 x 1 map, whose only sample IS the channel
    mean."""
    pts = edge_points(W, H=H)
    uv, _ = project(pts, EDGE_CAM, EDGE_ROOT, EDGE_IMAGE, EDGE_SCALE)
    with np.errstate(invalid="ignore"):
        near = (np.abs(np.abs(uv) - 1.0) < 1e-5).any(1) & np.isfinite(uv).all(1)
    assert near.sum() >= 40
    F = pc.signed_wide(H, W) if name == "signed_wide" else pc.ramp(H, W)
    gap = _forced_gap(F, pts[near], EDGE_CAM, EDGE_ROOT, EDGE_IMAGE, EDGE_SCALE)
    assert gap.max() <= 1e-12 if (H, W) == (1, 1) else gap.min() >= 1e-3, (gap.min(), gap.max())


@pytest.mark.parametrize("H,W", pc.SIZES)
def test_pixel_centre_points_cover_every_pixel_cpu(H, W):
    pts = pc.pixel_centre_points(H, W)
    assert len(pts) == H * W + (H - 1) * (W - 1)
    best, w = pc.tap_weights(pts, EDGE_CAM, EDGE_ROOT, EDGE_IMAGE, EDGE_SCALE, H, W)
    covered = {tuple(b) for b in best[w >= 0.5]}
    assert covered == {(r, c) for r in range(H) for c in range(W)}
    assert (w[H * W:] < 0.5).all() and (w[H * W:] > 0.0).all()          # the quad centres: four taps of 0.35 each


def test_maps_are_what_they_say_cpu():
    F = pc.impulse(9, 5, (3, 2))
    assert np.count_nonzero(F) == 256 and len(np.unique(F[0, :, 3, 2])) == 256 and (F[0, :, 3, 2] < 0).any()
    R = pc.ramp(8, 9)[0].astype(np.float64)
    assert np.abs(np.diff(R, 2, axis=1)).max() <= 1e-6 and np.abs(np.diff(R, 2, axis=2)).max() <= 1e-6 and np.ptp(R) > 0.5
    S = np.abs(pc.signed_wide(8, 8)[0])
    assert (pc.signed_wide(8, 8) < 0).mean() > 0.4 and 5e-4 <= S.min() <= 2e-3 and 50.0 <= S.max() <= 100.0


def test_impulse_probe_reaches_every_tap_cpu():
    """The 4 x 4-pixel neighbourhood at quarter-pixel spacing puts the impulse pixel at each of the 16 tap positions."""
    H, W, pixel = 9, 5, (4, 2)
    pts = pc.impulse_probe_points(H, W, pixel)
    uv, inside = project(pts, EDGE_CAM, EDGE_ROOT, EDGE_IMAGE, EDGE_SCALE)
    assert inside.all()
    fx = np.floor((uv[:, 0] + 1) / 2 * (W - 1)).astype(int)
    fy = np.floor((uv[:, 1] + 1) / 2 * (H - 1)).astype(int)
    seen = {(pixel[0] - y + 1, pixel[1] - x + 1) for y, x in zip(fy, fx)}
    assert {(i, j) for i in range(4) for j in range(4)} <= seen


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pixel_align_unit_compiles_without_scratch(tmp_path):
    """csrc/k1pa_kernels.hip is part of the build and its kernel keeps every value in registers (one wave per SIMD)."""
    from alignsdf_amd.build_native import SOURCES, TU_FLAGS
    assert "k1pa_kernels.hip" in SOURCES
    proc = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                           *TU_FLAGS.get("k1pa_kernels.hip", []), "-S", "--cuda-device-only", "k1pa_kernels.hip", "-o",
                           str(tmp_path / "k1pa.s"), "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True,
                          timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", proc.stderr)
    stats = {b.split()[0]: b for b in blocks[1:]}
    k = [b for name, b in stats.items() if "20sdf_mlp_pixel_kernel" in name]
    assert len(k) == 1, list(stats)
    get = lambda key: int(re.search(key + r": (\d+)", k[0]).group(1))
    assert get(r"ScratchSize \[bytes/lane\]") == 0 and get(r"Occupancy \[waves/SIMD\]") == 1
