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
