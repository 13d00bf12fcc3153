"""CPU side of the ray-tracing feature: the conditions of the GPU tests' ray sets on the fp64 truth alone, the rule in fp32 against
fp64 (the figures of profiles/sdf_trace_fp64_errors.txt), trace_refusal, camera_rays, TorchModuleDecoder.trace_rays against the numpy
statement of the rule, the _render.npz layout, and the compile-time budget of the tracing kernel (csrc/k1t_kernels.hip)."""
import os
import re
import subprocess
import weakref

import numpy as np
import pytest
import torch

from alignsdf_amd import synthetic as syn
from tests import sdf_trace_cases as tc

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alignsdf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEADS = ("hand", "obj")
SETS = [(tag, M, "M=%d" % M) for tag, M in tc.TRUTH_SETS] + [(tc.VIEW["tag"], "view", "view")]


def test_ray_sets_of_the_gpu_tests_are_decided_enough():
    """The condition of tests/test_gpu_sdf_trace.py, on the truth alone: at least 90 % of the rays of every head of every set are
    DECIDED at 1e-5 and every head has at least 50 HITs.  Measured: see profiles/sdf_trace_fp64_errors.txt."""
    for tag, key, label in SETS:
        truth = tc.trace_truth(tag, tc.SAMPLE, key)
        for name in HEADS:
            share, status = tc.decided(truth[name]).mean(), truth[name]["status"]
            print("SDFTRACE condition %s %s %s: decided %.3f HIT %d MISS %d INSIDE %d EXHAUSTED %d evals mean %.1f max %d" % (
                tag, label, name, share, (status == tc.HIT).sum(), (status == tc.MISS).sum(), (status == tc.INSIDE).sum(),
                (status == tc.EXHAUSTED).sum(), truth[name]["evals"].mean(), truth[name]["evals"].max()))
            assert share >= tc.MIN_DECIDED_SHARE and (status == tc.HIT).sum() >= tc.MIN_HITS, (tag, label, name, share)
            assert truth[name]["evals"].max() <= tc.RULE["max_steps"] + tc.RULE["refine_steps"] + 1


def test_fp32_rule_against_fp64_on_the_decided_rays():
    """The oracle's decoder in torch fp32 against fp64 under the same fp32 rule: the same status on every DECIDED ray, and the largest
    |dt| over DECIDED HITs per set and head - the figure profiles/sdf_trace_fp64_errors.txt records (`cpu <set> <head> ... max_dt`),
    which the GPU test takes 4 x of as the kernel's bound (one line per set and head: sdf_trace_cases.recorded refuses a file with
    none or several).  ASDF_RECORD_TRACE_ERRORS=1 puts this run's figures in their place; without it the run is held to 4 x the
    recorded ones (another CPU's fp32 GEMM sums in another order, as the kernel does)."""
    lines = []
    for tag, key, label in SETS:
        t64, t32 = tc.trace_truth(tag, tc.SAMPLE, key), tc.trace_truth(tag, tc.SAMPLE, key, torch.float32)
        for name in HEADS:
            ok = tc.decided(t64[name])
            assert np.array_equal(t32[name]["status"][ok], t64[name]["status"][ok]), (tag, label, name)
            hits = ok & (t64[name]["status"] == tc.HIT)
            e = float(np.abs(t32[name]["t"][hits].astype(np.float64) - t64[name]["t"][hits]).max())
            lines.append("cpu %s %s %s decided %.3f hits %d max_dt %.3e" % ("view" if label == "view" else tag, name, label, ok.mean(), hits.sum(), e))
            print("SDFTRACE", lines[-1])
            if not os.environ.get("ASDF_RECORD_TRACE_ERRORS"):
                assert e <= 4.0 * tc.recorded("cpu", "view" if label == "view" else tag, name), (tag, label, name, e)
    if os.environ.get("ASDF_RECORD_TRACE_ERRORS"):
        tc.record(lines)


def test_trace_refusal():
    from alignsdf_amd.hip_decoder import grad_refusal, trace_refusal
    for tag in ("nerf3", "both9", "hand6", "obj6", "grasp3", "grasp9", "bothcls9"):
        specs = syn.specs_for(tag)
        assert trace_refusal(False, specs["PointFeatSize"], specs["EncodeStyle"], False) is None, tag
    for tag in ("nerf9", "nerf15"):
        specs = syn.specs_for(tag)
        assert isinstance(trace_refusal(False, specs["PointFeatSize"], specs["EncodeStyle"], False), str), tag
    assert isinstance(trace_refusal(True, 3, "nerf", False), str)          # comb3
    assert isinstance(trace_refusal(False, 3, "nerf", True), str)          # pixel-aligned
    assert "gradient" in grad_refusal(True, 3, "nerf", False)              # (the gradient kernel's own table is as it was)


def _project(x, cam, root, scale):
    """pixel_alignment's formula in fp64: normalised point -> pixel."""
    x_cam = x * 2.0 / scale + root
    h = x_cam @ np.asarray(cam, np.float64).reshape(3, -1)[:, :3].T
    return h[:, :2] / h[:, 2:3]


def test_camera_rays():
    from alignsdf_amd.render import camera_rays, scale_intrinsics, tile_order
    cam = np.array([[[401.3, 3.7, 131.2, 0.0], [-0.9, 397.6, 124.9, 0.0], [0.002, -0.001, 1.0, 0.0]]])       # skewed, 3 x 4, batch axis
    root, scale = np.array([-0.021, 0.034, 0.61]), syn.SDF_SCALE_DEXYCB
    for H, W in ((19, 35), (16, 8), (8, 16), (1, 1), (256, 256)):
        k = scale_intrinsics(cam, W / 256.0, H / 256.0)
        cr = camera_rays(k, root, scale, H, W, (-1, -1, -1), (1, 1, 1))
        order, inverse = cr["order"], cr["inverse"]
        assert np.array_equal(np.sort(order), np.arange(H * W)) and np.array_equal(order[inverse], np.arange(H * W))
        assert np.array_equal(inverse[order], np.arange(H * W))
        assert cr["origins"].dtype == np.float32 and cr["origins"].shape == (H * W, 3) and cr["t0"].shape == (H * W,)
        assert np.abs(np.linalg.norm(cr["dirs"].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
        # points along a ray project back to the centre of its pixel
        i, j = order // W, order % W
        for t in (0.3, 1.7, 4.0):
            uv = _project(cr["origins"].astype(np.float64) + t * cr["dirs"].astype(np.float64), k, root, scale)
            assert np.abs(uv - np.stack([j + 0.5, i + 0.5], 1)).max() <= 2e-4 * max(H, W) / 256.0 + 2e-5, (H, W, t)
        # camera-space z per unit of t
        x = cr["origins"].astype(np.float64) + 2.0 * cr["dirs"]
        assert np.abs((x * 2.0 / scale + root)[:, 2] - 2.0 * cr["z_per_t"]).max() <= 1e-6
        # the segment is the part of the ray inside the box
        seen = cr["t0"] <= cr["t1"]
        assert seen.any()
        for t, inside in ((cr["t0"] + 1e-4, True), (cr["t1"] - 1e-4, True), (cr["t1"] + 1e-3, False)):
            p = cr["origins"][seen].astype(np.float64) + t[seen, None].astype(np.float64) * cr["dirs"][seen]
            assert ((np.abs(p) <= 1.0 + 1e-5).all(1) == inside).all()
    # tiles: the first 128 rays of a 32 x 32 view are its top-left 16 x 8 pixels, row-major
    order, _ = tile_order(32, 32)
    assert np.array_equal(order[:128], (np.arange(8)[:, None] * 32 + np.arange(16)[None, :]).reshape(-1))
    assert np.array_equal(order[128:256] % 32, np.tile(np.arange(16, 32), 8))
    # a box behind the camera: no ray sees it
    cr = camera_rays(cam, root, scale, 16, 16, (-0.5, -0.5, -9.0), (0.5, 0.5, -8.0))
    assert (cr["t0"] > cr["t1"]).all()
    # a projection with a translation column is not this camera model
    bad = cam.copy()
    bad[0, 0, 3] = 2.1
    with pytest.raises(ValueError):
        camera_rays(bad, root, scale, 4, 4, (-1, -1, -1), (1, 1, 1))


def _cpu_module_decoder(tag):
    """TorchModuleDecoder on the CPU: the class refuses to be constructed without a GPU (there is no CPU product path), the rule it runs
    is device independent."""
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    module = tc.module_for(tag)
    dec = TorchModuleDecoder.__new__(TorchModuleDecoder)
    dec.device, dec._module_ref, dec._copy, dec.specs, dec.reason = torch.device("cpu"), weakref.ref(module), None, syn.specs_for(tag), "test"
    dec.num_class, dec._sample = 0, None
    latent, mano, obj = syn.sample_inputs(tag, tc.SAMPLE)
    t = lambda d: None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}
    dec.set_sample(torch.from_numpy(latent), t(mano), t(obj))
    return dec


@pytest.mark.parametrize("tag,rule", [("grasp9", {}), ("both9", {"refine_steps": 0, "max_steps": 7}), ("nerf9", {"step_scale": 0.8})])
def test_module_path_trace_is_the_rule_bit_for_bit(tag, rule):
    """TorchModuleDecoder.trace_rays (torch, all rays in lockstep under masks) against `march` over the same module's decode_points:
    t, status, bracket and evals of every ray, both heads - including nerf9, which the kernel refuses."""
    dec = _cpu_module_decoder(tag)
    rays = tc.ray_set(97)
    rays[5, 6], rays[5, 7] = 1.0, 0.0
    rays[11, 1] = np.nan
    rays[17, 7] = rays[17, 6]
    rule = dict(tc.RULE, **rule)
    r = torch.from_numpy(rays)
    got = dec.trace_rays(r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7], want_bracket=True, want_evals=True, **rule)
    for k, name in enumerate(HEADS):
        want = tc.march(lambda pts, k=k: dec.decode_points(torch.from_numpy(pts))[k].numpy(), rays, full=True, **rule)
        for key in ("t", "status", "bracket", "evals"):
            g, w = got[name][key].numpy(), want[key]
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                                                         w.view(np.uint32) if w.dtype == np.float32 else w), (tag, name, key)
        assert want["status"][5] == tc.MISS and want["evals"][5] == 0 and want["evals"][11] == 0 and want["evals"][17] == 1
        assert len(np.unique(want["status"])) >= 2
    assert set(dec.trace_rays(r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7], obj=False)["hand"]) == {"t", "status"}


def test_render_npz_layout_and_render_without_a_camera(tmp_path):
    from alignsdf_amd import reconstruct as rc
    from alignsdf_amd.render import VIEW_MAPS, VIEW_STATS, render_view, save_view, synthetic_camera_source, trace_defaults
    tag, H, W = "grasp9", 12, 8
    specs = syn.specs_for(tag)
    dec = _cpu_module_decoder(tag)
    trace = trace_defaults(dict(specs, ClampingDistance=0.04))
    assert trace["max_step"] == 0.04 and trace_defaults(specs)["max_step"] == 0.05
    cam, root = synthetic_camera_source(H, W)("a", 0)
    view = render_view(dec, cam, root, specs["SdfScaleFactor"], H, W, box=tc.BOX, **trace)
    path = str(tmp_path / "meshes" / "a_render.npz")
    save_view(path, view, H, W, trace)
    with np.load(path) as z:
        assert set(z.files) == set(VIEW_MAPS) | set(VIEW_STATS) | {"H", "W"} | set(trace)
        assert int(z["H"]) == H and int(z["W"]) == W and float(z["max_step"]) == 0.04 and int(z["refine_steps"]) == 6
        for name in HEADS:
            assert z["depth_" + name].shape == (H, W) and z["depth_" + name].dtype == np.float32
            assert z["status_" + name].shape == (H, W) and z["status_" + name].dtype == np.int32
            hit = z["status_" + name] == tc.HIT
            assert np.isinf(z["depth_" + name][~hit]).all() and (z["depth_" + name][hit] > 0).all()
        part, normal = z["part"], z["normal"]
        assert part.dtype == np.uint8 and part.shape == (H, W) and normal.shape == (H, W, 3) and (part != 0).any()
        nearer = np.where(z["depth_hand"] <= z["depth_obj"], 1, 2)
        assert np.array_equal(part[part != 0], nearer[part != 0]) and np.array_equal(part == 0, np.isinf(np.minimum(z["depth_hand"], z["depth_obj"])))
        length = np.linalg.norm(normal.astype(np.float64), axis=2)
        assert np.abs(length[part != 0] - 1.0).max() <= 1e-5 and (normal[part == 0] == 0).all()
        assert float(z["evals_mean"]) > 1.0 and int(z["exhausted_hand"]) >= 0
    # --render without a camera: an error before anything is loaded or swept
    with pytest.raises(ValueError, match="camera_source"):
        rc.reconstruct(None, specs, str(tmp_path / "no_such_split.json"), str(tmp_path / "out"), 0, 1, render=(8, 8))
    assert not os.path.exists(str(tmp_path / "out"))
    with pytest.raises(SystemExit):
        rc.main(["-e", str(tmp_path / "no_such_model"), "--render", "8x8"])
    with pytest.raises(SystemExit):
        rc.main(["-e", str(tmp_path / "no_such_model"), "--synthetic", "--render", "8by8"])
    assert not os.path.exists(str(tmp_path / "no_such_model"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_tracing_kernel_budget(tmp_path):
    """The budget of its siblings (tests/test_sdf_grad_truth.py for k1g): __launch_bounds__(256, 1), no scratch, one wave per SIMD -
    from the compiler's resource report and the kernel's metadata, with the per-unit flags of the shipped build; the kernel's
    instructions are not read.  The registers are recorded, not pinned."""
    from alignsdf_amd.build_native import FLAGS, SOURCES, TU_FLAGS
    assert "k1t_kernels.hip" in SOURCES
    out = str(tmp_path / "k1t.s")
    proc = subprocess.run([HIPCC, *FLAGS, *TU_FLAGS.get("k1t_kernels.hip", []), "-S", "--cuda-device-only", "k1t_kernels.hip", "-o", out,
                           "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    block = [b for b in re.split(r"remark: Function Name: ", proc.stderr)[1:] if "20sdf_mlp_trace_kernelE" in b.split()[0]]
    assert len(block) == 1
    get = lambda key: int(re.search(key + r": (\d+)", block[0]).group(1))
    print("K1T resources: VGPRs %d AGPRs %d scratch %d occupancy %d" % (get("VGPRs"), get("AGPRs"), get(r"ScratchSize \[bytes/lane\]"),
                                                                       get(r"Occupancy \[waves/SIMD\]")))
    assert get(r"ScratchSize \[bytes/lane\]") == 0 and get(r"Occupancy \[waves/SIMD\]") >= 1
    with open(out) as fh:
        text = fh.read()
    assert re.search(r"\.max_flat_workgroup_size:\s+256", text[text.index("amdhsa.kernels"):]), "__launch_bounds__(256, 1)"
