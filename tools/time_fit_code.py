"""Per-step cost of the device-resident fit (fit.fit_code -> HipSdfDecoder.fit_code -> asdf_fit_code) against fit_sample's Python loop
(one autograd round trip and one torch.optim.Adam step per iteration; unchanged from the commit before the device loop), and the
per-sample time of the autodecode flow.

  1. M in {1024, 16384} targets (half per head, both heads: the decoder's own fields at another code), STEPS steps, wall time per
     step after a warm-up call, the two loops interleaved, median of REPS rounds and fit_code's fastest and slowest round.  fit_code's
     time includes the one wait at its end.
  2. autodecode.DeviceFitter on two grasp scenes (meshes by marching cubes of the grasp3 decoder's own fields at N = 64), the
     flow's defaults (800 steps, 12000 + 4000 samples per head): wall time per sample, mesh loading and sampling included, median
     and range of FLOW_REPS runs.

    python tools/time_fit_code.py [--label "<commit>"] > profiles/fit_code.txt"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.environ.get("ASDF_TREE", "."))
from alignsdf_amd import synthetic as syn  # noqa: E402
from alignsdf_amd.networks.model import build_decoder  # noqa: E402

REPS = int(os.environ.get("ASDF_TIMING_REPS", "5"))
STEPS = int(os.environ.get("ASDF_TIMING_STEPS", "100"))
FLOW_REPS = int(os.environ.get("ASDF_TIMING_FLOW_REPS", "3"))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def module_for(tag):
    return build_decoder(syn.specs_for(tag), {k: torch.from_numpy(v) for k, v in syn.full_state_dict(tag).items()}).eval()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--label", default="this tree")
    args = p.parse_args()
    from alignsdf_amd import autodecode as ad
    from alignsdf_amd.fit import fit_code, fit_sample, kinematic_affine_torch
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.marching_cubes import marching_cubes_device
    from alignsdf_amd.utils.mesh import lattice_points
    from alignsdf_amd.utils.utils import bind_sample
    t = lambda d: None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}
    print("# tools/time_fit_code.py | %s | %s | %d steps per call, median of %d interleaved rounds, wall time" % (
        args.label, torch.cuda.get_device_name(0), STEPS, REPS))
    tag = "grasp9"
    specs = syn.specs_for(tag)
    hip = HipSdfDecoder(module_for(tag))
    latent, mano, obj = syn.sample_inputs(tag, 3)
    other = torch.from_numpy(syn.sample_inputs(tag, 4)[0]).reshape(-1)
    E = tuple(e.float() for e in kinematic_affine_torch(specs["PointFeatSize"], specs["EncodeStyle"], specs["SdfScaleFactor"], t(mano), t(obj)))
    z0 = torch.from_numpy(latent).reshape(-1)
    for M in (1024, 16384):
        x = torch.from_numpy(np.random.default_rng(M).uniform(-1, 1, (M // 2, 3)).astype(np.float32)).cuda()
        bind_sample(hip, specs, other.reshape(1, -1), t(mano), t(obj))
        before = hip.math
        hip.set_math("f32")
        sh, so = (v.clone() for v in hip.decode_points(x))
        hip.set_math(before)
        kw = dict(sdf_hand=(x, sh), sdf_obj=(x, so), steps=STEPS, clamp=0.05)
        loops = {"fit_sample": lambda: fit_sample(hip, z0, E, lr=5e-3, prior=1e-4, **kw),
                 "fit_code": lambda: fit_code(hip, z0, E, lr=5e-3, decay=1.0, every=1, prior=1e-4, **kw)}
        ends = {}
        for name, fn in loops.items():          # warm-up: first-use allocations, the optimizer's and autograd's own set-up
            out = fn()
            ends[name] = (float(out[-1][0]), float(out[-1][-1]))
        times = {k: [] for k in loops}
        for _ in range(REPS):
            for k, fn in loops.items():
                times[k].append(wall(fn) / STEPS)
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("M=%-6d fit_sample %.3f ms / step | fit_code %.4f ms / step (rounds %.4f .. %.4f) | fit_sample / fit_code %.2f x | data term "
              "fit_sample %.3e -> %.3e, fit_code %.3e -> %.3e" % (M, med["fit_sample"], med["fit_code"], min(times["fit_code"]), max(times["fit_code"]),
                                                                   med["fit_sample"] / med["fit_code"], *ends["fit_sample"], *ends["fit_code"]))
    hip.close()

    tag, N = "grasp3", 64
    specs, module = syn.specs_for(tag), module_for(tag)
    hip = HipSdfDecoder(module)
    origin, voxel = [-1.0, -1.0, -1.0], 2.0 / (N - 1)
    idx = torch.stack(torch.meshgrid(*[torch.arange(N, dtype=torch.float32, device="cuda")] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = lattice_points(idx, origin, voxel)
    with tempfile.TemporaryDirectory() as root:
        names = []
        for sample in (3, 7):
            hip.set_sample(torch.from_numpy(syn.sample_inputs(tag, sample)[0]))
            hip.set_math("f32")
            for part, vol in zip(("hand", "obj"), hip.decode_points(pts)):
                v, f = marching_cubes_device(vol.reshape(N, N, N).contiguous(), 0.0)
                xyz = ad.from_decoder_frame(lattice_points(v, origin, voxel).cpu().numpy(), 1.0, (0, 0, 0), specs["SdfScaleFactor"])
                path = os.path.join(root, "obman", "test", "mesh_" + part, "%08d.obj" % sample)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                with open(path, "w") as fh:
                    fh.writelines("v %.9g %.9g %.9g\n" % tuple(r) for r in xyz)
                    fh.writelines("f %d %d %d\n" % tuple(int(i) + 1 for i in r) for r in f.cpu().numpy())
            names.append("%08d" % sample)
        hip.close()
        fitter = ad.DeviceFitter(module, specs)
        ad.run(specs, fitter, "obman", root, os.path.join(root, "warm"), end=1)
        per = []
        for _ in range(FLOW_REPS):
            t0 = time.perf_counter()
            _, records = ad.run(specs, fitter, "obman", root, os.path.join(root, "codes"))
            per.append(1e3 * (time.perf_counter() - t0) / len(records))
        print("autodecode flow: %d grasp3 scenes, %d steps, %d + %d samples per head: %.1f ms per sample (runs %.1f .. %.1f; wall, meshes read and "
              "sampled, code written); %s" % (len(records), records[0]["steps"], ad.SAMPLE_DEFAULTS["near"], ad.SAMPLE_DEFAULTS["uniform"],
                                              float(np.median(per)), min(per), max(per), ad.summary_line(records)))


if __name__ == "__main__":
    main()
