"""Cost of fitting B samples in one stream of launches (fit.fit_codes -> HipSdfDecoder.fit_codes -> asdf_fit_codes) against B consecutive
one-sample fits (fit.fit_code, the way before the batched call), and the autodecode flow with --batch 1 and --batch 8.

  1. B in {1, 2, 4, 8, 16, 32} samples of M in {1024, 4096, 8192, 32000} targets each (half per head, both heads: the decoder's own
     fields at another code; every sample its own points, code and embedding), STEPS steps, wall time of the whole call after a
     warm-up call, the two ways interleaved, median of REPS rounds.  Both include their one wait at the end.  Printed per cell: ms per
     sample-step of each way (with its fastest and slowest round) and their ratio, and sum_s grid_s of the batched launch against the
     part's compute units.
  2. autodecode.run with autodecode.DeviceFitter on eight grasp scenes (meshes by marching cubes of the grasp3 decoder's own fields at
     N = 64), 800 steps, at 8000 targets per sample (3000 + 1000 per head) and at the defaults (12000 + 4000 per head): wall time per
     sample with --batch 1 and --batch 8 (median and range of FLOW_REPS interleaved runs), and the host share of it (meshes read, sampled and valued; measured on its own).

    python tools/time_fit_codes.py [--label "<commit>"] > profiles/fit_codes.txt"""
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

REPS = int(os.environ.get("ASDF_TIMING_REPS", "3"))
STEPS = int(os.environ.get("ASDF_TIMING_STEPS", "100"))
BATCHES = tuple(int(b) for b in os.environ.get("ASDF_TIMING_BATCHES", "1,2,4,8,16,32").split(","))
LENGTHS = tuple(int(m) for m in os.environ.get("ASDF_TIMING_LENGTHS", "1024,4096,8192,32000").split(","))
SCENES = 8
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
    p.add_argument("--skip-flow", action="store_true")
    args = p.parse_args()
    from alignsdf_amd import autodecode as ad
    from alignsdf_amd.fit import fit_code, fit_codes, kinematic_affine_torch
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.marching_cubes import marching_cubes_device
    from alignsdf_amd.utils.mesh import lattice_points
    from alignsdf_amd.utils.utils import bind_sample
    t = lambda d: None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("# tools/time_fit_codes.py | %s | %s, %d compute units | %d steps per call, median of %d interleaved rounds, wall time" % (
        args.label, torch.cuda.get_device_name(0), num_cus, STEPS, REPS))
    tag = "grasp9"
    specs = syn.specs_for(tag)
    hip = HipSdfDecoder(module_for(tag))
    rule = dict(steps=STEPS, lr=5e-3, decay=1.0, every=1, prior=1e-4, clamp=0.05)
    for M in LENGTHS:
        items = []
        for s in range(max(BATCHES)):
            latent, mano, obj = syn.sample_inputs(tag, s)
            other = torch.from_numpy(syn.sample_inputs(tag, s + 1)[0])
            E = tuple(e.float() for e in kinematic_affine_torch(specs["PointFeatSize"], specs["EncodeStyle"], specs["SdfScaleFactor"], t(mano), t(obj)))
            x = torch.from_numpy(np.random.default_rng(1000 * s + M).uniform(-1, 1, (M // 2, 3)).astype(np.float32)).cuda()
            bind_sample(hip, specs, other.reshape(1, -1), t(mano), t(obj))
            before = hip.math
            hip.set_math("f32")
            sh, so = (v.clone() for v in hip.decode_points(x))
            hip.set_math(before)
            items.append({"latent": torch.from_numpy(latent).reshape(-1), "embed": E, "sdf_hand": (x, sh), "sdf_obj": (x, so)})
        grid = min((M + 127) // 128, num_cus)
        for B in BATCHES:
            batch = items[:B]
            ways = {"loop": lambda: [fit_code(hip, it["latent"], it["embed"], sdf_hand=it["sdf_hand"], sdf_obj=it["sdf_obj"], **rule) for it in batch],
                    "batch": lambda: fit_codes(hip, batch, **rule)}
            outs = {name: fn() for name, fn in ways.items()}          # warm-up: first-use allocations, the step table's upload
            same = all(torch.equal(outs["batch"][0][s], outs["loop"][s][0]) and torch.equal(outs["batch"][1][s], outs["loop"][s][1]) for s in range(B))
            times = {k: [] for k in ways}
            for _ in range(REPS):
                for k, fn in ways.items():
                    times[k].append(wall(fn) / (STEPS * B))
            med = {k: float(np.median(v)) for k, v in times.items()}
            print("M=%-6d B=%-3d fit_code x B %.4f (%.4f .. %.4f) ms / sample-step | fit_codes %.4f (%.4f .. %.4f) ms / sample-step | ratio %.2f x | "
                  "workgroups %5d of %d compute units (%.2f rounds) | bits equal: %s" % (
                      M, B, med["loop"], min(times["loop"]), max(times["loop"]), med["batch"], min(times["batch"]), max(times["batch"]),
                      med["loop"] / med["batch"], B * grid, num_cus, B * grid / num_cus, same))
            sys.stdout.flush()
    hip.close()
    if args.skip_flow:
        return

    tag, N = "grasp3", 64
    specs, module = syn.specs_for(tag), module_for(tag)
    hip = HipSdfDecoder(module)
    origin, voxel = [-1.0, -1.0, -1.0], 2.0 / (N - 1)
    idx = torch.stack(torch.meshgrid(*[torch.arange(N, dtype=torch.float32, device="cuda")] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = lattice_points(idx, origin, voxel)
    with tempfile.TemporaryDirectory() as root:
        for sample in range(SCENES):
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
        hip.close()
        pairs = ad.discover(root, "obman")
        for near, uniform in ((3000, 1000), (ad.SAMPLE_DEFAULTS["near"], ad.SAMPLE_DEFAULTS["uniform"])):
            fitter = ad.DeviceFitter(module, specs, sampling={"near": near, "uniform": uniform})
            ad.run(specs, fitter, "obman", root, os.path.join(root, "warm"), end=2, batch=2)
            ad.run(specs, fitter, "obman", root, os.path.join(root, "warm"), end=1)
            host = wall(lambda: [fitter._prepare(h, o, {}, np.zeros(256, np.float32)) for _, h, o in pairs]) / len(pairs)
            per, files = {}, {}
            runs = {1: [], 8: []}
            for _ in range(FLOW_REPS):
                for batch in (1, 8):
                    out = os.path.join(root, "codes_%d_%d" % (near, batch))
                    t0 = time.perf_counter()
                    _, records = ad.run(specs, fitter, "obman", root, out, batch=batch)
                    runs[batch].append(1e3 * (time.perf_counter() - t0) / len(records))
                    files[batch] = [open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out))]
            per = {batch: float(np.median(v)) for batch, v in runs.items()}
            print("autodecode flow: %d grasp3 scenes, %d steps, %d + %d samples per head (%d targets per sample): --batch 1 %.1f (%.1f .. %.1f) ms "
                  "per sample, --batch 8 %.1f (%.1f .. %.1f) ms per sample (%.2f x), of which the host's share (meshes read, sampled and valued) "
                  "%.1f ms per sample; files byte-identical: %s; %s" % (
                      len(records), records[0]["steps"], near, uniform, 2 * (near + uniform), per[1], min(runs[1]), max(runs[1]), per[8], min(runs[8]),
                      max(runs[8]), per[1] / per[8], host, files[1] == files[8], ad.summary_line(records)))
            sys.stdout.flush()


if __name__ == "__main__":
    main()
