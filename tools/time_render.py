"""Cost of one ray-cast view (render.render_view / HipSdfDecoder.trace_rays, csrc/k1t_kernels.hip) on one MI355X: grasp9, hand +
object, views of 64^2, 128^2 and 256^2 pixels inside the sample's zoom cube.

    python tools/time_render.py [H ...] [--cube 128] >> profiles/sdf_render.txt

Per view size, by device events, the runs of the forms interleaved (median of ASDF_TIMING_REPS rounds):
  kernel     trace_rays, both heads: ms per view, evaluations per ray (mean, max), ms per million evaluations
  points     decode_points under f32 math over as many evaluations as the view took: ms per million - the chain with every column busy;
             points / kernel = the slot efficiency of the queue
  per-step   the launch-per-step loop: render.trace_lockstep over decode_points (torch state updates, no compaction, one host read per step)
  module     TorchModuleDecoder.trace_rays on the same device
and the sample's own two-pass sweep time at the cube size from the same job."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ.get("ASDF_TREE", "."))
from alignsdf_amd import render as rd, synthetic as syn  # noqa: E402
from alignsdf_amd.networks.model import build_decoder  # noqa: E402
from alignsdf_amd.torch_decoder import TorchModuleDecoder  # noqa: E402
from alignsdf_amd.utils import mesh as mu  # noqa: E402
from alignsdf_amd.utils.utils import bind_sample, decoder_for  # noqa: E402

TAG, SAMPLE = "grasp9", 1
REPS = int(os.environ.get("ASDF_TIMING_REPS", "5"))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("sizes", nargs="*", type=int, default=[64, 128, 256])
    p.add_argument("--cube", type=int, default=128)
    p.add_argument("--no-module", action="store_true")
    args = p.parse_args()
    specs = syn.specs_for(TAG)
    dec = build_decoder(specs, {k: torch.from_numpy(v) for k, v in syn.full_state_dict(TAG).items()}).cuda().eval()
    t = lambda d: None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}
    latent, mano, obj = syn.sample_inputs(TAG, SAMPLE)
    latent, mano, obj = torch.from_numpy(latent), t(mano), t(obj)
    hip = decoder_for(dec, specs, mano)
    mod = TorchModuleDecoder(dec, specs, "timing comparator")
    N = args.cube
    two_pass = lambda: mu.decode_two_pass(True, True, dec, latent, mano, obj, specs, N, mc_only=True)
    r = two_pass()
    ms2 = [timed(two_pass)[0] for _ in range(REPS)]
    lo = [float(v) for v in r["origin"]]
    hi = [v + (N - 1) * float(r["voxel_size"]) for v in lo]
    print("# %s | %s sample %d, hand + object | zoom cube of N = %d: origin %s side %.4f | median of %d interleaved rounds, device events" % (
        torch.cuda.get_device_name(0), TAG, SAMPLE, N, " ".join("%.4f" % v for v in lo), hi[0] - lo[0], REPS))
    print("two-pass sweeps of the sample at N = %d (%s math, no marching cubes): %.2f ms (runs %s)" % (
        N, hip.math, float(np.median(ms2)), " ".join("%.2f" % m for m in ms2)))
    trace = rd.trace_defaults(specs)
    for H in args.sizes:
        W = H
        bind_sample(hip, specs, latent, mano, obj)
        bind_sample(mod, specs, latent, mano, obj)
        cam, root = rd.synthetic_camera_source(H, W)("s", SAMPLE)
        cr = rd.camera_rays(cam, root, specs["SdfScaleFactor"], H, W, lo, hi)
        up = lambda a: torch.from_numpy(a).cuda()
        o, d, t0, t1 = up(cr["origins"]), up(cr["dirs"]), up(cr["t0"]), up(cr["t1"])
        rays = rd.pack_rays(o, d, t0, t1, o.device)
        kernel = lambda: hip.trace_rays(o, d, t0, t1, want_evals=True, **trace)
        res = kernel()
        ev = torch.cat([res["hand"]["evals"], res["obj"]["evals"]]).cpu().numpy()
        E = int(ev.sum())
        pts = (torch.rand(max(E // 2, 1), 3, device="cuda") * (hi[0] - lo[0]) + torch.tensor(lo, device="cuda")).contiguous()
        before = hip.math
        hip.set_math("f32")

        def per_step():
            return [rd.trace_lockstep(lambda q, k=k: hip.decode_points(q)[k], rays, **trace) for k in (0, 1)]
        forms = [("kernel", kernel), ("points", lambda: hip.decode_points(pts)), ("per-step", per_step)]
        if not args.no_module:
            forms.append(("module", lambda: mod.trace_rays(o, d, t0, t1, **trace)))
        ms = {name: [] for name, _ in forms}
        out = {}
        for name, fn in forms:
            fn()                                   # warm-up
        for _ in range(REPS):
            for name, fn in forms:
                m, out[name] = timed(fn)
                ms[name].append(m)
        hip.set_math(before)
        med = {name: float(np.median(v)) for name, v in ms.items()}
        same = all(torch.equal(out["per-step"][k]["t"], out["kernel"][n]["t"]) for k, n in enumerate(("hand", "obj")))
        hits = {n: int((res[n]["status"] == rd.HIT).sum()) for n in ("hand", "obj")}
        spent = {n: int((res[n]["status"] == rd.EXHAUSTED).sum()) for n in ("hand", "obj")}
        print("%dx%d: %d rays, %d in the cube | HIT hand %d obj %d, EXHAUSTED hand %d obj %d | evaluations per ray and head: mean %.1f max %d, %.3f M in all" % (
            H, W, H * W, int((cr["t0"] <= cr["t1"]).sum()), hits["hand"], hits["obj"], spent["hand"], spent["obj"], ev.mean(), ev.max(), 1e-6 * E))
        for name, _ in forms:
            print("%dx%d %-9s %8.3f ms per view  (runs %s)" % (H, W, name, med[name], " ".join("%.3f" % m for m in ms[name])))
        print("%dx%d kernel %.3f ms per M evaluations, decode_points (f32) %.3f ms per M evaluations at the same count: slot efficiency %.2f" % (
            H, W, 1e6 * med["kernel"] / E, 1e6 * med["points"] / E, med["points"] / med["kernel"]))
        print("%dx%d kernel against the per-step loop: %.2f x (t of both heads bit-equal: %s)%s; against the two-pass sweeps: %.1f %% of their time" % (
            H, W, med["per-step"] / med["kernel"], same, "" if args.no_module else "; against the module path: %.1f x" % (med["module"] / med["kernel"]),
            100.0 * med["kernel"] / float(np.median(ms2))))


if __name__ == "__main__":
    main()
