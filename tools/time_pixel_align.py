"""Per-sample time of the two-pass flow (utils.mesh.decode_two_pass: coarse sweep, zoom cube, fine sweep) for a PixelAlign decoder
with a 64 x 64 feature map, three ways: the native pixel-aligned kernel (decoder_for(..., pixel_align="native")), the module path
(the default), and - as the floor - the fp32 chain (math "f32") on the same decoder without PixelAlign.  One JSON line per
(N, way): milliseconds per sample (median of --reps, each synchronised), and the bind (set_sample*) share of it.

    python tools/time_pixel_align.py --n 128 256 --reps 5
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ways", nargs="+", default=["native", "module", "floor"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from alignsdf_amd import synthetic as syn
    from alignsdf_amd.networks import model as arch
    from alignsdf_amd.utils.mesh import decode_two_pass
    from alignsdf_amd.utils.utils import decoder_for

    specs, cls, sd, _, _, _, _ = syn.variant_config("pixelalign")
    dec = getattr(arch, cls)(specs["LatentSize"], specs["PointFeatSize"], specs["EncodeStyle"], **specs["NetworkSpecs"]).eval().cuda()
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    feat, mano, cam = syn.pixel_align_sample(0)
    feat = torch.from_numpy(feat).cuda()
    mano = {k: torch.from_numpy(v) for k, v in mano.items()}
    cam = torch.from_numpy(cam)
    plain = dict(specs, PixelAlign=False)
    latent = feat.mean(3).mean(2).reshape(-1)          # the floor's latent: any code of the right size

    for N in args.n:
        for way in args.ways:
            if way == "floor":
                ev = decoder_for(dec, plain, mano)
                ev.set_math("f32")
                run = lambda: decode_two_pass(True, True, ev, latent, mano, None, plain, N)
            else:
                ev = decoder_for(dec, specs, mano, pixel_align=way)
                run = lambda: decode_two_pass(True, True, ev, feat, mano, None, specs, N, cam_intr=cam)
            run()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                r = run()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            rec = {"N": N, "way": way, "evaluator": type(ev).__name__, "ms_per_sample_median": float(np.median(times)),
                   "ms_min": float(np.min(times)), "reps": args.reps, "neg_voxels_fine": [int((r["vol_hand"] < 0).sum()), int((r["vol_obj"] < 0).sum())]}
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
