"""Cost of vertex normals (reconstruct(normals=True)) in the files flow that tools/time_reconstruct_files.py times: ms per sample with
and without normals, interleaved, and the gradient launches (HipSdfDecoder.decode_points_grad over one sample's kept vertices) on
their own, by device events.  grasp9 (trained decoders, kinematic embedding), hand + object, N = 128 and 256.

    python tools/time_normals.py [N ...] [--samples 6] [--label TEXT] >> profiles/sdf_grad_normals.txt

--plain-only times the flow without normals only (it then runs on a tree that does not know the option: the figure of the commit
before, taken on the same box in the same job)."""
import argparse
import glob
import json
import os
import sys
import tempfile
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.environ.get("ASDF_TREE", "."))
from alignsdf_amd import reconstruct as rc, synthetic as syn  # noqa: E402
from alignsdf_amd.networks.model import build_decoder  # noqa: E402

TAG = "grasp9"
REPS = int(os.environ.get("ASDF_TIMING_REPS", "5"))


class ShaderClock:
    """Samples the shader clock the driver reports (sysfs hwmon, read only) every 10 ms while the timed runs are in flight: the
    reading of an idle GPU says nothing about the clock the work ran at."""

    def __init__(self):
        self.paths = sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq1_input"))
        self.samples, self.stop = [], threading.Event()
        self.thread = threading.Thread(target=self.run, daemon=True)

    def run(self):
        while not self.stop.wait(0.01):
            try:
                self.samples.append(max(int(open(p).read()) for p in self.paths) * 1e-6)
            except (OSError, ValueError):
                pass

    def __enter__(self):
        if self.paths:
            self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        if self.paths:
            self.thread.join()

    def __str__(self):
        if not self.samples:
            return "not available"
        a = np.array(self.samples)
        return "median %.0f MHz, max %.0f MHz (%d samples; the busiest of the cards this process can see)" % (np.median(a), a.max(), len(a))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("sizes", nargs="*", type=int, default=[128, 256])
    p.add_argument("--samples", type=int, default=6)
    p.add_argument("--label", default="this tree")
    p.add_argument("--plain-only", action="store_true")
    args = p.parse_args()
    specs = syn.specs_for(TAG)
    dec = build_decoder(specs, {k: torch.from_numpy(v) for k, v in syn.full_state_dict(TAG).items()})
    tmp = tempfile.mkdtemp()
    split = os.path.join(tmp, "split.json")
    n = args.samples
    json.dump({"filenames": ["x/%08d.jpg" % i for i in range(n + 1)]}, open(split, "w"))
    src = rc.synthetic_code_source(TAG)
    print("# %s | %s | %s, hand + object, %d samples per run, median of %d interleaved runs" % (
        args.label, torch.cuda.get_device_name(0), TAG, n, REPS))
    for N in args.sizes:
        variants = [("without normals", {})] + ([] if args.plain_only else [("with normals", {"normals": True})])
        for _, kw in variants:                                             # warm-up of both forms
            rc.reconstruct(dec, specs, split, tmp, 0, 2, cube_dim=N, code_source=src, **kw)
        runs = {name: [] for name, _ in variants}
        recs = {}
        with ShaderClock() as clock:
            for _ in range(REPS):
                for name, kw in variants:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    recs[name] = rc.reconstruct(dec, specs, split, tmp, 1, n + 1, cube_dim=N, code_source=src, **kw)
                    torch.cuda.synchronize()
                    runs[name].append(1e3 * (time.perf_counter() - t) / n)
        med = {name: float(np.median(r)) for name, r in runs.items()}
        for name, _ in variants:
            print("N=%d files flow %-16s %7.2f ms/sample  (runs: %s)" % (N, name, med[name], " ".join("%.1f" % r for r in runs[name])))
        print("N=%d shader clock during the runs: %s" % (N, clock))
        if args.plain_only:
            continue
        extra = med["with normals"] - med["without normals"]
        print("N=%d normals cost %.2f ms/sample = %.1f %% of the sample; degenerate normals of the last sample: hand %d obj %d" % (
            N, extra, 100.0 * extra / med["without normals"], recs["with normals"][-1]["normals_degenerate_hand"],
            recs["with normals"][-1]["normals_degenerate_obj"]))
        # the gradient launches on their own: one sample's kept vertices, per head, by events
        from alignsdf_amd.utils import mesh as mu
        from alignsdf_amd.utils.utils import bind_sample, decoder_for
        lat, mano, obj = src("s", 1)
        r = next(iter(rc.pipelined_two_pass(dec, specs, [(0, lat, mano, obj)], N, host_copy=True, normals=True)))[1]
        hip = decoder_for(dec, specs, mano)
        bind_sample(hip, specs, lat, mano, obj)
        total = 0.0
        for part in ("hand", "obj"):
            kv, _, counts = r["kept_dev_" + part]
            pts = mu.lattice_points(kv[:int(counts.cpu()[0])], r["origin"], r["voxel_size"]).contiguous()
            print("N=%d %-4s kept vertices %d of the %d that marching cubes emitted (the flow's launch runs over the latter)" % (
                N, part, len(pts), len(kv)))
            hip.decode_points_grad(pts, hand=part == "hand", obj=part == "obj")
            ms = []
            for _ in range(REPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                hip.decode_points_grad(pts, hand=part == "hand", obj=part == "obj")
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            total += float(np.median(ms))
            print("N=%d gradient launch %-4s %6d vertices: %.3f ms (events; runs %s) = %.1f ns / vertex" % (
                N, part, len(pts), float(np.median(ms)), " ".join("%.3f" % m for m in ms), 1e6 * float(np.median(ms)) / max(len(pts), 1)))
        print("N=%d gradient launches per sample: %.3f ms = %.1f %% of the sample without normals" % (N, total, 100.0 * total / med["without normals"]))


if __name__ == "__main__":
    main()
