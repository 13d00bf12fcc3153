"""Cost of the interaction metrics (csrc/interaction.hip, reconstruct(interaction=...)).

  1. each kernel call on its own by device events at N = 128 and 256: lattice_overlap on one sample's two fine volumes (init + one
     streaming pass; the fraction of the HBM rate it reaches on its 2 N^3 x 4 bytes, against the 6.29 TB/s a plain read measures on
     this part) and surface_contact on the other head's values at the hand's kept vertices (three launches)
  2. the whole pass as the pipeline runs it (overlap, two decode_points, two reductions)
  3. the files flow at N = 128 with and without the option, ms per sample, interleaved
  4. grasp9: the trained decoder's penetration depth next to the analytic scene's at the same vertices (a property of the fixture)

    python tools/time_interaction.py [--tag grasp9] [--samples 6] >> profiles/interaction.txt"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.environ.get("ASDF_TREE", "."))
from alignsdf_amd import interaction as ia, reconstruct as rc, synthetic as syn  # noqa: E402
from alignsdf_amd.networks.model import build_decoder  # noqa: E402

REPS = int(os.environ.get("ASDF_TIMING_REPS", "7"))
HBM_TBS = 6.29          # measured streaming-read rate of the part


def events(fn, inner=20):
    """ms per call over `inner` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tag", default="grasp9")
    p.add_argument("--samples", type=int, default=6)
    p.add_argument("--label", default="this tree")
    args = p.parse_args()
    tag, n = args.tag, args.samples
    specs = syn.specs_for(tag)
    dec = build_decoder(specs, {k: torch.from_numpy(v) for k, v in syn.full_state_dict(tag).items()})
    src = rc.synthetic_code_source(tag)
    contact_m = ia.DEFAULT_CONTACT_M
    tau = ia.contact_tau(contact_m, specs["SdfScaleFactor"])
    med = lambda v: float(np.median(v))
    print("# %s | %s | %s, median of %d runs of 20 back-to-back calls" % (args.label, torch.cuda.get_device_name(0), tag, REPS))

    from alignsdf_amd.utils import mesh as mu
    from alignsdf_amd.utils.utils import bind_sample, decoder_for
    for N in (128, 256):
        lat, mano, obj = src("s", 1)
        r = next(iter(rc.pipelined_two_pass(dec, specs, [(0, lat, mano, obj)], N, host_copy=True)))[1]
        hip = decoder_for(dec, specs, mano)
        bind_sample(hip, specs, lat, mano, obj)
        vh, vo = r["vol_hand"], r["vol_obj"]
        kv, _, counts = r["kept_dev_hand"]
        other = hip.decode_points(mu.lattice_points(kv, r["origin"], r["voxel_size"]))[1]
        t_l = [events(lambda: ia.lattice_overlap(vh, vo)) for _ in range(REPS)]
        t_p = [events(lambda: ia.surface_contact(other, tau, counts)) for _ in range(REPS)]
        t_all = [events(lambda: ia.interaction_pass(hip, r, specs, contact_m), inner=5) for _ in range(REPS)]
        nbytes = 2 * N ** 3 * 4
        floor_us = nbytes / (HBM_TBS * 1e12) * 1e6
        words = ia.interaction_pass(hip, r, specs, contact_m)["words"].cpu().numpy()
        print("N=%d lattice_overlap %.1f us per call (init + pass; %d bytes: %.2f TB/s, %.0f %% of %.2f TB/s; the floor is %.1f us) | "
              "surface_contact over %d values (%d kept) %.1f us per call (three launches) | the whole pass %.1f us" % (
                  N, 1e3 * med(t_l), nbytes, nbytes / (med(t_l) * 1e-3) / 1e12, 100.0 * floor_us / (1e3 * med(t_l)), HBM_TBS, floor_us,
                  other.numel(), int(counts.cpu()[0]), 1e3 * med(t_p), 1e3 * med(t_all)))
        rec = ia.interaction_record(ia.split_words(words), float(r["voxel_size"]), specs["SdfScaleFactor"], contact_m)
        print("N=%d sample 1: %s" % (N, json.dumps(rec)))
        hip = r = None

    # ---- the files flow at N = 128
    tmp = tempfile.mkdtemp()
    split = os.path.join(tmp, "split.json")
    json.dump({"filenames": ["x/%08d.jpg" % i for i in range(n + 1)]}, open(split, "w"))
    variants = [("N=128 interaction", {"interaction": {"contact_m": contact_m}}), ("N=128", {})]
    dirs = {name: os.path.join(tmp, name.replace(" ", "_").replace("=", "")) for name, _ in variants}
    for name, kw in variants:
        rc.reconstruct(dec, specs, split, dirs[name], 0, 2, cube_dim=128, code_source=src, **kw)
    runs, recs = {name: [] for name, _ in variants}, {}
    for _ in range(REPS):
        for name, kw in variants:
            torch.cuda.synchronize()
            t = time.perf_counter()
            recs[name] = rc.reconstruct(dec, specs, split, dirs[name], 1, n + 1, cube_dim=128, code_source=src, **kw)
            torch.cuda.synchronize()
            runs[name].append(1e3 * (time.perf_counter() - t) / n)
    for name, _ in variants:
        print("%-17s files flow %7.2f ms/sample (runs: %s)" % (name, med(runs[name]), " ".join("%.1f" % t for t in runs[name])))
    print(ia.summary_line(ia.summarise(recs[variants[0][0]])))

    # ---- the fixture: trained decoder against the analytic scene, at the hand's written vertices
    if tag in syn.GRASP_TAGS:
        from alignsdf_amd.ply import read_ply
        to_cm = 2.0 / specs["SdfScaleFactor"] * 100.0
        for rec in recs[variants[0][0]]:
            v = read_ply(os.path.join(dirs[variants[0][0]], "meshes", "%s_hand.ply" % rec["name"]))[0]
            analytic = max(0.0, -float(syn.grasp_sdf(v, rec["index"])[1].min())) * to_cm
            print("sample %d: penetration depth %.4f cm by the trained decoder, %.4f cm by the analytic scene at the same vertices; "
                  "intersection %.4f cm^3" % (rec["index"], rec["interaction"]["penetration_depth_cm"], analytic, rec["interaction"]["intersection_volume_cm3"]))


if __name__ == "__main__":
    main()
