"""Cost and effect of the projection onto the zero level (HipSdfDecoder.project_points, reconstruct(polish=True)).

  1. one project_points call on the kept vertices of one sample, per head, by device events, against the means the package had before
     the kernel: project.project_lockstep over decode_points_grad (a launch per step plus a dozen small torch launches and a host
     read), interleaved; evaluations per point and the workgroup trip counts (a tile of 32 points takes the most evaluations any of
     them takes) next to it
  2. the files flow of tools/time_reconstruct_files.py, ms per sample, and the fp64 residual |sdf| at the written vertices (oracle
     chain in fp64 on the CPU), for N = 128 with polish, N = 128 without and N = 256 without - interleaved

    python tools/time_project.py [--tag both9] [--samples 6] >> profiles/sdf_project.txt"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.environ.get("ASDF_TREE", "."))
from alignsdf_amd import project as pj, reconstruct as rc, synthetic as syn  # noqa: E402
from alignsdf_amd.networks.model import build_decoder  # noqa: E402
from alignsdf_amd.ply import read_ply  # noqa: E402

REPS = int(os.environ.get("ASDF_TIMING_REPS", "7"))


def sdf64(tag, sample, pts, chunk=1 << 15):
    """{"hand" / "obj": |sdf| [M]} of the oracle's decode chain in fp64 on the CPU."""
    from oracle import sdf_oracle as orc
    dt = torch.float64
    sd, specs = syn.full_state_dict(tag), syn.specs_for(tag)
    latent, mano, obj = syn.sample_inputs(tag, sample)
    cast = lambda d: None if d is None else {k: torch.as_tensor(v).to(dt) for k, v in d.items()}
    mano, obj = cast(mano), cast(obj)
    hp, op = orc.effective_head_params(sd, "h", dt), orc.effective_head_params(sd, "o", dt)
    lat = torch.as_tensor(latent).to(dt).reshape(1, -1)
    x = torch.as_tensor(np.array(pts, np.float32)).to(dt)
    out = {"hand": [], "obj": []}
    with torch.no_grad():
        for i in range(0, len(x), chunk):
            h, o = orc.decode_sdf_multi_output(hp, op, lat, orc.point_features(x[i:i + chunk], specs, mano, obj), specs)
            out["hand"].append(h.reshape(-1).abs().numpy())
            out["obj"].append(o.reshape(-1).abs().numpy())
    return {k: np.concatenate(v) for k, v in out.items()}


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tag", default="both9")
    p.add_argument("--samples", type=int, default=6)
    p.add_argument("--label", default="this tree")
    args = p.parse_args()
    tag, n = args.tag, args.samples
    specs = syn.specs_for(tag)
    dec = build_decoder(specs, {k: torch.from_numpy(v) for k, v in syn.full_state_dict(tag).items()})
    src = rc.synthetic_code_source(tag)
    print("# %s | %s | %s, hand + object, median of %d interleaved runs" % (args.label, torch.cuda.get_device_name(0), tag, REPS))

    # ---- 1. the call on its own: one sample's kept vertices at N = 128
    from alignsdf_amd.utils import mesh as mu
    from alignsdf_amd.utils.utils import bind_sample, decoder_for
    N = 128
    lat, mano, obj = src("s", 1)
    r = next(iter(rc.pipelined_two_pass(dec, specs, [(0, lat, mano, obj)], N, host_copy=True)))[1]
    hip = decoder_for(dec, specs, mano)
    bind_sample(hip, specs, lat, mano, obj)
    voxel = float(r["voxel_size"])
    rule = dict(pj.PROJECT_DEFAULTS, max_move=voxel)
    for part in ("hand", "obj"):
        kv, _, counts = r["kept_dev_" + part]
        pts = mu.lattice_points(kv[:int(counts.cpu()[0])], r["origin"], voxel).contiguous()
        fused = lambda: hip.project_points(pts, part, **rule)
        loop = lambda: pj.project_lockstep(pj.grad_of_head(hip, part), pts, **rule)
        res, ref = fused(), loop()
        same = all(torch.equal(res[k].view(torch.int32), ref[k].view(torch.int32)) for k in pj.OUTPUTS)
        ev = res["evals"].cpu().numpy()
        tiles = np.pad(ev, (0, -len(ev) % 32)).reshape(-1, 32).max(1)
        st = res["status"].cpu().numpy()
        t_f, t_l, w_f, w_l, t_g = [], [], [], [], []
        for _ in range(REPS):
            t_f.append(events(fused))
            t_l.append(events(loop))
            w_f.append(wall(fused))
            w_l.append(wall(loop))
            t_g.append(events(lambda: hip.decode_points_grad(pts, hand=part == "hand", obj=part == "obj")))
        med = lambda v: float(np.median(v))
        print("N=%d %-4s %6d kept vertices: project_points %.3f ms by events (%.3f wall) | launch-per-step loop %.3f ms (%.3f wall) = "
              "%.2f x | one decode_points_grad launch %.3f ms | same bits: %s" % (
                  N, part, len(pts), med(t_f), med(w_f), med(t_l), med(w_l), med(t_l) / med(t_f), med(t_g), same))
        print("N=%d %-4s evaluations per point mean %.2f max %d; workgroup trip counts over %d tiles of 32 points: mean %.2f max %d "
              "(slot efficiency %.2f); CONVERGED %d SPENT %d STALLED %d BAD %d; |sdf| > |sdf_in| at %d" % (
                  N, part, ev.mean(), ev.max(), len(tiles), tiles.mean(), tiles.max(), ev.sum() / (32.0 * tiles.sum()),
                  *[int((st == c).sum()) for c in range(4)], int((res["sdf"].abs() > res["sdf_in"].abs()).sum())))
    hip = None

    # ---- 2. the files flow
    tmp = tempfile.mkdtemp()
    split = os.path.join(tmp, "split.json")
    json.dump({"filenames": ["x/%08d.jpg" % i for i in range(n + 1)]}, open(split, "w"))
    variants = [("N=128 polish", 128, {"polish": True}), ("N=128", 128, {}), ("N=256", 256, {})]
    dirs = {name: os.path.join(tmp, name.replace(" ", "_").replace("=", "")) for name, _, _ in variants}
    for name, N, kw in variants:                                             # warm-up of every form
        rc.reconstruct(dec, specs, split, dirs[name], 0, 2, cube_dim=N, code_source=src, **kw)
    runs, recs = {name: [] for name, _, _ in variants}, {}
    for _ in range(REPS):
        for name, N, kw in variants:
            torch.cuda.synchronize()
            t = time.perf_counter()
            recs[name] = rc.reconstruct(dec, specs, split, dirs[name], 1, n + 1, cube_dim=N, code_source=src, **kw)
            torch.cuda.synchronize()
            runs[name].append(1e3 * (time.perf_counter() - t) / n)
    for name, N, kw in variants:
        res = {part: [] for part in ("hand", "obj")}
        verts = 0
        for rec in recs[name][:3]:                                           # (fp64 on the CPU: three samples)
            for part in res:
                v = read_ply(os.path.join(dirs[name], "meshes", "%s_%s.ply" % (rec["name"], part)))[0]
                if len(v) > 20000:                                           # (a seeded draw: the truth runs on the CPU)
                    v = v[np.random.default_rng(rec["index"]).choice(len(v), 20000, replace=False)]
                res[part].append(sdf64(tag, rec["index"], v)[part])
                verts += len(v)
        line = "; ".join("%s median %.3g max %.3g" % (part, np.median(np.concatenate(a)), np.concatenate(a).max()) for part, a in res.items())
        print("%-13s files flow %7.2f ms/sample (runs: %s) | fp64 |sdf| at the written vertices of 3 samples (%d vertices, at most 20000 per file): %s" % (
            name, float(np.median(runs[name])), " ".join("%.1f" % t for t in runs[name]), verts, line))
        if kw:
            print("%-13s polish records of the last sample: hand %s obj %s" % (name, recs[name][-1]["polish_hand"], recs[name][-1]["polish_obj"]))


if __name__ == "__main__":
    main()
