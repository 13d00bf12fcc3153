"""`sweeps_<start>_<end>.json` of a shard, the run's merged `sweeps.json`, and the one line about them a user reads."""
import json
import os


def write_sweeps_json(out_dir, start_point, end_point, report, samples, cube_dim, components=None, stride=1):
    """`<output_dir>/sweeps_<start>_<end>.json` - next to `meshes/`, whose listing stays the reference's (reconstruct.py:34-35) -: which
    sweeps produced the volumes behind this shard's meshes.
    The default sweeps of a mesh-producing run rest on a measured, statistical certificate; a run whose sweeps
    were refused and repeated, whose modes were switched off, or which ended on the fp32 chain must say so NEXT TO ITS FILES, not only
    in a log line.  The reference writes nothing of the kind (utils/mesh.py:82-121 evaluates every voxel in fp32)."""
    hip = report.get("evaluator")
    body = {"range": [int(start_point), int(end_point)], "samples": int(samples), "cube_dim": int(cube_dim),
            "sweeps": hip.sweep_report(report.get("snapshot")) if hip is not None else None}
    if int(stride) != 1:
        body["stride"] = int(stride)               # (a strided shard: samples start, start + stride, ... below end)
    if components is not None:
        # f1, the largest-component filter (K8; PARITY UNPINNED against trimesh): how many components of >= 4 faces it dropped as open /
        # non-manifold - the only place where trimesh's fill_holes (utils/mesh.py:371 -> graph.split -> submesh(repair=True); not
        # reproduced) could have changed which component is written.  Expected 0 on marching-cubes surfaces
        body["dropped_open_components"] = int(components.get("open", 0))
        body["dropped_small_components"] = int(components.get("small", 0))
        body["surfaces_filtered"] = int(components.get("surfaces", 0))
    path = os.path.join(out_dir, "sweeps_%d_%d.json" % (int(start_point), int(end_point)))
    with open(path, "w") as f:
        json.dump(body, f, indent=1)
    return path


def merge_sweeps_json(out_dir, out_name="sweeps.json", ranges=None):
    """One `sweeps.json` for the whole run from the per-shard files (dist_reconstruct: rank 0, behind the gather): the per-shard
    records side by side plus the totals a reader looks for first.  `ranges` = the [start, end) shard ranges of THIS run: only their
    `sweeps_<start>_<end>.json` are merged (a glob also picked up the shards an earlier run with another world size had
    left in the directory); None = every shard file present.  On a multi-node run without a shared file system rank 0 sees its own
    host's shards only - `shards_missing` in the totals says how many of `ranges` had no file."""
    shards, missing = [], 0
    if ranges is None:
        wanted = sorted(n for n in os.listdir(out_dir) if n.startswith("sweeps_") and n.endswith(".json"))
    else:
        wanted = ["sweeps_%d_%d.json" % (int(a), int(b)) for a, b in ranges]
    for name in wanted:
        try:
            with open(os.path.join(out_dir, name)) as f:
                shards.append(json.load(f))
        except (OSError, ValueError):
            missing += 1                               # (a shard that failed before it wrote one, or another host's)
    shards.sort(key=lambda b: b["range"][0])
    tot = {"samples": sum(b["samples"] for b in shards), "sweeps_audited": 0, "sweeps_refused": 0, "sweeps_repeated": 0,
           "ordinary_sweeps": 0, "modes_switched_off": [], "fell_back_to_fp32_chain": False, "shards_missing": missing,
           "min_tau_over_sigma": None, "min_tau_over_estimate": None, "tail_ratio_max": None, "dropped_open_components": 0}
    for b in shards:
        sw = b.get("sweeps") or {}
        for k in ("sweeps_audited", "sweeps_refused", "sweeps_repeated"):
            tot[k] += int(sw.get(k, 0))
        tot["ordinary_sweeps"] += int(sw.get("coarse_pass", {}).get("ordinary_sweeps", 0)) + int(sw.get("fine_pass", {}).get("ordinary_sweeps", 0))
        tot["dropped_open_components"] += int(b.get("dropped_open_components", 0) or 0)
        for k in ("min_tau_over_sigma", "min_tau_over_estimate"):
            v = sw.get(k)
            if v is not None:
                tot[k] = v if tot[k] is None else min(tot[k], v)
        for v in (sw.get("tail_ratio_max") or {}).values():
            if v is not None:
                tot["tail_ratio_max"] = v if tot["tail_ratio_max"] is None else max(tot["tail_ratio_max"], v)
        tot["modes_switched_off"] += ["samples %d..%d: %s" % (b["range"][0], b["range"][1], m) for m in sw.get("modes_switched_off", [])]
        tot["fell_back_to_fp32_chain"] = tot["fell_back_to_fp32_chain"] or bool(sw.get("arithmetic", {}).get("fell_back_to_fp32_chain"))
    path = os.path.join(out_dir, out_name)
    with open(path, "w") as f:
        json.dump({"totals": tot, "shards": shards}, f, indent=1)
    return path


def sweeps_summary_line(tot):
    """The one line about the sweeps a user of dist_reconstruct actually reads, from merge_sweeps_json's totals."""
    if not tot.get("sweeps_audited") and not tot.get("sweeps_refused"):
        line = "sweeps: %d ordinary (every voxel of both passes at <= 1e-5; --fast selects the audited one-plane sweeps)" % tot.get("ordinary_sweeps", 0)
    else:
        f = lambda v: "n/a" if v is None else "%.1f" % v
        line = ("sweeps (--fast): %d audited one-plane, %d REFUSED and repeated, %d ordinary; certificate: min allowance / sigma %s, "
                "min allowance / estimate %s, largest tail ratio %s" % (
                    tot["sweeps_audited"], tot["sweeps_refused"], tot.get("ordinary_sweeps", 0), f(tot.get("min_tau_over_sigma")),
                    f(tot.get("min_tau_over_estimate")), f(tot.get("tail_ratio_max"))))
    if tot.get("modes_switched_off"):
        line += "; MODES SWITCHED OFF: %s" % "; ".join(tot["modes_switched_off"])
    if tot.get("fell_back_to_fp32_chain"):
        line += "; a decoder FELL BACK to the fp32 chain"
    if tot.get("dropped_open_components"):
        line += "; %d open components dropped by the largest-component filter (where trimesh's fill_holes could have differed)" % tot["dropped_open_components"]
    if tot.get("shards_missing"):
        line += "; %d shard report(s) missing" % tot["shards_missing"]
    return line
