"""Hand-object interaction metrics from the decoder's own two signed distance fields: penetration depth, intersection volume and
contact - what this literature reports for a grasp (ObMan, Grasping Field) and what the reference trains on (train.py:563-577,
ContactLossSigma 0.005 m at train.py:265) but never writes at inference time.

With two SDFs no mesh-mesh test is needed.  Two kernels (csrc/interaction.hip, worded in include/alignsdf_hip.h) reduce
  - the sample's two fine volumes, which share one zoom cube, to the OVERLAP record: voxels inside the hand, inside the object, inside
    both, and the box of the latter.  SIGNS only, so it holds for the one-plane sweeps of `fast` as well, whose volumes are exact only
    next to the surfaces and sign-correct elsewhere;
  - the OTHER head's SDF at one surface's kept vertices (decode_points at origin + v * voxel_size, rows past K8's kept count never
    read: the count stays on the device) to the CONTACT record: vertices inside, vertices within the contact distance, the deepest one.

Units: the decoder works in normalised units; metres = normalised x 2 / SdfScaleFactor, the reference's own conversion
(train.py:563-568).  Records are in cm and cm^3.  Frame: the decoder's own, BEFORE the eval-mode ICP moves the hand onto its ground
truth - the ICP's scale would rescale every length here by a factor that says nothing about the prediction.
"""
import ctypes
import json
import os

import numpy as np
import torch

from . import _native

PARTS = ("hand", "obj")
DEFAULT_CONTACT_M = 0.005          # ContactLossSigma of the reference (train.py:265)
WORDS = _native.OVERLAP_WORDS + 2 * _native.CONTACT_WORDS      # one sample's records side by side: overlap, hand, obj


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _device_f32(v):
    if not torch.is_tensor(v) or not v.is_cuda:
        raise TypeError("a CUDA tensor is needed (there is no CPU fallback)")
    v = v.detach()
    if v.dtype != torch.float32 or not v.is_contiguous():
        v = v.to(torch.float32).contiguous()
    return v


def lattice_overlap(vol_hand, vol_obj):
    """OVERLAP record (int32[16] on the device, _native.OVERLAP_*) of two fp32 device volumes [n0, n1, n2] on one lattice
    (asdf_interaction_lattice).  Nothing here waits for the stream."""
    a, b = _device_f32(vol_hand), _device_f32(vol_obj)
    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError("two volumes of one 3-d shape are needed, not %s and %s" % (tuple(a.shape), tuple(b.shape)))
    rec = torch.empty(_native.OVERLAP_WORDS, dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        _native.check(_native.lib().asdf_interaction_lattice(a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], a.shape[2], rec.data_ptr(),
                                                              _stream(a.device)), "asdf_interaction_lattice")
    return rec


def surface_contact(values, tau, count=None):
    """CONTACT record (int32[8] on the device, _native.CONTACT_*) of the fp32 device values [cap]: `count` (an int32 device tensor, its
    first word is read when the kernel runs; None = all) says how many of them count (asdf_interaction_points).  Nothing here waits
    for the stream."""
    f = _device_f32(values).reshape(-1)
    if count is not None and (not torch.is_tensor(count) or not count.is_cuda or count.dtype != torch.int32):
        raise TypeError("count: an int32 CUDA tensor (the kept counts of the component filter), or None")
    rec = torch.empty(_native.CONTACT_WORDS, dtype=torch.int32, device=f.device)
    with torch.cuda.device(f.device):
        _native.check(_native.lib().asdf_interaction_points(f.data_ptr() if f.numel() else None, f.numel(),
                                                             None if count is None else count.data_ptr(), float(tau), rec.data_ptr(),
                                                             _stream(f.device)), "asdf_interaction_points")
    return rec


def contact_tau(contact_m, scale_factor):
    """The contact distance in the decoder's normalised units."""
    return float(contact_m) * float(scale_factor) / 2.0


def check_option(interaction, specs):
    """The `interaction` option of the entry points -> contact_m.  ValueError when a branch is off: there is no second field."""
    if not isinstance(interaction, dict):
        interaction = {}
    contact_m = float(interaction.get("contact_m", DEFAULT_CONTACT_M))
    if not contact_m >= 0:
        raise ValueError("interaction: contact_m >= 0 is required, not %r" % (contact_m,))
    if not (specs.get("HandBranch", True) and specs.get("ObjectBranch", True)):
        raise ValueError("interaction needs both the hand and the object branch: the metrics relate the two fields")
    return contact_m


def interaction_pass(evaluator, result, specs, contact_m):
    """What the sample pipeline calls in post-processing, with `evaluator` BOUND to the sample of `result`: the overlap of its two fine
    volumes, then per surface the other head's SDF at its kept vertices (`kept_dev_<part>` = K8's (verts, faces, counts), polished
    where that is on) and their contact record.  Returns {"words": int32[WORDS] on the device - overlap, hand, obj; a missing surface
    leaves zeros -, "other_sdf_hand" / "other_sdf_obj": fp32 [capacity] where the surface exists}.  Nothing here waits for the stream."""
    from .utils.mesh import lattice_points
    tau = contact_tau(contact_m, specs["SdfScaleFactor"])
    out = {}
    recs = [lattice_overlap(result["vol_hand"], result["vol_obj"])]
    for k, part in enumerate(PARTS):
        if "kept_dev_" + part not in result:
            recs.append(torch.zeros(_native.CONTACT_WORDS, dtype=torch.int32, device=recs[0].device))
            continue
        kv, _, counts = result["kept_dev_" + part]
        other = evaluator.decode_points(lattice_points(kv, result["origin"], result["voxel_size"]))[1 - k]
        if other is None:
            raise ValueError("the evaluator has no %s head to measure the %s surface in" % (PARTS[1 - k], part))
        out["other_sdf_" + part] = other
        recs.append(surface_contact(other, tau, counts))
    out["words"] = torch.cat(recs)
    return out


def split_words(words, have=PARTS):
    """int32[WORDS] of interaction_pass (host) -> {"overlap", "hand", "obj"} as interaction_record takes them; surfaces that are not
    in `have` become None."""
    w = np.asarray(words, dtype=np.int32).reshape(-1)
    o, c = _native.OVERLAP_WORDS, _native.CONTACT_WORDS
    return {"overlap": w[:o], "hand": w[o:o + c] if "hand" in have else None, "obj": w[o + c:o + 2 * c] if "obj" in have else None}


def interaction_record(words, voxel_size, scale_factor, contact_m):
    """The host words of one sample ({"overlap": int32[16], "hand": int32[8] or None, "obj": ...}: `hand` = the hand's vertices in the
    OBJECT's field) as a plain dict.  Lengths in cm, volumes in cm^3, metres = normalised x 2 / scale_factor; `voxel_size` is the fine
    lattice's, in normalised units.  `contact` is the kernels' own comparison (a vertex with f <= tau exists), i.e. min_distance <=
    contact_m.  A missing surface has None in its vertex fields and contact comes from the one that exists."""
    N = _native
    to_cm = 2.0 / float(scale_factor) * 100.0
    voxel_cm3 = (float(voxel_size) * to_cm) ** 3
    ov = [int(v) for v in np.asarray(words["overlap"]).reshape(-1)]
    both = ov[N.OVERLAP_BOTH]
    rec = {"intersection_volume_cm3": both * voxel_cm3, "hand_volume_cm3": ov[N.OVERLAP_HAND] * voxel_cm3,
           "obj_volume_cm3": ov[N.OVERLAP_OBJ] * voxel_cm3, "intersection_voxels": both, "hand_voxels": ov[N.OVERLAP_HAND],
           "obj_voxels": ov[N.OVERLAP_OBJ], "nan_voxels": ov[N.OVERLAP_NAN],
           "intersection_box": [ov[N.OVERLAP_MIN:N.OVERLAP_MIN + 3], ov[N.OVERLAP_MAX:N.OVERLAP_MAX + 3]] if both else None,
           "contact_m": float(contact_m)}
    minima, near, nan_vertices = [], 0, 0
    for part, depth_key in (("hand", "penetration_depth_cm"), ("obj", "penetration_depth_obj_cm")):
        w = words.get(part)
        if w is None:
            rec.update({depth_key: None, part + "_vertices": None, part + "_vertices_inside": None, part + "_vertices_in_contact": None,
                        part + "_deepest_vertex": None})
            continue
        w = np.asarray(w, dtype=np.int32).reshape(-1)
        low = float(w[N.CONTACT_MIN_BITS:N.CONTACT_MIN_BITS + 1].view(np.float32)[0])
        some = int(w[N.CONTACT_ARGMIN]) >= 0
        rec.update({depth_key: max(0.0, -low) * to_cm if some else 0.0, part + "_vertices": int(w[N.CONTACT_COUNT]),
                    part + "_vertices_inside": int(w[N.CONTACT_INSIDE]), part + "_vertices_in_contact": int(w[N.CONTACT_NEAR]),
                    part + "_deepest_vertex": int(w[N.CONTACT_ARGMIN]) if some else None})
        near += int(w[N.CONTACT_NEAR])
        nan_vertices += int(w[N.CONTACT_NAN])
        if some:
            minima.append(low)
    rec["min_distance_cm"] = min(minima) * to_cm if minima else None
    rec["contact"] = bool(near > 0)
    rec["nan_vertices"] = nan_vertices
    return rec


def summarise(records):
    """Interaction dicts (or sample records that carry one under "interaction") -> {"samples", "mean_penetration_depth_cm",
    "mean_intersection_volume_cm3", "contact_ratio"}: the means over the samples that have the figure (None when none has)."""
    recs = [r.get("interaction", r) for r in records]
    recs = [r for r in recs if r is not None and "intersection_volume_cm3" in r]
    mean = lambda vals: float(np.mean(vals)) if vals else None
    return {"samples": len(recs),
            "mean_penetration_depth_cm": mean([r["penetration_depth_cm"] for r in recs if r.get("penetration_depth_cm") is not None]),
            "mean_intersection_volume_cm3": mean([r["intersection_volume_cm3"] for r in recs]),
            "contact_ratio": mean([1.0 if r["contact"] else 0.0 for r in recs])}


def summary_line(summary):
    """The one line a user reads at the end of a run."""
    f = lambda v, fmt: "n/a" if v is None else fmt % v
    return ("interaction: %d samples, mean penetration depth %s cm, mean intersection volume %s cm^3, contact ratio %s "
            "(decoder frame, before ICP)" % (summary["samples"], f(summary["mean_penetration_depth_cm"], "%.4f"),
                                            f(summary["mean_intersection_volume_cm3"], "%.4f"), f(summary["contact_ratio"], "%.3f")))


def _dump(path, body):
    tmp = path + ".tmp%d" % os.getpid()            # (renamed into place: ranks that finish together never leave half a file)
    with open(tmp, "w") as f:
        json.dump(body, f, indent=1)
    os.replace(tmp, path)
    return path


def write_interaction_json(out_dir, start_point, end_point, records, contact_m, stride=1):
    """`<output_dir>/interaction_<start>_<end>.json` next to meshes/ (like sweeps_<start>_<end>.json): the interaction dict of every
    sample of a shard with its index and name.  `records` = the sample records of SampleWriter."""
    body = {"range": [int(start_point), int(end_point)], "contact_m": float(contact_m),
            "samples": [dict({"index": r["index"], "name": r["name"]}, **r["interaction"]) for r in records if r.get("interaction")]}
    if int(stride) != 1:
        body["stride"] = int(stride)
    return _dump(os.path.join(out_dir, "interaction_%d_%d.json" % (int(start_point), int(end_point))), body)


def write_interaction_txt(out_dir, samples, summary, out_name="interaction.txt"):
    """interaction.txt in the style of evaluate.write_summary: one line per sample sorted by decreasing penetration depth, then the
    means and the contact ratio."""
    rows = sorted(samples, reverse=True, key=lambda r: -1.0 if r.get("penetration_depth_cm") is None else r["penetration_depth_cm"])
    path = os.path.join(out_dir, out_name)
    tmp = path + ".tmp%d" % os.getpid()            # (renamed into place, like the json files: the ranks of a sharded run share the directory)
    with open(tmp, "w") as f:
        f.write("summary of interaction (name, penetration depth cm, intersection volume cm3, min distance cm, contact)\n")
        for r in rows:
            f.write("{}, {}, {}, {}, {}\n".format(r.get("name"), r.get("penetration_depth_cm"), r["intersection_volume_cm3"],
                                                  r.get("min_distance_cm"), int(bool(r["contact"]))))
        f.write("mean penetration depth:{}\n".format(summary["mean_penetration_depth_cm"]))
        f.write("mean intersection volume:{}\n".format(summary["mean_intersection_volume_cm3"]))
        f.write("contact ratio:{}\n".format(summary["contact_ratio"]))
        f.write("samples:{}\n".format(summary["samples"]))
    os.replace(tmp, path)
    return path


def merge_interaction_json(out_dir, out_name="interaction.json", ranges=None):
    """One `interaction.json` ({"summary", "shards_missing", "samples" sorted by index}) and `interaction.txt` for the whole run from
    the per-shard files, following sweeps_report.merge_sweeps_json: `ranges` = the [start, end) shard ranges of THIS run (None = every
    shard file present).  Returns the path of interaction.json, or None - and writes nothing - when no shard file was found (a run
    without the option)."""
    if ranges is None:
        wanted = sorted(n for n in os.listdir(out_dir) if n.startswith("interaction_") and n.endswith(".json"))
    else:
        wanted = ["interaction_%d_%d.json" % (int(a), int(b)) for a, b in ranges]
    shards, missing = [], 0
    for name in wanted:
        try:
            with open(os.path.join(out_dir, name)) as f:
                shards.append(json.load(f))
        except (OSError, ValueError):
            missing += 1
    if not shards:
        return None
    samples = sorted((s for b in shards for s in b["samples"]), key=lambda s: s["index"])
    summary = summarise(samples)
    write_interaction_txt(out_dir, samples, summary)
    return _dump(os.path.join(out_dir, out_name), {"summary": summary, "contact_m": shards[0].get("contact_m"),
                                                    "shards_missing": missing, "samples": samples})


def add_interaction_arguments(p):
    p.add_argument("--interaction", action="store_true",
                   help="also report how the hand and the object relate, from the decoder's own two SDFs: penetration depth, intersection "
                        "volume and contact per sample (records, interaction_<start>_<end>.json, interaction.json / .txt), and every mesh "
                        "file gains `property float quality` = signed distance in metres to the other surface.  Taken in the decoder's "
                        "frame, before the eval-mode ICP.  Default: off")
    p.add_argument("--contact_mm", type=float, default=1e3 * DEFAULT_CONTACT_M,
                   help="--interaction: the distance in mm within which a vertex counts as in contact (default 5, the reference's "
                        "ContactLossSigma)")


def interaction_from_args(args):
    """{} without --interaction, else the `interaction` option of reconstruct()."""
    return {"interaction": {"contact_m": args.contact_mm / 1e3}} if args.interaction else {}


def measure_surfaces(evaluator, r, kept, specs, contact_m):
    """The interaction dict of ONE sample outside the pipeline (create_mesh_combined_decoder): `r` = decode_two_pass's result, `kept` =
    part -> (verts, faces, counts or None) on the device, in lattice units - what write_hand_and_object wrote into each file (the kept
    component, polished where that is on; a surface that was not written is absent) -, with `evaluator` still bound to the sample.
    Waits for the stream once, at the end."""
    work = {"vol_hand": r["vol_hand"], "vol_obj": r["vol_obj"], "origin": r["origin"], "voxel_size": r["voxel_size"]}
    have = [part for part in PARTS if part in kept]
    for part in have:
        work["kept_dev_" + part] = kept[part]
    words = interaction_pass(evaluator, work, specs, contact_m)["words"].cpu().numpy()
    return interaction_record(split_words(words, have), float(r["voxel_size"]), specs["SdfScaleFactor"], contact_m)
