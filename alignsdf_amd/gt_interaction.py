"""Ground-truth interaction: penetration depth, intersection volume and contact of the GROUND-TRUTH grasps, next to the numbers
`--interaction` writes for the predictions (interaction.py).

    python -m alignsdf_amd.gt_interaction -e EXP -t obman --data_root data [--contact_mm 5] [--voxel_mm 2] [--unit_m 1.0]

For every name with both <data_root>/<task>/test/mesh_hand/<name>.obj and mesh_obj/<name>.obj the two meshes become MeshFields
(mesh_sdf.py) and the two interaction kernels measure them as they measure the decoder's fields: the hand's vertices in the object's
field and the object's in the hand's (surface_contact), and both fields on one lattice (lattice_overlap).  The lattice covers the
INTERSECTION of the two bounding boxes grown by one voxel - only there can both fields be negative; an empty intersection is a zero
overlap record without a launch.  Everything is in the files' own frame and units (--unit_m metres per file unit); the volumes of the
single meshes are their enclosed volumes, not voxel counts.  Writes Eval_<task>/interaction_gt.json and interaction_gt.txt.
"""
import argparse
import json
import os

import numpy as np

from . import _native
from . import interaction as ia

DEFAULT_VOXEL_M = 0.002
INT_MAX = 0x7fffffff


def discover(data_root, task):
    """[(name, hand path, object path)] sorted by name: the test meshes that exist as a pair."""
    base = os.path.join(data_root, task, "test")
    hand_dir, obj_dir = os.path.join(base, "mesh_hand"), os.path.join(base, "mesh_obj")
    if not os.path.isdir(hand_dir) or not os.path.isdir(obj_dir):
        return []
    names = sorted(n[:-4] for n in os.listdir(hand_dir) if n.endswith(".obj") and os.path.isfile(os.path.join(obj_dir, n)))
    return [(n, os.path.join(hand_dir, n + ".obj"), os.path.join(obj_dir, n + ".obj")) for n in names]


def overlap_lattice(bounds_hand, bounds_obj, voxel):
    """(origin [3], dims [3]) of the lattice of spacing `voxel` over the intersection of two boxes ((lo, hi) each) grown by one voxel
    on every side, or None when they do not intersect."""
    lo = np.maximum(np.asarray(bounds_hand[0], np.float64), np.asarray(bounds_obj[0], np.float64))
    hi = np.minimum(np.asarray(bounds_hand[1], np.float64), np.asarray(bounds_obj[1], np.float64))
    if not (lo <= hi).all():
        return None
    voxel = float(voxel)
    dims = np.ceil((hi - lo) / voxel).astype(np.int64) + 3          # points lo .. >= hi, and one more on either side
    return (lo - voxel).tolist(), [int(n) for n in dims]


def empty_overlap_words():
    """The overlap record of nothing: what asdf_interaction_lattice leaves when no voxel is negative."""
    w = np.zeros(_native.OVERLAP_WORDS, np.int32)
    w[_native.OVERLAP_MIN:_native.OVERLAP_MIN + 3] = INT_MAX
    w[_native.OVERLAP_MAX:_native.OVERLAP_MAX + 3] = -1
    return w


def gt_record(words, voxel, unit_m, contact_m, hand_volume, obj_volume):
    """interaction_record of the host words with scale_factor = 2 / unit_m (normalised units = file units), then the two patches: the
    single volumes are the meshes' enclosed volumes (file units^3 -> cm^3) and their voxel counts - taken on the intersection's
    lattice only - are None."""
    rec = ia.interaction_record(words, voxel, 2.0 / float(unit_m), contact_m)
    cm3 = (float(unit_m) * 100.0) ** 3
    rec.update({"hand_volume_cm3": float(hand_volume) * cm3, "obj_volume_cm3": float(obj_volume) * cm3, "hand_voxels": None,
                "obj_voxels": None})
    return rec


def measure_pair(hand, obj, voxel, unit_m, contact_m):
    """The record of one grasp from its two MeshFields (GPU).  Waits for the stream once."""
    import torch
    tau = ia.contact_tau(contact_m, 2.0 / float(unit_m))
    lat = overlap_lattice(hand.bounds(), obj.bounds(), voxel)
    recs = [None if lat is None else ia.lattice_overlap(hand.volume(lat[0], voxel, lat[1]), obj.volume(lat[0], voxel, lat[1])),
            ia.surface_contact(obj.at(hand.verts).sdf, tau), ia.surface_contact(hand.at(obj.verts).sdf, tau)]
    words = torch.cat([r for r in recs if r is not None]).cpu().numpy()
    if lat is None:
        words = np.concatenate([empty_overlap_words(), words])
    return gt_record(ia.split_words(words), voxel, unit_m, contact_m, hand.enclosed_volume(), obj.enclosed_volume())


def comparison_line(gt_summary, pred_summary):
    f = lambda v, fmt: "n/a" if v is None else fmt % v
    cols = (("mean_penetration_depth_cm", "penetration depth cm", "%.4f"), ("mean_intersection_volume_cm3", "intersection volume cm^3", "%.4f"),
            ("contact_ratio", "contact ratio", "%.3f"))
    return "ground truth vs prediction: " + ", ".join("%s %s vs %s" % (label, f(gt_summary.get(k), fmt), f(pred_summary.get(k), fmt))
                                                      for k, label, fmt in cols)


def write_outputs(out_dir, samples, contact_m, voxel_m, unit_m):
    """interaction_gt.json ({"summary", "contact_m", "voxel_m", "unit_m", "samples"}) and interaction_gt.txt through interaction.py's
    writers; returns (json path, summary, the comparison line or None)."""
    os.makedirs(out_dir, exist_ok=True)
    summary = ia.summarise(samples)
    ia.write_interaction_txt(out_dir, samples, summary, out_name="interaction_gt.txt")
    path = ia._dump(os.path.join(out_dir, "interaction_gt.json"), {"summary": summary, "contact_m": float(contact_m), "voxel_m": float(voxel_m),
                                                                  "unit_m": float(unit_m), "samples": samples})
    line = None
    try:
        with open(os.path.join(out_dir, "interaction.json")) as f:
            line = comparison_line(summary, json.load(f)["summary"])
    except (OSError, ValueError, KeyError):
        pass
    return path, summary, line


def run(experiment_directory, task, data_root, contact_m=ia.DEFAULT_CONTACT_M, voxel_m=DEFAULT_VOXEL_M, unit_m=1.0):
    from .mesh_sdf import MeshField
    from .surface_sampling import load_obj
    voxel = float(voxel_m) / float(unit_m)
    samples = []
    for index, (name, hand_path, obj_path) in enumerate(discover(data_root, task)):
        hand, obj = MeshField(*load_obj(hand_path)), MeshField(*load_obj(obj_path))
        rec = measure_pair(hand, obj, voxel, unit_m, contact_m)
        samples.append(dict({"index": index, "name": name, "skipped_faces": hand.info["skipped"] + obj.info["skipped"]}, **rec))
    return write_outputs(os.path.join(experiment_directory, "Eval_" + task), samples, contact_m, voxel_m, unit_m)


def main(argv=None):
    p = argparse.ArgumentParser(description="Interaction metrics of the ground-truth grasps (mesh signed distance fields)")
    p.add_argument("-e", "--experiment", required=True, help="experiment directory: Eval_<task>/interaction_gt.json / .txt are written there")
    p.add_argument("-t", "--task", default="obman")
    p.add_argument("--data_root", default="data")
    p.add_argument("--contact_mm", type=float, default=1e3 * ia.DEFAULT_CONTACT_M, help="contact distance in mm (default 5)")
    p.add_argument("--voxel_mm", type=float, default=1e3 * DEFAULT_VOXEL_M, help="lattice spacing of the intersection volume in mm (default 2)")
    p.add_argument("--unit_m", type=float, default=1.0, help="metres per unit of the mesh files (default 1)")
    a = p.parse_args(argv)
    path, summary, line = run(a.experiment, a.task, a.data_root, a.contact_mm / 1e3, a.voxel_mm / 1e3, a.unit_m)
    print(ia.summary_line(summary).replace("(decoder frame, before ICP)", "(ground-truth meshes)"))
    if line:
        print(line)
    print(path)


if __name__ == "__main__":
    main()
