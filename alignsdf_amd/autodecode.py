"""Auto-decode: latent codes fitted to ground-truth meshes - the codes `reconstruct --codes` reads, made without an encoder.

    python -m alignsdf_amd.autodecode -e EXP -t obman --data_root data --out CODES
           [--poses DIR] [--init DIR] [--unit_m 1.0] [--centre x y z]
           [--steps 800 --lr 5e-3 --decay 0.1 --every 400 --prior 1e-4 --clamp 0.05]
           [--near 12000 --uniform 4000 --seed 0] [--start N --end N] [--batch B]

For every name with both <data_root>/<task>/test/mesh_hand/<name>.obj and mesh_obj/<name>.obj (gt_interaction.discover) the two
meshes are mapped into the decoder's normalised space,

    x = (p unit_m - centre) SdfScaleFactor / 2          (to_decoder_frame; centre = rot_center of --poses/<name>.npz, else --centre)

become MeshFields there (mesh_sdf.py) and give the (xyz, sdf) samples of each head whose branch is on (mesh_sdf.sdf_samples); the code
is fitted to them on the device (fit.fit_code: the whole Adam loop is one stream of launches) from --init/<name>.npz or from zeros,
and written as CODES/<name>.npz with `latent` [1, 256] and the pose arrays of --poses copied through - what
code_sources.npz_code_source reads.  A pose-aligned decoder (PointFeatSize > 3, EncodeStyle not "nerf") is bound with the sample's
kinematic embedding and needs --poses: without it the run ends before any work.  CODES/autodecode.json holds, per sample, the first and
the last data term, the step count and the fields' `info`.  Per sample the host waits for the device once: when it reads the fitted
code to write the file.  --batch B fits B samples at a time in ONE stream of launches (fit.fit_codes: every step's launches carry all
B), with one wait per batch; the files and the records are those of --batch 1, byte for byte.
"""
import argparse
import json
import os

import numpy as np

from .gt_interaction import discover

POSE_KEYS = ("global_trans", "rot_center", "obj_trans")
FIT_DEFAULTS = {"steps": 800, "lr": 5e-3, "decay": 0.1, "every": 400, "prior": 1e-4, "clamp": 0.05}
SAMPLE_DEFAULTS = {"near": 12000, "uniform": 4000, "seed": 0}


def to_decoder_frame(p, unit_m, centre, scale_factor):
    """Mesh file coordinates -> the decoder's normalised space: (p unit_m - centre) scale_factor / 2, in fp64.  `centre` in metres."""
    return (np.asarray(p, np.float64) * float(unit_m) - np.asarray(centre, np.float64).reshape(3)) * (float(scale_factor) / 2.0)


def from_decoder_frame(x, unit_m, centre, scale_factor):
    """The inverse of to_decoder_frame: (x 2 / scale_factor + centre) / unit_m - sample_writer's placement of a written mesh with
    scale = 2 / (scale_factor unit_m) and offset = centre / unit_m."""
    return (np.asarray(x, np.float64) * (2.0 / float(scale_factor)) + np.asarray(centre, np.float64).reshape(3)) / float(unit_m)


def pose_aligned(specs):
    return int(specs["PointFeatSize"]) > 3 and specs["EncodeStyle"] != "nerf"


def load_poses(poses_dir, name, require_all=False):
    """The pose arrays of <poses_dir>/<name>.npz as float32 numpy ({} without a directory).  require_all (a pose-aligned decoder):
    ValueError naming the file when one of POSE_KEYS is missing."""
    if poses_dir is None:
        return {}
    path = os.path.join(poses_dir, name + ".npz")
    with np.load(path) as z:
        poses = {k: np.asarray(z[k], np.float32) for k in POSE_KEYS if k in z.files}
    if require_all and len(poses) != len(POSE_KEYS):
        raise ValueError("%s: a pose-aligned decoder needs %s, the file lacks %s" % (
            path, ", ".join(POSE_KEYS), ", ".join(k for k in POSE_KEYS if k not in poses)))
    return poses


def load_init(init_dir, name, latent_size=256):
    """The start code [latent_size]: `latent` of <init_dir>/<name>.npz, or zeros."""
    if init_dir is None:
        return np.zeros(latent_size, np.float32)
    with np.load(os.path.join(init_dir, name + ".npz")) as z:
        lat = np.asarray(z["latent"], np.float32).reshape(-1)
    if lat.size != latent_size:
        raise ValueError("%s: latent of %d elements, expected %d" % (name, lat.size, latent_size))
    return lat


def write_code(out_dir, name, latent, poses):
    """<out_dir>/<name>.npz in npz_code_source's layout: latent [1, L] and the pose arrays as they came."""
    path = os.path.join(out_dir, name + ".npz")
    np.savez(path, latent=np.asarray(latent, np.float32).reshape(1, -1), **poses)
    return path


class DeviceFitter:
    """fit_one of run() on the GPU: meshes -> MeshFields in the decoder's frame -> sdf samples -> fit.fit_code; fit_many: the same for a
    batch of samples through fit.fit_codes."""

    def __init__(self, decoder_module, specs, unit_m=1.0, centre=(0.0, 0.0, 0.0), fit=None, sampling=None):
        self.module, self.specs, self.unit_m = decoder_module, specs, float(unit_m)
        self.centre = np.asarray(centre, np.float64).reshape(3)
        self.fit = dict(FIT_DEFAULTS, **(fit or {}))
        self.sampling = dict(SAMPLE_DEFAULTS, **(sampling or {}))

    def _prepare(self, hand_path, obj_path, poses, start):
        """One sample up to the fit: (decoder, fit.fit_code's / fit.fit_codes' item, the fields)."""
        import torch
        from .mesh_sdf import MeshField, sdf_samples
        from .surface_sampling import load_obj
        from .utils.utils import decoder_for, sample_embedding
        specs = self.specs
        t = lambda keys: {k: torch.from_numpy(poses[k]) for k in keys if k in poses} or None
        mano, obj = t(("global_trans", "rot_center")), t(("obj_trans",))
        centre = np.asarray(poses["rot_center"], np.float64).reshape(3) if "rot_center" in poses else self.centre
        dec = decoder_for(self.module, specs, mano)
        fields, samples = {}, {}
        for part, path, on in (("hand", hand_path, specs.get("HandBranch", True)), ("obj", obj_path, specs.get("ObjectBranch", True))):
            if not on:
                continue
            verts, faces = load_obj(path)
            fields[part] = MeshField(to_decoder_frame(verts, self.unit_m, centre, specs["SdfScaleFactor"]), faces, device=dec.device)
            samples[part] = sdf_samples(fields[part], self.sampling["near"], self.sampling["uniform"], seed=self.sampling["seed"])
        embed = sample_embedding(specs, mano, obj, getattr(dec, "combined", False))
        item = {"latent": torch.from_numpy(np.asarray(start, np.float32)), "embed": embed, "sdf_hand": samples.get("hand"),
                "sdf_obj": samples.get("obj")}
        return dec, item, fields

    @staticmethod
    def _record(packed, steps, fields):
        return packed[:-2].astype(np.float32), {"first": float(packed[-2]), "last": float(packed[-1]), "steps": int(steps),
                                                "mesh_info": {part: f.info for part, f in fields.items()}}

    def __call__(self, name, hand_path, obj_path, poses, start):
        return self.fit_many([(name, hand_path, obj_path, poses, start)])[0]

    def fit_many(self, jobs):
        """fit_batch of run(): jobs = [(name, hand_path, obj_path, poses, start), ...] -> [(latent [L], record), ...], the samples'
        fits enqueued as one stream of launches (fit.fit_codes) and one wait for the whole batch.  Every result is that of the job
        alone, bit for bit.  Samples that ended up on different evaluators are fitted one by one."""
        import torch
        from .fit import fit_codes
        prepared = [self._prepare(hand_path, obj_path, poses, start) for _, hand_path, obj_path, poses, start in jobs]
        if len(jobs) > 1 and any(dec is not prepared[0][0] for dec, _, _ in prepared):
            return [self(*job) for job in jobs]
        # (a decoder the fit kernel refuses - CombinedDecoder, NeRF-encoded features - is fitted by the same rule on the module path)
        latents, history = fit_codes(prepared[0][0], [item for _, item, _ in prepared], module=self.module, specs=self.specs, **self.fit)
        # the one wait of the batch: the fitted codes (and, with them, the two ends of each history)
        steps = history.shape[1]
        ends = history[:, [0, -1]] if steps else history.new_zeros((len(jobs), 2))
        packed = torch.cat([latents.double(), ends], 1).cpu().numpy()
        return [self._record(packed[s], steps, fields) for s, (_, _, fields) in enumerate(prepared)]


def run(specs, fit_one, task, data_root, out_dir, poses_dir=None, init_dir=None, start=None, end=None, batch=1):
    """The flow around `fit_one(name, hand_path, obj_path, poses, start_code) -> (latent [L], record)`: discovery, the [start, end)
    range of the sorted pairs, the codes and autodecode.json.  batch > 1: the pairs go, in order, in groups of `batch` (the last one
    short) to `fit_one.fit_many([(name, hand_path, obj_path, poses, start_code), ...]) -> [(latent, record), ...]`; the files and the
    records are those of batch == 1, in the same order.  ValueError before any work for a pose-aligned decoder without poses.
    Returns (json path, records)."""
    if pose_aligned(specs) and poses_dir is None:
        raise ValueError("a pose-aligned decoder (PointFeatSize %d, EncodeStyle %r) is fitted under the sample's pose: pass --poses <dir of "
                         "<name>.npz with global_trans, rot_center and obj_trans>" % (specs["PointFeatSize"], specs["EncodeStyle"]))
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch %d: at least 1" % batch)
    pairs = discover(data_root, task)[(None if start is None else int(start)):(None if end is None else int(end))]
    os.makedirs(out_dir, exist_ok=True)
    records = []
    for at in range(0, len(pairs), batch):
        jobs = []
        for name, hand_path, obj_path in pairs[at:at + batch]:
            poses = load_poses(poses_dir, name, require_all=pose_aligned(specs))
            jobs.append((name, hand_path, obj_path, poses, load_init(init_dir, name, int(specs.get("LatentSize", 256)))))
        results = [fit_one(*jobs[0])] if batch == 1 else fit_one.fit_many(jobs)
        if len(results) != len(jobs):
            raise RuntimeError("fit_many returned %d results for %d samples" % (len(results), len(jobs)))
        for (name, _, _, poses, _), (latent, rec) in zip(jobs, results):
            write_code(out_dir, name, latent, poses)
            records.append(dict({"name": name}, **rec))
    path = os.path.join(out_dir, "autodecode.json")
    with open(path, "w") as f:
        json.dump({"task": task, "samples": records}, f, indent=1)
    return path, records


def summary_line(records):
    if not records:
        return "autodecode: no mesh pairs found"
    first, last = np.mean([r["first"] for r in records]), np.mean([r["last"] for r in records])
    return "autodecode: %d samples, %d steps each, mean data term %.4e -> %.4e" % (len(records), records[0]["steps"], first, last)


def main(argv=None):
    p = argparse.ArgumentParser(description="Fit latent codes to ground-truth meshes on the device (SDF auto-decoding)")
    p.add_argument("-e", "--experiment", required=True, help="experiment directory (specs.json, ModelParameters/latest.pth)")
    p.add_argument("-t", "--task", default="obman")
    p.add_argument("--data_root", default="data")
    p.add_argument("--out", required=True, help="directory of the <name>.npz codes (reconstruct --codes reads it)")
    p.add_argument("--poses", default=None, help="directory of <name>.npz with global_trans / rot_center / obj_trans")
    p.add_argument("--init", default=None, help="directory of <name>.npz start codes (default: zeros)")
    p.add_argument("--unit_m", type=float, default=1.0, help="metres per unit of the mesh files (default 1)")
    p.add_argument("--centre", type=float, nargs=3, default=(0.0, 0.0, 0.0), help="centre of the normalised space in metres, without --poses")
    for k, v in FIT_DEFAULTS.items():
        p.add_argument("--" + k, type=type(v), default=v)
    for k, v in SAMPLE_DEFAULTS.items():
        p.add_argument("--" + k, type=type(v), default=v)
    p.add_argument("--start", type=int, default=None)
    p.add_argument("--end", type=int, default=None)
    p.add_argument("--batch", type=int, default=1, help="samples fitted in one stream of launches (default 1: one after the other)")
    a = p.parse_args(argv)
    from .reconstruct import load_experiment
    specs, module = load_experiment(a.experiment)
    if pose_aligned(specs) and a.poses is None:
        p.error("a pose-aligned decoder needs --poses")
    fitter = DeviceFitter(module, specs, a.unit_m, a.centre, {k: getattr(a, k) for k in FIT_DEFAULTS}, {k: getattr(a, k) for k in SAMPLE_DEFAULTS})
    path, records = run(specs, fitter, a.task, a.data_root, a.out, a.poses, a.init, a.start, a.end, a.batch)
    print(summary_line(records))
    print(path)


if __name__ == "__main__":
    main()
