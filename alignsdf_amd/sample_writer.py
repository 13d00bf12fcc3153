"""What reconstruct() does with the results of the sample pipeline: every sample's files and its record (SampleWriter), the PLY files
themselves on a worker thread (FileWriter)."""
import logging
import os
import time

import numpy as np

from .gt_prefetch import GroundTruthPrefetcher
from .sweeps_report import write_sweeps_json
from .utils import mesh as mesh_utils


class FileWriter:
    """PLY files are written on a worker thread (tobytes + write release the GIL): the consumer hands over host arrays and
    moves on to the next sample.  A failed write (disk full, permissions) surfaces at the NEXT write_ply / poll - one sample later,
    not after the whole shard has been decoded - and close() waits for every file; close(failing=True), from a `finally` that is
    unwinding another exception, only logs what the writer still has to report so that the original error survives."""

    def __init__(self):
        from concurrent.futures import ThreadPoolExecutor
        from .frontend import quick_gil_handover
        self._switch_interval = quick_gil_handover()
        self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="asdf-ply")
        self.jobs = []

    def poll(self):
        """Raise the failure of any write that has finished; forget the ones that succeeded."""
        pending, first = [], None
        for path, j in self.jobs:
            if not j.done():
                pending.append((path, j))
                continue
            err = j.exception()
            if err is not None:
                import logging
                logging.error("PLY write of %s failed: %s", path, err)      # every failed path is named, the first is raised
                if first is None:
                    first = err
        self.jobs = pending                        # (a failure is reported once)
        if first is not None:
            raise first

    def write_ply(self, path, verts, faces, normals=None, quality=None):
        from .ply import write_ply
        self.poll()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        extra = () if quality is None else (quality,)          # (the option travels only when it is on)
        self.jobs.append((path, self.pool.submit(write_ply, path, verts, faces, normals, *extra)))

    def write_view(self, path, view, H, W, trace):
        from .render import save_view
        self.poll()
        self.jobs.append((path, self.pool.submit(save_view, path, view, H, W, trace)))

    def close(self, failing=False):
        from .frontend import restore_gil_handover
        self.pool.shutdown(wait=True)
        restore_gil_handover(self._switch_interval)
        jobs, self.jobs = self.jobs, []
        first = None
        for path, j in jobs:
            err = j.exception()
            if err is not None:
                if failing:
                    import logging
                    logging.error("PLY write of %s failed: %s", path, err)
                elif first is None:
                    first = err
        if first is not None:
            raise first


class SampleWriter:
    """The consumer of one reconstruct() run: per sample, the kept component of every surface becomes a PLY file (the hand aligned to
    its ground truth in eval mode, the object under the hand's transform), the label files follow, and a record says what was written.
    close() ends the helpers and leaves the shard's sweeps report next to meshes/."""

    def __init__(self, output_dir, shard, cube_dim, hand_on, scale=None, viz=False, ground_truth=None, normals=False, interaction=None):
        """`shard` = (start_point, end_point, stride), for the sweeps report; `ground_truth` = (task, data_root, allow_missing_gt) in
        eval mode - the hand is what gets aligned, so without a hand branch there is no prefetcher.  `normals`: the results carry
        `host_kept_normals_*` (pipelined_two_pass(normals=True)) and every file is written with them.  `interaction` =
        {"contact_m", "scale_factor"}: the results carry `host_interaction` (pipelined_two_pass(interaction=...)) - every record gains
        `interaction`, every file `quality`, and close() leaves the shard's interaction_<start>_<end>.json next to the sweeps report."""
        self.output_dir, self.shard, self.cube_dim, self.normals = output_dir, shard, cube_dim, bool(normals)
        self.interaction = interaction
        self.mesh_dir = os.path.join(output_dir, "meshes")
        os.makedirs(self.mesh_dir, exist_ok=True)
        self.hand_on, self.scale, self.viz = hand_on, scale, viz
        self.gt = GroundTruthPrefetcher(*ground_truth) if ground_truth is not None and hand_on else None
        self.writer = FileWriter()
        self.records = []
        self.sweeps = {}                                               # the pipeline's `report`: which evaluator ran, its counters
        self.components = {"open": 0, "small": 0, "surfaces": 0}      # what K8 dropped, and why (write_sweeps_json)
        self.t_prev = time.perf_counter()

    def path(self, name, part):
        return os.path.join(self.mesh_dir, "%s_%s" % (name, part))

    def prefetch(self, name):
        if self.gt is not None:
            self.gt.prefetch(self.path(name, "hand") + ".ply")  # parsed + sampled by the time the ICP hook wants it

    def begin_hand(self, key, r):
        """Eval mode: the ICP of the hand mesh, slotted between two decoder passes (see pipelined_two_pass).  Everything
        it needs is on the device already - the largest component straight from K8, sampled there (bit-identical to the
        host sampler), normalised there - and the ground truth's samples come from the prefetch worker: the hook only
        enqueues, write_part only waits for the result."""
        if "verts_hand" in r:
            from .icp import start_alignment_device
            target = self.gt.get(self.path(key[1], "hand") + ".ply")
            r["icp_job"] = None if target is None else start_alignment_device(*r["kept_dev_hand"], r["origin"], r["voxel_size"], target)
        else:
            self.gt.discard(self.path(key[1], "hand") + ".ply")          # no hand surface: the prefetched ground truth is not needed

    def kept(self, r, part):
        c = r["host_kept_counts_" + part].numpy()
        self.components["open"] += int(c[4])
        self.components["small"] += int(c[5])
        self.components["surfaces"] += 1
        return r["host_kept_verts_" + part][:c[0]], r["host_kept_faces_" + part][:c[1]]

    def write_part(self, base, r, part, rec, offset=None, scale=None):
        """One surface: its kept component placed, the hand's eval-mode ICP finished, the file handed to the writer.  Returns the
        ICP's (trans, scale) - zeros / one when none ran."""
        r["copy_done_" + part].synchronize()          # side-stream D2H of this mesh only
        _, faces, points = mesh_utils.place_vertices(*self.kept(r, part), r["origin"], r["voxel_size"], offset, scale)
        job = None
        if part == "hand" and self.gt is not None:
            job = r.pop("icp_job", None)
            if job is None:
                rec["icp_skipped"] = True          # allow_missing_gt: no ground-truth mesh, written unaligned
        points, trans, icp_scale = mesh_utils.apply_icp(job, points)
        if "host_polish_counts_" + part in r:          # (pipelined_two_pass(polish=True): the kept vertices are the polished ones)
            from .project import count_record
            rec["polish_" + part] = count_record(r["host_polish_counts_" + part].numpy())
        normals = None
        if self.normals:
            # (unit normals of the kept vertices: the ICP's translation and positive scale leave them as they are)
            normals = r["host_kept_normals_" + part][:len(points)].numpy()
            rec["normals_degenerate_" + part] = mesh_utils.count_degenerate(normals)
        if self.interaction is not None:
            # quality: the signed distance in metres to the OTHER surface, by the other head's SDF at this vertex - in the decoder's
            # frame (the eval-mode ICP moves the positions, not these values)
            r["copy_done_interaction"].synchronize()
            quality = r["host_other_sdf_" + part][:len(points)].numpy() * np.float32(2.0 / self.interaction["scale_factor"])
            self.writer.write_ply(base + ".ply", points, faces, normals, quality)
        elif normals is not None:
            self.writer.write_ply(base + ".ply", points, faces, normals)
        else:
            self.writer.write_ply(base + ".ply", points, faces)
        return trans, icp_scale

    def write_render(self, path, r, rec):
        """<name>_render.npz next to the meshes: the maps of the sample's view (pipelined_two_pass(render=...)), and its statistics in
        the record."""
        from .render import VIEW_MAPS, VIEW_STATS
        r["copy_done_render"].synchronize()
        H, W = r["render"]["size"]
        view = {k: r["host_render_" + k].numpy() for k in VIEW_MAPS + VIEW_STATS if "host_render_" + k in r}
        rec["render_evals_mean"] = float(view["evals_mean"])
        rec["render_exhausted_hand"], rec["render_exhausted_obj"] = int(view["exhausted_hand"]), int(view["exhausted_obj"])
        self.writer.write_view(path, view, H, W, r["render"]["trace"])

    def write_labels(self, base, r, rec, offset, scale):
        verts, faces, vertices = mesh_utils.place_vertices(r["host_verts_hand"], r["host_faces_hand"], r["origin"], r["voxel_size"])
        labels = r["host_labels_hand"].float()
        mesh_utils.write_label_outputs(vertices, faces, labels, base, offset, scale, self.viz)
        rec["labels_hand"] = np.bincount(labels.long().numpy(), minlength=1).tolist()

    def write(self, index, name, r):
        """The files and the record of one sample."""
        rec = {"index": index, "name": name, "V_hand": r["V_hand"], "F_hand": r["F_hand"], "V_obj": r["V_obj"],
               "F_obj": r["F_obj"], "voxel_size": float(r["voxel_size"]), "origin": r["origin"]}
        # the object is written with the hand's ICP translation / scale as offset / scale whenever the hand branch
        # is on - zeros / one outside eval mode or when the hand has no surface (utils/mesh.py:123-133,186-195)
        offset, sc = (np.array([0, 0, 0]), np.array([1])) if self.hand_on else (None, self.scale)
        for part in ("hand", "obj"):
            base = self.path(name, part)
            if "verts_" + part not in r:
                if "mc_error_" + part in r:
                    logging.warning("Cannot reconstruct mesh from '{}'".format(base + ".ply"))
                    print(r["mc_error_" + part])
            elif part == "obj":
                self.write_part(base, r, part, rec, offset, sc)
            else:
                offset, sc = self.write_part(base, r, part, rec)
                rec["icp_trans"], rec["icp_scale"] = np.asarray(offset).reshape(-1).tolist(), float(np.asarray(sc).reshape(-1)[0])
                if "host_labels_hand" in r:
                    self.write_labels(base, r, rec, offset, sc)
        if "render" in r:
            self.write_render(self.path(name, "render") + ".npz", r, rec)
        if self.interaction is not None and "host_interaction" in r:
            from .interaction import PARTS, interaction_record, split_words
            r["copy_done_interaction"].synchronize()
            words = split_words(r["host_interaction"].numpy(), [part for part in PARTS if "verts_" + part in r])
            rec["interaction"] = interaction_record(words, rec["voxel_size"], self.interaction["scale_factor"], self.interaction["contact_m"])
        now = time.perf_counter()
        rec["seconds"], self.t_prev = now - self.t_prev, now
        self.records.append(rec)
        return rec

    def write_report(self):
        if self.sweeps:
            start, end, stride = self.shard
            write_sweeps_json(self.output_dir, start, end, self.sweeps, len(self.records), self.cube_dim, self.components, stride)
        if self.interaction is not None:
            from .interaction import write_interaction_json
            start, end, stride = self.shard
            write_interaction_json(self.output_dir, start, end, self.records, self.interaction["contact_m"], stride)

    def close(self, failing=False):
        """End the helpers and write the shard's sweeps report.  failing=True, while another exception unwinds: what they still have to
        report is logged and never replaces the error in flight (a failing close must not mask the error being raised)."""
        if failing:
            _logged("writing the sweep report of a failed shard", self.write_report)      # (it exists even when the shard did not finish)
            if self.gt is not None:
                _logged("closing the ground-truth prefetcher", self.gt.close)
            self.writer.close(failing=True)
            return
        if self.gt is not None:
            self.gt.close()
        self.writer.close()                      # every file is on disk (or its error raised) before reconstruct() returns
        self.write_report()


def _logged(what, step):
    try:
        step()
    except Exception as e:
        logging.error("%s failed: %s", what, e)
