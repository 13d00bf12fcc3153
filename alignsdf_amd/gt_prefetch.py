"""Eval mode's ground-truth meshes, read and sampled ahead of the consumer: the shared worker process (gt_worker.py) and the
prefetcher reconstruct() asks for them."""
import os
import threading

import torch

from .utils import mesh as mesh_utils


_gt_proc = None
_gt_lock = threading.Lock()


def _ground_truth_process():
    """The ground-truth worker process (gt_worker.py), started on first use and shared by every reconstruct() call of this
    process: its start (interpreter + numpy, ~0.2 s) is paid once, not per call.  A worker that has died is replaced."""
    global _gt_proc
    with _gt_lock:
        if _gt_proc is None or _gt_proc.poll() is not None:
            import atexit
            import subprocess
            import sys
            env = dict(os.environ)
            root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
            first = _gt_proc is None
            _gt_proc = subprocess.Popen([sys.executable, "-m", "alignsdf_amd.gt_worker"], stdin=subprocess.PIPE,
                                        stdout=subprocess.PIPE, env=env)
            if first:
                atexit.register(_stop_ground_truth_process)
        return _gt_proc


def _stop_ground_truth_process():
    global _gt_proc
    proc, _gt_proc = _gt_proc, None
    if proc is not None and proc.poll() is None:
        try:
            proc.stdin.close()
            proc.wait(timeout=5)
        except Exception:
            proc.kill()


class GroundTruthPrefetcher:
    """Eval mode reads one ground-truth mesh per sample (utils/mesh.py:386-389) and samples 30 000 points from it
    (deep_sdf/metrics/icp_trans_scale.py:19-23): file parsing and sampling run in a worker process, one or two samples ahead of
    the consumer, so that neither sits between two decoder passes.  get() returns the pinned [samples, 3] fp64 target points, or
    None when the file is missing and allow_missing_gt is set; a missing file otherwise raises like the reference's trimesh.load.
    The work itself runs in a PROCESS (alignsdf_amd/gt_worker.py, numpy only - like the reference's DataLoader worker): 15 ms of
    parsing and sampling per sample in a thread would hold the interpreter lock exactly when the main thread has to turn a coarse
    pass's boxes into the next launch (measured: 1.3 ms of GPU idle per pass in eval mode).  The thread here only moves requests
    and replies over the pipes (blocking reads release the lock).  ASDF_GT_WORKER=thread keeps everything in-process."""

    def __init__(self, task, data_root, allow_missing_gt=False, samples=30000, seed=1):
        from concurrent.futures import ThreadPoolExecutor
        from .frontend import quick_gil_handover
        self._switch_interval = quick_gil_handover()
        self.task, self.data_root, self.allow_missing, self.samples, self.seed = task, data_root, allow_missing_gt, samples, seed
        self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="asdf-gt")
        self.proc = None if os.environ.get("ASDF_GT_WORKER", "process") == "thread" else _ground_truth_process()
        self.jobs = {}
        # pinned staging for the target samples, allocated once (pinning per sample takes a runtime lock that the main thread's
        # launches queue behind); a slot is reused four samples later, long after its ICP has been waited for
        self.ring = [torch.empty((samples, 3), dtype=torch.float64).pin_memory() for _ in range(4)] if torch.cuda.is_available() else []
        self.turn = 0

    def _load(self, path):
        from . import gt_worker
        if self.proc is None:
            return gt_worker.load_samples(path, self.samples, self.seed)
        with _gt_lock:                                  # (one request / reply pair at a time on the shared pipes)
            gt_worker.write_message(self.proc.stdin, (path, self.samples, self.seed))
            reply = gt_worker.read_message(self.proc.stdout)
        if reply is None and self.proc.poll() is not None:
            raise RuntimeError("ground-truth worker process ended with code %s" % self.proc.returncode)
        if isinstance(reply, tuple) and reply and reply[0] == "error":
            raise RuntimeError("ground-truth mesh %s: %s" % (path, reply[1]))
        return reply

    def prefetch(self, ply_filename_out):
        if ply_filename_out not in self.jobs:
            path = mesh_utils.ground_truth_mesh_path(ply_filename_out, self.task, self.data_root)
            self.jobs[ply_filename_out] = (path, self.pool.submit(self._load, path))

    def get(self, ply_filename_out):
        self.prefetch(ply_filename_out)
        path, job = self.jobs.pop(ply_filename_out)
        pts = job.result()
        if pts is not None:
            pts = torch.from_numpy(pts)
            if self.ring:
                slot = self.ring[self.turn % len(self.ring)]
                self.turn += 1
                slot.copy_(pts)
                pts = slot
        if pts is None:
            if not self.allow_missing:
                raise FileNotFoundError("eval_mode: ground-truth mesh %s not found (data_root=%r); pass allow_missing_gt to write "
                                        "unaligned meshes instead" % (path, self.data_root))
            import logging
            logging.warning("eval_mode: ground-truth mesh %s not found; writing the unaligned mesh (allow_missing_gt)" % path)
        return pts

    def discard(self, ply_filename_out):
        """A prefetched sample the consumer does not need after all (no hand surface: nothing to align): drop its job - a failure
        of a mesh nobody reads is not an error, and nothing stays behind in self.jobs."""
        job = self.jobs.pop(ply_filename_out, None)
        if job is not None:
            job[1].cancel()

    def close(self):
        from .frontend import restore_gil_handover
        for _, job in self.jobs.values():           # (prefetched, never asked for)
            job.cancel()
        self.jobs.clear()
        self.pool.shutdown(wait=True)               # (the worker process is shared by later calls and ends with the interpreter)
        restore_gil_handover(self._switch_interval)
