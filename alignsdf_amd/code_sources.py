"""Where reconstruct() gets the per-sample codes from: a `code_source(sample_name, index) -> (latent, mano_results, obj_results)`
callable stands in for the reference's per-image front end (see reconstruct.py).  Two sources: precomputed `.npz` codes on disk and
the deterministic synthetic codes of the tests and the benchmark; CodeUploader serves the callers that want the codes on the device."""
import os

import numpy as np
import torch

from . import synthetic


class CodeUploader:
    """(Round 6: the code sources below no longer upload - host-side codes stay on the host and the HIP decoder reads them from pinned
    memory, see _code_converter; this class serves the module path and callers that ask for device tensors.)
    Per-sample codes (a latent vector, a few pose matrices: a few KB) -> device WITHOUT making the host wait for the stream.  A
    plain `.to(device)` of pageable memory is a synchronous copy in stream order: with two decoder passes of the next sample queued
    (round 5: samples are enqueued in one go) the caller sat 50 ms behind them, the queue ran dry, and everything the host did next -
    K8, the ground-truth hand-over, the sampler and the ICP of eval mode - ran with the GPU idle in between (4.4 ms per sample in
    the eval-mode trace).  Here: a ring of pinned staging buffers, the copy on a side stream, and the compute stream waits for the
    copy's event on the DEVICE."""

    SLOTS = 8

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.stream = None
        self.ring = {}        # (shape, dtype) -> [turn, [(pinned buffer, event of the copy that last read it)]]

    def __call__(self, array):
        t = torch.from_numpy(np.ascontiguousarray(array))
        if self.device.type != "cuda":
            return t.to(self.device)
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.device)
        key = (tuple(t.shape), t.dtype)
        entry = self.ring.setdefault(key, [0, []])
        if len(entry[1]) < self.SLOTS:
            entry[1].append([torch.empty(t.shape, dtype=t.dtype).pin_memory(), None])
            slot = entry[1][-1]
        else:
            slot = entry[1][entry[0] % self.SLOTS]
            entry[0] += 1
            slot[1].synchronize()                          # (eight uploads ago: long done)
        slot[0].copy_(t)
        compute = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            # (allocated from the SIDE stream's pool: a block of the compute stream's pool may still be in use by kernels queued
            # there, and this copy does not wait for them)
            out = torch.empty(t.shape, dtype=t.dtype, device=self.device)
            out.copy_(slot[0], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        out.record_stream(compute)
        compute.wait_event(done)
        slot[1] = done
        return out


def _code_converter(device, on_host):
    """What a code source does with an array that is on the host.  on_host=True (the default, round 6): a float32 CPU tensor - the HIP
    decoder's set_sample stages it in pinned memory and its fold reads it from there in stream order (asdf_decoder_set_sample_host): no
    copy engine, no runtime blit kernel behind a persistent sweep, and the pose matrices are consumed on the
    host anyway (hip_decoder.kinematic_affine).  The module path uploads what it needs itself (torch_decoder.TorchModuleDecoder.
    set_sample, through a CodeUploader).  on_host=False: a device tensor through CodeUploader."""
    if on_host:
        return lambda array: torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32))
    return CodeUploader(device)


def synthetic_code_source(tag="nerf3", device="cuda", on_host=True):
    """Deterministic per-sample codes (64 distinct samples, cycled; the grasp family: its 16 trained scenes)."""
    up = _code_converter(device, on_host)

    def source(name, index):
        s = index % (synthetic.GRASP_SAMPLES if tag in synthetic.GRASP_TAGS else 64)
        lat, m, o = synthetic.sample_inputs(tag, s)
        lat = up(lat)
        if m is None:
            return lat, None, None
        return lat, {k: up(v) for k, v in m.items()}, {k: up(v) for k, v in o.items()}
    return source


def npz_code_source(code_dir, device="cuda", on_host=True, mano_model=None):
    """Codes saved by an external encoder run: <code_dir>/<sample>.npz with `latent` [1,256] and optionally
    `global_trans` [1,16,4,4], `rot_center` [1,1,3], `obj_trans` [1,4,4].  A file may hold MANO parameters instead of the first two -
    `mano_pose` [1, 3 + ncomps] and `mano_shape` [1,10]: with `mano_model` (a mano.ManoModel) the source makes global_trans and
    rot_center from them by mano.mano_torch ON THE HOST - hip_decoder.kinematic_affine consumes these matrices on the host, a device
    tensor there would be a synchronising read.  Such a file without a model is an error; a file with global_trans is read as ever."""
    up = _code_converter(device, on_host)

    def source(name, index):
        z = np.load(os.path.join(code_dir, name + ".npz"))
        lat = up(np.asarray(z["latent"], dtype=np.float32))
        mano = obj = None
        if "global_trans" in z.files:
            mano = {"global_trans": up(np.asarray(z["global_trans"], dtype=np.float32)),
                    "rot_center": up(np.asarray(z["rot_center"], dtype=np.float32))}
        elif "mano_pose" in z.files:
            if mano_model is None:
                raise ValueError("%s.npz holds mano_pose / mano_shape instead of global_trans: a MANO model is needed (--mano_model)" % name)
            from .mano import mano_torch
            pose = torch.from_numpy(np.asarray(z["mano_pose"], dtype=np.float32).reshape(1, -1))
            shape = torch.from_numpy(np.asarray(z["mano_shape"], dtype=np.float32).reshape(1, 10))
            with torch.no_grad():
                _, _, _, global_trans, center = mano_torch(mano_model, pose, shape, center_idx=0)
            mano = {"global_trans": up(global_trans.numpy()), "rot_center": up(center.numpy())}
        if "obj_trans" in z.files:
            obj = {"obj_trans": up(np.asarray(z["obj_trans"], dtype=np.float32))}
        return lat, mano, obj
    return source


def code_source_from_args(args, specs, parser):
    """--codes DIR | --synthetic; neither is an error (there is no silent default)."""
    if args.code_dir:
        model = None
        if getattr(args, "mano_model", None):
            from .mano import ManoModel
            model = ManoModel.from_npz(args.mano_model)
        return npz_code_source(args.code_dir, mano_model=model)
    if getattr(args, "synthetic", False):
        return synthetic_code_source("nerf3" if specs["PointFeatSize"] == 3 else "both9")
    parser.error("no latent codes: pass --codes <dir of <sample>.npz written by the encoder run> (or --synthetic for a benchmark run)")
