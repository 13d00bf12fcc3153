"""The stock-module path of the decoder operator: decoder variants the HIP kernels do not cover are evaluated
by calling the nn.Module itself on PyTorch-ROCm device tensors, exactly like the reference's chunk loop does
(utils/mesh.py:46-63: slice, embed, `decode_sdf_multi_output`, write back) - only the lattice coordinates come from the
native library (the same device function the HIP kernels use, so the lattice is the reference's bit for bit), and the
negative-voxel box / marching cubes behind it are the native kernels as always.

Variants served here: `use_tanh`, the LayerNorm form (`weight_norm` false), `xyz_in_all` (networks/model.py:118-119,131-132,
166-176,314-315), a pose-aligned model evaluated without `mano_results` (the NeRF branch of utils/mesh.py:53-55),
`PixelAlign` (utils/utils.py:536-566), and any module whose parameters are not SeparateDecoder / CombinedDecoder shaped.
It is a GPU path like the rest of the package: CPU tensors raise.
"""
import copy
import itertools
import ctypes
import logging
import weakref

import numpy as np
import torch

from . import _native
from .code_sources import CodeUploader

CHUNK = 2 ** 18          # max_batch of reconstruct.py:93


def kinematic_embedding(xyz, mano_results, point_feat_size, scale_factor, obj_results, encode_style):
    """utils.utils.kinematic_embedding (utils/utils.py:376-430) on device tensors, op for op (batch of one sample)."""
    M = xyz.shape[0]
    wrist = xyz * 2 / scale_factor
    hand = obj = None
    if encode_style in ("hand", "both"):
        mano_xyz = wrist + mano_results["rot_center"].reshape(1, 3).to(xyz)
        homo = torch.cat([mano_xyz, torch.ones(M, 1, device=xyz.device)], 1)
        inv_g = torch.linalg.inv(mano_results["global_trans"].reshape(16, 4, 4).to(xyz))
        inv_pts = torch.matmul(inv_g.unsqueeze(0), homo.reshape(M, 1, 4, 1)).squeeze(-1)
        inv_xyz = inv_pts[:, :, :3] / inv_pts[:, :, 3:4]
        if (point_feat_size == 6 and encode_style == "hand") or (point_feat_size == 9 and encode_style == "both"):
            inv_xyz = inv_xyz[:, :1, :]
        hand = torch.cat([mano_xyz.unsqueeze(1), inv_xyz], 1).reshape(M, -1) * scale_factor / 2
    if encode_style in ("obj", "both"):
        homo_w = torch.cat([wrist, torch.ones(M, 1, device=xyz.device)], 1)
        inv_o = torch.linalg.inv(obj_results["obj_trans"].reshape(4, 4).to(xyz))
        o = torch.matmul(inv_o, homo_w.t()).t()
        obj = (o[:, :3] / o[:, 3:4]) * scale_factor / 2
    if encode_style == "hand":
        return hand
    if encode_style == "obj":
        return torch.cat([xyz, obj], 1)
    return torch.cat([hand, obj], 1)


def nerf_embedding(xyz, multires):
    """get_nerf_embedder(multires) (utils/utils.py:433-463,521-533): [x, sin(2^k x), cos(2^k x)]."""
    outs = [xyz]
    for freq in 2.0 ** torch.linspace(0.0, multires - 1, steps=multires):
        outs += [torch.sin(xyz * freq), torch.cos(xyz * freq)]
    return torch.cat(outs, -1)


def pixel_alignment(img_feat, xyz, cam_intr, mano_results, image_size, scale_factor):
    """utils.utils.pixel_alignment (utils/utils.py:536-558): per-point bicubic samples of the image feature map at the
    projection of the point (camera space = wrist space + root joint); points that project outside the image take the
    feature map's mean."""
    pred_root = mano_results["joints"][:, [0]].to(xyz)
    x = xyz.reshape((img_feat.shape[0], -1, 3))
    xyz_cam = (x * 2 / scale_factor) + pred_root
    B, P = img_feat.shape[0], x.shape[1]
    homo = torch.cat([xyz_cam, torch.ones([B, P, 1], device=xyz.device)], 2)
    xy_img = torch.bmm(cam_intr.to(xyz), homo.transpose(1, 2)).transpose(1, 2)
    xy_img = (xy_img[:, :, :2] / xy_img[:, :, [2]]).unsqueeze(2)
    uv = xy_img / image_size * 2 - 1
    feat = torch.nn.functional.grid_sample(img_feat, uv, align_corners=True, mode="bicubic")[:, :, :, 0].transpose(1, 2)
    uv = uv.squeeze().reshape((-1, 2))
    inside = (uv[:, 0] >= -1.0) & (uv[:, 0] <= 1.0) & (uv[:, 1] >= -1.0) & (uv[:, 1] <= 1.0)
    outside = (~inside).reshape((B, P, -1))
    feat[torch.where(outside)[:2]] = img_feat.mean(3).mean(2)[torch.where(outside)[:1]]
    return feat.reshape((B * P, -1))


def needs_module_path(decoder, specs=None, mano_results=None):
    """Why (a string) this decoder / sample cannot run on the HIP kernels, or None when it can."""
    if specs is not None and specs.get("PixelAlign", False):
        return "PixelAlign: the latent is a per-point sample of an image feature map"
    if isinstance(decoder, torch.nn.Module):
        if getattr(decoder, "use_tanh", False):
            return "use_tanh"
        if getattr(decoder, "xyz_in_all", False):
            return "xyz_in_all"
        # shapes: NetworkSpecs other than the shipped dims [512] * 4 / latent_in [2] / LatentSize 256 are legal
        # (networks/model.py:192-282) and run on the module
        from .hip_decoder import unsupported_reason
        sd = decoder.state_dict()
        if not hasattr(decoder, "point_feat_size") or not hasattr(decoder, "encode_style"):
            return "not a SeparateDecoder / CombinedDecoder shaped module"
        why = unsupported_reason(sd, getattr(decoder, "latent_size", (specs or {}).get("LatentSize", 256)), decoder.point_feat_size,
                                 decoder.encode_style)
        if why is not None:
            return why
    if specs is not None and specs["PointFeatSize"] > 3 and specs["EncodeStyle"] != "nerf" and mano_results is None:
        return "pose-aligned model without mano_results: NeRF branch of utils/mesh.py:53-55"
    return None


class TorchModuleDecoder:
    """The interface of HipSdfDecoder (set_sample / decode_grid / decode_points / classify_points) on a plain module call.

    The caller's module is neither moved nor switched: it is held through a weak reference, called in eval mode with its
    training flag restored afterwards, and - when its parameters live on another device (the reference keeps checkpoints on the
    CPU until `.cuda()`) - evaluated through a device COPY that is refreshed whenever a parameter tensor is replaced or written
    (the reference reconstructs from inside its training loop, train.py:668).  `specs` None = the legacy single-output
    contract of deep_sdf.utils.decode_sdf (deep_sdf/utils.py:64-75): `module(cat(latent, xyz))` or `module(xyz)` when there is
    no latent, returning [M, 1] (the first element if the module returns a tuple)."""

    math = "torch"
    combined = False
    nerf_features = False
    event_log = None
    coarse_mode = fine_mode = "exact"

    def __init__(self, module, specs, reason, device=None):
        if not isinstance(module, torch.nn.Module):
            raise TypeError("the module path needs the nn.Module itself (%s)" % reason)
        if not torch.cuda.is_available() or _native.lib().asdf_device_count() < 1:
            raise _native.NativeError(-4, "no gfx950 (MI355X) device visible - there is no CPU path")
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self._module_ref = weakref.ref(module)
        self._copy = None            # (fingerprint, device copy) when the caller's parameters are not on self.device
        self.specs = specs
        self.reason = reason
        self.num_class = int(getattr(module, "num_class", 0)) if getattr(module, "use_classifier", False) else 0
        self._sample = None
        logging.warning("decoder runs on the PyTorch-ROCm module path (%s); the HIP kernels do not cover this variant", reason)

    @property
    def module(self):
        """The module to call: the caller's own when it lives on this device, otherwise an up-to-date device copy."""
        m = self._module_ref()
        if m is None:
            raise ReferenceError("the decoder module has been garbage-collected")
        params = list(m.parameters())
        if not params or all(p.device == self.device for p in params):
            return m
        # parameters AND buffers (a LayerNorm-free module has none, a BatchNorm-style one does): a change of either refreshes the copy
        fp = tuple((t.data_ptr(), t._version) for t in itertools.chain(params, m.buffers()))
        if self._copy is None or self._copy[0] != fp:
            # old-style weight_norm leaves the effective weight of its last forward on the module as a NON-leaf tensor, which
            # deepcopy refuses.  The caller's module is not touched: the copy is made with a memo that hands deepcopy a
            # detached clone for every such tensor - the forward pre-hook recomputes it on every call, so the stand-in loses nothing.
            # Cost: one deepcopy + upload per CHANGE of the caller's CPU parameters - inside a training loop that is every step;
            # keep the module on the device there.
            memo = {}
            for sub in m.modules():
                for val in vars(sub).values():
                    if torch.is_tensor(val) and not val.is_leaf:
                        memo[id(val)] = val.detach().clone()
            self._copy = (fp, copy.deepcopy(m, memo).to(self.device).eval())
        return self._copy[1]

    def set_sample(self, latent_vec, mano_results=None, obj_results=None, cam_intr=None):
        # (codes that arrive on the host - the code sources leave them there - go through the pinned ring + side stream: a plain
        # .to(device) of pageable memory waits for everything queued on the stream)
        def up(t):
            if t is None:
                return None
            t = t.detach()
            if t.device.type == "cpu" and self.device.type == "cuda":
                if getattr(self, "_uploader", None) is None:
                    self._uploader = CodeUploader(self.device)
                return self._uploader(t.to(torch.float32).numpy())
            return t.to(self.device)
        dev = lambda d: None if d is None else {k: up(v) for k, v in d.items()}
        lat = up(latent_vec)
        self._sample = (None if lat is None else lat.to(torch.float32), dev(mano_results), dev(obj_results), up(cam_intr))

    def fall_back_if_overflowed(self, bbox_host, epoch=None):
        return False

    def range_violations(self, clear=True):
        return 0

    def close(self):
        self._sample = None
        self._copy = None

    # -- the reference's chunk loop body (utils/mesh.py:47-56 + utils/utils.py:561-572; deep_sdf/utils.py:64-75 without specs) ---
    def _decode_chunk(self, module, xyz):
        latent, mano, obj, cam = self._sample
        specs = self.specs
        if specs is None:
            out = module(xyz if latent is None else torch.cat([latent.reshape(1, -1).expand(xyz.shape[0], -1), xyz], 1))
            return (out[0], out[1] if len(out) > 1 and torch.is_tensor(out[1]) and out[1].dim() == 2 else None, None) \
                if isinstance(out, (tuple, list)) else (out, None, None)
        q = xyz
        if specs["PointFeatSize"] > 3:
            if mano is not None and specs["EncodeStyle"] != "nerf":
                q = kinematic_embedding(xyz, mano, specs["PointFeatSize"], specs["SdfScaleFactor"], obj, specs["EncodeStyle"])
            else:
                q = nerf_embedding(xyz, (specs["PointFeatSize"] - 3) // 6)
        if specs.get("PixelAlign", False):
            lat = pixel_alignment(latent, q[:, :3], cam, mano, specs["ImageSize"][0], specs["SdfScaleFactor"])
        else:
            lat = latent.reshape(1, -1).expand(q.shape[0], -1)
        return module(torch.cat([lat, q], 1))

    def _decode(self, xyz, want_scores=False):
        if self._sample is None:
            raise ValueError("no sample bound: call set_sample first")
        M = xyz.shape[0]
        hand = torch.empty(M, dtype=torch.float32, device=self.device)
        obj = torch.empty(M, dtype=torch.float32, device=self.device)
        has_obj = True
        scores = torch.empty((M, self.num_class), dtype=torch.float32, device=self.device) if want_scores else None
        module = self.module
        was_training = module.training
        module.eval()
        try:
            with torch.no_grad():
                for head in range(0, M, CHUNK):
                    h, o, c = self._decode_chunk(module, xyz[head:head + CHUNK])
                    hand[head:head + CHUNK] = h.reshape(-1)
                    if o is None:
                        has_obj = False
                    else:
                        obj[head:head + CHUNK] = o.reshape(-1)
                    if want_scores:
                        scores[head:head + CHUNK] = c
        finally:
            module.train(was_training)
        return hand, (obj if has_obj else None), scores

    def coarse_begin(self, N, origin3, voxel_size, grid_mode=_native.GRID_REFERENCE, hand=True, obj=True):
        """The coarse pass of the two-pass flow (same interface as HipSdfDecoder.coarse_begin; always an ordinary sweep)."""
        h, o, bbox = self.decode_grid(N, origin3, voxel_size, grid_mode, hand=hand, obj=obj)
        return {"rec": bbox, "keep": (h, o)}

    def coarse_finish(self, ticket):
        return ticket["rec"].cpu().numpy()

    def fine_begin(self, N, origin3, voxel_size, grid_mode=_native.GRID_REFERENCE, hand=True, obj=True, mc_only=False):
        """The fine pass (same interface as HipSdfDecoder.fine_begin; always an ordinary sweep, nothing to guard)."""
        h, o, _ = self.decode_grid(N, origin3, voxel_size, grid_mode, want_bbox=False, hand=hand, obj=obj)
        return h, o, None

    def fine_needs_repeat(self, ticket):
        return False

    def sweep_snapshot(self):
        return None

    def sweep_report(self, since=None):
        """The module path runs ordinary fp32 sweeps only (same interface as HipSdfDecoder.sweep_report)."""
        return {"evaluator": "module on PyTorch-ROCm (%s)" % self.reason, "arithmetic": {"at_start": "f32 (torch)", "now": "f32 (torch)",
                "fell_back_to_fp32_chain": False}, "sweeps_audited": 0, "sweeps_refused": 0, "sweeps_repeated": 0, "modes_switched_off": []}

    def decode_points(self, xyz):
        h, o, _ = self._decode(xyz.detach().to(self.device, torch.float32).contiguous())
        return h, o

    def decode_points_grad(self, xyz, hand=True, obj=True):
        """The interface of HipSdfDecoder.decode_points_grad by torch autograd through the module's own forward (one backward per
        head and chunk): (sdf_hand [M], grad_hand [M,3], sdf_obj [M], grad_obj [M,3]), None for a head switched off or absent."""
        if self._sample is None:
            raise ValueError("no sample bound: call set_sample first")
        xyz = xyz.detach().to(self.device, torch.float32).contiguous()
        M = xyz.shape[0]
        new = lambda on, *shape: torch.empty(shape, dtype=torch.float32, device=self.device) if on else None
        out = [new(hand, M), new(hand, M, 3), new(obj, M), new(obj, M, 3)]
        module = self.module
        was_training = module.training
        module.eval()
        try:
            with torch.enable_grad():
                for head in range(0, M, CHUNK):
                    x = xyz[head:head + CHUNK].clone().requires_grad_()
                    values = self._decode_chunk(module, x)[:2]
                    for k, (on, v) in enumerate(zip((hand, obj), values)):
                        if not on:
                            continue
                        if v is None:
                            out[2 * k] = out[2 * k + 1] = None
                            continue
                        g, = torch.autograd.grad(v.sum(), x, retain_graph=True)
                        out[2 * k][head:head + CHUNK] = v.detach().reshape(-1)
                        out[2 * k + 1][head:head + CHUNK] = g
        finally:
            module.train(was_training)
        return tuple(out)

    def _head_columns(self):
        """The columns of the module's point-feature vector that the hand / object MLP reads (networks/model.py:288-299), or None where
        the features are not affine in xyz or the module is not a SeparateDecoder with specs."""
        specs = self.specs
        if specs is None or specs.get("PixelAlign", False) or not hasattr(self.module, "linh0"):
            return None
        pf, style = int(specs["PointFeatSize"]), specs["EncodeStyle"]
        if style == "nerf" and pf > 3:
            return None
        a = torch.arange(pf, device=self.device)
        return {"nerf": (a, a), "hand": (a, a[:3]), "obj": (a[:3], a), "both": (a[:-3], torch.cat([a[:3], a[-3:]]))}[style]

    def decode_embedded(self, latent, embed, xyz):
        """(sdf_hand [M], sdf_obj [M]) of the module at xyz [M, 3] for a latent [L] and point embeddings in HipSdfDecoder.set_sample's
        layout (feat = E[:, :3] x + E[:, 3]) - as a torch graph: differentiable in all three.
          SeparateDecoder, features affine in xyz: embed = (hand [pf_h, 4], obj [pf_o, 4]); one module call per head (the two
            embeddings need not agree on the columns the heads share).
          CombinedDecoder, features affine in xyz: embed = (E [pf, 4],) - or None for plain xyz; one module call.
          NeRF-encoded features: embed must be None (no affine embedding exists; the encoding is the module path's own).
        ValueError for a pixel-aligned decoder (its latent is a feature map, not a code) and a module without specs."""
        specs = self.specs
        if specs is None or specs.get("PixelAlign", False):
            raise ValueError("decode_embedded: a decoder with specs and a per-sample latent code only")
        module = self.module
        was_training = module.training
        module.eval()
        try:
            xyz = xyz.to(self.device, torch.float32)
            lat = latent.reshape(1, -1).to(self.device, torch.float32).expand(xyz.shape[0], -1)
            pf, style = int(specs["PointFeatSize"]), specs["EncodeStyle"]
            affine = lambda E: xyz @ E[:, :3].t() + E[:, 3]
            if style == "nerf" and pf > 3:
                if embed is not None:
                    raise ValueError("decode_embedded: a NeRF-encoded decoder takes raw xyz; no affine embedding applies")
                out = module(torch.cat([lat, nerf_embedding(xyz, (pf - 3) // 6)], 1))
                return out[0].reshape(-1), out[1].reshape(-1)
            cols = self._head_columns()
            if cols is None:                    # CombinedDecoder: the one MLP reads the whole feature vector
                feats = xyz if embed is None else affine(embed[0].to(self.device, torch.float32))
                if feats.shape[1] != pf:
                    raise ValueError("decode_embedded: the embedding gives %d point features, the module reads %d" % (feats.shape[1], pf))
                out = module(torch.cat([lat, feats], 1))
                return out[0].reshape(-1), out[1].reshape(-1)
            if embed is None:
                if pf != 3:
                    raise ValueError("decode_embedded: this decoder needs a point embedding per head")
                embed = (torch.eye(3, 4, device=self.device),) * 2
            out = []
            for h, (E, c) in enumerate(zip(embed, cols)):
                q = torch.zeros(xyz.shape[0], pf, dtype=torch.float32, device=self.device).index_copy(1, c, affine(E.to(self.device, torch.float32)))
                out.append(module(torch.cat([lat, q], 1))[h].reshape(-1))
        finally:
            module.train(was_training)
        return tuple(out)

    def decode_points_vjp(self, xyz, w_hand=None, w_obj=None, want_sdf=True):
        """The interface of HipSdfDecoder.decode_points_vjp by torch autograd through the module's own forward on the bound sample:
        SdfVjp(sdf_hand, sdf_obj, d_latent [L], d_embed, d_fold = None).  d_latent comes from a latent that requires grad; d_embed[h] =
        g_feat^T [xyz, 1] over head h's own feature columns (g_feat = the gradient with respect to the point features), None for NeRF
        features.  ValueError for a pixel-aligned sample."""
        from .hip_decoder import SdfVjp
        if self._sample is None:
            raise ValueError("no sample bound: call set_sample first")
        specs = self.specs
        if specs is not None and specs.get("PixelAlign", False):
            raise ValueError("decode_points_vjp: a pixel-aligned sample has no per-sample latent code to differentiate")
        xyz = xyz.detach().to(self.device, torch.float32).contiguous()
        M = xyz.shape[0]
        ws = [None if w is None else w.detach().to(self.device, torch.float32).reshape(-1) for w in (w_hand, w_obj)]
        for w in ws:
            if w is not None and w.numel() != M:
                raise ValueError("weights have %d elements, expected %d" % (w.numel(), M))
        latent, mano, obj, _ = self._sample
        cols = self._head_columns()
        module = self.module
        was_training = module.training
        module.eval()
        sdf = [None, None]
        d_latent = torch.zeros(latent.numel(), dtype=torch.float32, device=self.device)
        d_embed = None if cols is None else [torch.zeros(len(c), 4, dtype=torch.float32, device=self.device) for c in cols]
        try:
            with torch.enable_grad():
                for head in range(0, M, CHUNK):
                    x = xyz[head:head + CHUNK]
                    lat = latent.detach().reshape(1, -1).clone().requires_grad_()
                    q = x
                    if specs is not None and specs["PointFeatSize"] > 3:
                        if mano is not None and specs["EncodeStyle"] != "nerf":
                            q = kinematic_embedding(x, mano, specs["PointFeatSize"], specs["SdfScaleFactor"], obj, specs["EncodeStyle"])
                        else:
                            q = nerf_embedding(x, (specs["PointFeatSize"] - 3) // 6)
                    q = q.detach().requires_grad_()
                    values = module(torch.cat([lat.expand(x.shape[0], -1), q], 1))[:2]
                    x1 = torch.cat([x, torch.ones(x.shape[0], 1, dtype=torch.float32, device=self.device)], 1)
                    for k, (w, v) in enumerate(zip(ws, values)):
                        if w is None or v is None:
                            continue
                        if want_sdf:
                            if sdf[k] is None:
                                sdf[k] = torch.empty(M, dtype=torch.float32, device=self.device)
                            sdf[k][head:head + CHUNK] = v.detach().reshape(-1)
                        g_lat, g_q = torch.autograd.grad((v.reshape(-1) * w[head:head + CHUNK]).sum(), (lat, q), retain_graph=True)
                        d_latent += g_lat.reshape(-1)
                        if d_embed is not None:
                            d_embed[k] += g_q[:, cols[k]].t() @ x1
        finally:
            module.train(was_training)
        return SdfVjp(sdf[0], sdf[1], d_latent, None if d_embed is None else tuple(d_embed), None)

    def trace_rays(self, origins, dirs, t0, t1, hand=True, obj=True, max_steps=64, refine_steps=6, step_scale=1.0, min_step=1e-3,
                   max_step=0.05, want_bracket=False, want_evals=False):
        """The interface and the rule of HipSdfDecoder.trace_rays on the module (render.trace_lockstep): per head, all rays in lockstep
        under masks, one module call per step.  Covers every variant the module path covers.  A head the module does not have is None."""
        from .render import pack_rays, trace_lockstep
        if self._sample is None:
            raise ValueError("no sample bound: call set_sample first")
        rays = pack_rays(origins, dirs, t0, t1, self.device)
        res = {}
        for k, (name, on) in enumerate((("hand", hand), ("obj", obj))):
            res[name] = None
            if not on:
                continue
            absent = []

            def sdf_of(points, k=k):
                v = self._decode(points)[k]
                if v is None:
                    absent.append(True)
                    return torch.ones(points.shape[0], dtype=torch.float32, device=self.device)
                return v
            with torch.no_grad():
                r = trace_lockstep(sdf_of, rays, max_steps, refine_steps, step_scale, min_step, max_step)
            if absent:
                continue
            res[name] = {key: r[key] for key, keep in (("t", True), ("status", True), ("bracket", want_bracket), ("evals", want_evals)) if keep}
        return res

    def project_points(self, xyz, head, max_iters=8, tol=1e-6, max_move=2.0 / 127, min_grad2=1e-12):
        """The interface and the rule of HipSdfDecoder.project_points on the module (project.project_lockstep over this decoder's own
        decode_points_grad): all points in lockstep under masks, one differentiated module call per step.  Covers every variant the
        module path covers."""
        from .project import grad_of_head, project_lockstep
        if self._sample is None:
            raise ValueError("no sample bound: call set_sample first")
        xyz = xyz.detach().to(self.device, torch.float32).reshape(-1, 3).contiguous()
        return project_lockstep(grad_of_head(self, head), xyz, max_iters, tol, max_move, min_grad2)

    def classify_points(self, xyz, want_sdf=True):
        if not self.num_class:
            raise ValueError("this decoder has no classifier_head (specs['ClassifierBranch'] is off)")
        h, o, s = self._decode(xyz.detach().to(self.device, torch.float32).contiguous(), want_scores=True)
        return (h if want_sdf else None), (o if want_sdf else None), s, s.argmax(dim=1)

    def decode_grid(self, N, origin3, voxel_size, grid_mode=_native.GRID_REFERENCE, want_bbox=True, hand=True, obj=True, check_range=None):
        """Both heads on the N^3 lattice (the module always evaluates both, like the reference); lattice coordinates from
        asdf_debug_grid_coords, i.e. the device function of the HIP kernels."""
        L = _native.lib()
        coords = torch.empty((N ** 3, 3), dtype=torch.float32, device=self.device)
        org = (ctypes.c_float * 3)(*[float(np.float32(o)) for o in origin3])
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _native.check(L.asdf_debug_grid_coords(int(N), org, ctypes.c_float(float(np.float32(voxel_size))), int(grid_mode), 0, N ** 3,
                                                   coords.data_ptr(), stream), "asdf_debug_grid_coords")
            vh, vo, _ = self._decode(coords)
            vh = vh.reshape(N, N, N)
            vo = vo.reshape(N, N, N) if vo is not None else None
            obj = obj and vo is not None
            bbox = None
            if want_bbox:
                S = _native.BOX_STRIDE
                bbox = torch.empty(_native.BOX_WORDS, dtype=torch.int32, device=self.device)
                tmp = torch.empty(_native.BOX_WORDS, dtype=torch.int32, device=self.device)
                for k, (on, vol) in enumerate(((hand, vh), (obj, vo))):
                    if on:
                        _native.check(L.asdf_neg_bbox(vol.data_ptr(), N, N, N, tmp.data_ptr(), stream), "asdf_neg_bbox")
                        bbox[S * k:S * k + S] = tmp[:S]
                    else:       # an empty box: min = INT_MAX, max = -1, count and range word 0
                        bbox[S * k:S * k + S] = torch.tensor([0x7fffffff] * 3 + [-1] * 3 + [0, 0], dtype=torch.int32, device=self.device)
                bbox[list(_native.BOX_RANGE_WORDS)] = 0
        return (vh if hand else None), (vo if obj else None), bbox
