"""The MANO hand layer (csrc/mano.hip; the rule is worded in include/alignsdf_hip.h): pose coefficients and shape values in, 778 vertices,
21 joints and the 16 joint transforms out - the `global_trans` / `rot_center` every pose-aligned path of this package consumes - and the
reverse mode of all of it, so that a pose can be FITTED (mano_fit.py).

Only the configuration networks/manobranch.py uses is built: PCA pose coefficients behind three global axis-angle values, the right
hand, manopth/manolayer.py:126-271 with rodrigues_layer.py:43-54.  `mano_torch` states the rule in torch, in any dtype and on any
device - fp64 on the host is the truth the kernels are held to -; `ManoLayer` runs the kernels on device tensors.

No MANO asset ships with the package (its licence forbids that): `ManoModel.from_npz` reads what tools/mano_pkl_to_npz.py writes from
the official pickle, `ManoModel.synthetic` makes a hand-sized stand-in from the counter-based generator for tests and measurements.
"""
import ctypes

import numpy as np
import torch

from . import _native, synthetic

NUM_JOINTS = 16
PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)
# the 21 output joints: 16 chain translations then 5 tip vertices, in the order of the reference's visualisation utilities
JOINT_ORDER = (0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20)
RIGHT_TIPS = (745, 317, 444, 556, 673)
MAX_VERTS = 1024            # ASDF_MANO_MAX_VERTS
ARRAYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "hands_mean", "comps", "tips")


class ManoModel:
    """The arrays of one hand model, fp32 / int32 on the host: v_template [V, 3], shapedirs [V, 3, 10], posedirs [V, 3, 135],
    J_regressor [16, V] (dense), weights [V, 16], hands_mean [45], comps [45, 45] (PCA rows; a layer takes the first ncomps),
    tips [5] (vertex ids), faces [F, 3]."""

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, weights, hands_mean, comps, tips, faces):
        f32 = lambda a, shape: np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))
        self.v_template = f32(v_template, (-1, 3))
        V = self.V = int(self.v_template.shape[0])
        self.shapedirs = f32(shapedirs, (V, 3, 10))
        self.posedirs = f32(posedirs, (V, 3, 135))
        self.J_regressor = f32(J_regressor, (NUM_JOINTS, V))
        self.weights = f32(weights, (V, NUM_JOINTS))
        self.hands_mean = f32(hands_mean, (45,))
        self.comps = f32(comps, (-1, 45))
        self.tips = np.ascontiguousarray(np.asarray(tips, np.int32).reshape(5))
        self.faces = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))
        if not 1 <= V <= MAX_VERTS:
            raise ValueError("a model of 1..%d vertices is needed, got %d" % (MAX_VERTS, V))
        if self.tips.min() < 0 or self.tips.max() >= V:
            raise ValueError("tip vertex ids outside [0, %d)" % V)
        self._cache = {}

    @classmethod
    def from_npz(cls, path):
        with np.load(path) as z:
            return cls(*[z[k] for k in ARRAYS], z["faces"])

    def save_npz(self, path):
        np.savez(path, faces=self.faces, **{k: getattr(self, k) for k in ARRAYS})

    @classmethod
    def synthetic(cls, seed=0, V=778):
        """A stand-in with MANO's structure and size (extent about 0.1 m): vertex v hangs on joint v % 16 - it sits near that joint, the
        joint's regressor row and the vertex's skinning row are heaviest there - but every row is dense, non-negative and sums to 1."""
        s = 41000 + 100 * int(seed)
        own = np.arange(V) % NUM_JOINTS
        rest = np.zeros((NUM_JOINTS, 3))
        for j in range(1, NUM_JOINTS):
            f, l = divmod(j - 1, 3)
            rest[j] = (0.045 + 0.022 * l, 0.019 * (f - 2), 0.004 * (f - 2) ** 2 - 0.008)
        rest += 0.003 * synthetic.normal((NUM_JOINTS, 3), s + 1)
        rest[0] = 0.0
        v_template = rest[own] + 0.007 * synthetic.normal((V, 3), s + 2)
        shapedirs = 0.003 * synthetic.normal((V, 3, 10), s + 3)
        posedirs = 0.002 * synthetic.normal((V, 3, 135), s + 4)
        reg = synthetic.uniform((NUM_JOINTS, V), s + 5) * (0.02 + (own[None, :] == np.arange(NUM_JOINTS)[:, None]))
        reg /= reg.sum(1, keepdims=True)
        w = synthetic.uniform((V, NUM_JOINTS), s + 6) ** 4 * 0.3 + 2.0 * (own[:, None] == np.arange(NUM_JOINTS)[None, :])
        w /= w.sum(1, keepdims=True)
        hands_mean = 0.2 * synthetic.normal((45,), s + 7)
        comps = synthetic.normal((45, 45), s + 8) / np.sqrt(45.0)
        rounds = max(V // NUM_JOINTS, 1)
        # (MANO's own tip ids where the model has them - the reference layer hard-codes those -, else a vertex of each last finger joint)
        tips = np.array(RIGHT_TIPS if V > max(RIGHT_TIPS) else
                        [min((3 * f + 3) + NUM_JOINTS * ((rounds - 1 - f) % rounds), V - 1 - f) for f in range(5)])
        faces = np.stack([np.arange(V - 2), np.arange(1, V - 1), np.arange(2, V)], 1) if V >= 3 else np.zeros((0, 3))
        return cls(v_template, shapedirs, posedirs, reg, w, hands_mean, comps, tips, faces)

    def tensors(self, dtype, device):
        """The arrays as torch tensors of `dtype` on `device` (made once per pair; tips stay int64)."""
        key = (dtype, str(device))
        if key not in self._cache:
            t = {k: torch.from_numpy(getattr(self, k)).to(device=device, dtype=dtype) for k in ARRAYS[:-1]}
            t["tips"] = torch.from_numpy(self.tips.astype(np.int64)).to(device)
            self._cache[key] = t
        return self._cache[key]


def rodrigues(axisang):
    """Rotation matrices [N, 3, 3] of axis-angle rows [N, 3] by way of a unit quaternion, as the reference layer goes: the angle is the
    norm of axisang + 1e-8 (every component shifted), which keeps a zero rotation finite and differentiable; the quaternion
    (cos, sin * axis) of half that angle is normalised once more before it becomes a matrix."""
    angle = torch.linalg.vector_norm(axisang + 1e-8, dim=1, keepdim=True)
    half = angle * 0.5
    quat = torch.cat([half.cos(), half.sin() * (axisang / angle)], 1)
    w, x, y, z = (quat / torch.linalg.vector_norm(quat, dim=1, keepdim=True)).unbind(1)
    # (squares as squares and each mixed product formed once: autograd then adds up the uses of w, x, y, z in the reference's order -
    # with w * w in place of the square, d_pose left the reference's fp32 bits by up to 1.9e-6)
    ww, xx, yy, zz = w.square(), x.square(), y.square(), z.square()
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    rows = ((ww + xx - yy - zz, 2 * xy - 2 * wz, 2 * wy + 2 * xz),
            (2 * wz + 2 * xy, ww - xx + yy - zz, 2 * yz - 2 * wx),
            (2 * xz - 2 * wy, 2 * wx + 2 * yz, ww - xx - yy + zz))
    return torch.stack([torch.stack(row, -1) for row in rows], -2)


def _homogeneous(rot, t):
    """[..., 4, 4] from rot [..., 3, 3] and t [..., 3]."""
    top = torch.cat([rot, t.unsqueeze(-1)], -1)
    last = top.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(*top.shape[:-2], 1, 4)
    return torch.cat([top, last], -2)


def mano_torch(model, pose, shape, trans=None, *, center_idx=0, flat_hand_mean=False):
    """(verts [B, V, 3], joints [B, 21, 3], hand_pose [B, 45], global_trans [B, 16, 4, 4], center [B, 1, 3] or None) of
    pose [B, 3 + ncomps] and shape [B, 10], in their dtype on their device; differentiable by autograd.  `hand_pose` is the
    reference layer's third return: coefficients x components, without the mean.  With `trans` [B, 3] it is added to vertices and
    joints; without, joint `center_idx` (None: nothing) is subtracted and returned.  The sums run in the reference layer's order."""
    B, nc = int(pose.shape[0]), int(pose.shape[1]) - 3
    if not 1 <= nc <= 45:
        raise ValueError("pose needs 3 + ncomps columns, ncomps in 1..45")
    m = model.tensors(pose.dtype, pose.device)
    hand_pose = pose[:, 3:].mm(m["comps"][:nc])
    mean = torch.zeros_like(m["hands_mean"]) if flat_hand_mean else m["hands_mean"]
    full = torch.cat([pose[:, :3], mean.unsqueeze(0) + hand_pose], 1)
    rots = rodrigues(full.reshape(-1, 3)).reshape(B, NUM_JOINTS * 9)
    pose_map = (rots - torch.eye(3, dtype=pose.dtype, device=pose.device).view(1, 9).repeat(B, NUM_JOINTS))[:, 9:]
    rots = rots.view(B, NUM_JOINTS, 3, 3)

    v_shaped = torch.matmul(m["shapedirs"], shape.transpose(1, 0)).permute(2, 0, 1) + m["v_template"].unsqueeze(0)
    J = torch.matmul(m["J_regressor"], v_shaped)
    v_posed = v_shaped + torch.matmul(m["posedirs"], pose_map.transpose(0, 1)).permute(2, 0, 1)

    # the chain, a level at a time: root, then the three joints of each of the five fingers
    levels = [_homogeneous(rots[:, 0], J[:, 0]).unsqueeze(1)]
    above, above_j = levels[0].repeat(1, 5, 1, 1).view(B * 5, 4, 4), J[:, :1]
    for level in (1, 2, 3):
        idx = [level + 3 * f for f in range(5)]
        rel = _homogeneous(rots[:, idx], J[:, idx] - above_j).view(B * 5, 4, 4)
        above, above_j = torch.matmul(above, rel), J[:, idx]
        levels.append(above.view(B, 5, 4, 4))
    by_level = [0] + [1 + 5 * ((j - 1) % 3) + (j - 1) // 3 for j in range(1, NUM_JOINTS)]
    global_trans = torch.cat(levels, 1)[:, by_level]

    # skinning: every transform loses what its rotation makes of its own rest joint (rows [R | t - R J]), the transforms are blended
    # per vertex with the skinning weights, and a vertex is its blend applied to its posed rest position
    carried = torch.matmul(global_trans[..., :3], J.unsqueeze(-1))              # [B, 16, 4, 1]: R J over a zero
    rest_free = torch.cat([global_trans[..., :3], global_trans[..., 3:] - carried], -1)
    blend = torch.matmul(rest_free.permute(0, 2, 3, 1), m["weights"].t())       # [B, 4, 4, V]
    px, py, pz = (v_posed[..., k].unsqueeze(1) for k in range(3))               # [B, 1, V] each
    verts = (blend[:, :3, 0] * px + blend[:, :3, 1] * py + blend[:, :3, 2] * pz + blend[:, :3, 3]).transpose(1, 2)

    joints = torch.cat([global_trans[:, :, :3, 3], verts[:, m["tips"]]], 1)[:, list(JOINT_ORDER)]
    center = None
    if trans is not None:
        joints, verts = joints + trans.unsqueeze(1), verts + trans.unsqueeze(1)
    elif center_idx is not None:
        center = joints[:, center_idx].unsqueeze(1)
        joints, verts = joints - center, verts - center
    return verts, joints, hand_pose, global_trans, center


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


class DeviceModel:
    """A model's workspace on one device: uploaded and prepared once (asdf_mano_prepare), read by every forward / reverse launch."""

    def __init__(self, model, ncomps, device, flat_hand_mean=False):
        self.V, self.ncomps, self.device = model.V, int(ncomps), torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("a CUDA device is needed (there is no CPU fallback)")
        n = ctypes.c_size_t()
        _native.check(_native.lib().asdf_mano_workspace_bytes(self.V, self.ncomps, ctypes.byref(n)), "asdf_mano_workspace_bytes")
        self.bytes = n.value
        self.ws = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        mean = np.zeros(45, np.float32) if flat_hand_mean else model.hands_mean
        src = [up(model.v_template), up(model.shapedirs), up(model.posedirs), up(model.J_regressor), up(model.weights), up(mean),
               up(model.comps[:self.ncomps]), up(model.tips)]
        with torch.cuda.device(self.device):
            _native.check(_native.lib().asdf_mano_prepare(self.V, self.ncomps, *[t.data_ptr() for t in src], self.ws.data_ptr(), self.bytes,
                                                          _stream(self.device)), "asdf_mano_prepare")
        self._src = src         # (stream-ordered: the uploads stay alive with the workspace)
        self.comps = src[6]     # [ncomps, 45] on the device: the adjoint of the third return

    def forward(self, pose, shape, trans, center_idx, want=(True,) * 5):
        """The launch: (verts, joints, global_trans, center, hand_pose), None where `want` says no (and center without centring)."""
        B = int(pose.shape[0])
        new = lambda on, *s: torch.empty((B,) + s, dtype=torch.float32, device=self.device) if on else None
        centring = trans is None and center_idx is not None
        out = (new(want[0], self.V, 3), new(want[1], 21, 3), new(want[2], NUM_JOINTS, 4, 4), new(want[3] and centring, 1, 3), new(want[4], 45))
        with torch.cuda.device(self.device):
            _native.check(_native.lib().asdf_mano_forward(self.ws.data_ptr(), self.bytes, self.V, self.ncomps, B, _ptr(pose), _ptr(shape),
                                                          _ptr(trans), -1 if center_idx is None else int(center_idx),
                                                          *[_ptr(o) for o in out], _stream(self.device)), "asdf_mano_forward")
        return out

    def backward(self, pose, shape, trans, center_idx, d_verts, d_joints, d_global_trans, d_center, out=None):
        """The reverse launch: (d_pose [B, 3 + ncomps], d_shape [B, 10]); any cotangent may be None."""
        B = int(pose.shape[0])
        d_pose, d_shape = out if out is not None else (torch.empty((B, 3 + self.ncomps), dtype=torch.float32, device=self.device),
                                                       torch.empty((B, 10), dtype=torch.float32, device=self.device))
        with torch.cuda.device(self.device):
            _native.check(_native.lib().asdf_mano_backward(self.ws.data_ptr(), self.bytes, self.V, self.ncomps, B, _ptr(pose), _ptr(shape),
                                                           _ptr(trans), -1 if center_idx is None else int(center_idx), _ptr(d_verts),
                                                           _ptr(d_joints), _ptr(d_global_trans), _ptr(d_center), d_pose.data_ptr(),
                                                           d_shape.data_ptr(), _stream(self.device)), "asdf_mano_backward")
        return d_pose, d_shape


def _plain(t, shape):
    return None if t is None else t.detach().to(torch.float32).reshape(shape).contiguous()


class _ManoFunction(torch.autograd.Function):
    """The forward kernel with the reverse kernel as its backward.  The kernels treat `trans` as a constant; it is added to every vertex
    and joint, so its gradient is the sum of their cotangents and is formed here, in torch, when it is asked for."""

    @staticmethod
    def forward(ctx, dev, center_idx, pose, shape, trans):
        B = int(pose.shape[0])
        p, s, t = _plain(pose, (B, 3 + dev.ncomps)), _plain(shape, (B, 10)), _plain(trans, (B, 3))
        verts, joints, gt, center, hand_pose = dev.forward(p, s, t, center_idx)
        ctx.dev, ctx.center_idx, ctx.trans, ctx.B = dev, center_idx, t, B
        ctx.save_for_backward(p, s)
        ctx.set_materialize_grads(False)
        if center is None:
            center = verts.new_zeros(0)
            ctx.mark_non_differentiable(center)
        return verts, joints, hand_pose, gt, center

    @staticmethod
    def backward(ctx, d_verts, d_joints, d_hand_pose, d_gt, d_center):
        p, s = ctx.saved_tensors
        dev, B = ctx.dev, ctx.B
        if ctx.trans is not None or ctx.center_idx is None:
            d_center = None
        d_pose, d_shape = dev.backward(p, s, ctx.trans, ctx.center_idx, _plain(d_verts, (B, dev.V, 3)), _plain(d_joints, (B, 21, 3)),
                                       _plain(d_gt, (B, NUM_JOINTS, 4, 4)), _plain(d_center, (B, 3)))
        if d_hand_pose is not None:         # (the third return is a plain product of the coefficients: its adjoint is one too)
            d_pose[:, 3:] += d_hand_pose.to(torch.float32).reshape(B, 45) @ dev.comps.t()
        d_trans = None
        if ctx.trans is not None and ctx.needs_input_grad[4]:
            d_trans = d_pose.new_zeros(B, 3)
            for d in (d_verts, d_joints):
                if d is not None:
                    d_trans = d_trans + d.to(torch.float32).reshape(B, -1, 3).sum(1)
        return None, None, d_pose, d_shape, d_trans


class ManoLayer:
    """Callable like the reference layer in the one configuration networks/manobranch.py builds (PCA coefficients, axis-angle root):
    layer(pose_coeffs [B, 3 + ncomps], th_betas [B, 10] or None, th_trans [B, 3] or None) -> (verts, joints, hand_pose, global_trans,
    center).  Device tensors run the kernels (a torch.autograd.Function whose backward is the reverse kernel), host tensors run
    mano_torch.  One difference, to keep the call free of read-backs: a `th_trans` that is given is added, whatever its value - the
    reference centres instead when its norm is zero."""

    def __init__(self, model, ncomps=6, center_idx=0, flat_hand_mean=False):
        if not 1 <= int(ncomps) <= 45:
            raise ValueError("ncomps in 1..45 is needed")
        if center_idx is not None and not 0 <= int(center_idx) < 21:
            raise ValueError("center_idx in 0..20 (or None) is needed")
        self.model, self.ncomps, self.center_idx, self.flat_hand_mean = model, int(ncomps), center_idx, bool(flat_hand_mean)
        self._dev = {}

    def device_model(self, device):
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = DeviceModel(self.model, self.ncomps, device, self.flat_hand_mean)
        return self._dev[key]

    def __call__(self, th_pose_coeffs, th_betas=None, th_trans=None, root_palm=False, share_betas=False):
        if root_palm or share_betas:
            raise NotImplementedError("root_palm / share_betas: networks/manobranch.py passes neither")
        pose = th_pose_coeffs
        if pose.dim() != 2 or pose.shape[1] != 3 + self.ncomps:
            raise ValueError("pose coefficients [B, %d] are needed, got %s" % (3 + self.ncomps, tuple(pose.shape)))
        B = int(pose.shape[0])
        shape = pose.new_zeros(B, 10) if th_betas is None or th_betas.numel() == 1 else th_betas
        if not pose.is_cuda:
            return mano_torch(self.model, pose, shape, th_trans, center_idx=self.center_idx, flat_hand_mean=self.flat_hand_mean)
        if B == 0:
            raise ValueError("an empty batch")
        dev = self.device_model(pose.device)
        verts, joints, hand_pose, gt, center = _ManoFunction.apply(dev, self.center_idx, pose, shape, th_trans)
        return verts, joints, hand_pose, gt, (center.reshape(B, 1, 3) if center.numel() else None)


def mano_results(layer, pose, shape, mano_root=None):
    """The dict ManoBranch.forward builds without absolute_depth (networks/manobranch.py:150-153): camera-space verts / joints around
    `mano_root` [B, 3] (None: the origin), and the quantities the pose-aligned decoders read."""
    verts, joints, hand_pose, global_trans, rot_center = layer(pose, shape)
    B = int(verts.shape[0])
    center3d = verts.new_zeros(B, 1, 3) if mano_root is None else mano_root.reshape(B, 1, 3).to(verts)
    return {"verts": center3d + verts, "joints": center3d + joints, "shape": shape, "pcas": pose, "pose": hand_pose,
            "center3d": center3d, "global_trans": global_trans, "rot_center": rot_center}
