"""The cases of the MANO layer's tests, shared by the goldens' recipe (tests/golden/make_mano_goldens.py), the host tests
(test_mano_truth.py) and the device tests (test_gpu_mano.py).  Inputs come from the counter-based generator, so every machine makes the
same bits; the model is ManoModel.synthetic(MODEL_SEED, V) and is regenerated, never stored.

What the set covers: V = 778 (three full passes of a 256-thread workgroup and a last pass of 10 vertices) and V = 70 (less than a
workgroup, more than a wave); ncomps 6, 15 and 45; the all-zero pose with a zero mean (every joint on the 1e-8 branch of the norm),
a single angle of 1e-6, moderate poses (sigma 0.6), a joint turned beyond pi; shape 0, +2 and -2; centring on joint 0 and a
translation without centring; B = 1 and B = 3 (whose first sample is the B = 1 sample of "moderate6").
"""
import collections

import numpy as np

from alignsdf_amd import synthetic

MODEL_SEED = 3
Case = collections.namedtuple("Case", "name V ncomps flat_mean center_idx pose shape trans")


def _pose(seed, ncomps, B=1, sigma=0.6):
    return (sigma * synthetic.normal((B, 3 + ncomps), 52000 + seed)).astype(np.float32)


def _shape(seed, B=1):
    return synthetic.normal((B, 10), 53000 + seed).astype(np.float32)


def _trans(seed, B=1):
    return (0.3 * synthetic.normal((B, 3), 54000 + seed)).astype(np.float32)


def _cases():
    out = []
    add = lambda *a: out.append(Case(*a))
    z = lambda *s: np.zeros(s, np.float32)
    for V in (778, 70):
        tag = str(V)
        add("zero" + tag, V, 6, True, 0, z(1, 9), z(1, 10), None)
        tiny = z(1, 18)
        tiny[0, 1] = 1e-6
        add("tiny" + tag, V, 15, True, 0, tiny, z(1, 10), None)
        add("moderate6_" + tag, V, 6, False, 0, _pose(1, 6), _shape(1), None)
        add("moderate15_trans_" + tag, V, 15, False, None, _pose(2, 15), np.full((1, 10), 2.0, np.float32), _trans(2))
        add("moderate45_" + tag, V, 45, False, 0, _pose(3, 45), np.full((1, 10), -2.0, np.float32), None)
        far = _pose(4, 45, sigma=0.3)
        far[0, :3] = (2.3, -1.9, 1.6)          # |root axis-angle| = 3.39 > pi
        add("beyond_pi_" + tag, V, 45, False, None, far, _shape(4), _trans(4))
        batch_pose, batch_shape = _pose(5, 6, B=3), _shape(5, B=3)
        batch_pose[0], batch_shape[0] = _pose(1, 6)[0], _shape(1)[0]
        add("batch3_" + tag, V, 6, False, 0, batch_pose, batch_shape, None)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
OUTPUTS = ("verts", "joints", "hand_pose", "global_trans", "center")
GRADS = ("d_pose", "d_shape")


def cotangents(case):
    """Seeded cotangents of (verts, joints, global_trans, center) for the case, float32; center's is None when no centre is taken."""
    B, s = case.pose.shape[0], 55000 + 10 * CASES.index(case)
    n = lambda i, *shape: synthetic.normal((B,) + shape, s + i).astype(np.float32)
    return {"verts": n(0, case.V, 3), "joints": n(1, 21, 3), "global_trans": n(2, 16, 4, 4),
            "center": n(3, 1, 3) if case.trans is None and case.center_idx is not None else None}


def model_of(case):
    from alignsdf_amd.mano import ManoModel
    return ManoModel.synthetic(MODEL_SEED, case.V)


def statement(case, dtype, device="cpu"):
    """mano_torch's outputs and its autograd gradients for the case's cotangents, as float64 numpy arrays."""
    import torch
    from alignsdf_amd.mano import mano_torch
    model = model_of(case)
    t = lambda a: None if a is None else torch.from_numpy(a).to(device=device, dtype=dtype)
    pose, shape = t(case.pose).requires_grad_(True), t(case.shape).requires_grad_(True)
    out = dict(zip(OUTPUTS, mano_torch(model, pose, shape, t(case.trans), center_idx=case.center_idx,
                                                       flat_hand_mean=case.flat_mean)))
    cot = cotangents(case)
    loss = sum((out[k] * t(c)).sum() for k, c in cot.items() if c is not None)
    d_pose, d_shape = torch.autograd.grad(loss, (pose, shape))
    res = {k: v.detach().cpu().double().numpy() for k, v in out.items() if v is not None}
    res.update(d_pose=d_pose.cpu().double().numpy(), d_shape=d_shape.cpu().double().numpy())
    return res


# The known-answer fit: 300 Adam steps at lr 0.02 from the truth + 0.3 N(0, 1) in the pose and a zero shape.  The fp64 statement ended
# at FIT_FP64_FINAL_RMS where tests/test_mano_truth.py was written (rms vertex distance 1.996e-2 -> 1.381e-7; the fp32 statement:
# 1.40e-7; the reference layer, on a model of its own, went 3.3e-2 -> 8.9e-6); the bound is ten times that, for the host test and for
# the device fit (test_gpu_mano_fit.py) alike.
FIT_FP64_FINAL_RMS = 1.381e-7
FIT_RMS_BOUND = 10.0 * FIT_FP64_FINAL_RMS
FIT_STEPS, FIT_LR, FIT_NCOMPS = 300, 0.02, 15


def fit_problem(dtype=None, device="cpu"):
    """(model, pose*, shape*, target vertices, start pose) of the known-answer fit."""
    import torch
    from alignsdf_amd.mano import mano_torch
    model = model_of(BY_NAME["zero778"])
    t = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype or torch.float64)
    pose_true = t(0.4 * synthetic.normal((1, 3 + FIT_NCOMPS), 56001))
    shape_true = t(0.8 * synthetic.normal((1, 10), 56002))
    with torch.no_grad():
        target = mano_torch(model, pose_true, shape_true, center_idx=0)[0]
    start = pose_true + 0.3 * t(synthetic.normal((1, 3 + FIT_NCOMPS), 56003))
    return model, pose_true, shape_true, target, start
