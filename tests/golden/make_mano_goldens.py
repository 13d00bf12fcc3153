"""Generate tests/golden/ref_mano_layer.npz by RUNNING THE REFERENCE's hand layer (manopth/manolayer.py of zerchen/AlignSDF) on the host,
on the synthetic models and inputs of tests/mano_cases.py.  Runs only where the reference tree is (make_ref_goldens.REF, or the
directory named by ALIGNSDF_REFERENCE); what it writes is data: per case the inputs (pose, shape, trans), the layer's fp32 outputs
(verts, joints, hand_pose, global_trans, center), its fp32 autograd gradients (d_pose, d_shape) of sum(output x cotangent) over the
seeded cotangents of mano_cases.cotangents, and for every one of those `E_ref`: the largest difference between the layer's fp32
result and the SAME layer's fp64 result on the same inputs - the reference's own rounding error, the bound of the tests.

The layer is built without its constructor (which wants the licensed pickle and chumpy): ManoLayer.__new__, nn.Module.__init__, then the
buffers the constructor would register, from the synthetic model.  Its forward hard-codes the right hand's tip vertex ids; for a model
without those vertices (V = 70) the same forward is compiled with the model's ids in their place - nothing else differs.
"""
import inspect
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from make_ref_goldens import REF  # noqa: E402
import mano_cases  # noqa: E402
from alignsdf_amd.mano import RIGHT_TIPS  # noqa: E402


def reference_layer_class():
    ref = os.environ.get("ALIGNSDF_REFERENCE", REF)
    for name in ("chumpy", "cv2", "mano.webuser.smpl_handpca_wrapper_HAND_only"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["mano.webuser.smpl_handpca_wrapper_HAND_only"].ready_arguments = None
    sys.path.insert(0, ref)
    from manopth import manolayer
    return manolayer


def reference_layer(module, model, ncomps, center_idx, flat_mean, dtype):
    layer = module.ManoLayer.__new__(module.ManoLayer)
    torch.nn.Module.__init__(layer)
    layer.center_idx, layer.robust_rot, layer.rot, layer.flat_hand_mean, layer.side = center_idx, False, 3, flat_mean, "right"
    layer.use_pca, layer.joint_rot_mode, layer.root_rot_mode, layer.ncomps = True, "axisang", "axisang", ncomps
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    layer.register_buffer("th_betas", torch.zeros(1, 10, dtype=dtype))
    layer.register_buffer("th_shapedirs", t(model.shapedirs))
    layer.register_buffer("th_posedirs", t(model.posedirs))
    layer.register_buffer("th_v_template", t(model.v_template).unsqueeze(0))
    layer.register_buffer("th_J_regressor", t(model.J_regressor))
    layer.register_buffer("th_weights", t(model.weights))
    layer.register_buffer("th_hands_mean", t(np.zeros(45, np.float32) if flat_mean else model.hands_mean).unsqueeze(0))
    layer.register_buffer("th_selected_comps", t(model.comps[:ncomps]))
    layer.kintree_parents = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]
    if tuple(int(i) for i in model.tips) != RIGHT_TIPS:
        src = textwrap.dedent(inspect.getsource(module.ManoLayer.forward))
        assert src.count(repr(list(RIGHT_TIPS))) == 1
        ns = {}
        exec(compile(src.replace(repr(list(RIGHT_TIPS)), repr([int(i) for i in model.tips])), "<forward with the model's tips>", "exec"),
             module.__dict__, ns)
        layer.forward = types.MethodType(ns["forward"], layer)
    return layer


def run(module, case, dtype):
    model = mano_cases.model_of(case)
    layer = reference_layer(module, model, case.ncomps, case.center_idx, case.flat_mean, dtype)
    pose = torch.from_numpy(case.pose).to(dtype).requires_grad_(True)
    shape = torch.from_numpy(case.shape).to(dtype).requires_grad_(True)
    kw = {} if case.trans is None else {"th_trans": torch.from_numpy(case.trans).to(dtype)}
    verts, joints, hand_pose, global_trans, center = layer(pose, th_betas=shape, **kw)
    out = {"verts": verts, "joints": joints, "hand_pose": hand_pose, "global_trans": global_trans, "center": center}
    cot = mano_cases.cotangents(case)
    loss = sum((out[k] * torch.from_numpy(c).to(dtype)).sum() for k, c in cot.items() if c is not None)
    d_pose, d_shape = torch.autograd.grad(loss, (pose, shape))
    res = {k: v.detach().numpy() for k, v in out.items() if v is not None}
    res.update(d_pose=d_pose.numpy(), d_shape=d_shape.numpy())
    return res


def main():
    module = reference_layer_class()
    arrays = {}
    for case in mano_cases.CASES:
        r32, r64 = run(module, case, torch.float32), run(module, case, torch.float64)
        arrays[case.name + ".pose"], arrays[case.name + ".shape"] = case.pose, case.shape
        if case.trans is not None:
            arrays[case.name + ".trans"] = case.trans
        for k, v in r32.items():
            assert v.dtype == np.float32 and np.isfinite(v).all(), (case.name, k)
            arrays["%s.%s" % (case.name, k)] = v
            arrays["%s.E_ref.%s" % (case.name, k)] = np.float64(np.abs(v.astype(np.float64) - r64[k]).max())
        print(case.name, {k: "%.2e" % arrays["%s.E_ref.%s" % (case.name, k)] for k in r32})
    path = os.path.join(HERE, "ref_mano_layer.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
