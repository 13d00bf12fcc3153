"""Fit MANO parameters - to target vertices or joints, or to the hand the SDF decoder describes - and the flow that writes the
`pred_mano/` and `optim_mano/` directories the evaluator reads (evaluate.evaluate_mano; the reference's evaluator reads them too, its
own tree never writes the second).

The loop is Adam on (pose, shape).  Per step: one MANO forward, for the SDF term one decode_points_grad at the 778 vertices, one MANO
backward, one optimiser step - on device tensors the two MANO launches are the kernels of csrc/mano.hip (mano.ManoLayer), on host
tensors the torch statement.  Nothing is read back inside the loop; the loss history stays where the parameters are and is read once at
the end.

  python -m alignsdf_amd.mano_fit -e EXP -t TASK --codes DIR --mano_model FILE.npz [--steps N --lr X ...]
"""
import argparse
import collections
import json
import os

import numpy as np
import torch

from . import mano, ply

ManoFit = collections.namedtuple("ManoFit", "pose shape verts joints losses")
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8
FLOW_DEFAULTS = {"steps": 100, "lr": 0.01, "pose_prior": 1e-4, "shape_prior": 1e-4}


def sdf_cotangent(f, grad, scale_factor):
    """The cotangent of the centred vertices under mean_v |f(x_v)|, x_v = vertex * scale_factor / 2: sign(f) grad f * sf / (2 V)."""
    return torch.sign(f).unsqueeze(-1) * grad * (float(scale_factor) / (2.0 * f.shape[0]))


def fit_mano(layer, pose0, shape0, *, verts_target=None, joints_target=None, decoder=None, head="hand", scale_factor=None, steps=100,
             lr=0.01, pose_prior=0.0, shape_prior=0.0):
    """Adam on (pose [B, 3 + ncomps], shape [B, 10]) from (pose0, shape0), on their device and in their dtype, over the sum of
      mean squared distance to verts_target [B, V, 3] and / or joints_target [B, 21, 3] (each mean over B and the points),
      the SDF term mean_v |f_head(x_v)| at x_v = centred vertex * scale_factor / 2 - the inverse of kinematic_embedding's
        xyz * 2 / sf + rot_center - with value and gradient from decoder.decode_points_grad (a HipSdfDecoder, or a TorchModuleDecoder
        where grad_refusal() says no) and the cotangent sdf_cotangent into the layer's reverse; the sample bound to the decoder stays as
        it is - this fits a MANO hand TO the SDF hand (B = 1, a layer that centres),
      pose_prior * mean(coefficients^2) and shape_prior * mean(shape^2).
    Returns ManoFit(pose, shape, verts, joints of the fitted parameters, losses [steps] float64 on the host: the objective before each
    step)."""
    if verts_target is None and joints_target is None and decoder is None:
        raise ValueError("nothing to fit to: give verts_target, joints_target or decoder")
    pose, shape = pose0.detach().clone(), shape0.detach().clone()
    B = int(pose.shape[0])
    if decoder is not None:
        if scale_factor is None:
            raise ValueError("the SDF term needs scale_factor (specs['SdfScaleFactor'])")
        if B != 1 or layer.center_idx is None:
            raise ValueError("the SDF term fits one hand in the decoder's centred frame: B = 1 and a layer with center_idx")
        if head not in ("hand", "obj"):
            raise ValueError("head %r" % (head,))
    steps = int(steps)
    params = (pose, shape)
    m, v = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    losses = torch.zeros(max(steps, 1), dtype=pose.dtype, device=pose.device)
    for k in range(steps):
        p, s = pose.detach().requires_grad_(True), shape.detach().requires_grad_(True)      # (leaves over the parameters' own storage)
        verts, joints = layer(p, s)[:2]
        loss = verts.new_zeros(())
        if verts_target is not None:
            loss = loss + ((verts - verts_target) ** 2).sum(-1).mean()
        if joints_target is not None:
            loss = loss + ((joints - joints_target) ** 2).sum(-1).mean()
        if pose_prior:
            loss = loss + pose_prior * (p[:, 3:] ** 2).mean()
        if shape_prior:
            loss = loss + shape_prior * (s ** 2).mean()
        through = loss
        if decoder is not None:
            x = (verts.detach()[0] * (float(scale_factor) / 2.0)).to(torch.float32)
            got = decoder.decode_points_grad(x, hand=head == "hand", obj=head == "obj")
            f, g = got[:2] if head == "hand" else got[2:]
            loss = loss + f.abs().mean().to(loss.dtype)
            through = through + (verts[0] * sdf_cotangent(f, g, scale_factor).to(verts.dtype)).sum()
        d_pose, d_shape = torch.autograd.grad(through, (p, s))
        losses[k] = loss.detach()
        with torch.no_grad():
            for q, d, m1, m2 in zip((pose, shape), (d_pose, d_shape), m, v):
                m1.mul_(ADAM_B1).add_(d, alpha=1 - ADAM_B1)
                m2.mul_(ADAM_B2).addcmul_(d, d, value=1 - ADAM_B2)
                step = lr / (1 - ADAM_B1 ** (k + 1))
                q.addcdiv_(m1, (m2 / (1 - ADAM_B2 ** (k + 1))).sqrt_().add_(ADAM_EPS), value=-step)
    with torch.no_grad():
        verts, joints = layer(pose, shape)[:2]
    return ManoFit(pose, shape, verts, joints, losses[:steps].cpu().double().numpy())


def write_mano(directory, name, verts, joints, shape, pose, faces):
    """<directory>/<name>.json with the reference's keys (joints [21, 3], vertices [V, 3], shape [10], pose [45]) and <name>.ply."""
    os.makedirs(directory, exist_ok=True)
    host = lambda t: np.asarray(t.detach().cpu().double().numpy() if torch.is_tensor(t) else t, np.float64)
    rec = {"joints": host(joints).reshape(21, 3).tolist(), "vertices": host(verts).reshape(-1, 3).tolist(),
           "shape": host(shape).reshape(-1).tolist(), "pose": host(pose).reshape(-1).tolist()}
    with open(os.path.join(directory, name + ".json"), "w") as f:
        json.dump(rec, f)
    ply.write_ply(os.path.join(directory, name + ".ply"), host(verts).reshape(-1, 3), faces)
    return rec


def load_mano_codes(code_dir, name):
    """(latent [1, L], mano_pose [1, 3 + ncomps], mano_shape [1, 10], obj_trans or None, mano_root [1, 3] or None) of one codes file."""
    with np.load(os.path.join(code_dir, name + ".npz")) as z:
        if "mano_pose" not in z.files or "mano_shape" not in z.files:
            raise ValueError("%s.npz holds no mano_pose / mano_shape: nothing to start the fit from" % name)
        f32 = lambda k: np.asarray(z[k], np.float32) if k in z.files else None
        return f32("latent"), f32("mano_pose").reshape(1, -1), f32("mano_shape").reshape(1, 10), f32("obj_trans"), f32("mano_root")


def gradient_decoder(evaluator, module, specs, made=None):
    """The evaluator the SDF term asks for value and gradient: `evaluator` itself unless its grad_refusal() names a reason
    (CombinedDecoder, NeRF-encoded point features, a pixel-aligned sample) - then a TorchModuleDecoder over `module`, the product path
    of refused decoders, made once per reason in `made`.  NotImplementedError when there is no nn.Module to call."""
    refusal = getattr(evaluator, "grad_refusal", None)
    why = refusal() if callable(refusal) and not hasattr(evaluator, "decode_embedded") else None
    if why is None:
        return evaluator
    if not isinstance(module, torch.nn.Module):
        raise NotImplementedError("the gradient kernel does not cover this decoder (%s) and there is no nn.Module for the module path" % why)
    made = {} if made is None else made
    if why not in made:
        from .torch_decoder import TorchModuleDecoder
        made[why] = TorchModuleDecoder(module, specs, "mano_fit: " + why, evaluator.device)
    return made[why]


def run(specs, decoder_module, model, code_dir, out_root, names=None, device="cuda", steps=100, lr=0.01, pose_prior=1e-4, shape_prior=1e-4,
        center_idx=0, decoder=None):
    """The flow: per sample of code_dir, the hand of the given parameters into <out_root>/pred_mano/, then the parameters fitted to the
    decoder's hand SDF (under the given parameters' own pose alignment; gradient_decoder picks the evaluator) into
    <out_root>/optim_mano/.  Hands are written in the camera frame around `mano_root` where the file has one, else root-centred.
    Returns [{"name", "first", "last", "steps"}]."""
    from .utils import utils
    device = torch.device(device)
    if names is None:
        names = sorted(f[:-4] for f in os.listdir(code_dir) if f.endswith(".npz"))
    layers, records, fallbacks = {}, [], {}
    for name in names:
        latent, pose, shape, obj_trans, root = load_mano_codes(code_dir, name)
        nc = pose.shape[1] - 3
        layer = layers.setdefault(nc, mano.ManoLayer(model, ncomps=nc, center_idx=center_idx))
        pose_d, shape_d = torch.from_numpy(pose).to(device), torch.from_numpy(shape).to(device)
        root_d = None if root is None else torch.from_numpy(root.reshape(1, 3)).to(device)
        with torch.no_grad():
            given = mano.mano_results(layer, pose_d, shape_d, root_d)
        write_mano(os.path.join(out_root, "pred_mano"), name, given["verts"][0], given["joints"][0], shape, given["pose"][0], model.faces)
        # the decoder is bound under the GIVEN parameters' alignment (matrices on the host, where kinematic_affine consumes them)
        host = {k: given[k].detach().cpu() for k in ("global_trans", "rot_center")}
        obj = None if obj_trans is None else {"obj_trans": torch.from_numpy(obj_trans)}
        dec = decoder if decoder is not None else gradient_decoder(utils.decoder_for(decoder_module, specs, host, device), decoder_module,
                                                                   specs, fallbacks)
        utils.bind_sample(dec, specs, torch.from_numpy(latent), host, obj)
        fit = fit_mano(layer, pose_d, shape_d, decoder=dec, head="hand", scale_factor=specs["SdfScaleFactor"], steps=steps, lr=lr,
                       pose_prior=pose_prior, shape_prior=shape_prior)
        shift = 0.0 if root_d is None else root_d.reshape(1, 3)
        with torch.no_grad():
            hand_pose = fit.pose[:, 3:] @ torch.from_numpy(model.comps[:nc]).to(device)
        write_mano(os.path.join(out_root, "optim_mano"), name, fit.verts[0] + shift, fit.joints[0] + shift, fit.shape, hand_pose, model.faces)
        records.append({"name": name, "first": float(fit.losses[0]) if len(fit.losses) else float("nan"),
                        "last": float(fit.losses[-1]) if len(fit.losses) else float("nan"), "steps": int(steps)})
    return records


def main(argv=None):
    p = argparse.ArgumentParser(description="Fit MANO parameters to the decoder's hand SDF; writes pred_mano/ and optim_mano/")
    p.add_argument("-e", "--experiment", required=True, help="experiment directory (specs.json, ModelParameters/latest.pth)")
    p.add_argument("-t", "--task", default="obman")
    p.add_argument("--codes", dest="code_dir", required=True, help="directory of <name>.npz with latent, mano_pose, mano_shape")
    p.add_argument("--mano_model", required=True, help="the .npz tools/mano_pkl_to_npz.py writes")
    for k, v in FLOW_DEFAULTS.items():
        p.add_argument("--" + k, type=type(v), default=v)
    a = p.parse_args(argv)
    from .reconstruct import load_experiment
    specs, module = load_experiment(a.experiment)
    out_root = os.path.join(a.experiment, "Eval_" + a.task)
    records = run(specs, module, mano.ManoModel.from_npz(a.mano_model), a.code_dir, out_root, **{k: getattr(a, k) for k in FLOW_DEFAULTS})
    if records:
        print("mano_fit: %d samples, %d steps each, mean objective %.4e -> %.4e" % (
            len(records), a.steps, np.mean([r["first"] for r in records]), np.mean([r["last"] for r in records])))
    print(out_root)


if __name__ == "__main__":
    main()
