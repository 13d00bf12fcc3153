"""Shared pieces of the reverse-mode SDF tests (tests/test_sdf_vjp_truth.py on the CPU, tests/test_gpu_sdf_vjp.py on the GPU):
`vjp_truth` - the manual reverse chain of a SeparateDecoder sample on oracle.sdf_oracle's pieces, as sdf_grad_cases.grad_truth is the
manual forward mode - the weights of every comparison, and the oracle's own autograd.

A ReLU unit within rounding of its kink may legitimately take either mask in fp32, and here one flipped point pollutes a SUM over the
points.  So every comparison uses weights w = N(0, 1) from a fixed seed, SET TO 0 ON THE POINTS THAT ARE NOT CLEAR in the fp64 truth
(sdf_grad_cases.CLEAR_EPS); the share of clear points is a condition of every set, asserted again where the weights are made."""
import functools

import numpy as np
import torch

from alignsdf_amd import synthetic as syn
from tests import sdf_grad_cases as gc
from tests.sdf_grad_cases import CLEAR_EPS, FULL_TAGS, MIN_CLEAR_SHARE, list_points, points      # noqa: F401

HEADS = ("hand", "obj")
LIST_LENGTHS = (1, 31, 32, 33, 127, 128, 129, 257, 4097)      # edges of the 32-per-wave / 128-per-workgroup tiling, on both9
SAMPLE = gc.SAMPLE
W_SEED = 77


def _pose(tag, sample, dtype):
    latent, mano, obj = syn.sample_inputs(tag, sample)
    cast = lambda d: None if d is None else {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}
    return torch.as_tensor(latent).to(dtype).reshape(-1), cast(mano), cast(obj)


def _forward_head(params, x0, dtype):
    """One head of the oracle's MLP on inputs x0 [M, L + pf]: (sdf [M], masks [4 x [M, width]], minz [M])."""
    h, masks = x0, []
    minz = torch.full((x0.shape[0],), float("inf"), dtype=dtype)
    for layer, (w, b) in enumerate(params):
        if layer == 2:
            h = torch.cat([h, x0], 1)
        z = h @ w.t() + b
        if layer < 4:
            minz = torch.minimum(minz, z.abs().min(1).values)
            keep = (z > 0).to(dtype)
            masks.append(keep)
            h = z * keep
    return torch.tanh(z[:, 0]), masks, minz


def vjp_truth(tag, sample, pts, w, dtype=torch.float64):
    """The reverse chain by hand, for weights w = {"hand" / "obj": [M] or None} = dL / d sdf:
        u = w (1 - s^2);  d3 = (u w4) m3;  d2 = (W3^T d3) m2;  d1 = (W2a^T d2) m1;  d0 = (W1^T d1) m0
        d_fold[head][layer 0 / 2][o] = sum_p d0 / d2 [p, o] (x_p, 1)
        d_latent = sum over heads and layers of W_lat^T dc;  d_embed[head][f][d] = sum over layers and o of W_pt[o, f] d_fold[o][d]
    Returns {"sdf": {head: [M]}, "minz": {head: [M]}, "d_fold" [2, 2, 512, 4], "d_latent" [L], "d_embed": (hand [pf_h, 4], obj [pf_o,
    4])} as numpy in `dtype`; a head whose weights are None has zero blocks."""
    from oracle import sdf_oracle as orc
    sd, specs = gc.state_dict(tag), syn.specs_for(tag)
    latent, mano, obj = _pose(tag, sample, dtype)
    x = torch.as_tensor(np.asarray(pts, np.float32)).to(dtype)
    M, L = x.shape[0], latent.numel()
    feats = orc.point_features(x, specs, mano, obj)
    inputs = torch.cat([latent.reshape(1, -1).expand(M, -1), feats], 1)
    x1 = torch.cat([x, torch.ones(M, 1, dtype=dtype)], 1)
    out = {"sdf": {}, "minz": {}, "d_fold": torch.zeros(2, 2, 512, 4, dtype=dtype), "d_latent": torch.zeros(L, dtype=dtype), "d_embed": []}
    for k, (name, letter, cols) in enumerate(zip(HEADS, "ho", gc._head_slices(specs["EncodeStyle"], L, feats.shape[1]))):
        params = orc.effective_head_params(sd, letter, dtype)
        pf = len(cols) - L
        sdf, (m0, m1, m2, m3), minz = _forward_head(params, inputs[:, cols], dtype)
        out["sdf"][name], out["minz"][name] = sdf.numpy(), minz.numpy()
        d_embed = torch.zeros(pf, 4, dtype=dtype)
        if w.get(name) is not None:
            (W0, _), (W1, _), (W2, _), (W3, _), (W4, _) = params
            n1 = W1.shape[0]
            u = torch.as_tensor(np.asarray(w[name])).to(dtype) * (1.0 - sdf * sdf)
            d3 = (u[:, None] * W4[0][None, :]) * m3
            d2 = (d3 @ W3) * m2
            d1 = (d2 @ W2[:, :n1]) * m1
            d0 = (d1 @ W1) * m0
            f0, f2 = d0.t() @ x1, d2.t() @ x1                      # [512, 4] = (dA[:, 0..2], dc)
            out["d_fold"][k, 0], out["d_fold"][k, 1] = f0, f2
            out["d_latent"] += W0[:, :L].t() @ f0[:, 3] + W2[:, n1:n1 + L].t() @ f2[:, 3]
            d_embed = W0[:, L:].t() @ f0 + W2[:, n1 + L:].t() @ f2
        out["d_embed"].append(d_embed.numpy())
    out["d_fold"], out["d_latent"], out["d_embed"] = out["d_fold"].numpy(), out["d_latent"].numpy(), tuple(out["d_embed"])
    return out


def oracle_autograd_vjp(tag, sample, pts, w, dtype=torch.float32, pose_grads=False):
    """d_latent and d_embed (and, with pose_grads, dL / d rot_center and dL / d obj_trans) of L = sum_heads sum_p w_p sdf_p by torch
    autograd through the oracle's decode chain in `dtype`: point_features + decode_sdf_multi_output.  d_embed[h] = g_feat^T [x, 1]
    over the head's own feature columns (g_feat: the gradient with respect to the point features)."""
    from oracle import sdf_oracle as orc
    sd, specs = gc.state_dict(tag), syn.specs_for(tag)
    latent, mano, obj = _pose(tag, sample, dtype)
    if pose_grads:
        mano["rot_center"].requires_grad_()
        obj["obj_trans"].requires_grad_()
    hp, op = orc.effective_head_params(sd, "h", dtype), orc.effective_head_params(sd, "o", dtype)
    x = torch.as_tensor(np.asarray(pts, np.float32)).to(dtype)
    lat = latent.reshape(1, -1).clone().requires_grad_()
    feats_of_pose = orc.point_features(x, specs, mano, obj)
    feats = feats_of_pose.detach().clone().requires_grad_()
    L = latent.numel()
    vals = orc.decode_sdf_multi_output(hp, op, lat, feats, specs)
    x1 = torch.cat([x, torch.ones(x.shape[0], 1, dtype=dtype)], 1)
    d_latent, d_embed, g_total = torch.zeros(L, dtype=dtype), [], torch.zeros_like(feats)
    for name, v, cols in zip(HEADS, vals, gc._head_slices(specs["EncodeStyle"], L, feats.shape[1])):
        fc = torch.as_tensor(cols[L:] - L)
        if w.get(name) is None:
            d_embed.append(np.zeros((len(fc), 4), np.float64))
            continue
        g_lat, g_feat = torch.autograd.grad((v.reshape(-1) * torch.as_tensor(np.asarray(w[name])).to(dtype)).sum(), (lat, feats), retain_graph=True)
        d_latent += g_lat.reshape(-1)
        g_total += g_feat
        d_embed.append((g_feat[:, fc].t() @ x1).numpy())
    res = {"d_latent": d_latent.numpy(), "d_embed": tuple(d_embed)}
    if pose_grads:
        res["rot_center"], res["obj_trans"] = (g.numpy() for g in torch.autograd.grad((feats_of_pose * g_total).sum(), (mano["rot_center"], obj["obj_trans"])))
    return res


@functools.lru_cache(maxsize=None)
def case(tag, sample, key):
    """(points, weights) of one point set, computed once and never modified; `key` = ("list", M) or ("full", M).  weights = {"hand",
    "obj"}: N(0, 1) from W_SEED, 0 on the points that are not clear in the truth."""
    pts = list_points(key[1]) if key[0] == "list" else points(key[1])
    M = len(pts)
    rng = np.random.default_rng(W_SEED)
    raw = {name: rng.standard_normal(M).astype(np.float32) for name in HEADS}
    probe = vjp_truth(tag, sample, pts, {})
    w = {}
    for name in HEADS:
        clear = probe["minz"][name] > CLEAR_EPS
        assert clear.any() and (M <= 256 or clear.mean() >= MIN_CLEAR_SHARE), (tag, key, name, clear.mean())
        w[name] = np.where(clear, raw[name], np.float32(0.0)).astype(np.float32)
    return pts, w


def weights_for(w, heads):
    return {name: (w[name] if name in heads else None) for name in HEADS}


# ---- the fit scenario (tests/test_gpu_sdf_vjp.py, tools/time_vjp.py) ---------------------------------------------------------------------
FIT_TAG, FIT_SAMPLE = "grasp9", 3
FIT_START_SHIFTS = ((0.03, 0.0, 0.0), (0.0, -0.03, 0.0))


def fit_scenario(hip):
    """(z0, E0, surface_hand, surface_obj): the start and the targets of the fit, made on the native decoder `hip` of FIT_TAG (GPU).
    Targets per head: the first 512 CONVERGED results of project_points from 3000 uniform points in [-0.6, 0.6]^3 (seed 5 + head) on
    the TRUE sample; start: the code moved by 0.3 |z| along a random direction (seed 11), the hand shifted by (0.03, 0, 0), the object
    by (0, -0.03, 0)."""
    from alignsdf_amd.fit import kinematic_affine_torch, shift_embed
    from alignsdf_amd.project import CONVERGED
    from alignsdf_amd.utils.utils import bind_sample
    specs = syn.specs_for(FIT_TAG)
    latent, mano, obj = syn.sample_inputs(FIT_TAG, FIT_SAMPLE)
    t = lambda d: None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}
    bind_sample(hip, specs, torch.from_numpy(latent), t(mano), t(obj))
    targets = []
    for head in range(2):
        start = np.random.default_rng(5 + head).uniform(-0.6, 0.6, (3000, 3)).astype(np.float32)
        # (a point may travel: the default trust box of one 128-lattice voxel is made for marching-cubes vertices)
        r = hip.project_points(torch.from_numpy(start).cuda(), head, max_iters=32, tol=1e-5, max_move=1.0)
        ok = r["xyz_out"].cpu().numpy()[r["status"].cpu().numpy() == CONVERGED][:512]
        assert len(ok) >= 64, (head, len(ok))
        targets.append(torch.from_numpy(ok))
    z = torch.from_numpy(latent).reshape(-1).double()
    n = torch.from_numpy(np.random.default_rng(11).standard_normal(z.numel()))
    z0 = (z + 0.3 * z.norm() * n / n.norm()).float()
    E = kinematic_affine_torch(specs["PointFeatSize"], specs["EncodeStyle"], specs["SdfScaleFactor"], t(mano), t(obj))
    E0 = tuple(shift_embed(e, torch.tensor(s, dtype=torch.float64)).float() for e, s in zip(E, FIT_START_SHIFTS))
    return z0, E0, targets[0], targets[1]
