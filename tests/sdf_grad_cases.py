"""Shared pieces of the SDF-gradient tests (tests/test_sdf_grad_truth.py on the CPU, tests/test_gpu_sdf_grad.py on the GPU): the point
sets, and `grad_truth` - sdf and d sdf / d xyz of a SeparateDecoder sample in fp64 forward mode, built on oracle.sdf_oracle.

A ReLU unit within rounding of its kink may legitimately take either mask in fp32, and one flip moves a gradient component by several
1e-3.  So every comparison of gradients runs over the CLEAR points of a head: those whose smallest |pre-activation| over the head's
hidden units (`minz`) exceeds CLEAR_EPS.  The share of clear points is a condition of every set (test_sdf_grad_truth.py asserts it
on the truth alone)."""
import functools

import numpy as np
import torch

from alignsdf_amd import synthetic as syn

CLEAR_EPS = 1e-5
MIN_CLEAR_SHARE = 0.85          # of every head of every set with more than 256 points
LIST_LENGTHS = (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 4097)      # edges of the 8-per-wave / 32-per-workgroup tiling, on both9
FULL_TAGS = ("nerf3", "grasp3", "grasp9", "bothcls9")              # one 4096-point set each
SAMPLE = 1


def points(M, seed=1):
    """[M, 3] float32 uniform in [-1, 1]^3."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (M, 3)).astype(np.float32)


def list_points(M):
    return points(M, 100 + M)


def point_sets():
    """[(label, tag, sample, points)] of every set the GPU tests compare gradients on."""
    out = [("both9 M=%d" % M, "both9", SAMPLE, list_points(M)) for M in LIST_LENGTHS]
    out += [("%s M=4096" % tag, tag, SAMPLE, points(4096)) for tag in FULL_TAGS]
    return out


@functools.lru_cache(maxsize=None)
def state_dict(tag):
    return syn.full_state_dict(tag)


def _head_slices(style, L, pf):
    """Columns of [latent | point features] that the hand / object MLP reads (networks/model.py:288-299)."""
    a = np.arange(L + pf)
    if style == "nerf":
        return a, a
    if style == "hand":
        return a, a[:L + 3]
    if style == "obj":
        return a[:L + 3], a
    return a[:-3], np.concatenate([a[:L + 3], a[-3:]])


def grad_truth(tag, sample, pts, dtype=torch.float64):
    """{"hand" / "obj": {"sdf" [M], "grad" [M, 3], "minz" [M]}} (numpy, `dtype`) of synthetic sample `sample` of configuration `tag` at
    the normalised points `pts`: forward mode through the oracle's own pieces - effective_head_params, point_features - with the
    value's ReLU mask on the tangents (derivative 0 at 0, as torch) and grad = (1 - tanh(s)^2) ds.  dtype=torch.float32 runs the same
    in fp32 (not a yardstick: the GPU tests' fp32 yardstick is autograd through the oracle, oracle_autograd)."""
    from oracle import sdf_oracle as orc
    sd, specs = state_dict(tag), syn.specs_for(tag)
    latent, mano, obj = syn.sample_inputs(tag, sample)
    cast = lambda d: None if d is None else {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}
    mano, obj = cast(mano), cast(obj)
    x = torch.as_tensor(np.asarray(pts, np.float32)).to(dtype)
    M, L = x.shape[0], latent.size
    feats_of = lambda q: orc.point_features(q, specs, mano, obj)
    feats = feats_of(x)
    dfeats = [torch.func.jvp(feats_of, (x,), (torch.eye(3, dtype=dtype)[k].expand(M, 3).contiguous(),))[1] for k in range(3)]
    pf = feats.shape[1]
    inputs = torch.cat([torch.as_tensor(latent).to(dtype).reshape(1, -1).expand(M, -1), feats], 1)
    dinputs = [torch.cat([torch.zeros(M, L, dtype=dtype), d], 1) for d in dfeats]
    out = {}
    for name, letter, cols in zip(("hand", "obj"), "ho", _head_slices(specs["EncodeStyle"], L, pf)):
        params = orc.effective_head_params(sd, letter, dtype)
        x0, t0 = inputs[:, cols], [d[:, cols] for d in dinputs]
        h, t = x0, t0
        minz = torch.full((M,), float("inf"), dtype=dtype)
        for layer, (w, b) in enumerate(params):
            if layer == 2:
                h, t = torch.cat([h, x0], 1), [torch.cat([a, c], 1) for a, c in zip(t, t0)]
            z = h @ w.t() + b
            t = [a @ w.t() for a in t]
            if layer < 4:
                minz = torch.minimum(minz, z.abs().min(1).values)
                keep = (z > 0).to(dtype)
                h, t = z * keep, [a * keep for a in t]
        sdf = torch.tanh(z[:, 0])
        grad = torch.stack([(1.0 - sdf * sdf) * a[:, 0] for a in t], 1)
        out[name] = {"sdf": sdf.numpy(), "grad": grad.numpy(), "minz": minz.numpy()}
    return out


def clear_mask(truth_head, eps=CLEAR_EPS):
    return truth_head["minz"] > eps


def oracle_autograd(tag, sample, pts, dtype=torch.float32):
    """{"hand" / "obj": {"sdf", "grad"}} by torch autograd through the oracle's decode chain (point_features + separate_decoder) in
    `dtype`: in fp32 the reference's arithmetic on the CPU - the yardstick e_or."""
    from oracle import sdf_oracle as orc
    sd, specs = state_dict(tag), syn.specs_for(tag)
    latent, mano, obj = syn.sample_inputs(tag, sample)
    cast = lambda d: None if d is None else {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}
    mano, obj = cast(mano), cast(obj)
    hp, op = orc.effective_head_params(sd, "h", dtype), orc.effective_head_params(sd, "o", dtype)
    x = torch.as_tensor(np.asarray(pts, np.float32)).to(dtype).requires_grad_()
    lat = torch.as_tensor(latent).to(dtype).reshape(1, -1)
    h, o = orc.decode_sdf_multi_output(hp, op, lat, orc.point_features(x, specs, mano, obj), specs)
    out = {}
    for name, v in (("hand", h), ("obj", o)):
        g, = torch.autograd.grad(v.sum(), x, retain_graph=True)
        out[name] = {"sdf": v.detach().reshape(-1).numpy(), "grad": g.numpy()}
    return out


@functools.lru_cache(maxsize=None)
def module_for(tag, dtype=torch.float32):
    """alignsdf_amd.networks.model.SeparateDecoder loaded with the weights of `tag`, in `dtype` (one per process: the evaluators hold
    their module through a weak reference)."""
    from alignsdf_amd.networks.model import build_decoder
    return build_decoder(syn.specs_for(tag), state_dict(tag)).to(dtype).eval()


def module_autograd(tag, sample, pts, dtype=torch.float64):
    """The same through the package's nn.Module (the oracle supplies only the point features)."""
    from oracle import sdf_oracle as orc
    specs = syn.specs_for(tag)
    latent, mano, obj = syn.sample_inputs(tag, sample)
    cast = lambda d: None if d is None else {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}
    dec = module_for(tag, dtype)
    x = torch.as_tensor(np.asarray(pts, np.float32)).to(dtype).requires_grad_()
    lat = torch.as_tensor(latent).to(dtype).reshape(1, -1).expand(x.shape[0], -1)
    res = dec(torch.cat([lat, orc.point_features(x, specs, cast(mano), cast(obj))], 1))
    out = {}
    for name, v in (("hand", res[0]), ("obj", res[1])):
        g, = torch.autograd.grad(v.sum(), x, retain_graph=True)
        out[name] = {"sdf": v.detach().reshape(-1).numpy(), "grad": g.numpy()}
    return out
