"""The reverse-mode form of the fp32 chain (csrc/k1v_kernels.hip, sdf_mlp_vjp_kernel.h; asdf_decode_points_vjp;
HipSdfDecoder.decode_points_vjp; alignsdf_amd.fit) held to an fp64 reverse chain written by hand (tests/sdf_vjp_cases.vjp_truth).

Yardsticks, as tests/test_gpu_sdf_grad.py - per output array among d_latent, d_embed and d_fold, with e = max |got - truth| and weights
that are 0 on the points that are not clear in the truth (sdf_vjp_cases):

    e_k    native
    e_mod  TorchModuleDecoder.decode_points_vjp (torch autograd through the module on the GPU; it has no d_fold)
    e_or   fp32 on the CPU: autograd through the oracle for d_latent and d_embed, vjp_truth(dtype=float32) for d_fold

    e_k <= 3 max(e_mod, e_or) + 5e-7 max(1, max |truth|);   on 4096 points or more also rms_k <= 1.5 max(rms_mod, rms_or)

Every line printed with the prefix SDFVJP is one case's measured errors (profiles/sdf_vjp_fp64_errors.txt)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from alignsdf_amd import _native
from alignsdf_amd import synthetic as syn
from tests import sdf_grad_cases as gc
from tests import sdf_vjp_cases as vc

pytestmark = pytest.mark.gpu
HEADS = vc.HEADS
COMBOS = (("hand", "obj"), ("hand",), ("obj",))
EINVAL = -1          # ASDF_EINVAL
FOLD, LAT, EMB = 2 * 2 * 512 * 4, 256, 2 * _native.MAX_POINT_FEATS * 4


def _t(d):
    return None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def _bind(dec, tag, sample):
    from alignsdf_amd.utils.utils import bind_sample
    latent, mano, obj = syn.sample_inputs(tag, sample)
    bind_sample(dec, syn.specs_for(tag), torch.from_numpy(latent), _t(mano), _t(obj))


@pytest.fixture(scope="module")
def decoders():
    """One native decoder per configuration, built on first use."""
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    made = {}

    def get(tag):
        if tag not in made:
            made[tag] = HipSdfDecoder(gc.module_for(tag))
        return made[tag]
    yield get
    for d in made.values():
        d.close()


def _module_path(tag, sample):
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    mod = TorchModuleDecoder(gc.module_for(tag), syn.specs_for(tag), "held to the reverse-mode truth")
    _bind(mod, tag, sample)
    return mod


def _np(v):
    return None if v is None else v.detach().cpu().numpy()


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _yardsticks(tag, sample, key, heads):
    """(fp64 truth, fp32 oracle autograd, fp32 manual chain) of a set and a choice of heads; computed once, never modified."""
    pts, w = vc.case(tag, sample, key)
    ws = vc.weights_for(w, heads)
    return (vc.vjp_truth(tag, sample, pts, ws), vc.oracle_autograd_vjp(tag, sample, pts, ws, torch.float32),
            vc.vjp_truth(tag, sample, pts, ws, torch.float32))


def _err(a, b):
    d = np.asarray(a, np.float64).ravel() - np.asarray(b, np.float64).ravel()
    return float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))


def _flat_embed(pair):
    return np.concatenate([np.asarray(e, np.float64).ravel() for e in pair])


def _arrays(res):
    """SdfVjp -> {"d_latent", "d_embed", "d_fold"} as flat float64 arrays (d_fold left out where the path has none)."""
    out = {"d_latent": _np(res.d_latent).astype(np.float64).ravel(), "d_embed": _flat_embed([_np(e) for e in res.d_embed])}
    if res.d_fold is not None:
        out["d_fold"] = _np(res.d_fold).astype(np.float64).ravel()
    return out


def _run_set(label, tag, key, heads, decoders):
    pts, w = vc.case(tag, vc.SAMPLE, key)
    truth, orc32, man32 = _yardsticks(tag, vc.SAMPLE, key, heads)
    M = len(pts)
    hip = decoders(tag)
    _bind(hip, tag, vc.SAMPLE)
    x = _cuda(pts)
    wh, wo = (_cuda(w[name]) if name in heads else None for name in HEADS)
    res = hip.decode_points_vjp(x, wh, wo)
    again = hip.decode_points_vjp(x, wh, wo)
    mod = _module_path(tag, vc.SAMPLE).decode_points_vjp(x, wh, wo)
    got, gmod = _arrays(res), _arrays(mod)
    want = {"d_latent": truth["d_latent"], "d_embed": _flat_embed(truth["d_embed"]), "d_fold": truth["d_fold"]}
    cpu32 = {"d_latent": orc32["d_latent"], "d_embed": _flat_embed(orc32["d_embed"]), "d_fold": man32["d_fold"]}
    for name in ("d_latent", "d_embed", "d_fold"):
        top = float(np.abs(want[name]).max())
        (e_k, r_k), (e_or, r_or) = _err(got[name], want[name]), _err(cpu32[name], want[name])
        e_mod, r_mod = _err(gmod[name], want[name]) if name in gmod else (0.0, 0.0)
        print("SDFVJP %-18s %-8s heads %-8s M=%-5d max|truth| %.2e: e_k %.2e e_mod %.2e e_or %.2e | rms %.2e %.2e %.2e" % (
            label, name, "+".join(heads), M, top, e_k, e_mod, e_or, r_k, r_mod, r_or))
        assert np.isfinite(got[name]).all(), (label, name)
        assert e_k <= 3.0 * max(e_mod, e_or) + 5e-7 * max(1.0, top), (label, name, heads, e_k, e_mod, e_or)
        if M >= 4096:
            assert r_k <= 1.5 * max(r_mod, r_or), (label, name, heads, r_k, r_mod, r_or)
    # (c) the values are decode_points' bits under math f32; a head that is off has no values and zero blocks
    before = hip.math
    hip.set_math("f32")
    h, o = hip.decode_points(x)
    hip.set_math(before)
    for k, (name, ref, v) in enumerate(zip(HEADS, (h, o), (res.sdf_hand, res.sdf_obj))):
        if name in heads:
            assert np.array_equal(_np(v), _np(ref)), (label, name)
            assert np.abs(_np(v) - truth["sdf"][name]).max() <= 1e-5, (label, name)
        else:
            assert v is None and not _np(res.d_fold)[k].any() and not _np(res.d_embed[k]).any(), (label, name)
    # (d) the same call twice: every bit
    for a, b in zip((res.sdf_hand, res.sdf_obj, res.d_latent, res.d_embed[0], res.d_embed[1], res.d_fold),
                    (again.sdf_hand, again.sdf_obj, again.d_latent, again.d_embed[0], again.d_embed[1], again.d_fold)):
        assert (a is None and b is None) or np.array_equal(_np(a), _np(b)), label
    return res


# ---- (a), (b): point lists and full sets, with (c) and (d) on each ------------------------------------------------------------------------
@pytest.mark.parametrize("M", vc.LIST_LENGTHS)
def test_point_list_lengths(M, decoders):
    """The 32-per-wave and 128-per-workgroup edges and one list longer than a grid of single tiles - on both9 (an affine embedding,
    different per head), both heads, the hand alone, the object alone."""
    for heads in COMBOS:
        _run_set("both9 list", "both9", ("list", M), heads, decoders)


@pytest.mark.parametrize("tag", vc.FULL_TAGS)
def test_full_sets(tag, decoders):
    _run_set("%s full" % tag, tag, ("full", 4096), ("hand", "obj"), decoders)


# ---- (e) zeros ----------------------------------------------------------------------------------------------------------------------------
def test_zeros_and_head_sums(decoders):
    hip = decoders("both9")
    _bind(hip, "both9", vc.SAMPLE)
    pts, w = vc.case("both9", vc.SAMPLE, ("list", 257))
    x, wh, wo = _cuda(pts), _cuda(w["hand"]), _cuda(w["obj"])
    z = torch.zeros(257, device="cuda")
    r0 = hip.decode_points_vjp(x, z, z)
    for v in (r0.d_latent, r0.d_embed[0], r0.d_embed[1], r0.d_fold):
        assert (_np(v) == 0).all()
    assert r0.sdf_hand is not None and np.isfinite(_np(r0.sdf_hand)).all()
    both, only_h, only_o = hip.decode_points_vjp(x, wh, wo), hip.decode_points_vjp(x, wh, None), hip.decode_points_vjp(x, None, wo)
    assert not _np(only_h.d_fold)[1].any() and not _np(only_o.d_fold)[0].any()
    assert np.array_equal(_np(only_h.d_fold)[0], _np(both.d_fold)[0]) and np.array_equal(_np(only_o.d_fold)[1], _np(both.d_fold)[1])
    top = float(np.abs(_np(both.d_latent)).max())
    assert top > 0 and np.abs(_np(only_h.d_latent) + _np(only_o.d_latent) - _np(both.d_latent)).max() <= 1e-6 * top
    # one point's weight set to zero = that point left out of the list
    keep = np.flatnonzero(w["hand"] != 0)
    part = hip.decode_points_vjp(_cuda(pts[keep]), _cuda(w["hand"][keep]), None)
    assert np.abs(_np(part.d_latent) - _np(only_h.d_latent)).max() <= 1e-5 * top


# ---- (f) C ABI ----------------------------------------------------------------------------------------------------------------------------
def _call(L, h, x, M, wh, wo, outs, st):
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return L.asdf_decode_points_vjp(h, ptr(x), M, ptr(wh), ptr(wo), *[ptr(o) for o in outs], st)


def _sevens(M):
    return [torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for n in (M, M, FOLD, LAT, EMB)]


def test_c_abi_arguments(decoders):
    hip = decoders("both9")
    _bind(hip, "both9", vc.SAMPLE)
    L = _native.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pts, w = vc.case("both9", vc.SAMPLE, ("list", 33))
    x, wh, wo = _cuda(pts), _cuda(w["hand"]), _cuda(w["obj"])
    math_before = (hip.math, hip._L.asdf_decoder_get_math(hip._h))
    untouched = lambda outs: all((_np(o) == 7.0).all() for o in outs)
    for args in ((None, x, 33), (hip._h, None, 33), (hip._h, x, -1)):
        outs = _sevens(33)
        assert _call(L, args[0], args[1], args[2], wh, wo, outs, st) == EINVAL and untouched(outs)
    # M == 0 and both weights NULL: the d_* outputs are zero-filled, the values are not written
    for M, a, b in ((0, wh, wo), (33, None, None)):
        outs = _sevens(33)
        assert _call(L, hip._h, x, M, a, b, outs, st) == 0
        assert untouched(outs[:2]) and all((_np(o) == 0).all() for o in outs[2:])
    # NULL outputs are skipped; the others are what the method returns
    ref = hip.decode_points_vjp(x, wh, wo)
    full = [_np(ref.sdf_hand), _np(ref.sdf_obj), _np(ref.d_fold).ravel()]
    for skip in range(5):
        outs = _sevens(33)
        assert _call(L, hip._h, x, 33, wh, wo, [None if k == skip else o for k, o in enumerate(outs)], st) == 0
        assert (_np(outs[skip]) == 7.0).all()
        for k in range(3):
            assert k == skip or np.array_equal(_np(outs[k]), full[k]), (skip, k)
        assert skip == 3 or np.array_equal(_np(outs[3]), _np(ref.d_latent))
    assert (hip.math, hip._L.asdf_decoder_get_math(hip._h)) == math_before


def test_unbound_and_refused_decoders():
    """An unbound decoder: EINVAL.  comb3, nerf9 and a pixel-bound decoder: ENOGRAD from the C call, NotImplementedError with the
    reason from the method - and sdf_at_points then runs on the module path."""
    from alignsdf_amd.fit import sdf_at_points
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    L = _native.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, w = torch.zeros(4, 3, device="cuda"), torch.ones(4, device="cuda")
    fresh = HipSdfDecoder(gc.module_for("nerf3"))
    outs = _sevens(4)
    assert _call(L, fresh._h, x, 4, w, w, outs, st) == EINVAL and all((_np(o) == 7.0).all() for o in outs)
    fresh.close()
    comb = HipSdfDecoder(syn.full_state_dict("comb3"), 256, 3, "nerf")
    comb.set_sample(torch.from_numpy(syn.latent_code(1)))
    nerf9 = HipSdfDecoder(syn.full_state_dict("nerf9"), 256, 9, "nerf")
    nerf9.set_sample(torch.from_numpy(syn.latent_code(1)))
    specs, _, sd, _, _, _, _ = syn.variant_config("pixelalign")
    pa = HipSdfDecoder(sd, 256, 3, "nerf", pixel_align=True)
    feat, mano, cam = syn.pixel_align_sample(0, 8, 8)
    pa.set_sample_pixel(torch.from_numpy(feat).cuda(), cam, mano["joints"][0, 0], specs["ImageSize"][0], specs["SdfScaleFactor"])
    for dec, word in ((comb, "CombinedDecoder"), (nerf9, "NeRF"), (pa, "pixel")):
        outs = _sevens(4)
        assert _call(L, dec._h, x, 4, w, w, outs, st) == _native.ENOGRAD and all((_np(o) == 7.0).all() for o in outs)
        assert word in dec.vjp_refusal()
        with pytest.raises(NotImplementedError, match=word):
            dec.decode_points_vjp(x, w, w)
        with pytest.raises(NotImplementedError, match=word):
            sdf_at_points(dec, torch.zeros(256), (torch.eye(3, 4), torch.eye(3, 4)), x)
        dec.close()
    # ... and sdf_at_points runs on the module path of the refused variants that have a latent code: values of the native decoder's
    # decode_points, gradients those of TorchModuleDecoder.decode_points_vjp; there is no affine embedding to differentiate on nerf9
    pts = _cuda(vc.points(64, 2))
    a, b = _cuda(vc.points(64, 3)[:, 0]), _cuda(vc.points(64, 3)[:, 1])
    for tag, embed in (("comb3", None), ("comb3", (torch.eye(3, 4).cuda().requires_grad_(),)), ("nerf9", None)):
        specs = syn.specs_for(tag)
        hip = HipSdfDecoder(syn.full_state_dict(tag), 256, specs["PointFeatSize"], "nerf")
        assert hip.vjp_refusal() is not None
        hip.set_sample(torch.from_numpy(syn.latent_code(1)))
        hn, on = hip.decode_points(pts)
        hip.close()
        mod = TorchModuleDecoder(gc.module_for(tag), specs, "module path of sdf_at_points: %s" % mod_reason(tag))
        lat = torch.from_numpy(syn.latent_code(1)).reshape(-1).cuda().requires_grad_()
        x = pts.clone().requires_grad_()
        h, o = sdf_at_points(mod, lat, embed, x)
        assert np.abs(_np(h) - _np(hn)).max() <= 1e-5 and np.abs(_np(o) - _np(on)).max() <= 1e-5, tag
        ((h * a).sum() + (o * b).sum()).backward()
        mod.set_sample(torch.from_numpy(syn.latent_code(1)))
        ref = mod.decode_points_vjp(pts, a, b)
        top = float(np.abs(_np(ref.d_latent)).max())
        assert top > 0 and np.abs(_np(lat.grad) - _np(ref.d_latent)).max() <= 1e-5 * top, tag
        assert np.isfinite(_np(x.grad)).all() and np.abs(_np(x.grad)).max() > 0, tag
        if embed is not None:
            g = _np(embed[0].grad)          # (E = identity: dL / dE = g_feat^T [x, 1] and g_feat = dL / dx, so its last column is the sum of x.grad over the points)
            assert np.isfinite(g).all() and np.abs(g).max() > 0
            assert np.abs(g[:, 3] - _np(x.grad).sum(0)).max() <= 1e-5 * max(1.0, float(np.abs(g).max())), tag
    with pytest.raises(ValueError):
        sdf_at_points(mod, lat, (torch.eye(3, 4),) * 2, pts)          # (nerf9: no affine embedding applies)
    # the module path of a configuration the kernel covers: the same function, differentiable, close to the native values
    mod = TorchModuleDecoder(gc.module_for("nerf3"), syn.specs_for("nerf3"), "module path of sdf_at_points")
    lat = torch.from_numpy(syn.latent_code(1)).reshape(-1).cuda().requires_grad_()
    E = (torch.eye(3, 4).cuda().requires_grad_(), torch.eye(3, 4).cuda())
    h, o = sdf_at_points(mod, lat, E, pts)
    (h.sum() + o.sum()).backward()
    assert lat.grad is not None and E[0].grad is not None and np.isfinite(_np(lat.grad)).all()
    hip = HipSdfDecoder(gc.module_for("nerf3"))
    hn, on = sdf_at_points(hip, lat.detach(), (E[0].detach(), E[1]), pts)
    assert np.abs(_np(hn) - _np(h)).max() <= 1e-5 and np.abs(_np(on) - _np(o)).max() <= 1e-5
    hip.close()


def mod_reason(tag):
    from alignsdf_amd.hip_decoder import vjp_refusal
    specs = syn.specs_for(tag)
    return vjp_refusal(tag.startswith("comb"), specs["PointFeatSize"], specs["EncodeStyle"], False)


# ---- (g) sdf_at_points ----------------------------------------------------------------------------------------------------------------------
def test_sdf_at_points_backward_is_the_kernel(decoders):
    from alignsdf_amd.fit import kinematic_affine_torch, sdf_at_points
    tag = "both9"
    hip = decoders(tag)
    specs = syn.specs_for(tag)
    latent, mano, obj = syn.sample_inputs(tag, vc.SAMPLE)
    pts, w = vc.case(tag, vc.SAMPLE, ("list", 257))
    E = [e.float().cuda().requires_grad_() for e in kinematic_affine_torch(specs["PointFeatSize"], specs["EncodeStyle"], specs["SdfScaleFactor"], _t(mano), _t(obj))]
    lat = torch.from_numpy(latent).reshape(-1).cuda().requires_grad_()
    x = _cuda(pts).requires_grad_()
    a, b = _cuda(w["hand"]), _cuda(w["obj"])
    h, o = sdf_at_points(hip, lat, E, x)
    ((h * a).sum() + (o * b).sum()).backward()
    # the sample sdf_at_points bound is still bound: the same launches by hand
    ref = hip.decode_points_vjp(x.detach(), a, b)
    assert np.array_equal(_np(h), _np(ref.sdf_hand)) and np.array_equal(_np(o), _np(ref.sdf_obj))
    assert np.array_equal(_np(lat.grad), _np(ref.d_latent))
    assert np.array_equal(_np(E[0].grad), _np(ref.d_embed[0])) and np.array_equal(_np(E[1].grad), _np(ref.d_embed[1]))
    _, gh, _, go = hip.decode_points_grad(x.detach())
    assert np.array_equal(_np(x.grad), _np(a.reshape(-1, 1) * gh + b.reshape(-1, 1) * go))
    # ... and the embedding built in torch is the one bind_sample folds: the truth of the set applies
    truth = _yardsticks(tag, vc.SAMPLE, ("list", 257), ("hand", "obj"))[0]
    assert np.abs(_np(lat.grad) - truth["d_latent"]).max() <= 1e-4 * max(1.0, np.abs(truth["d_latent"]).max())


# ---- (h) the fit -----------------------------------------------------------------------------------------------------------------------------
FIT_TAG = vc.FIT_TAG


@pytest.mark.parametrize("path", ["native", "module"])
def test_fit_recovers_the_sample(path, decoders):
    """fit_sample's defaults (40 steps, lr 2e-3, prior 1e-3).  The reference, fp64 on the oracle alone: loss 2.77e-2 -> 1.52e-3, ratio
    0.055 (0.046 - 0.076 over lr 2e-3 / 5e-3 and noise / shift 0.3 / 0.03, 0.5 / 0.05): the bound 0.25 is 4.5 x that, for fp32 and
    mask flips along the trajectory; and what is left of each start shift (start shift + fitted shift) is shorter than the 0.03 it
    started with."""
    from alignsdf_amd.fit import fit_sample
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    hip = decoders(FIT_TAG)
    z0, E0, sh, so = vc.fit_scenario(hip)
    dec = hip if path == "native" else TorchModuleDecoder(gc.module_for(FIT_TAG), syn.specs_for(FIT_TAG), "fit on the module path")
    z, E, shifts, history = fit_sample(dec, z0, E0, sh, so)
    ratio = history[-1] / history[0]
    left = _np(shifts).astype(np.float64) + np.array([[0.03, 0.0, 0.0], [0.0, -0.03, 0.0]])
    print("SDFVJP fit %-6s loss %.3e -> %.3e ratio %.3f | shifts left %.4f %.4f | history %s" % (
        path, history[0], history[-1], ratio, np.linalg.norm(left[0]), np.linalg.norm(left[1]), " ".join("%.2e" % v for v in history[::5])))
    assert len(history) == 40 and ratio <= 0.25, (path, history[0], history[-1])
    assert np.linalg.norm(left[0]) < 0.03 and np.linalg.norm(left[1]) < 0.03, (path, left)
