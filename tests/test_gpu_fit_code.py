"""Auto-decode on the device (asdf_fit_code: csrc/decoder.hip, the loss form of csrc/sdf_mlp_vjp_kernel.h, the Adam step of
csrc/k1vb_kernels.hip - the fit's one loop over a batch of one; HipSdfDecoder.fit_code; alignsdf_amd.fit.fit_code / fit_code_lockstep; alignsdf_amd.autodecode).

The device loop is held to the same rule taken one step at a time with the host in the loop - bit for bit in the code, to the rounding
of an fp64 sum in the history -, its gradient to the fp64 reverse chain of tests/sdf_vjp_cases, its outcome to the rule run in fp64 on
the module, and the flow to the meshes it was given.  Every line printed with the prefix FITCODE is a measured figure
(profiles/fit_code_fp64_errors.txt)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from alignsdf_amd import _native
from alignsdf_amd import synthetic as syn
from tests import fit_code_cases as fc
from tests import sdf_grad_cases as gc
from tests import sdf_vjp_cases as vc

pytestmark = pytest.mark.gpu
TAG, SAMPLE, CLAMP, LR = fc.TAG, fc.SAMPLE, fc.CLAMP, 5e-3
L = 256


def _t(d):
    return None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def _np(v):
    return None if v is None else v.detach().cpu().numpy()


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(_np(a) if torch.is_tensor(a) else a).view(np.int32)


def _sample(tag, sample):
    """(latent [L] torch, embeddings for set_sample or None)"""
    from alignsdf_amd.utils.utils import sample_embedding
    latent, mano, obj = syn.sample_inputs(tag, sample)
    return torch.from_numpy(latent).reshape(-1), sample_embedding(syn.specs_for(tag), _t(mano), _t(obj))


def _bind(dec, tag, sample):
    latent, embed = _sample(tag, sample)
    dec.set_sample(latent.reshape(1, -1), embed)
    return latent, embed


@pytest.fixture(scope="module")
def decoders():
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    made = {}

    def get(tag):
        if tag not in made:
            made[tag] = HipSdfDecoder(gc.module_for(tag))
        return made[tag]
    yield get
    for d in made.values():
        d.close()


def _f32_values(hip, x):
    before = hip.math
    hip.set_math("f32")
    try:
        return hip.decode_points(x)
    finally:
        hip.set_math(before)


def _one_step_reference(hip, x, ts, ns, z, z0, prior, clamp, lr=LR):
    """adam_step_host on decode_points_vjp's d_latent for weights made in torch from decode_points' fp32 values; also the data term."""
    from alignsdf_amd.fit import adam_step_host, adam_step_table, clamped_l1_rule, prior_factor
    f = _f32_values(hip, x)
    ws, data = [None, None], 0.0
    for h in range(2):
        if ts[h] is not None and ns[h] > 0:
            l, ws[h] = clamped_l1_rule(f[h], ts[h], clamp, ns[h])
            data += float(l.double().sum()) * (1.0 / ns[h])
    d = np.zeros(L, np.float32) if ws[0] is None and ws[1] is None else _np(hip.decode_points_vjp(x, ws[0], ws[1], want_sdf=False).d_latent)
    a, s = adam_step_table(1, lr)[0]
    zero = np.zeros(L, np.float32)
    return adam_step_host(_np(z), zero, zero, d, _np(z0), prior_factor(prior, L), a, s)[0], data, ws


def _run_one_step(hip, M, variant):
    latent, _ = _bind(hip, TAG, SAMPLE)
    x = _cuda(vc.list_points(M))
    th, to, nh, no = fc.targets(M, variant)
    ts = (_cuda(th), _cuda(to))
    want, data, _ = _one_step_reference(hip, x, ts, (nh, no), latent, latent, 0.0, CLAMP)
    z, history = hip.fit_code(x, ts[0], ts[1], nh, no, latent, steps=1, lr=LR, decay=1.0, every=1, prior=0.0, clamp=CLAMP)
    moved = int((_np(z) != _np(latent)).sum())
    print("FITCODE one step M=%-6d %-8s: %d of %d entries moved, data term %.6e (lockstep %.6e)" % (M, variant, moved, L, float(history[0]), data))
    assert np.array_equal(_bits(z), _bits(want)), (M, variant, np.abs(_np(z) - want).max())
    assert moved > 0 and abs(float(history[0]) - data) <= 1e-12 * data


# ---- one step, bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", vc.LIST_LENGTHS)
def test_one_step_is_the_host_rule_on_the_kernels_gradient(M, decoders):
    for variant in fc.VARIANTS:
        _run_one_step(decoders(TAG), M, variant)


def test_one_step_on_a_list_longer_than_the_grid(decoders):
    """More than 128 points per compute unit: some workgroup takes a second tile and carries its fp64 loss sum across tiles."""
    M = fc.long_list(torch.cuda.get_device_properties(0).multi_processor_count)
    for variant in fc.VARIANTS:
        _run_one_step(decoders(TAG), M, variant)


# ---- K steps, bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 25])
def test_k_steps_equal_the_lockstep_loop(K, decoders):
    from alignsdf_amd.fit import fit_code_lockstep
    hip = decoders(TAG)
    M = 257
    x = _cuda(vc.list_points(M))
    kw = dict(steps=K, lr=LR, decay=0.5, every=10, prior=1e-3, clamp=CLAMP)
    for variant in ("both", "disjoint"):
        th, to, nh, no = fc.targets(M, variant)
        ts = (_cuda(th), _cuda(to))
        latent, embed = _bind(hip, TAG, SAMPLE)
        z0 = torch.zeros(L)
        z, history = hip.fit_code(x, ts[0], ts[1], nh, no, latent, z0=z0, **kw)
        bound = _np(_f32_values(hip, x)[0])                 # the decoder is left bound to the fitted code
        _bind(hip, TAG, SAMPLE)
        z2, history2 = hip.fit_code(x, ts[0], ts[1], nh, no, latent, z0=z0, **kw)
        assert np.array_equal(_bits(z), _bits(z2)) and np.array_equal(_np(history), _np(history2)), "the same call twice"
        zl, hl = fit_code_lockstep(hip, latent, embed, x, ts[0], ts[1], nh, no, z0=z0, **kw)
        rel = float((history - hl).abs().max() / hl.abs().max())
        print("FITCODE K=%-2d %-8s: data term %.6e -> %.6e, |z - z_start| %.3e, history vs lockstep rel %.1e" % (
            K, variant, float(history[0]), float(history[-1]), float((z.cpu() - latent).norm()), rel))
        assert np.array_equal(_bits(z), _bits(zl)), (K, variant, float((z - zl).abs().max()))
        assert ((history - hl).abs() <= 1e-12 * hl.abs()).all(), (K, variant, rel)
        hip.set_sample(z.reshape(1, -1), embed)
        assert np.array_equal(bound, _np(_f32_values(hip, x)[0]))


# ---- edges of the rule on the device -------------------------------------------------------------------------------------------------------
def test_values_exactly_at_the_clamp_and_on_the_target(decoders):
    from alignsdf_amd.fit import adam_step_host, adam_step_table, clamped_l1_rule, prior_factor
    hip = decoders(TAG)
    latent, _ = _bind(hip, TAG, SAMPLE)
    M = 257
    x = _cuda(vc.list_points(M))
    f = [_np(v) for v in _f32_values(hip, x)]
    th, to, nh, no = fc.targets(M, "both")
    for sign in (1.0, -1.0):
        # c = |f| of one hand point of this sign: on that point f == sign c exactly
        j = int(np.argmax(sign * f[0]))
        c = float(abs(f[0][j]))
        assert sign * f[0][j] > 0
        t = th.copy()
        t[j] = np.float32(0.0)                               # r = +-c: not zero, and f = +-c passes the inclusive mask
        ts = (_cuda(t), _cuda(to))
        _bind(hip, TAG, SAMPLE)
        want, data, ws = _one_step_reference(hip, x, ts, (nh, no), latent, latent, 0.0, c)
        assert float(ws[0][j]) == sign * float(np.float32(1.0 / nh)), "the clamp's mask is inclusive"
        z, history = hip.fit_code(x, ts[0], ts[1], nh, no, latent, steps=1, lr=LR, decay=1.0, every=1, prior=0.0, clamp=c)
        assert np.array_equal(_bits(z), _bits(want)) and abs(float(history[0]) - data) <= 1e-12 * data, sign
        # ... and with that point's weight forced off the result differs: the point did pull
        t[j] = np.float32(np.nan)
        _bind(hip, TAG, SAMPLE)
        z_off, _ = hip.fit_code(x, _cuda(t), ts[1], nh, no, latent, steps=1, lr=LR, decay=1.0, every=1, prior=0.0, clamp=c)
        assert not np.array_equal(_bits(z), _bits(z_off))
    # f == t on every point of both heads, unclamped: w = 0 everywhere, the data term is 0 and only the prior moves the code
    _bind(hip, TAG, SAMPLE)
    z0 = torch.zeros(L)
    z, history = hip.fit_code(x, _cuda(f[0]), _cuda(f[1]), M, M, latent, z0=z0, steps=1, lr=LR, decay=1.0, every=1, prior=0.5, clamp=float("inf"))
    a, s = adam_step_table(1, LR)[0]
    zero = np.zeros(L, np.float32)
    want = adam_step_host(_np(latent), zero, zero, zero, zero, prior_factor(0.5, L), a, s)[0]
    assert float(history[0]) == 0.0 and np.array_equal(_bits(z), _bits(want)) and not np.array_equal(_bits(z), _bits(latent))
    l, w = clamped_l1_rule(torch.from_numpy(f[0]), torch.from_numpy(f[0]), float("inf"), M)
    assert not l.any() and not w.any()


def test_no_work_leaves_the_code_and_refusals_are_refusals(decoders):
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    hip = decoders(TAG)
    latent, _ = _bind(hip, TAG, SAMPLE)
    bound = hip._bound
    x = _cuda(vc.list_points(33))
    th, to, nh, no = fc.targets(33, "both")
    z, history = hip.fit_code(x, _cuda(th), _cuda(to), nh, no, latent, steps=0)
    assert np.array_equal(_bits(z), _bits(latent)) and history.numel() == 0 and hip._bound is bound
    z, history = hip.fit_code(x[:0], _cuda(th[:0]), _cuda(to[:0]), 0, 0, latent, steps=3)
    assert np.array_equal(_bits(z), _bits(latent)) and not _np(history).any() and hip._bound is bound
    # the C call: an unbound decoder is EINVAL, the decoders the reverse-mode form refuses are ENOGRAD
    lib = _native.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    zc, table = latent.clone().cuda(), torch.ones(2, device="cuda")
    state = torch.empty(_native.FIT_STATE_BYTES // 4, device="cuda")
    t33 = _cuda(th)

    def call(dec):
        return lib.asdf_fit_code(dec._h, ptr(x), 33, ptr(t33), 33, None, 0, ctypes.c_float(CLAMP), ptr(zc), None, ctypes.c_float(0.0), ptr(table), 1,
                                 ptr(state), _native.FIT_STATE_BYTES, None, st)
    fresh = HipSdfDecoder(gc.module_for("nerf3"))
    assert call(fresh) == -1                                   # ASDF_EINVAL
    fresh.close()
    for tag, pf, word in (("comb3", 3, "CombinedDecoder"), ("nerf9", 9, "NeRF")):
        dec = HipSdfDecoder(syn.full_state_dict(tag), 256, pf, "nerf")
        dec.set_sample(torch.from_numpy(syn.latent_code(1)))
        assert call(dec) == _native.ENOGRAD and word in dec.fit_code_refusal()
        with pytest.raises(NotImplementedError, match=word):
            dec.fit_code(x, t33, None, 33, 0, latent, steps=1)
        dec.close()
    assert np.array_equal(_bits(zc), _bits(latent))


def test_no_head_has_targets_only_the_prior_moves_the_code(decoders):
    """n_hand = n_obj = 0 with M > 0: no data term.  The code takes `steps` Adam steps on the prior alone - adam_step_host with d_latent =
    0, bit for bit -, the history is exactly zero, and the decoder is left bound to the result.  The C call answers ASDF_OK."""
    from alignsdf_amd.fit import adam_step_host, adam_step_table, prior_factor
    hip = decoders(TAG)
    latent, embed = _bind(hip, TAG, SAMPLE)
    M, steps = 33, 3
    x = _cuda(vc.list_points(M))
    z, history = hip.fit_code(x, None, None, 0, 0, latent, z0=torch.zeros(L), steps=steps, lr=LR, decay=0.5, every=2, prior=0.5, clamp=CLAMP)
    bound = [_np(v).copy() for v in _f32_values(hip, x)]
    zero = np.zeros(L, np.float32)
    want, m, v = _np(latent), zero, zero
    for a, s in adam_step_table(steps, LR, 0.5, 2):
        want, m, v = adam_step_host(want, m, v, zero, zero, prior_factor(0.5, L), a, s)
    assert np.array_equal(_bits(z), _bits(want)) and not np.array_equal(_bits(z), _bits(latent))
    assert tuple(history.shape) == (steps,) and not _np(history).view(np.int64).any(), _np(history)
    assert not _np(hip._fit_state[3 * L:4 * L]).view(np.int32).any(), "d_latent is +0"
    hip.set_sample(z.reshape(1, -1), embed)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(bound, _f32_values(hip, x)))
    # the ABI, directly: one step without targets
    _bind(hip, TAG, SAMPLE)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    zc, table = latent.clone().cuda(), _cuda(adam_step_table(1, LR).reshape(-1))
    state = torch.empty(_native.FIT_STATE_BYTES // 4, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = _native.lib().asdf_fit_code(hip._h, ptr(x), M, None, 0, None, 0, ctypes.c_float(CLAMP), ptr(zc), None, ctypes.c_float(0.5), ptr(table), 1,
                                       ptr(state), _native.FIT_STATE_BYTES, None, st)
    torch.cuda.synchronize()
    assert code == 0                                           # ASDF_OK; (z0 = the start code: the prior's gradient is 0 and the code stays)
    assert np.array_equal(_bits(zc), _bits(latent))


# ---- against an fp64 truth, one step ---------------------------------------------------------------------------------------------------------
def test_loss_form_gradient_against_the_fp64_reverse_chain(decoders):
    """d_latent of the loss form (read from the call's state buffer: [z | m | v | d_latent | z0]) against vjp_truth with weights formed
    in fp64, on the points that are clear in fp64; the points that are not carry a NaN target - n stays the list's length, as the
    truth's weights have it.  The tolerance is tests/test_gpu_sdf_vjp.py's for d_latent."""
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    hip = decoders(TAG)
    latent, _ = _bind(hip, TAG, SAMPLE)
    case = fc.truth_case()
    pts, M = case["pts"], len(case["pts"])
    x = _cuda(pts)
    ts = [_cuda(np.where(case["clear"][name], case["t"][name], np.float32(np.nan)).astype(np.float32)) for name in vc.HEADS]
    hip.fit_code(x, ts[0], ts[1], M, M, latent, steps=1, lr=LR, decay=1.0, every=1, prior=0.0, clamp=CLAMP)
    got = _np(hip._fit_state[3 * L:4 * L]).astype(np.float64)
    truth = vc.vjp_truth(TAG, SAMPLE, pts, case["w64"])["d_latent"]
    w32 = {name: case["w64"][name].astype(np.float32) for name in vc.HEADS}
    mod = TorchModuleDecoder(gc.module_for(TAG), syn.specs_for(TAG), "held to the loss form's truth")
    lat, mano, obj = syn.sample_inputs(TAG, SAMPLE)
    mod.set_sample(torch.from_numpy(lat), _t(mano), _t(obj))
    g_mod = _np(mod.decode_points_vjp(x, _cuda(w32["hand"]), _cuda(w32["obj"])).d_latent).astype(np.float64)
    g_or = vc.oracle_autograd_vjp(TAG, SAMPLE, pts, w32, torch.float32)["d_latent"].astype(np.float64)
    err = lambda a: (float(np.abs(a - truth).max()), float(np.sqrt(np.mean((a - truth) ** 2))))
    (e_k, r_k), (e_mod, r_mod), (e_or, r_or) = err(got), err(g_mod), err(g_or)
    top = float(np.abs(truth).max())
    print("FITCODE loss-form d_latent M=%d max|truth| %.2e: e_k %.2e e_mod %.2e e_or %.2e | rms %.2e %.2e %.2e | clear %.3f %.3f" % (
        M, top, e_k, e_mod, e_or, r_k, r_mod, r_or, case["clear"]["hand"].mean(), case["clear"]["obj"].mean()))
    assert top > 0 and np.isfinite(got).all()
    assert e_k <= 3.0 * max(e_mod, e_or) + 5e-7 * max(1.0, top), (e_k, e_mod, e_or)
    assert r_k <= 1.5 * max(r_mod, r_or), (r_k, r_mod, r_or)


# ---- outcome -----------------------------------------------------------------------------------------------------------------------------
def test_fit_ends_where_the_fp64_rule_ends(decoders):
    """Targets: the nerf3 decoder's own two fields at a known code z*, 2048 points per head (seeds 21, 22); fit from 0 for 200 steps.
    The yardstick is the same rule in fp64 on the module; the fp32 module path's distance from it in final data term (taken in fp64 at
    each path's final code) is measured here, and the device fit may end at most 4 times as far - both are fp32 restatements of one
    rule and Adam amplifies their roundings alike - with a floor of 1 % of the fp64 run's final term."""
    from alignsdf_amd.fit import fit_code_lockstep
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    tag = "nerf3"
    hip = decoders(tag)
    z_star, _ = _bind(hip, tag, 1)
    xs = [np.random.default_rng(seed).uniform(-1.0, 1.0, (2048, 3)).astype(np.float32) for seed in (21, 22)]
    x = _cuda(np.concatenate(xs))
    f = _f32_values(hip, x)
    nan = torch.full((2048,), float("nan"), device="cuda")
    th, to = torch.cat([f[0][:2048], nan]), torch.cat([nan, f[1][2048:]])
    kw = dict(steps=200, lr=5e-3, decay=0.1, every=100, prior=1e-4, clamp=0.05)      # the flow's schedule in shape: a tenth of the rate over the second half
    start = torch.zeros(L)
    hip.set_sample(start.reshape(1, -1))
    z_dev, history = hip.fit_code(x, th, to, 2048, 2048, start, **kw)
    mod = TorchModuleDecoder(gc.module_for(tag), syn.specs_for(tag), "the outcome's yardstick")
    z_64, h64 = fit_code_lockstep(mod, start, None, x, th, to, 2048, 2048, dtype=torch.float64, **kw)
    z_32, _ = fit_code_lockstep(mod, start, None, x, th, to, 2048, 2048, **kw)
    term = lambda z: float(fit_code_lockstep(mod, z.double(), None, x, th, to, 2048, 2048, dtype=torch.float64, **dict(kw, steps=1))[1][0])
    t_dev, t_64, t_32 = term(z_dev), term(z_64), term(z_32)
    gap = abs(t_32 - t_64)
    print("FITCODE outcome: data term %.6e at the start; final fp64 %.6e, fp32 module %.6e (gap %.3e), device %.6e (off by %.3e); "
          "|z_dev - z*| / |z*| %.3f" % (float(h64[0]), t_64, t_32, gap, t_dev, abs(t_dev - t_64), float((z_dev.cpu() - z_star).norm() / z_star.norm())))
    assert t_64 < float(h64[0]), "the fp64 rule itself descends"
    assert abs(t_dev - t_64) <= max(4.0 * gap, 0.01 * t_64), (t_dev, t_64, t_32)


# ---- the flow ----------------------------------------------------------------------------------------------------------------------------
def _write_obj(path, verts, faces):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        for p in np.asarray(verts, np.float64):
            fh.write("v %.9g %.9g %.9g\n" % tuple(float(c) for c in p))
        for t in np.asarray(faces):
            fh.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


def _experiment(root, tag):
    os.makedirs(os.path.join(root, "ModelParameters"))
    with open(os.path.join(root, "specs.json"), "w") as fh:
        json.dump(syn.specs_for(tag), fh)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in syn.full_state_dict(tag).items()}
    torch.save({"model_state_dict": {"module.decoder." + k: v for k, v in sd.items()}}, os.path.join(root, "ModelParameters", "latest.pth"))


def test_autodecode_then_reconstruct(tmp_path, decoders):
    """Two grasp scenes of the grasp3 decoder: meshes by marching cubes of its own fields at N = 64, auto-decoded (150 steps),
    reconstructed from the written codes at N = 64.  Per scene and head, with d = mean |MeshField.at(vertices of a reconstruction)| in
    the field of the mesh the code was fitted to:
      - d of the fitted code's reconstruction is at most ONE VOXEL of that lattice (2 / 63): both surfaces are 64-lattice meshes, and a
        fit further off than their own resolution is not a fit (a wrong frame, scale or head is off by far more);
      - it is smaller than d of the reconstruction from the OTHER scene's fitted code - a baseline that has a surface, and must;
      - it is smaller than d of the reconstruction from the zero code, where that one has a surface.  On this decoder the zero code's
        fields have no zero level inside the cube, so no file is written: the test shows that (the sign of the field on the lattice)
        before it accepts a missing file, and a missing file with a zero level present fails."""
    from alignsdf_amd import autodecode as ad, reconstruct as rc
    from alignsdf_amd.code_sources import npz_code_source
    from alignsdf_amd.marching_cubes import marching_cubes_device
    from alignsdf_amd.mesh_sdf import MeshField
    from alignsdf_amd.ply import read_ply
    from alignsdf_amd.utils.mesh import lattice_points
    tag, N, names = "grasp3", 64, ("00000003", "00000007")
    specs = syn.specs_for(tag)
    hip = decoders(tag)
    origin, voxel = [-1.0, -1.0, -1.0], 2.0 / (N - 1)
    idx = torch.stack(torch.meshgrid(*[torch.arange(N, dtype=torch.float32, device="cuda")] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = lattice_points(idx, origin, voxel)
    truth = {}
    for name, sample in zip(names, (3, 7)):
        _bind(hip, tag, sample)
        for part, vol in zip(("hand", "obj"), _f32_values(hip, pts)):
            v, f = marching_cubes_device(vol.reshape(N, N, N).contiguous(), 0.0)
            xyz = lattice_points(v, origin, voxel)
            truth[name, part] = MeshField(xyz, f)
            _write_obj(str(tmp_path / "data" / "obman" / "test" / ("mesh_" + part) / (name + ".obj")),
                       ad.from_decoder_frame(_np(xyz), 1.0, (0, 0, 0), specs["SdfScaleFactor"]), _np(f))
    split = str(tmp_path / "split.json")
    with open(split, "w") as fh:
        json.dump({"filenames": ["data/obman/test/rgb/%s.jpg" % n for n in names]}, fh)
    for run in ("fit", "zero", "swap"):
        _experiment(str(tmp_path / run), tag)
    codes, zeros, swapped = str(tmp_path / "codes"), str(tmp_path / "codes0"), str(tmp_path / "codes_swapped")
    ad.main(["-e", str(tmp_path / "fit"), "-t", "obman", "--data_root", str(tmp_path / "data"), "--out", codes, "--steps", "150",
             "--near", "6000", "--uniform", "2000"])
    report = {r["name"]: r for r in json.load(open(os.path.join(codes, "autodecode.json")))["samples"]}
    assert list(report) == list(names) and all(r["steps"] == 150 and r["last"] < r["first"] for r in report.values())
    source = npz_code_source(codes)
    os.makedirs(zeros), os.makedirs(swapped)
    for n, other in zip(names, names[::-1]):
        lat, mano, obj = source(n, 0)
        assert tuple(lat.shape) == (1, 256) and mano is None and obj is None and bool(torch.isfinite(lat).all()) and bool(lat.any())
        ad.write_code(zeros, n, np.zeros(256, np.float32), {})
        ad.write_code(swapped, other, lat.numpy(), {})
    for run, code_dir in (("fit", codes), ("zero", zeros), ("swap", swapped)):
        recs = rc.main(["--model", str(tmp_path / run), "--split", split, "--codes", code_dir, "--cube_dim", str(N)])
        assert len(recs) == 2
    # where the zero code leaves no file, that must be because its field has no zero level in the cube at all - shown, not assumed
    hip.set_sample(torch.zeros(1, 256))
    zero_has_level = {part: bool((vol < 0).any()) and bool((vol > 0).any()) for part, vol in zip(("hand", "obj"), _f32_values(hip, pts))}
    for name in names:
        for part in ("hand", "obj"):
            dist = {}
            for run in ("fit", "zero", "swap"):
                path = str(tmp_path / run / "Eval_obman" / "meshes" / ("%s_%s.ply" % (name, part)))
                dist[run] = float(truth[name, part].at(_cuda(np.asarray(read_ply(path)[0], np.float32))).sdf.abs().mean()) if os.path.exists(path) else None
            show = lambda v: "no surface" if v is None else "%.5f" % v
            print("FITCODE flow %s %-4s: mean |gt field| on the reconstruction: fitted %s, the other scene's code %s, the zero code %s "
                  "(data term %.4e -> %.4e)" % (name, part, show(dist["fit"]), show(dist["swap"]), show(dist["zero"]), report[name]["first"], report[name]["last"]))
            assert dist["fit"] is not None and dist["swap"] is not None, (name, part, dist)
            assert dist["fit"] <= voxel, (name, part, dist)
            assert dist["fit"] < dist["swap"], (name, part, dist)
            if dist["zero"] is None:
                assert not zero_has_level[part], (name, part, "the zero code has a zero level, but no file was written")
            else:
                assert dist["fit"] < dist["zero"], (name, part, dist)


# ---- decoders the kernel refuses: the same rule on the module path --------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["nerf9", "comb3"])
def test_refused_decoders_are_fitted_on_the_module_path(tag, tmp_path):
    """NeRF-encoded features and CombinedDecoder: the forward kernels cover them (decoder_for hands out a HipSdfDecoder), the fit kernel
    does not.  fit.fit_code given the module runs fit_code_lockstep on a TorchModuleDecoder of it - the result of calling that
    directly, bit for bit, and a descent; without the module it is a NotImplementedError with the reason.  And the flow's fitter
    gets there by itself: DeviceFitter on such an experiment writes a code."""
    from alignsdf_amd import autodecode as ad
    from alignsdf_amd.fit import fit_code, fit_code_lockstep, fit_targets
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    from alignsdf_amd.utils.utils import decoder_for
    from tests import mesh_sdf_cases as mc
    specs, module = syn.specs_for(tag), gc.module_for(tag)
    hip = decoder_for(module, specs, None)
    assert hasattr(hip, "fit_code_refusal") and hip.fit_code_refusal() is not None
    target, start = torch.from_numpy(syn.latent_code(1)).reshape(-1), torch.from_numpy(syn.latent_code(2)).reshape(-1)
    x = _cuda(vc.points(96, 4))
    hip.set_sample(target.reshape(1, -1))
    f = _f32_values(hip, x)
    kw = dict(steps=6, lr=5e-3, decay=1.0, every=1, prior=1e-4, clamp=0.2)
    with pytest.raises(NotImplementedError, match="module"):
        fit_code(hip, start, None, sdf_hand=(x, f[0]), sdf_obj=(x, f[1]), **kw)
    z, history = fit_code(hip, start, None, sdf_hand=(x, f[0]), sdf_obj=(x, f[1]), module=module, specs=specs, **kw)
    mod = TorchModuleDecoder(module, specs, "the fallback, called directly")
    zl, hl = fit_code_lockstep(mod, start, None, *fit_targets(mod, (x, f[0]), (x, f[1])), **kw)
    print("FITCODE module path %-5s: data term %.4e -> %.4e in 6 steps" % (tag, float(history[0]), float(history[-1])))
    assert np.array_equal(_bits(z), _bits(zl)) and np.array_equal(_np(history), _np(hl))
    assert float(history[-1]) < float(history[0]) and not np.array_equal(_bits(z), _bits(start))
    # the flow: a torus "hand" and a box "object" in the decoder's frame, a few steps
    (hv, hf), (bv, bf) = mc.torus(*mc.TORUS_EDGE), mc.box()
    for part, v, faces in (("hand", hv, hf), ("obj", bv, bf)):
        _write_obj(str(tmp_path / "data" / "obman" / "test" / ("mesh_" + part) / "00000001.obj"),
                   ad.from_decoder_frame(0.5 * np.asarray(v, np.float64), 1.0, (0, 0, 0), specs["SdfScaleFactor"]), faces)
    fitter = ad.DeviceFitter(module, specs, fit=dict(kw, steps=4), sampling={"near": 300, "uniform": 100})
    path, records = ad.run(specs, fitter, "obman", str(tmp_path / "data"), str(tmp_path / "codes"))
    lat = np.load(str(tmp_path / "codes" / "00000001.npz"))["latent"]
    assert records[0]["steps"] == 4 and records[0]["last"] < records[0]["first"] and lat.shape == (1, 256) and np.isfinite(lat).all() and lat.any()
