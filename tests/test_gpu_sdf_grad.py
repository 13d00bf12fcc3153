"""The gradient form of the fp32 chain (csrc/k1g_kernels.hip, sdf_mlp_grad_kernel.h; asdf_decode_points_grad;
HipSdfDecoder.decode_points_grad) held to an fp64 forward-mode truth (tests/sdf_grad_cases.grad_truth), and the vertex normals the
mesh flows write from it.

Yardsticks, as tests/test_gpu_pixel_align_fp64.py - per head, over the CLEAR points of a set (no hidden unit within 1e-5 of its kink:
there fp32 may legitimately take either ReLU mask, and one flip moves a component by several 1e-3):

    e_k    largest |grad native - grad truth|
    e_mod  the same for TorchModuleDecoder.decode_points_grad (torch autograd through the module on the GPU)
    e_or   the same for fp32 autograd through the oracle on the CPU

    e_k <= 3 max(e_mod, e_or) + 5e-7 max(1, max |grad truth|);   on 4096 points or more also rms_k <= 1.5 max(rms_mod, rms_or)
    on the other points: every output finite and |grad native| <= 2 max |grad truth|

Every line printed with the prefix SDFGRAD is one case's measured errors (profiles/sdf_grad_fp64_errors.txt)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from alignsdf_amd import _native
from alignsdf_amd import synthetic as syn
from tests import sdf_grad_cases as gc

pytestmark = pytest.mark.gpu
RMS_FACTOR, RMS_MIN_POINTS = 1.5, 4096
HEADS = ("hand", "obj")


# ---- evaluators -----------------------------------------------------------------------------------------------------------------------
def _t(d):
    return None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def _native_decoder(tag, weights=None):
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    if weights is not None:
        pf, style = syn.specs_for(tag)["PointFeatSize"], syn.specs_for(tag)["EncodeStyle"]
        return HipSdfDecoder(weights, 256, pf, style)
    return HipSdfDecoder(gc.module_for(tag))


def _bind(dec, tag, sample):
    from alignsdf_amd.utils.utils import bind_sample
    latent, mano, obj = syn.sample_inputs(tag, sample)
    bind_sample(dec, syn.specs_for(tag), torch.from_numpy(latent), _t(mano), _t(obj))


@pytest.fixture(scope="module")
def decoders():
    """One native decoder per configuration, built on first use."""
    made = {}

    def get(tag):
        if tag not in made:
            made[tag] = _native_decoder(tag)
        return made[tag]
    yield get
    for d in made.values():
        d.close()


def _module_path(tag, sample):
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    mod = TorchModuleDecoder(gc.module_for(tag), syn.specs_for(tag), "held to the gradient truth")
    _bind(mod, tag, sample)
    return mod


def _np(v):
    return None if v is None else v.detach().cpu().numpy()


def _as_heads(res):
    """decode_points_grad's tuple -> {"hand" / "obj": {"sdf", "grad"}} (numpy), a head that is off left out."""
    out = {}
    for k, name in enumerate(HEADS):
        if res[2 * k] is not None:
            out[name] = {"sdf": _np(res[2 * k]), "grad": _np(res[2 * k + 1])}
    return out


# ---- truth and criterion ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _truth(tag, sample, key):
    """(points, fp64 truth, fp32 oracle autograd) of a point set; `key` = ("list", M) or ("full", M).  Computed once, never modified."""
    pts = gc.list_points(key[1]) if key[0] == "list" else gc.points(key[1])
    return pts, gc.grad_truth(tag, sample, pts), gc.oracle_autograd(tag, sample, pts)


def _err(a, b, keep):
    d = (np.asarray(a, np.float64) - b)[keep]
    return (float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))) if d.size else (0.0, 0.0)


def _check(label, truth, orc32, got, mod):
    for name in got:
        t, clear = truth[name], gc.clear_mask(truth[name])
        M = len(clear)
        assert clear.any() and (M <= 256 or clear.mean() >= gc.MIN_CLEAR_SHARE), (label, name, clear.mean())
        g = got[name]["grad"]
        assert np.isfinite(g).all() and np.isfinite(got[name]["sdf"]).all(), (label, name)
        gmax = float(np.abs(t["grad"]).max())
        e_k, r_k = _err(g, t["grad"], clear)
        e_mod, r_mod = _err(mod[name]["grad"], t["grad"], clear)
        e_or, r_or = _err(orc32[name]["grad"], t["grad"], clear)
        e_sdf = float(np.abs(got[name]["sdf"] - t["sdf"]).max())
        print("SDFGRAD %-26s %-4s M=%-5d clear %6.2f%% max|grad| %.2f: e_k %.2e e_mod %.2e e_or %.2e | rms %.2e %.2e %.2e | sdf %.2e" % (
            label, name, M, 100.0 * clear.mean(), gmax, e_k, e_mod, e_or, r_k, r_mod, r_or, e_sdf))
        assert e_k <= 3.0 * max(e_mod, e_or) + 5e-7 * max(1.0, gmax), (label, name, e_k, e_mod, e_or)
        if M >= RMS_MIN_POINTS:
            assert r_k <= RMS_FACTOR * max(r_mod, r_or), (label, name, r_k, r_mod, r_or)
        assert (np.abs(g[~clear]) <= 2.0 * gmax).all(), (label, name)


def _run_set(label, tag, key, decoders):
    """decode_points_grad on the set against the truth; value identity with decode_points; returns (points, native results)."""
    pts, truth, orc32 = _truth(tag, gc.SAMPLE, key)
    hip = decoders(tag)
    _bind(hip, tag, gc.SAMPLE)
    x = torch.from_numpy(pts).cuda()
    res = hip.decode_points_grad(x)
    got = _as_heads(res)
    mod = _as_heads(_module_path(tag, gc.SAMPLE).decode_points_grad(x))
    _check(label, truth, orc32, got, mod)
    # the value column is the fp32 chain of decode_points: the same bits under set_math("f32"), within the parity bar otherwise
    before = hip.math
    h, o = hip.decode_points(x)
    assert np.abs(_np(h) - got["hand"]["sdf"]).max() <= 1e-5 and np.abs(_np(o) - got["obj"]["sdf"]).max() <= 1e-5, label
    hip.set_math("f32")
    h, o = hip.decode_points(x)
    hip.set_math(before)
    assert np.array_equal(_np(h), got["hand"]["sdf"]) and np.array_equal(_np(o), got["obj"]["sdf"]), label
    return x, res


# ---- 1. point lists and full sets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", gc.LIST_LENGTHS)
def test_point_list_lengths(M, decoders):
    """Partial quads of columns, partial waves, one workgroup, many - on both9 (an affine embedding, different per head); and the
    reversed list gives the reversed outputs bit for bit: a point's result does not depend on its quad, wave or workgroup."""
    x, res = _run_set("both9 list", "both9", ("list", M), decoders)
    hip = decoders("both9")
    rev = hip.decode_points_grad(torch.flip(x, [0]).contiguous())
    for a, b in zip(res, rev):
        assert np.array_equal(_np(a), _np(b)[::-1])


@pytest.mark.parametrize("tag", gc.FULL_TAGS)
def test_full_sets(tag, decoders):
    x, res = _run_set("%s full" % tag, tag, ("full", 4096), decoders)
    hip = decoders(tag)
    rev = hip.decode_points_grad(torch.flip(x, [0]).contiguous())
    for a, b in zip(res, rev):
        assert np.array_equal(_np(a), _np(b)[::-1])


# ---- 2. heads, pointers, refusals ------------------------------------------------------------------------------------------------------
def test_single_heads_and_null_pointers(decoders):
    hip = decoders("both9")
    _bind(hip, "both9", gc.SAMPLE)
    pts = gc.list_points(257)
    x = torch.from_numpy(pts).cuda()
    math_before = (hip.math, hip._L.asdf_decoder_get_math(hip._h))
    shape_before = _native.lib().asdf_get_mfma_shape()
    full = [_np(v) for v in hip.decode_points_grad(x)]
    only_h = hip.decode_points_grad(x, obj=False)
    only_o = hip.decode_points_grad(x, hand=False)
    assert only_h[2] is None and only_h[3] is None and only_o[0] is None and only_o[1] is None
    assert np.array_equal(_np(only_h[0]), full[0]) and np.array_equal(_np(only_h[1]), full[1])
    assert np.array_equal(_np(only_o[2]), full[2]) and np.array_equal(_np(only_o[3]), full[3])
    # through the C ABI: each NULL output pointer leaves the other three arrays as they are; M = 0 is OK
    L = _native.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for skip in range(4):
        bufs = [torch.full(s, 7.0, dtype=torch.float32, device="cuda") for s in ((257,), (257, 3), (257,), (257, 3))]
        ptr = [None if k == skip else ctypes.c_void_p(b.data_ptr()) for k, b in enumerate(bufs)]
        assert L.asdf_decode_points_grad(hip._h, x.data_ptr(), 257, *ptr, st) == 0
        for k, b in enumerate(bufs):
            assert np.array_equal(_np(b), np.full_like(full[k], 7.0) if k == skip else full[k]), (skip, k)
    assert L.asdf_decode_points_grad(hip._h, None, 0, None, None, None, None, st) == 0
    assert L.asdf_decode_points_grad(hip._h, None, 5, None, None, None, None, st) == L.asdf_decode_points(hip._h, None, 5, None, None, st) != 0
    assert L.asdf_decode_points_grad(None, x.data_ptr(), 5, None, None, None, None, st) == L.asdf_decode_points(None, x.data_ptr(), 5, None, None, st) != 0
    assert (hip.math, hip._L.asdf_decoder_get_math(hip._h)) == math_before
    assert L.asdf_get_mfma_shape() == shape_before
    e = hip.decode_points_grad(x[:0])
    assert e[0].shape == (0,) and e[1].shape == (0, 3)


def test_unbound_decoder_returns_what_decode_points_returns():
    hip = _native_decoder("nerf3")
    try:
        L = _native.lib()
        x = torch.zeros(4, 3, device="cuda")
        out = torch.zeros(4, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        want = L.asdf_decode_points(hip._h, x.data_ptr(), 4, out.data_ptr(), None, st)
        assert want != 0 and L.asdf_decode_points_grad(hip._h, x.data_ptr(), 4, out.data_ptr(), None, None, None, st) == want
    finally:
        hip.close()


def test_refusals():
    """comb3 and a pixel-aligned decoder: the C call returns the refusal code (with a text), the method raises NotImplementedError."""
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    L = _native.lib()
    assert _native.ENOGRAD < 0 and b"gradient" in L.asdf_strerror(_native.ENOGRAD)
    x = torch.zeros(4, 3, device="cuda")
    sdf, grad = torch.zeros(4, device="cuda"), torch.zeros(4, 3, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    comb = HipSdfDecoder(syn.full_state_dict("comb3"), 256, 3, "nerf")
    comb.set_sample(torch.from_numpy(syn.latent_code(1)))
    assert L.asdf_decode_points_grad(comb._h, x.data_ptr(), 4, sdf.data_ptr(), grad.data_ptr(), None, None, st) == _native.ENOGRAD
    with pytest.raises(NotImplementedError):
        comb.decode_points_grad(x)
    comb.close()
    specs, _, sd, _, _, _, _ = syn.variant_config("pixelalign")
    pa = HipSdfDecoder(sd, 256, 3, "nerf", pixel_align=True)
    feat, mano, cam = syn.pixel_align_sample(0, 8, 8)
    pa.set_sample_pixel(torch.from_numpy(feat).cuda(), cam, mano["joints"][0, 0], specs["ImageSize"][0], specs["SdfScaleFactor"])
    assert L.asdf_decode_points_grad(pa._h, x.data_ptr(), 4, sdf.data_ptr(), grad.data_ptr(), None, None, st) == _native.ENOGRAD
    with pytest.raises(NotImplementedError):
        pa.decode_points_grad(x)
    pa.close()
    nerf9 = HipSdfDecoder(syn.full_state_dict("nerf9"), 256, 9, "nerf")
    nerf9.set_sample(torch.from_numpy(syn.latent_code(1)))
    assert L.asdf_decode_points_grad(nerf9._h, x.data_ptr(), 4, sdf.data_ptr(), grad.data_ptr(), None, None, st) == _native.ENOGRAD
    with pytest.raises(NotImplementedError):
        nerf9.decode_points_grad(x)
    nerf9.close()


# ---- 3. re-binding -----------------------------------------------------------------------------------------------------------------------
def _held_to_truth(label, tag, sample, res, pts):
    truth = gc.grad_truth(tag, sample, pts)
    got = _as_heads(res)
    for name in HEADS:
        clear = gc.clear_mask(truth[name])
        e = _err(got[name]["grad"], truth[name]["grad"], clear)[0]
        gmax = float(np.abs(truth[name]["grad"]).max())
        print("SDFGRAD %-26s %-4s M=%-5d clear %6.2f%% max|grad| %.2f: e_k %.2e (bound 1e-5: a stale sample costs 1e-2 or more)" % (
            label, name, len(pts), 100.0 * clear.mean(), gmax, e))
        # the project's parity bar; the gradients of two samples differ by 1e-2 and more (asserted by the callers)
        assert clear.any() and e <= 1e-5 * max(1.0, gmax), (label, name, e)


def test_two_samples_alternate_on_one_decoder(decoders):
    hip = decoders("grasp9")
    pts = gc.list_points(257)
    x = torch.from_numpy(pts).cuda()
    seen = {}
    for sample in (1, 2, 1, 2):
        _bind(hip, "grasp9", sample)
        res = hip.decode_points_grad(x)
        if sample in seen:
            for a, b in zip(res, seen[sample]):
                assert np.array_equal(_np(a), b)
        else:
            seen[sample] = [_np(v).copy() for v in res]
            _held_to_truth("grasp9 rebind sample %d" % sample, "grasp9", sample, res, pts)
    assert np.abs(seen[1][1] - seen[2][1]).max() > 1e-2


def test_two_decoders_alternate_on_one_stream(decoders):
    one, two = decoders("grasp9"), decoders("both9")
    pts = gc.list_points(257)
    x = torch.from_numpy(pts).cuda()
    _bind(one, "grasp9", 3)
    _bind(two, "both9", 2)
    first = None
    for _ in range(2):
        ra, rb = one.decode_points_grad(x), two.decode_points_grad(x)
        if first is None:
            first = ([_np(v).copy() for v in ra], [_np(v).copy() for v in rb])
            _held_to_truth("grasp9 beside both9", "grasp9", 3, ra, pts)
            _held_to_truth("both9 beside grasp9", "both9", 2, rb, pts)
        else:
            for a, b in zip(ra, first[0]):
                assert np.array_equal(_np(a), b)
            for a, b in zip(rb, first[1]):
                assert np.array_equal(_np(a), b)
    assert np.abs(first[0][1] - first[1][1]).max() > 1e-2


# ---- 4. the flows: vertex normals in the written files, N = 32 on grasp9 ---------------------------------------------------------------
FLOW_TAG, FLOW_N = "grasp9", 32


def _flow_decoder():
    return gc.module_for(FLOW_TAG), syn.specs_for(FLOW_TAG)


def _check_normals_file(label, path_plain, path_normals, sample, degenerate, recompute=True):
    """The properties of one file written with normals; returns its normals."""
    from alignsdf_amd.ply import read_ply
    from alignsdf_amd.utils.utils import bind_sample, decoder_for
    pv, pf = read_ply(path_plain)
    v, f, n = read_ply(path_normals, with_normals=True)
    assert n is not None and np.array_equal(v, pv) and np.array_equal(f, pf), label
    length = np.sqrt((n.astype(np.float64) ** 2).sum(1))
    zero = ~n.any(axis=1)
    assert (np.abs(length[~zero] - 1.0) <= 1e-6).all() and int(zero.sum()) == degenerate, (label, int(zero.sum()), degenerate)
    if recompute:
        part = "hand" if path_normals.endswith("_hand.ply") else "obj"
        dec, specs = _flow_decoder()
        latent, mano, obj = syn.sample_inputs(FLOW_TAG, sample)
        hip = decoder_for(dec, specs, _t(mano))
        bind_sample(hip, specs, torch.from_numpy(latent), _t(mano), _t(obj))
        res = hip.decode_points_grad(torch.from_numpy(v).cuda())
        g = _np(res[1] if part == "hand" else res[3]).astype(np.float64)
        want = g / np.sqrt((g * g).sum(1, keepdims=True))
        truth = gc.grad_truth(FLOW_TAG, sample, v)[part]
        clear = gc.clear_mask(truth) & ~zero
        t = truth["grad"] / np.sqrt((truth["grad"] ** 2).sum(1, keepdims=True))
        worst, vs_truth = float(np.abs(n - want)[clear].max()), float(np.abs(n - t)[clear].max())
        print("SDFGRAD %-26s %-4s V=%-5d clear %6.2f%%: file normal vs recomputed %.2e, vs fp64 truth %.2e, degenerate %d" % (
            label, part, len(v), 100.0 * clear.mean(), worst, vs_truth, degenerate))
        assert clear.any() and worst <= 1e-5, (label, worst)
        # outward: the SDF grows along the normal (the truth's own gradient has a positive component along it)
        assert ((n * truth["grad"]).sum(1)[clear] > 0).all(), label
    return n


def _no_gradient_launch(*a, **k):
    raise AssertionError("a gradient launch in a run without normals")


def test_create_mesh_writes_normals(tmp_path, monkeypatch):
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.utils.mesh import create_mesh_combined_decoder
    dec, specs = _flow_decoder()
    latent, mano, obj = syn.sample_inputs(FLOW_TAG, 1)
    args = (True, True, False, dec, torch.from_numpy(latent), _t(mano), _t(obj), None, specs)
    plain, withn = str(tmp_path / "plain"), str(tmp_path / "normals")
    with monkeypatch.context() as m:          # without the option: no gradient launch
        m.setattr(HipSdfDecoder, "decode_points_grad", _no_gradient_launch)
        s0 = create_mesh_combined_decoder(*args, plain, N=FLOW_N, return_stats=True)
    s1 = create_mesh_combined_decoder(*args, withn, N=FLOW_N, return_stats=True, normals=True)
    assert "normals_degenerate_hand" not in s0 and s1["hand"] == s0["hand"] and s1["obj"] == s0["obj"] and s0["hand"][0] > 0 and s0["obj"][0] > 0
    for part in HEADS:
        _check_normals_file("create_mesh N=32", "%s_%s.ply" % (plain, part), "%s_%s.ply" % (withn, part), 1, s1["normals_degenerate_" + part])


def test_reconstruct_writes_normals(tmp_path, monkeypatch):
    """reconstruct() without normals (no gradient launch: the method is replaced by one that raises), with normals, and with normals
    in eval mode (the alignment is a translation and a positive scale: the hand's normals are the same bits)."""
    import json
    import os
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.ply import read_ply
    from alignsdf_amd.reconstruct import reconstruct, synthetic_code_source
    from alignsdf_amd.utils.mesh import ground_truth_mesh_path
    dec, specs = _flow_decoder()
    names = ["00000021", "00000022"]
    split = str(tmp_path / "split.json")
    with open(split, "w") as fh:
        json.dump({"filenames": ["skip/0.jpg"] + ["data/obman/test/rgb/%s.jpg" % n for n in names]}, fh)
    src = synthetic_code_source(FLOW_TAG)
    plain_dir, normal_dir, eval_dir, data_root = (str(tmp_path / d) for d in ("plain", "normals", "eval", "data"))
    kw = dict(cube_dim=FLOW_N, code_source=src)

    def refuse(*a, **k):
        raise AssertionError("a gradient launch in a run without normals")
    with monkeypatch.context() as m:
        m.setattr(HipSdfDecoder, "decode_points_grad", refuse)
        plain = reconstruct(dec, specs, split, plain_dir, 1, 3, **kw)
    assert not any(k.startswith("normals_") for r in plain for k in r)
    recs = reconstruct(dec, specs, split, normal_dir, 1, 3, normals=True, **kw)
    file_of = lambda d, name, part: os.path.join(d, "meshes", "%s_%s.ply" % (name, part))
    normals = {}
    for rec, before in zip(recs, plain):
        assert rec["V_hand"] == before["V_hand"] > 0 and rec["V_obj"] == before["V_obj"] > 0
        for part in HEADS:
            normals[rec["name"], part] = _check_normals_file("reconstruct N=32 %s" % rec["name"], file_of(plain_dir, rec["name"], part),
                                                             file_of(normal_dir, rec["name"], part), rec["index"],
                                                             rec["normals_degenerate_" + part])
    # eval mode: the ground truth of each sample is its own plain hand mesh under a known similarity
    for name in names:
        pv, pf = read_ply(file_of(plain_dir, name, "hand"))
        gt_path = ground_truth_mesh_path(file_of(eval_dir, name, "hand"), "obman", data_root)
        os.makedirs(os.path.dirname(gt_path), exist_ok=True)
        with open(gt_path, "w") as fh:
            for p in pv.astype(np.float64) * 1.09 + np.array([0.02, -0.01, 0.03]):
                fh.write("v %.9f %.9f %.9f\n" % tuple(p))
            for t in pf:
                fh.write("f %d %d %d\n" % tuple(t + 1))
    evald = reconstruct(dec, specs, split, eval_dir, 1, 3, normals=True, eval_mode=True, data_root=data_root, **kw)
    for rec in evald:
        assert "icp_skipped" not in rec and abs(rec["icp_scale"] - 1.09) < 5e-3
        for part in HEADS:
            v, f, n = read_ply(file_of(eval_dir, rec["name"], part), with_normals=True)
            assert np.array_equal(f, read_ply(file_of(plain_dir, rec["name"], part))[1])
            assert np.array_equal(n, normals[rec["name"], part]), (rec["name"], part)


def test_normals_on_a_nerf9_decoder_raise_before_any_file(tmp_path):
    import json
    import os
    from alignsdf_amd import reconstruct as rc
    from alignsdf_amd.networks.model import build_decoder
    specs = syn.specs_for("nerf9")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in syn.full_state_dict("nerf9").items()}
    dec = build_decoder(specs, sd)
    split = str(tmp_path / "split.json")
    with open(split, "w") as fh:
        json.dump({"filenames": ["data/obman/test/rgb/00000001.jpg", "data/obman/test/rgb/00000002.jpg"]}, fh)
    out = str(tmp_path / "out")
    with pytest.raises(NotImplementedError):
        rc.reconstruct(dec, specs, split, out, 0, 2, cube_dim=FLOW_N, code_source=rc.synthetic_code_source("nerf9"), normals=True)
    assert not os.listdir(os.path.join(out, "meshes"))
    # the command line: --normals on the same experiment
    model = tmp_path / "experiment"
    os.makedirs(model / "ModelParameters")
    with open(model / "specs.json", "w") as fh:
        json.dump(specs, fh)
    torch.save({"model_state_dict": {"module.decoder." + k: v for k, v in sd.items()}}, str(model / "ModelParameters" / "latest.pth"))
    with pytest.raises(NotImplementedError):
        rc.main(["--model", str(model), "--split", split, "--synthetic", "--normals", "--cube_dim", str(FLOW_N)])
    meshes = model / "Eval_obman" / "meshes"
    assert not meshes.exists() or not os.listdir(meshes)


def test_dist_reconstruct_command_line_with_normals(tmp_path):
    """`python -m alignsdf_amd.dist_reconstruct ... --normals` (one rank; eval mode without ground truth, one process): every file
    carries unit normals and every record of the summary its degenerate counts."""
    import json
    import os
    import subprocess
    import sys
    from alignsdf_amd.ply import read_ply
    from tests.test_experiment_io import make_experiment
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = str(tmp_path / "experiment")
    _, split = make_experiment(exp, "nerf3", ["00000012", "00000047"])
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, "-m", "alignsdf_amd.dist_reconstruct", "-e", exp, "-t", "obman", "--split", split, "--synthetic",
           "--allow_missing_gt", "--data_root", str(tmp_path / "data"), "--cube_dim", str(FLOW_N), "--normals"]
    proc = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    records = json.load(open(os.path.join(exp, "Eval_obman", "reconstruct_summary.json")))["records"]
    assert len(records) == 2
    for rec in records:
        for part in HEADS:
            v, f, n = read_ply(os.path.join(exp, "Eval_obman", "meshes", "%s_%s.ply" % (rec["name"], part)), with_normals=True)
            assert len(v) == len(n) > 0 and len(f) > 0
            zero = ~n.any(axis=1)
            assert int(zero.sum()) == rec["normals_degenerate_" + part]
            assert (np.abs(np.sqrt((n.astype(np.float64) ** 2).sum(1))[~zero] - 1.0) <= 1e-6).all()
