"""HipSdfDecoder.trace_rays / asdf_trace_rays (csrc/k1t_kernels.hip) on the GPU.

  1. bit-for-bit replay: tests/sdf_trace_cases.march over decode_points under set_math("f32") gives t, status, bracket and evals of
     every ray - the kernel samples where the rule says, and its sdf at a sample is decode_points' bit for bit
  2. slot independence: a ray's result does not depend on which column it sits in or on what its neighbours do
  3. fp64 truth, independent of the point kernel: on DECIDED rays the status is the truth's, on DECIDED HITs |t - t64| is within 4 x the
     fp32-against-fp64 figure the CPU test recorded (profiles/sdf_trace_fp64_errors.txt; 4 x: the kernel sums its products in another
     order than torch's fp32 GEMM)
  4. the edges of the rule, 5. the C ABI, 6. render_view and reconstruct(render=...)"""
import ctypes
import filecmp
import json
import os

import numpy as np
import pytest
import torch

from alignsdf_amd import _native
from alignsdf_amd import synthetic as syn
from tests import sdf_trace_cases as tc

pytestmark = pytest.mark.gpu
HEADS = ("hand", "obj")
KEYS = ("t", "status", "bracket", "evals")


def _t(d):
    return None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def _bind(dec, tag, sample=tc.SAMPLE):
    from alignsdf_amd.utils.utils import bind_sample
    latent, mano, obj = syn.sample_inputs(tag, sample)
    bind_sample(dec, syn.specs_for(tag), torch.from_numpy(latent), _t(mano), _t(obj))


@pytest.fixture(scope="module")
def decoders():
    """One native decoder per configuration, built on first use and bound to sample 1."""
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    made = {}

    def get(tag):
        if tag not in made:
            made[tag] = HipSdfDecoder(tc.module_for(tag))
            _bind(made[tag], tag)
        return made[tag]
    yield get
    for d in made.values():
        d.close()


def _np(res):
    return {name: {k: v.cpu().numpy() for k, v in r.items()} for name, r in res.items() if r is not None}


def _trace(hip, rays, **kw):
    r = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).cuda()
    kw = dict({"want_bracket": True, "want_evals": True}, **kw)
    return _np(hip.trace_rays(r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7], **kw))


def _point_evaluators(hip):
    """{"hand" / "obj": f(points) -> sdf} over decode_points; the caller holds the decoder under set_math("f32")."""
    def head(k):
        return lambda pts: hip.decode_points(torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda())[k].cpu().numpy()
    return {"hand": head(0), "obj": head(1)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same_bits(label, got, want, rows=None):
    for name in HEADS:
        for k in KEYS:
            g, w = got[name][k], want[name][k]
            if rows is not None:
                g, w = g[rows[0]], w[rows[1]]
            bad = np.nonzero(_bits(g).reshape(len(g), -1) != _bits(w).reshape(len(w), -1))[0]
            assert not len(bad), (label, name, k, len(bad), bad[:5].tolist(), g[bad[:3]].tolist(), w[bad[:3]].tolist())


def _replay(hip, rays, **rule):
    before = hip.math
    hip.set_math("f32")
    try:
        f = _point_evaluators(hip)
        return {name: tc.march(f[name], rays, **dict(tc.RULE, **rule)) for name in HEADS}
    finally:
        hip.set_math(before)


# ---- 1. replay ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,M", [("both9", M) for M in tc.LIST_LENGTHS] + [("grasp9", 768)])
def test_trace_replays_the_rule_over_decode_points_bit_for_bit(decoders, tag, M):
    hip = decoders(tag)
    rays = tc.ray_set(M)
    got, want = _trace(hip, rays, **tc.RULE), _replay(hip, rays)
    for name in HEADS:
        s = got[name]["status"]
        print("SDFTRACE replay %s M=%d %s: HIT %d MISS %d INSIDE %d EXHAUSTED %d evals mean %.1f max %d" % (
            tag, M, name, (s == tc.HIT).sum(), (s == tc.MISS).sum(), (s == tc.INSIDE).sum(), (s == tc.EXHAUSTED).sum(),
            got[name]["evals"].mean(), got[name]["evals"].max()))
        assert got[name]["evals"].max() <= tc.RULE["max_steps"] + tc.RULE["refine_steps"] + 1
    _assert_same_bits("%s M=%d" % (tag, M), got, want)


# ---- 2. slot independence ------------------------------------------------------------------------------------------------------------------
def test_a_rays_result_does_not_depend_on_its_slot_or_its_neighbours(decoders):
    hip = decoders("both9")
    rays = tc.ray_set(1000)
    base = _trace(hip, rays, **tc.RULE)
    perm = np.random.default_rng(5).permutation(len(rays))
    _assert_same_bits("permuted", _trace(hip, rays[perm], **tc.RULE), base, rows=(np.arange(len(rays)), perm))
    holes = rays.copy()
    holes[1::2, 6], holes[1::2, 7] = 1.0, 0.0            # every second ray over before its first sample
    got = _trace(hip, holes, **tc.RULE)
    keep = np.arange(0, len(rays), 2)
    _assert_same_bits("every second ray a MISS", got, base, rows=(keep, keep))
    for name in HEADS:
        assert (got[name]["status"][1::2] == tc.MISS).all() and (got[name]["evals"][1::2] == 0).all()
        assert np.isposinf(got[name]["t"][1::2]).all()


# ---- 3. fp64 truth ----------------------------------------------------------------------------------------------------------------------------
def _recorded(tag, name):
    """The CPU test's fp32-against-fp64 figure for (tag, head): the one `cpu <tag> <head> ... max_dt <x>` line of the errors file."""
    return tc.recorded("cpu", tag, name)


def _check_against_truth(label, tag, got, truth):
    """Status on DECIDED rays, t on DECIDED HITs; returns {head: measured max |dt|}."""
    out = {}
    for name in HEADS:
        ok = tc.decided(truth[name])
        assert ok.mean() >= tc.MIN_DECIDED_SHARE, (label, name, ok.mean())
        assert np.array_equal(got[name]["status"][ok], truth[name]["status"][ok]), (
            label, name, np.nonzero(ok & (got[name]["status"] != truth[name]["status"]))[0][:8].tolist())
        hits = ok & (truth[name]["status"] == tc.HIT)
        assert hits.sum() >= 1
        e = float(np.abs(got[name]["t"][hits].astype(np.float64) - truth[name]["t"][hits]).max())
        bound = 4.0 * _recorded(tag, name)
        print("SDFTRACE truth %s %s: decided %.1f%% hits %d max|dt| %.3e bound %.3e" % (label, name, 100 * ok.mean(), hits.sum(), e, bound))
        out[name] = e
        assert e <= bound, (label, name, e, bound)
    return out


@pytest.mark.parametrize("tag", ["grasp9", "grasp3"])
def test_trace_against_the_fp64_truth(decoders, tag):
    rays = tc.ray_set(768)
    got = _trace(decoders(tag), rays, **tc.RULE)
    truth = tc.trace_truth(tag, tc.SAMPLE, 768)
    measured = _check_against_truth("%s M=768" % tag, tag, got, truth)
    if os.environ.get("ASDF_RECORD_TRACE_ERRORS"):          # (the committed file is written on request only)
        tc.record(["gpu %s %s M=768 max_dt %.3e" % (tag, name, measured[name]) for name in HEADS])


# ---- 4. edges of the rule ------------------------------------------------------------------------------------------------------------------
def test_edges_of_the_rule(decoders):
    hip = decoders("grasp9")
    rays = tc.ray_set(768)
    base = _trace(hip, rays, **tc.RULE)
    limit = tc.RULE["max_steps"] + tc.RULE["refine_steps"] + 1
    for name in HEADS:
        assert base[name]["evals"].max() <= limit and (base[name]["status"] == tc.HIT).sum() >= tc.MIN_HITS
    # a ray that starts inside a surface: from just behind a hit of the hand, along the same direction
    hit = np.nonzero(base["hand"]["status"] == tc.HIT)[0][:64]
    inside = rays[hit].copy()
    inside[:, 6] = base["hand"]["bracket"][hit, 1]          # t_hi: f <= 0 there
    got = _trace(hip, inside, obj=False, **tc.RULE)["hand"]
    assert (got["status"] == tc.INSIDE).all() and np.array_equal(got["t"], inside[:, 6]) and (got["evals"] == 1).all()
    # max_steps = 1: the first sample is the last march
    got = _trace(hip, rays, **dict(tc.RULE, max_steps=1))
    for name in HEADS:
        first_pos = base[name]["status"] != tc.INSIDE
        assert (got[name]["status"][first_pos] == tc.EXHAUSTED).all() and np.array_equal(got[name]["t"][first_pos], rays[first_pos, 6])
        assert (got[name]["evals"] == 1).all()
    # refine_steps = 0: t from the raw bracket, which is the first bracket of the refined run's march
    got = _trace(hip, rays, **dict(tc.RULE, refine_steps=0))
    want = _replay(hip, rays, refine_steps=0)
    _assert_same_bits("refine_steps=0", got, want)
    for name in HEADS:
        h = got[name]["status"] == tc.HIT
        assert np.array_equal(h, base[name]["status"] == tc.HIT)
        b = got[name]["bracket"][h]
        assert (b[:, 0] < b[:, 1]).all() and (b[:, 2] > 0).all() and (b[:, 3] <= 0).all()
        assert (b[:, 0] <= base[name]["bracket"][h, 0]).all() and (b[:, 1] >= base[name]["bracket"][h, 1]).all()
        assert (got[name]["t"][h] >= b[:, 0]).all() and (got[name]["t"][h] <= b[:, 1]).all()
    # t0 == t1: one sample
    point = rays.copy()
    point[:, 7] = point[:, 6]
    got = _trace(hip, point, **tc.RULE)
    for name in HEADS:
        assert (got[name]["evals"] == 1).all() and np.isin(got[name]["status"], (tc.MISS, tc.INSIDE)).all()
    # a non-finite origin / direction / end: MISS with no evaluation, the neighbours untouched
    bad = rays[:256].copy()
    bad[3, 0], bad[40, 4], bad[77, 7], bad[130, 6] = np.nan, np.inf, np.inf, -np.inf
    got = _trace(hip, bad, **tc.RULE)
    rows = np.array([3, 40, 77, 130])
    good = np.setdiff1d(np.arange(256), rows)
    _assert_same_bits("non-finite rays", got, base, rows=(good, good))
    for name in HEADS:
        assert (got[name]["status"][rows] == tc.MISS).all() and (got[name]["evals"][rows] == 0).all() and np.isposinf(got[name]["t"][rows]).all()


# ---- 5. ABI ------------------------------------------------------------------------------------------------------------------------------
def _abi_call(hip, rays_dev, M, params, outs, handle=True):
    with torch.cuda.device(hip.device):
        return hip._L.asdf_trace_rays(hip._h if handle else None, rays_dev.data_ptr() if rays_dev is not None else None, M,
                                      ctypes.byref(params) if params is not None else None,
                                      *[o.data_ptr() if o is not None else None for o in outs], hip._stream())


def test_abi_null_outputs_refusals_and_state(decoders):
    hip = decoders("both9")
    L = hip._L
    assert L.asdf_version() == _native.ABI_VERSION == 132
    rays = torch.from_numpy(tc.ray_set(257)).cuda()
    M = 257
    P = lambda **kw: _native.TraceParams(*[dict(tc.RULE, **kw)[k] for k in ("max_steps", "refine_steps", "step_scale", "min_step", "max_step")])
    full = _trace(hip, rays.cpu().numpy(), **tc.RULE)
    SENT_F, SENT_I = 12345.0, -77

    def buffers():
        mk = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda")
        return [mk((M,), torch.float32, SENT_F), mk((M,), torch.int32, SENT_I), mk((M, 4), torch.float32, SENT_F), mk((M,), torch.int32, SENT_I)] * 1

    names = [(h, k) for h in HEADS for k in KEYS]
    # each output pointer null in turn: the others are written as in the full call
    for drop in range(8):
        outs = buffers() + buffers()
        passed = [None if k == drop else o for k, o in enumerate(outs)]
        assert _abi_call(hip, rays, M, P(), passed) == 0
        torch.cuda.synchronize()
        for k, (h, key) in enumerate(names):
            got = outs[k].cpu().numpy()
            if k == drop:
                assert (got == (SENT_F if got.dtype == np.float32 else SENT_I)).all()
            else:
                assert np.array_equal(_bits(got), _bits(full[h][key])), (drop, h, key)
    # a head with neither t nor status is not run: its bracket / evals stay as they were
    outs = buffers() + buffers()
    passed = [None, None] + outs[2:]
    assert _abi_call(hip, rays, M, P(), passed) == 0
    torch.cuda.synchronize()
    assert (outs[2] == SENT_F).all() and (outs[3] == SENT_I).all()
    assert np.array_equal(_bits(outs[4].cpu().numpy()), _bits(full["obj"]["t"]))
    # M == 0, and no output at all: OK, nothing written
    outs = buffers() + buffers()
    assert _abi_call(hip, rays, 0, P(), outs) == 0 and _abi_call(hip, None, 0, P(), outs) == 0
    assert _abi_call(hip, rays, M, P(), [None] * 8) == 0
    torch.cuda.synchronize()
    assert all(((o == SENT_F) if o.dtype == torch.float32 else (o == SENT_I)).all() for o in outs)
    # EINVAL
    EINVAL = -1
    assert _abi_call(hip, rays, M, P(), outs, handle=False) == EINVAL
    assert _abi_call(hip, rays, -1, P(), outs) == EINVAL
    assert _abi_call(hip, None, M, P(), outs) == EINVAL
    assert _abi_call(hip, rays, M, None, outs) == EINVAL
    for kw in ({"max_steps": 0}, {"refine_steps": -1}, {"min_step": 0.0}, {"min_step": -1.0}, {"max_step": 0.0}, {"max_step": float("nan")}):
        assert _abi_call(hip, rays, M, P(**kw), outs) == EINVAL, kw
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    fresh = HipSdfDecoder(tc.module_for("both9"))
    try:
        assert _abi_call(fresh, rays, M, P(), outs) == EINVAL          # no sample bound
    finally:
        fresh.close()
    torch.cuda.synchronize()
    assert all(((o == SENT_F) if o.dtype == torch.float32 else (o == SENT_I)).all() for o in outs)


def test_math_mode_and_sweeps_are_left_alone(decoders):
    hip = decoders("both9")
    rays = tc.ray_set(257)
    for mode in ("f32", "f16x3"):
        before = hip.math
        hip.set_math(mode)
        try:
            N = 24
            vh, vo, _ = hip.decode_grid(N, [-1.0, -1.0, -1.0], 2.0 / (N - 1))
            vh, vo = vh.clone(), vo.clone()
            got = _trace(hip, rays, **tc.RULE)
            assert hip.math == mode
            wh, wo, _ = hip.decode_grid(N, [-1.0, -1.0, -1.0], 2.0 / (N - 1))
            assert torch.equal(vh, wh) and torch.equal(vo, wo)
            _assert_same_bits("trace under %s" % mode, got, _trace(hip, rays, **tc.RULE))
        finally:
            hip.set_math(before)


def test_uncovered_decoders_are_refused():
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    rays = torch.from_numpy(tc.ray_set(33)).cuda()
    P = _native.TraceParams(64, 6, 1.0, 1e-3, 0.05)

    def refused(hip):
        assert isinstance(hip.trace_refusal(), str)
        outs = [torch.zeros(33, device="cuda"), torch.zeros(33, dtype=torch.int32, device="cuda"), None, None] * 2
        code = _abi_call(hip, rays, 33, P, outs)
        assert code == _native.ENOTRACE == -9 and b"ray-tracing kernel" in hip._L.asdf_strerror(code)
        with pytest.raises(NotImplementedError):
            hip.trace_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7])

    for tag, pf in (("comb3", 3), ("nerf9", 9)):
        hip = HipSdfDecoder(syn.full_state_dict(tag), 256, pf, "nerf")
        try:
            hip.set_sample(torch.from_numpy(syn.latent_code(1)))
            refused(hip)
        finally:
            hip.close()
    # a pixel-aligned sample on the native path
    specs, _, sd, _, _, _, _ = syn.variant_config("pixelalign")
    hip = HipSdfDecoder(sd, 256, 3, "nerf", pixel_align=True)
    try:
        feat, mano, cam = syn.pixel_align_sample(0, 8, 8)
        hip.set_sample_pixel(torch.from_numpy(feat).cuda(), cam, mano["joints"][0, 0], specs["ImageSize"][0], specs["SdfScaleFactor"])
        refused(hip)
    finally:
        hip.close()


# ---- 6. render_view and the flow --------------------------------------------------------------------------------------------------------------
def test_render_view_native_against_the_module_path(decoders):
    from alignsdf_amd.render import render_view, trace_defaults
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    tag, H, W = tc.VIEW["tag"], tc.VIEW["H"], tc.VIEW["W"]
    specs = syn.specs_for(tag)
    cam, root = tc.view_camera()
    hip = decoders(tag)
    mod = TorchModuleDecoder(tc.module_for(tag), specs, "held to the native render")
    _bind(mod, tag)
    trace = trace_defaults(specs)
    assert trace == tc.RULE
    a = {k: v.cpu().numpy() for k, v in render_view(hip, cam, root, specs["SdfScaleFactor"], H, W, box=tc.BOX, **trace).items()}
    b = {k: v.cpu().numpy() for k, v in render_view(mod, cam, root, specs["SdfScaleFactor"], H, W, box=tc.BOX, **trace).items()}
    truth = tc.trace_truth(tag, tc.SAMPLE, "view")
    _, cr = tc.view_rays()
    inv = cr["inverse"]
    ok = {name: tc.decided(truth[name])[inv].reshape(H, W) for name in HEADS}
    both = ok["hand"] & ok["obj"]
    assert both.mean() >= tc.MIN_DECIDED_SHARE
    metres_per_t = np.abs(cr["z_per_t"]).max()
    for name in HEADS:
        assert a["depth_" + name].shape == (H, W) and a["status_" + name].dtype == np.int32
        assert np.array_equal(a["status_" + name][ok[name]], truth[name]["status"][inv].reshape(H, W)[ok[name]])
        assert np.array_equal(b["status_" + name][ok[name]], truth[name]["status"][inv].reshape(H, W)[ok[name]])
        hit = ok[name] & (a["status_" + name] == tc.HIT)
        assert hit.sum() >= tc.MIN_HITS and np.isinf(a["depth_" + name][a["status_" + name] != tc.HIT]).all()
        # the bound of the fp64 test (4 x the CPU's figure for this set and head), in metres
        bound = 4.0 * _recorded("view", name) * metres_per_t
        e = np.abs(a["depth_" + name][hit].astype(np.float64) - b["depth_" + name][hit]).max()
        print("SDFTRACE view %s: hits %d depth native-module %.3e m bound %.3e m" % (name, hit.sum(), e, bound))
        assert e <= bound
    assert a["part"].dtype == np.uint8 and np.array_equal(a["part"][both], b["part"][both])
    assert set(np.unique(a["part"])) == {0, 1, 2}
    for view in (a, b):
        length = np.linalg.norm(view["normal"].astype(np.float64), axis=2)
        assert np.abs(length[view["part"] != 0] - 1.0).max() <= 1e-5 and (view["normal"][view["part"] == 0] == 0).all()
    same = both & (a["part"] != 0)
    cos = (a["normal"][same].astype(np.float64) * b["normal"][same]).sum(1)
    print("SDFTRACE view normals: worst cos %.6f median %.8f" % (cos.min(), np.median(cos)))
    assert np.median(cos) >= 1.0 - 1e-6


def test_reconstruct_writes_render_files_and_leaves_the_meshes_alone(tmp_path):
    from alignsdf_amd.reconstruct import reconstruct, synthetic_code_source
    from alignsdf_amd.render import VIEW_MAPS, synthetic_camera_source
    tag = "grasp9"
    specs = syn.specs_for(tag)
    split = str(tmp_path / "split.json")
    with open(split, "w") as fh:
        json.dump({"filenames": ["s/a.png", "s/b.png"]}, fh)
    dirs = {}
    for label, extra in (("plain", {}), ("render", {"render": (32, 32), "camera_source": synthetic_camera_source(32, 32)})):
        dirs[label] = str(tmp_path / label)
        recs = reconstruct(tc.module_for(tag), specs, split, dirs[label], 0, 2, cube_dim=32, code_source=synthetic_code_source(tag), **extra)
        assert len(recs) == 2
        if extra:
            for r in recs:
                assert r["render_evals_mean"] > 0 and r["render_exhausted_hand"] >= 0 and r["render_exhausted_obj"] >= 0
        else:
            assert all("render_evals_mean" not in r for r in recs)
    for name in ("a", "b"):
        for part in HEADS:
            f = "meshes/%s_%s.ply" % (name, part)
            assert filecmp.cmp(os.path.join(dirs["plain"], f), os.path.join(dirs["render"], f), shallow=False), f
        assert not os.path.exists(os.path.join(dirs["plain"], "meshes/%s_render.npz" % name))
        with np.load(os.path.join(dirs["render"], "meshes/%s_render.npz" % name)) as z:
            assert set(VIEW_MAPS) <= set(z.files) and int(z["H"]) == 32 and int(z["W"]) == 32 and int(z["max_steps"]) == 64
            assert z["depth_hand"].shape == (32, 32) and z["normal"].shape == (32, 32, 3) and z["part"].dtype == np.uint8
            assert (z["part"] != 0).sum() > 0


@pytest.mark.parametrize("tag", ["nerf9", "comb3"])
def test_reconstruct_renders_a_refused_decoder_on_the_module_path(tmp_path, tag):
    """nerf9 and comb3 sweep on the kernels and are refused by the tracing kernel: the flow keeps their native sweeps (the meshes are
    the files of a run without render) and traces the view on the module - the maps are render_view's over a TorchModuleDecoder bound
    to the same sample, in every bit."""
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.networks.model import build_decoder
    from alignsdf_amd.reconstruct import reconstruct, synthetic_code_source
    from alignsdf_amd.render import VIEW_MAPS, render_view, synthetic_camera_source, trace_defaults
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    from alignsdf_amd.utils.utils import bind_sample, decoder_for
    specs = syn.specs_for(tag)
    module = build_decoder(specs, syn.full_state_dict(tag)).eval()
    source, cameras, N, H, W = synthetic_code_source(tag), synthetic_camera_source(16, 16), 32, 16, 16
    hip = decoder_for(module, specs, source("a", 0)[1])
    assert isinstance(hip, HipSdfDecoder) and isinstance(hip.trace_refusal(), str)
    split = str(tmp_path / "split.json")
    with open(split, "w") as fh:
        json.dump({"filenames": ["s/a.png"]}, fh)
    dirs = {}
    for label, extra in (("plain", {}), ("render", {"render": (H, W), "camera_source": cameras})):
        dirs[label] = str(tmp_path / label)
        recs = reconstruct(module, specs, split, dirs[label], 0, 1, cube_dim=N, code_source=source, **extra)
    assert recs[0]["render_evals_mean"] > 0
    for part in HEADS:
        f = "meshes/a_%s.ply" % part
        if os.path.exists(os.path.join(dirs["plain"], f)):
            assert filecmp.cmp(os.path.join(dirs["plain"], f), os.path.join(dirs["render"], f), shallow=False), f
    mod = TorchModuleDecoder(module, specs, "the flow's view, again")
    bind_sample(mod, specs, *source("a", 0))
    lo = [float(v) for v in recs[0]["origin"]]
    hi = [v + (N - 1) * recs[0]["voxel_size"] for v in lo]
    want = render_view(mod, *cameras("a", 0), specs["SdfScaleFactor"], H, W, box=(lo, hi), **trace_defaults(specs))
    with np.load(os.path.join(dirs["render"], "meshes/a_render.npz")) as z:
        for k in VIEW_MAPS:
            assert np.array_equal(_bits(z[k]), _bits(want[k].cpu().numpy())), k
        assert np.isin(z["status_hand"], (tc.MISS, tc.HIT, tc.INSIDE, tc.EXHAUSTED)).all()
        print("SDFTRACE refused %s: pixels hit hand %d obj %d, evals mean %.1f" % (
            tag, (z["status_hand"] == tc.HIT).sum(), (z["status_obj"] == tc.HIT).sum(), float(z["evals_mean"])))
