"""HipSdfDecoder.project_points / asdf_project_points (csrc/k1p_kernels.hip) on the GPU.

  1. bit identity: the kernel equals project.project_lockstep over the same decoder's decode_points_grad in every bit of every output,
     at every edge of the 8-per-wave / 32-per-workgroup tiling, on both heads and under three rules; its sdf / grad are decode_points'
     (f32) and decode_points_grad's at the returned point
  2. fp64 truth on the three sets of tests/sdf_project_cases.truth_sets()
  3. no side effects, 4. the C ABI and the refusals, 5. the module path, 6. polish in the mesh flows"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from alignsdf_amd import _native
from alignsdf_amd import project as pj
from alignsdf_amd import synthetic as syn
from tests import sdf_grad_cases as gc
from tests import sdf_project_cases as pc

pytestmark = pytest.mark.gpu
HEADS = ("hand", "obj")
KEYS = pj.OUTPUTS
EINVAL = -1


def _t(d):
    return None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def _bind(dec, tag, sample=pc.SAMPLE):
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
            made[tag] = HipSdfDecoder(gc.module_for(tag))
            _bind(made[tag], tag)
        return made[tag]
    yield get
    for d in made.values():
        d.close()


def _dev(pts):
    return torch.from_numpy(np.array(pts, np.float32)).cuda()          # (a copy: the shared sets are read-only)


def _same_bits(a, b):
    """torch.equal on the bit patterns (a BAD row returns its non-finite input: NaN != NaN)."""
    a, b = (v.view(torch.int32) if v.dtype == torch.float32 else v for v in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _assert_same(label, got, want):
    for k in KEYS:
        if not _same_bits(got[k], want[k]):
            g, w = got[k].reshape(len(got[k]), -1), want[k].reshape(len(want[k]), -1)
            bad = torch.nonzero((g.view(torch.int32) != w.view(torch.int32)).any(1)).reshape(-1)
            raise AssertionError((label, k, len(bad), bad[:5].tolist(), g[bad[:3]].tolist(), w[bad[:3]].tolist()))


# ---- 1. bit identity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", pc.LIST_LENGTHS)
def test_kernel_equals_the_lockstep_rule_over_decode_points_grad_bit_for_bit(decoders, M):
    hip = decoders("both9")
    for head in HEADS:
        x = _dev(pc.mixed_set(M, head))
        for name, rule in pc.rules("both9", head).items():
            got = hip.project_points(x, head, **rule)
            want = pj.project_lockstep(pj.grad_of_head(hip, head), x, **rule)
            st = got["status"]
            print("SDFPROJECT identity M=%d %s rule %s: CONVERGED %d SPENT %d STALLED %d BAD %d evals mean %.2f max %d" % (
                M, head, name, *[int((st == c).sum()) for c in range(4)], float(got["evals"].float().mean()), int(got["evals"].max())))
            assert int(got["evals"].max()) <= rule["max_iters"] + 1
            assert int((st == pj.BAD).sum()) == (2 if M >= 9 else 0)
            _assert_same("M=%d %s %s" % (M, head, name), got, want)
            # at the returned point: decode_points' sdf under f32, decode_points_grad's gradient
            ok = st != pj.BAD
            before = hip.math
            hip.set_math("f32")
            try:
                sdf = hip.decode_points(got["xyz_out"][ok])[0 if head == "hand" else 1]
            finally:
                hip.set_math(before)
            res = hip.decode_points_grad(got["xyz_out"][ok], hand=head == "hand", obj=head == "obj")
            s2, g2 = (res[0], res[1]) if head == "hand" else (res[2], res[3])
            assert _same_bits(got["sdf"][ok], sdf) and _same_bits(got["sdf"][ok], s2) and _same_bits(got["grad"][ok], g2), (M, head, name)
            assert _same_bits(got["sdf_in"][ok], hip.decode_points_grad(x[ok], hand=head == "hand", obj=head == "obj")[0 if head == "hand" else 2])
            # BAD rows: the input and zeros
            assert _same_bits(got["xyz_out"][~ok], x[~ok]) and not got["sdf"][~ok].any() and not got["grad"][~ok].any()
            assert not got["sdf_in"][~ok].any() and not got["evals"][~ok].any()


def test_a_points_result_does_not_depend_on_its_slot_or_its_neighbours(decoders):
    hip = decoders("both9")
    pts = pc.mixed_set(1000, "hand")
    rule = pc.rules()["3/1"]
    base = hip.project_points(_dev(pts), "hand", **rule)
    perm = np.random.default_rng(5).permutation(len(pts))
    got = hip.project_points(_dev(pts[perm]), "hand", **rule)
    p = torch.from_numpy(perm).cuda()
    _assert_same("permuted", got, {k: v[p] for k, v in base.items()})
    # in place: the input buffer as xyz_out
    x = _dev(pts)
    out = {k: torch.empty_like(v) for k, v in base.items()}
    P = _native.ProjectParams(rule["max_iters"], rule["tol"], rule["max_move"], rule["min_grad2"])
    assert _abi_call(hip, x, len(pts), 0, P, [x] + [out[k] for k in KEYS[1:]]) == 0
    torch.cuda.synchronize()
    _assert_same("in place", dict(out, xyz_out=x), base)


# ---- 2. truth ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", pc.TRUTH_LABELS)
def test_converged_points_sit_on_the_fp64_zero_level(decoders, label):
    """Measured on an MI355X (figures printed as SDFPROJECT truth): see profiles/sdf_project.txt."""
    _, tag, head, pts = next(s for s in pc.truth_sets() if s[0] == label)
    hip = decoders(tag)
    rule = pc.rules(tag, head)["8/1"]
    got = {k: v.cpu().numpy() for k, v in hip.project_points(_dev(pts), head, **rule).items()}
    conv = got["status"] == pj.CONVERGED
    out64 = pc.sdf64(tag, pc.SAMPLE, got["xyz_out"])[head]
    in64 = pc.sdf64(tag, pc.SAMPLE, pts)[head]
    # the yardstick of test_gpu_sdf_grad.py: fp32 autograd through the oracle on the CPU, at the returned points, plus its floor
    orc32 = gc.oracle_autograd(tag, pc.SAMPLE, got["xyz_out"])[head]["sdf"]
    e = float(np.abs(orc32.astype(np.float64) - out64).max()) + 5e-7
    worst = float(np.abs(out64[conv]).max())
    print("SDFPROJECT truth %s: CONVERGED %d of %d (share %.4f), evals mean %.2f max %d, fp64 |sdf| before median %.3g max %.3g, after "
          "median %.3g max %.3g (CONVERGED max %.3g, bound %.3g = tol + e, e %.3g)" % (
              label, conv.sum(), len(pts), conv.mean(), got["evals"].mean(), got["evals"].max(), np.median(np.abs(in64)),
              np.abs(in64).max(), np.median(np.abs(out64)), np.abs(out64).max(), worst, pc.TOL + e, e))
    assert conv.mean() >= 0.995
    assert worst <= pc.TOL + e
    assert np.median(np.abs(in64)) >= 100.0 * np.median(np.abs(out64))
    assert (np.abs(got["sdf"][conv]) <= np.float32(pc.TOL)).all() and got["evals"].max() <= rule["max_iters"] + 1


# ---- 3. no side effects ----------------------------------------------------------------------------------------------------------------------
def test_math_mode_and_sweeps_are_left_alone(decoders):
    hip = decoders("both9")
    x = _dev(pc.list_set(257))
    rule = pc.rules()["8/1"]
    shape_before = hip._L.asdf_get_mfma_shape()
    for mode in ("f32", "f16x3"):
        before = hip.math
        hip.set_math(mode)
        try:
            N = 24
            vh, vo, _ = hip.decode_grid(N, [-1.0, -1.0, -1.0], 2.0 / (N - 1))
            vh, vo = vh.clone(), vo.clone()
            got = hip.project_points(x, "hand", **rule)
            assert hip.math == mode and hip._L.asdf_get_mfma_shape() == shape_before
            wh, wo, _ = hip.decode_grid(N, [-1.0, -1.0, -1.0], 2.0 / (N - 1))
            assert torch.equal(vh, wh) and torch.equal(vo, wo)
            _assert_same("project under %s" % mode, got, hip.project_points(x, "hand", **rule))
        finally:
            hip.set_math(before)


# ---- 4. ABI ------------------------------------------------------------------------------------------------------------------------------
def _abi_call(hip, xyz, M, head, params, outs, handle=True):
    with torch.cuda.device(hip.device):
        return hip._L.asdf_project_points(hip._h if handle else None, xyz.data_ptr() if xyz is not None else None, M, head,
                                          ctypes.byref(params) if params is not None else None,
                                          *[o.data_ptr() if o is not None else None for o in outs], hip._stream())


def test_abi_invalid_arguments_empty_list_and_null_outputs(decoders):
    hip = decoders("both9")
    M = 257
    x = _dev(pc.mixed_set(M, "obj"))
    rule = pc.rules("both9", "obj")["8/1"]
    P = lambda **kw: _native.ProjectParams(*[dict(rule, **kw)[k] for k in ("max_iters", "tol", "max_move", "min_grad2")])
    full = hip.project_points(x, 1, **rule)
    SENT_F, SENT_I = 12345.0, -77

    def buffers():
        return [torch.full(full[k].shape, SENT_I if full[k].dtype == torch.int32 else SENT_F, dtype=full[k].dtype, device="cuda") for k in KEYS]

    untouched = lambda outs: all(bool((o == (SENT_I if o.dtype == torch.int32 else SENT_F)).all()) for o in outs)
    # each output pointer null in turn: the others are written as in the full call
    for drop in range(len(KEYS)):
        outs = buffers()
        assert _abi_call(hip, x, M, 1, P(), [None if k == drop else o for k, o in enumerate(outs)]) == 0
        torch.cuda.synchronize()
        for k, key in enumerate(KEYS):
            assert untouched([outs[k]]) if k == drop else _same_bits(outs[k], full[key]), (drop, key)
    # M == 0, and no output at all: OK, nothing written
    outs = buffers()
    assert _abi_call(hip, x, 0, 1, P(), outs) == 0 and _abi_call(hip, None, 0, 1, P(), outs) == 0
    assert _abi_call(hip, x, M, 1, P(), [None] * 6) == 0
    empty = hip.project_points(x[:0], "obj", **rule)
    assert empty["xyz_out"].shape == (0, 3) and empty["status"].shape == (0,)
    # EINVAL
    assert _abi_call(hip, x, M, 1, P(), outs, handle=False) == EINVAL
    assert _abi_call(hip, x, -1, 1, P(), outs) == EINVAL
    assert _abi_call(hip, None, M, 1, P(), outs) == EINVAL
    assert _abi_call(hip, x, M, 1, None, outs) == EINVAL
    assert _abi_call(hip, x, M, 2, P(), outs) == EINVAL and _abi_call(hip, x, M, -1, P(), outs) == EINVAL
    for kw in ({"max_iters": -1}, {"tol": -1e-6}, {"tol": float("nan")}, {"max_move": 0.0}, {"max_move": -1.0}, {"max_move": float("nan")},
               {"min_grad2": 0.0}, {"min_grad2": -1.0}, {"min_grad2": float("nan")}):
        assert _abi_call(hip, x, M, 1, P(**kw), outs) == EINVAL, kw
        with pytest.raises(ValueError):
            hip.project_points(x, 1, **dict(rule, **kw))
    with pytest.raises(ValueError):
        hip.project_points(x, "foot", **rule)
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    fresh = HipSdfDecoder(gc.module_for("both9"))
    try:
        assert _abi_call(fresh, x, M, 1, P(), outs) == EINVAL          # no sample bound
    finally:
        fresh.close()
    torch.cuda.synchronize()
    assert untouched(outs)
    # the accepted edges of the rule: max_iters = 0 is one evaluation, tol = 0 is allowed
    r0 = hip.project_points(x, 1, **dict(rule, max_iters=0))
    ok = r0["status"] != pj.BAD
    assert (r0["evals"][ok] == 1).all() and _same_bits(r0["xyz_out"], x) and _same_bits(r0["sdf"], r0["sdf_in"])
    assert set(r0["status"][ok].unique().tolist()) <= {pj.CONVERGED, pj.SPENT}
    assert torch.equal(r0["status"][ok] == pj.CONVERGED, r0["sdf"][ok].abs() <= 1e-6)
    rz = hip.project_points(x, 1, **dict(rule, tol=0.0))
    assert int(rz["evals"].max()) <= 9 and _same_bits(rz["sdf_in"], full["sdf_in"])


def test_uncovered_decoders_are_refused():
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    x = _dev(pc.list_set(33))
    P = _native.ProjectParams(8, 1e-6, 0.05, 1e-12)

    def refused(hip):
        assert isinstance(hip.project_refusal(), str)
        outs = [torch.zeros(33, 3, device="cuda"), torch.zeros(33, device="cuda"), None, None, torch.zeros(33, dtype=torch.int32, device="cuda"), None]
        code = _abi_call(hip, x, 33, 0, P, outs)
        assert code == _native.ENOPROJECT == -10 and b"projection kernel" in hip._L.asdf_strerror(code)
        with pytest.raises(NotImplementedError):
            hip.project_points(x, "hand")
        with pytest.raises(NotImplementedError):
            pj.require_polish(hip)

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


# ---- 5. the module path --------------------------------------------------------------------------------------------------------------------
def test_module_path_runs_the_rule_over_its_own_gradients():
    from alignsdf_amd.networks.model import build_decoder
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    tag, M = "nerf9", 257
    specs = syn.specs_for(tag)
    module = build_decoder(specs, {k: torch.from_numpy(np.asarray(v)) for k, v in syn.full_state_dict(tag).items()}).eval()
    mod = TorchModuleDecoder(module, specs, "the projection kernel refuses NeRF-encoded features")
    _bind(mod, tag)
    assert pj.project_refusal_of(mod) is None
    x = _dev(pc.mixed_set(M, "hand"))
    rule = pc.rules()["8/1"]
    for head in HEADS:
        got = mod.project_points(x, head, **rule)
        want = pj.project_lockstep(pj.grad_of_head(mod, head), x, **rule)
        _assert_same("nerf9 module %s" % head, got, want)
        st = got["status"]
        print("SDFPROJECT module nerf9 %s: CONVERGED %d SPENT %d STALLED %d BAD %d evals max %d" % (
            head, *[int((st == c).sum()) for c in range(4)], int(got["evals"].max())))
        assert int((st == pj.BAD).sum()) == 2 and int(got["evals"].max()) <= 9
        conv = st == pj.CONVERGED
        assert (got["sdf"][conv].abs() <= 1e-6).all()
        ok = st != pj.BAD
        res = mod.decode_points_grad(got["xyz_out"][ok], hand=head == "hand", obj=head == "obj")
        assert _same_bits(got["sdf"][ok], res[0] if head == "hand" else res[2])


# ---- 6. the flows: polished vertices in the written files, N = 32 on grasp9 -------------------------------------------------------------
FLOW_TAG, FLOW_N = "grasp9", 32


def _flow_decoder():
    return gc.module_for(FLOW_TAG), syn.specs_for(FLOW_TAG)


def _check_polished_file(label, path_plain, path_polished, sample, voxel, counts):
    """The properties of one polished file against its unpolished twin; returns its vertices."""
    from alignsdf_amd.ply import read_ply
    part = "hand" if path_polished.endswith("_hand.ply") else "obj"
    pv, pf = read_ply(path_plain)
    v, f = read_ply(path_polished)
    assert np.array_equal(f, pf) and v.shape == pv.shape and len(v) > 0, label
    before = np.abs(pc.sdf64(FLOW_TAG, sample, pv)[part])
    after = np.abs(pc.sdf64(FLOW_TAG, sample, v)[part])
    moved = np.abs(v.astype(np.float64) - pv).max()
    print("SDFPROJECT flow %s %s V=%d: fp64 |sdf| median %.3g -> %.3g, max %.3g -> %.3g, largest move %.3g of a voxel, counts %s" % (
        label, part, len(v), np.median(before), np.median(after), before.max(), after.max(), moved / voxel, counts))
    assert np.median(before) >= 100.0 * np.median(after), label
    # one fine voxel per axis (both files hold origin + v * voxel_size rounded to fp32)
    assert moved <= voxel + 4 * np.finfo(np.float32).eps * float(np.abs(pv).max() + 1.0), (label, moved, voxel)
    assert set(counts) == {"converged", "spent", "stalled", "bad", "kept"} and counts["bad"] == 0
    assert counts["converged"] + counts["spent"] + counts["stalled"] == len(v) and 0 <= counts["kept"] <= len(v)
    return v


def _no_projection_launch(*a, **k):
    raise AssertionError("a projection launch in a run without polish")


def test_create_mesh_writes_polished_vertices(tmp_path, monkeypatch):
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.utils.mesh import create_mesh_combined_decoder
    dec, specs = _flow_decoder()
    latent, mano, obj = syn.sample_inputs(FLOW_TAG, 1)
    args = (True, True, False, dec, torch.from_numpy(latent), _t(mano), _t(obj), None, specs)
    plain, polished = str(tmp_path / "plain"), str(tmp_path / "polished")
    with monkeypatch.context() as m:          # without the option: no projection launch
        m.setattr(HipSdfDecoder, "project_points", _no_projection_launch)
        s0 = create_mesh_combined_decoder(*args, plain, N=FLOW_N, return_stats=True)
    s1 = create_mesh_combined_decoder(*args, polished, N=FLOW_N, return_stats=True, polish=True)
    assert "polish_hand" not in s0 and s1["hand"] == s0["hand"] and s1["obj"] == s0["obj"] and s0["hand"][0] > 0 and s0["obj"][0] > 0
    from alignsdf_amd.utils.mesh import decode_two_pass
    voxel = float(decode_two_pass(True, True, dec, torch.from_numpy(latent), _t(mano), _t(obj), specs, FLOW_N)["voxel_size"])
    for part in HEADS:
        _check_polished_file("create_mesh N=32", "%s_%s.ply" % (plain, part), "%s_%s.ply" % (polished, part), 1, voxel, s1["polish_" + part])


def test_reconstruct_writes_polished_vertices_and_their_normals(tmp_path, monkeypatch):
    """reconstruct() without polish (no projection launch: the method is replaced by one that raises), with polish, and with polish
    and normals (the normals are those of the polished positions)."""
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.ply import read_ply
    from alignsdf_amd.reconstruct import reconstruct, synthetic_code_source
    from alignsdf_amd.utils.utils import bind_sample, decoder_for
    dec, specs = _flow_decoder()
    names = ["00000021", "00000022"]
    split = str(tmp_path / "split.json")
    with open(split, "w") as fh:
        json.dump({"filenames": ["skip/0.jpg"] + ["data/obman/test/rgb/%s.jpg" % n for n in names]}, fh)
    kw = dict(cube_dim=FLOW_N, code_source=synthetic_code_source(FLOW_TAG))
    plain_dir, polish_dir, both_dir = (str(tmp_path / d) for d in ("plain", "polished", "both"))
    with monkeypatch.context() as m:
        m.setattr(HipSdfDecoder, "project_points", _no_projection_launch)
        plain = reconstruct(dec, specs, split, plain_dir, 1, 3, **kw)
    assert not any(k.startswith("polish_") for r in plain for k in r)
    recs = reconstruct(dec, specs, split, polish_dir, 1, 3, polish=True, **kw)
    both = reconstruct(dec, specs, split, both_dir, 1, 3, polish=True, normals=True, **kw)
    file_of = lambda d, name, part: os.path.join(d, "meshes", "%s_%s.ply" % (name, part))
    for rec, before, withn in zip(recs, plain, both):
        assert rec["V_hand"] == before["V_hand"] > 0 and rec["V_obj"] == before["V_obj"] > 0
        for part in HEADS:
            v = _check_polished_file("reconstruct N=32 %s" % rec["name"], file_of(plain_dir, rec["name"], part),
                                     file_of(polish_dir, rec["name"], part), rec["index"], rec["voxel_size"], rec["polish_" + part])
            # with normals as well: the same vertices, and the normals of THESE positions
            assert withn["polish_" + part] == rec["polish_" + part]
            nv, nf, n = read_ply(file_of(both_dir, rec["name"], part), with_normals=True)
            assert n is not None and np.array_equal(nv, v) and np.array_equal(nf, read_ply(file_of(plain_dir, rec["name"], part))[1])
            latent, mano, obj = syn.sample_inputs(FLOW_TAG, rec["index"])
            hip = decoder_for(dec, specs, _t(mano))
            bind_sample(hip, specs, torch.from_numpy(latent), _t(mano), _t(obj))
            grad_at = lambda p: (lambda r: (r[1] if part == "hand" else r[3]).cpu().numpy().astype(np.float64))(hip.decode_points_grad(_dev(p)))
            unit = lambda g: g / np.sqrt((g * g).sum(1, keepdims=True))
            truth = gc.grad_truth(FLOW_TAG, rec["index"], v)[part]
            clear = gc.clear_mask(truth) & n.any(axis=1)
            worst = float(np.abs(n - unit(grad_at(v)))[clear].max())
            pv = read_ply(file_of(plain_dir, rec["name"], part))[0]
            apart = float(np.abs(unit(grad_at(v)) - unit(grad_at(pv)))[clear].max())
            print("SDFPROJECT flow normals %s %s: file normal vs recomputed at the polished vertices %.2e (at the unpolished ones they "
                  "differ by up to %.2e), clear %.1f%%" % (rec["name"], part, worst, apart, 100.0 * clear.mean()))
            assert clear.any() and worst <= 1e-5


def test_polish_on_a_nerf9_decoder_raises_before_any_file(tmp_path):
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
        rc.reconstruct(dec, specs, split, out, 0, 2, cube_dim=FLOW_N, code_source=rc.synthetic_code_source("nerf9"), polish=True)
    assert not os.listdir(os.path.join(out, "meshes"))
    # the command line: --polish on the same experiment
    model = tmp_path / "experiment"
    os.makedirs(model / "ModelParameters")
    with open(model / "specs.json", "w") as fh:
        json.dump(specs, fh)
    torch.save({"model_state_dict": {"module.decoder." + k: v for k, v in sd.items()}}, str(model / "ModelParameters" / "latest.pth"))
    with pytest.raises(NotImplementedError):
        rc.main(["--model", str(model), "--split", split, "--synthetic", "--polish", "--cube_dim", str(FLOW_N)])
    meshes = model / "Eval_obman" / "meshes"
    assert not meshes.exists() or not os.listdir(meshes)
    # the step-by-step path refuses before it sweeps as well
    from alignsdf_amd.utils.mesh import create_mesh_combined_decoder
    latent, mano, obj = syn.sample_inputs("nerf9", 1)
    with pytest.raises(NotImplementedError):
        create_mesh_combined_decoder(True, True, False, dec, torch.from_numpy(latent), _t(mano), _t(obj), None, specs,
                                     str(tmp_path / "step"), N=FLOW_N, polish=True)
    assert not os.path.exists(str(tmp_path / "step_hand.ply"))


def test_command_line_polish_flag(tmp_path):
    """--polish on reconstruct's command line reaches the pipeline: the records carry the counts, the files the polished vertices."""
    from alignsdf_amd import reconstruct as rc
    from alignsdf_amd.ply import read_ply
    tag = "nerf3"                              # (--synthetic draws the codes of nerf3 / both9 by PointFeatSize: the weights have to match)
    specs = syn.specs_for(tag)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in syn.full_state_dict(tag).items()}
    split = str(tmp_path / "split.json")
    with open(split, "w") as fh:
        json.dump({"filenames": ["data/obman/test/rgb/00000012.jpg"]}, fh)
    runs = {}
    for name, flags in (("plain", []), ("polished", ["--polish"])):
        model = tmp_path / name
        os.makedirs(model / "ModelParameters")
        with open(model / "specs.json", "w") as fh:
            json.dump(specs, fh)
        torch.save({"model_state_dict": {"module.decoder." + k: v for k, v in sd.items()}}, str(model / "ModelParameters" / "latest.pth"))
        runs[name] = rc.main(["--model", str(model), "--split", split, "--synthetic", "--cube_dim", str(FLOW_N)] + flags)
    assert runs["plain"][0]["V_hand"] > 0 and runs["plain"][0]["V_obj"] > 0
    assert "polish_hand" not in runs["plain"][0] and runs["polished"][0]["polish_hand"]["converged"] > 0
    for part in HEADS:
        a = read_ply(str(tmp_path / "plain" / "Eval_obman" / "meshes" / ("00000012_%s.ply" % part)))
        b = read_ply(str(tmp_path / "polished" / "Eval_obman" / "meshes" / ("00000012_%s.ply" % part)))
        assert np.array_equal(a[1], b[1]) and a[0].shape == b[0].shape and not np.array_equal(a[0], b[0])
