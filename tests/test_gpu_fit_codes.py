"""Many samples' codes fitted in one stream of launches (asdf_fit_codes: csrc/decoder.hip, csrc/k1vb_kernels.hip;
HipSdfDecoder.fit_codes; alignsdf_amd.fit.fit_codes; autodecode --batch).

The oracle is the one-sample call: HipSdfDecoder.fit_code on a SECOND decoder object bound with set_sample.  Every sample of a batch
must come out with exactly its bits - the code and the fp64 history - whatever its position and company.  That call runs the same
device loop over a batch of one (on the decoder's own constants images and scratch), so one test anchors the batch outside the fit's
kernels: fit.fit_code_lockstep, the rule one step at a time with the host in the loop."""
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
TAG = vc.FIT_TAG                  # grasp9: the pose-aligned grasp decoder
SAMPLES = (3, 4, 5, 7)            # different synthetic samples: different codes and embeddings
LENGTHS = (1, 127, 129, 300)      # one point; a tile less one; a tile and one; three tiles, the last partial
RULE = dict(steps=5, lr=5e-3, decay=0.5, every=2, prior=1e-3, clamp=fc.CLAMP)
L = 256


def _t(d):
    return None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def _np(v):
    return None if v is None else v.detach().cpu().numpy()


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(_np(a) if torch.is_tensor(a) else a).view(np.int32)


def _sample(sample):
    from alignsdf_amd.utils.utils import sample_embedding
    latent, mano, obj = syn.sample_inputs(TAG, sample)
    return torch.from_numpy(latent).reshape(-1), sample_embedding(syn.specs_for(TAG), _t(mano), _t(obj))


@pytest.fixture(scope="module")
def pair():
    """(the decoder under test, the oracle's decoder): two objects of the same module."""
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    decs = HipSdfDecoder(gc.module_for(TAG)), HipSdfDecoder(gc.module_for(TAG))
    yield decs
    for d in decs:
        d.close()


def _item(sample, M, variant, z0=None, seed=5):
    """One sample of a batch: its points, targets, counts, start code, embedding and prior centre."""
    latent, embed = _sample(sample)
    th, to, nh, no = fc.targets(M, variant, seed)
    return {"x": _cuda(vc.list_points(M)), "th": _cuda(th), "to": _cuda(to), "nh": nh, "no": no, "latent": latent, "embed": embed, "z0": z0}


_alone = {}


def _oracle(oracle, item, key, rule):
    """fit_code of this sample alone (computed once per key, shared)."""
    k = (key, tuple(sorted(rule.items())))
    if k not in _alone:
        oracle.set_sample(item["latent"].reshape(1, -1), item["embed"])
        z, h = oracle.fit_code(item["x"], item["th"], item["to"], item["nh"], item["no"], item["latent"], z0=item["z0"], **rule)
        _alone[k] = (_np(z).copy(), _np(h).copy())
    return _alone[k]


def _batch(hip, items, rule):
    z0 = [it["z0"] for it in items]
    return hip.fit_codes([it["x"] for it in items], [it["th"] for it in items], [it["to"] for it in items], [it["nh"] for it in items],
                         [it["no"] for it in items], torch.stack([it["latent"] for it in items]), [it["embed"] for it in items],
                         z0=None if all(c is None for c in z0) else z0, **rule)


def _same_bits(z, h, want, what):
    wz, wh = want
    assert np.array_equal(_bits(z), _bits(wz)), (what, "code", float(np.abs(_np(z) - wz).max()))
    assert np.array_equal(_np(h).view(np.int64), wh.view(np.int64)), (what, "history", _np(h), wh)


def _four(variant):
    """The B = 4 batch of the first two tests: (items, the target variant of each)."""
    z0s = (torch.zeros(L), None, torch.from_numpy(syn.latent_code(9)).reshape(-1), None)
    kinds = [variant] * 4 if variant != "mixed" else ["obj", "both", "disjoint", "hand"]
    return [_item(s, M, kind, z0) for s, M, kind, z0 in zip(SAMPLES, LENGTHS, kinds, z0s)], kinds


# ---- 1. each sample equals fit_code alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", fc.VARIANTS + ("mixed",))
def test_each_sample_of_a_batch_equals_fit_code_alone(variant, pair):
    """B = 4, M = 1, 127, 129, 300; every target variant, and "mixed": a different variant per sample, so that the heads differ inside
    one launch.  z0 is given for samples 0 and 2 and defaulted for 1 and 3.  ("disjoint" at M = 1 leaves the object's set empty.)"""
    hip, oracle = pair
    items, kinds = _four(variant)
    z, h = _batch(hip, items, RULE)
    assert tuple(z.shape) == (4, L) and tuple(h.shape) == (4, RULE["steps"]) and h.dtype == torch.float64
    for s, (it, kind) in enumerate(zip(items, kinds)):
        want = _oracle(oracle, it, (SAMPLES[s], LENGTHS[s], kind, s), RULE)
        print("FITCODES %-8s sample %d M=%-3d %-8s: data term %.6e -> %.6e" % (variant, s, LENGTHS[s], kind, float(h[s, 0]), float(h[s, -1])))
        _same_bits(z[s], h[s], want, (variant, s))
        assert float(h[s, 0]) > 0.0
    # (a sample whose points all lie beyond the clamp, with its prior centred on its start, rightly stays: not every code moves)
    moved = [not np.array_equal(_bits(z[s]), _bits(it["latent"])) for s, it in enumerate(items)]
    assert sum(moved) >= 2, moved


def test_each_sample_of_a_batch_equals_the_lockstep_loop(pair):
    """The anchor that is not the batch of one: fit.fit_code_lockstep on the oracle's decoder takes the rule one step at a time through
    decode_points, the weight form of the reverse-mode kernel and adam_step_host on the host - no kernel of the fit.  The "mixed"
    batch above: every code to the bit, every history to the rounding of an fp64 sum (1e-12 relative, as
    tests/test_gpu_fit_code.py::test_k_steps_equal_the_lockstep_loop holds the same comparison)."""
    from alignsdf_amd.fit import fit_code_lockstep
    hip, oracle = pair
    items, kinds = _four("mixed")
    z, h = _batch(hip, items, RULE)
    for s, (it, kind) in enumerate(zip(items, kinds)):
        zl, hl = fit_code_lockstep(oracle, it["latent"], it["embed"], it["x"], it["th"], it["to"], it["nh"], it["no"], z0=it["z0"], **RULE)
        rel = float(((h[s] - hl).abs() / hl.abs()).max())
        print("FITCODES lockstep sample %d M=%-3d %-8s: history vs lockstep rel %.1e" % (s, LENGTHS[s], kind, rel))
        assert np.array_equal(_bits(z[s]), _bits(zl)), (s, kind, float((z[s] - zl).abs().max()))
        assert ((h[s] - hl).abs() <= 1e-12 * hl.abs()).all(), (s, kind, rel)


# ---- 2. more workgroups than compute units, and the persistent stride ----------------------------------------------------------------------------
def test_more_workgroups_than_compute_units(pair):
    """One sample of 128 num_cus + 129 points - num_cus + 2 tiles on num_cus workgroups: two of them take a second tile, and the last
    tile holds one point - between samples of 300 and 1 points: 3 + num_cus + 1 workgroups in the launch."""
    hip, oracle = pair
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = 128 * num_cus + 129
    rule = dict(RULE, steps=2, every=1)
    items = [_item(3, 300, "both"), _item(4, big, "disjoint"), _item(5, 1, "hand")]
    z, h = _batch(hip, items, rule)
    for s, it in enumerate(items):
        _same_bits(z[s], h[s], _oracle(oracle, it, ("big", s), rule), ("rounds", s))


# ---- 3. position and company do not matter ---------------------------------------------------------------------------------------------------
def test_position_and_company_do_not_matter(pair):
    hip, _ = pair
    items = [_item(3, 129, "both", torch.zeros(L)), _item(4, 300, "disjoint"), _item(5, 1, "hand")]
    z, h = _batch(hip, items, RULE)
    z2, h2 = _batch(hip, items, RULE)
    assert np.array_equal(_bits(z), _bits(z2)) and np.array_equal(_np(h).view(np.int64), _np(h2).view(np.int64)), "the same call twice"
    for order in ((2, 0, 1), (1, 2, 0)):
        zp, hp = _batch(hip, [items[i] for i in order], RULE)
        for at, i in enumerate(order):
            _same_bits(zp[at], hp[at], (_np(z[i]), _np(h[i])), ("order", order, i))
    for i, it in enumerate(items):
        z1, h1 = _batch(hip, [it], RULE)
        _same_bits(z1[0], h1[0], (_np(z[i]), _np(h[i])), ("alone", i))


# ---- 4. the decoder is left alone ------------------------------------------------------------------------------------------------------------
def test_the_decoder_is_left_alone(pair):
    hip, _ = pair
    latent, embed = _sample(7)
    hip.set_sample(latent.reshape(1, -1), embed)
    x = _cuda(vc.list_points(257))
    before = [_np(v).copy() for v in hip.decode_points(x)]
    math, native_math = hip.math, hip._L.asdf_decoder_get_math(hip._h)
    status, bound = hip._status(False), hip._bound
    _batch(hip, [_item(3, 129, "both"), _item(4, 300, "hand")], RULE)
    assert hip.math == math and hip._L.asdf_decoder_get_math(hip._h) == native_math and hip._bound is bound
    assert np.array_equal(hip._status(False), status)
    after = [_np(v) for v in hip.decode_points(x)]
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, after))


# ---- 5. the ABI ------------------------------------------------------------------------------------------------------------------------------
def _abi_call(dec):
    """A valid two-sample call as a dict of ctypes arguments, and the tensors behind it."""
    lib = _native.lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    ms = [33, 130]
    keep = {"x": _cuda(np.concatenate([vc.list_points(m) for m in ms])),
            "t": _cuda(np.concatenate([fc.targets(m, "hand")[0] for m in ms])),
            "z": torch.stack([_sample(3)[0], _sample(4)[0]]).cuda().contiguous(),
            "embed": torch.zeros(2, 2, _native.MAX_POINT_FEATS, 4, device="cuda"), "table": torch.ones(4, device="cuda"),
            "history": torch.full((2, 2), -1.0, dtype=torch.float64, device="cuda")}
    m_arr = (ctypes.c_int64 * 2)(*ms)
    nbytes = ctypes.c_size_t(0)
    assert lib.asdf_fit_codes_workspace_bytes(dec._h, 2, m_arr, ctypes.byref(nbytes)) == 0 and nbytes.value > 0
    keep["ws"] = torch.empty(nbytes.value + 64, dtype=torch.uint8, device="cuda")
    args = {"dec": dec._h, "B": 2, "xyz": ptr(keep["x"]), "m": m_arr, "th": ptr(keep["t"]), "nh": (ctypes.c_int32 * 2)(*ms), "to": None, "no": None,
            "clamp": ctypes.c_float(fc.CLAMP), "z": ptr(keep["z"]), "z0": None, "embed": ptr(keep["embed"]), "prior": ctypes.c_float(1e-3),
            "table": ptr(keep["table"]), "steps": 2, "ws": ptr(keep["ws"]), "ws_bytes": nbytes.value, "history": ptr(keep["history"]),
            "stream": ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)}
    return lib, args, keep


def test_abi_refusals_and_no_work(pair):
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    hip, _ = pair
    lib, args, keep = _abi_call(hip)
    call = lambda **over: lib.asdf_fit_codes(*dict(args, **over).values())
    start = _np(keep["z"]).copy()
    EINVAL = -1
    bad = {"B < 1": dict(B=0), "null m": dict(m=None), "null xyz": dict(xyz=None), "null z": dict(z=None), "null embed": dict(embed=None),
           "null table": dict(table=None), "null workspace": dict(ws=None), "targets without counts": dict(nh=None),
           "m[s] < 1": dict(m=(ctypes.c_int64 * 2)(33, 0)), "n > m[s]": dict(nh=(ctypes.c_int32 * 2)(34, 130)),
           "n < 0": dict(nh=(ctypes.c_int32 * 2)(33, -1)), "a sample without targets": dict(nh=(ctypes.c_int32 * 2)(33, 0)),
           "no head at all": dict(th=None, nh=None), "clamp 0": dict(clamp=ctypes.c_float(0.0)), "clamp NaN": dict(clamp=ctypes.c_float(float("nan"))),
           "prior < 0": dict(prior=ctypes.c_float(-1e-3)), "steps < 0": dict(steps=-1),
           "misaligned workspace": dict(ws=ctypes.c_void_p(keep["ws"].data_ptr() + 4)), "short workspace": dict(ws_bytes=args["ws_bytes"] - 1),
           "more points than 32 bits": dict(m=(ctypes.c_int64 * 2)(2 ** 31 - 1, 130))}
    for what, over in bad.items():
        assert call(**over) == EINVAL, what
    nbytes = ctypes.c_size_t(0)
    assert lib.asdf_fit_codes_workspace_bytes(hip._h, 0, args["m"], ctypes.byref(nbytes)) == EINVAL
    assert lib.asdf_fit_codes_workspace_bytes(hip._h, 2, (ctypes.c_int64 * 2)(2 ** 31 - 1, 130), ctypes.byref(nbytes)) == EINVAL
    assert lib.asdf_fit_codes_workspace_bytes(hip._h, 2, args["m"], None) == EINVAL
    # steps == 0: ASDF_OK, z and the history untouched - and so they are after every refusal above
    assert call(steps=0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(keep["z"]), _bits(start)) and bool((keep["history"] == -1.0).all())
    z, h = hip.fit_codes([keep["x"][:33]], [keep["t"][:33]], None, [33], None, keep["z"][:1], [_sample(3)[1]], steps=0)
    assert np.array_equal(_bits(z[0]), _bits(start[0])) and tuple(h.shape) == (1, 0)
    # the valid call runs
    assert call() == 0
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(keep["z"]), _bits(start)) and bool((keep["history"] > 0.0).all())
    # decoders the reverse-mode form refuses
    for tag, pf, word in (("comb3", 3, "CombinedDecoder"), ("nerf9", 9, "NeRF")):
        dec = HipSdfDecoder(syn.full_state_dict(tag), 256, pf, "nerf")
        assert call(dec=dec._h) == _native.ENOGRAD and word in dec.fit_codes_refusal()
        with pytest.raises(NotImplementedError, match=word):
            dec.fit_codes([keep["x"][:33]], [keep["t"][:33]], None, [33], None, keep["z"][:1], [None], steps=1)
        dec.close()


@pytest.mark.parametrize("tag", ["nerf9", "comb3"])
def test_refused_decoders_run_the_loop_over_fit_code(tag):
    from alignsdf_amd.fit import fit_code, fit_codes
    from alignsdf_amd.utils.utils import decoder_for
    specs, module = syn.specs_for(tag), gc.module_for(tag)
    hip = decoder_for(module, specs, None)
    assert hip.fit_codes_refusal() is not None
    x = _cuda(vc.points(96, 4))
    items = []
    for target, start in ((1, 2), (3, 4)):
        hip.set_sample(torch.from_numpy(syn.latent_code(target)))
        f = hip.decode_points(x)
        items.append({"latent": torch.from_numpy(syn.latent_code(start)).reshape(-1), "embed": None, "sdf_hand": (x, f[0].clone()),
                      "sdf_obj": (x, f[1].clone())})
    kw = dict(steps=3, lr=5e-3, decay=1.0, every=1, prior=1e-4, clamp=0.2)
    with pytest.raises(NotImplementedError, match="module"):
        fit_codes(hip, items, **kw)
    z, h = fit_codes(hip, items, module=module, specs=specs, **kw)
    assert tuple(z.shape) == (2, L) and tuple(h.shape) == (2, 3)
    for s, it in enumerate(items):
        zl, hl = fit_code(hip, it["latent"], None, sdf_hand=it["sdf_hand"], sdf_obj=it["sdf_obj"], module=module, specs=specs, **kw)
        assert np.array_equal(_bits(z[s]), _bits(zl)) and np.array_equal(_np(h[s]), _np(hl)), (tag, s)


# ---- 6. the flow -----------------------------------------------------------------------------------------------------------------------------
def _write_obj(path, verts, faces):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        for p in np.asarray(verts, np.float64):
            fh.write("v %.9g %.9g %.9g\n" % tuple(float(c) for c in p))
        for t in np.asarray(faces):
            fh.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


def test_autodecode_in_batches_writes_the_files_of_one_by_one(tmp_path):
    """Three synthetic scenes (a torus "hand" and a box "object", each scene at its own scale) under the grasp3 decoder; --batch 2 is
    one full and one short batch."""
    from alignsdf_amd import autodecode as ad
    from tests import mesh_sdf_cases as mc
    tag = "grasp3"
    specs, module = syn.specs_for(tag), gc.module_for(tag)
    names = ("00000001", "00000002", "00000005")
    (hv, hf), (bv, bf) = mc.torus(*mc.TORUS_EDGE), mc.box()
    for name, scale in zip(names, (0.5, 0.4, 0.6)):
        for part, v, faces in (("hand", hv, hf), ("obj", bv, bf)):
            _write_obj(str(tmp_path / "data" / "obman" / "test" / ("mesh_" + part) / (name + ".obj")),
                       ad.from_decoder_frame(scale * np.asarray(v, np.float64), 1.0, (0, 0, 0), specs["SdfScaleFactor"]), faces)
    fitter = ad.DeviceFitter(module, specs, fit=dict(RULE, steps=4), sampling={"near": 300, "uniform": 100})
    outs = {}
    for batch in (1, 2):
        path, records = ad.run(specs, fitter, "obman", str(tmp_path / "data"), str(tmp_path / ("codes%d" % batch)), batch=batch)
        outs[batch] = (records, json.load(open(path)), [dict(np.load(str(tmp_path / ("codes%d" % batch) / (n + ".npz")))) for n in names])
    assert [r["name"] for r in outs[2][0]] == list(names) and outs[1][0] == outs[2][0] and outs[1][1] == outs[2][1]
    for one, two in zip(outs[1][2], outs[2][2]):
        assert list(one) == list(two) and all(np.array_equal(_bits(one[k]), _bits(two[k])) for k in one)
        assert one["latent"].shape == (1, L) and one["latent"].any()
    codes = [o["latent"] for o in outs[1][2]]
    assert not np.array_equal(codes[0], codes[1]) and all(r["steps"] == 4 and r["last"] < r["first"] for r in outs[1][0])
