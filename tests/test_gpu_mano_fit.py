"""fit_mano through the kernels of csrc/mano.hip, and the flow around it.

  - the known-answer vertex fit of tests/mano_cases.py, on the device: the same start, steps and lr, held to the SAME bound (ten times
    what the fp64 statement reached on the host);
  - the SDF term on the synthetic pose-aligned decoder "both9": one step's d_pose / d_shape from the reverse kernel against the fp64
    statement's VJP, both fed the cotangent built from the decoder's own (f, grad f).  Bound: 4 x the reference layer's own worst
    RELATIVE fp32 error on d_pose / d_shape over the V = 778 cases of tests/golden/ref_mano_layer.npz (E_ref over the gradient's largest
    magnitude), times this gradient's largest magnitude - the rule of test_gpu_mano.py carried to a cotangent the fixture has no
    E_ref for;
  - 30 steps of that fit lower the objective.  Start (pose 0.2 N(0, 1) with a zero root rotation, shape 0) and lr 0.02 were rehearsed
    on the host against the analytic shape the head was fitted to - clip(0.5 (|x - c| - 0.35), +-0.05), synthetic.analytic_sdf under
    make_ref_goldens' clamp -: mean |f| went 0.0310 -> 0.0161 in 30 steps there;
  - mano_fit's flow on two samples writes the four files per sample, and evaluate_mano reads them into finite columns;
  - a decoder the gradient kernel refuses (CombinedDecoder "comb3") goes through the flow on the module path.
"""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import mano_cases
from tests import sdf_grad_cases as gc
from tests.mano_cases import FIT_LR, FIT_NCOMPS, FIT_RMS_BOUND, FIT_STEPS, fit_problem
from alignsdf_amd import mano, mano_fit
from alignsdf_amd import synthetic as syn

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mano_layer.npz")
TAG, NCOMPS = "both9", 15


def test_known_answer_vertex_fit_on_the_device():
    model, _, _, target, start = fit_problem(torch.float32, "cuda")
    layer = mano.ManoLayer(model, ncomps=FIT_NCOMPS, center_idx=0)
    res = mano_fit.fit_mano(layer, start, torch.zeros(1, 10, device="cuda"), verts_target=target, steps=FIT_STEPS, lr=FIT_LR)
    rms = lambda v: float(((v.double() - target.double()) ** 2).sum(-1).mean().sqrt())
    first, last = rms(layer(start, torch.zeros(1, 10, device="cuda"))[0]), rms(res.verts)
    print("known-answer fit, kernels: rms %.3e -> %.3e (bound %.3e)" % (first, last, FIT_RMS_BOUND))
    assert res.pose.is_cuda and res.losses.shape == (FIT_STEPS,)
    assert first > 1e-2 and last <= FIT_RMS_BOUND


@pytest.fixture(scope="module")
def sdf_setup():
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.utils.utils import bind_sample
    specs = syn.specs_for(TAG)
    dec = HipSdfDecoder(gc.module_for(TAG))
    latent, mano_in, obj_in = syn.sample_inputs(TAG, 0)
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    bind_sample(dec, specs, torch.from_numpy(latent), t(mano_in), t(obj_in))
    model = mano.ManoModel.synthetic(mano_cases.MODEL_SEED, 778)
    pose = (0.2 * syn.normal((1, 3 + NCOMPS), 57001)).astype(np.float32)
    pose[0, :3] = 0.0
    yield dec, specs, model, pose
    dec.close()


def test_sdf_term_gradient_against_the_fp64_statement(sdf_setup):
    dec, specs, model, pose = sdf_setup
    sf = specs["SdfScaleFactor"]
    layer = mano.ManoLayer(model, ncomps=NCOMPS, center_idx=0)
    dm = layer.device_model("cuda")
    p, s = torch.from_numpy(pose).cuda(), torch.zeros(1, 10, device="cuda")
    verts = dm.forward(p, s, None, 0)[0]
    f, g = dec.decode_points_grad(verts[0] * (sf / 2.0), hand=True, obj=False)[:2]
    cot = mano_fit.sdf_cotangent(f, g, sf).reshape(1, 778, 3).contiguous()
    assert float(cot.abs().max()) > 0
    d_pose, d_shape = dm.backward(p, s, None, 0, cot, None, None, None)
    p64, s64 = torch.from_numpy(pose).double().requires_grad_(True), torch.zeros(1, 10, dtype=torch.float64, requires_grad=True)
    v64 = mano.mano_torch(model, p64, s64, center_idx=0)[0]
    t_pose, t_shape = torch.autograd.grad((v64 * cot.cpu().double()).sum(), (p64, s64))
    with np.load(GOLDEN) as z:
        rel = {k: max(float(z["%s.E_ref.%s" % (c.name, k)]) / float(np.abs(z["%s.%s" % (c.name, k)]).max())
                      for c in mano_cases.CASES if c.V == 778) for k in ("d_pose", "d_shape")}
    for name, got, want in (("d_pose", d_pose, t_pose), ("d_shape", d_shape, t_shape)):
        err, bound = float((got.cpu().double() - want).abs().max()), 4.0 * rel[name] * float(want.abs().max())
        print("sdf term %s: err %.3e  bound %.3e  (largest %.3e, reference's relative fp32 error %.3e)" % (
            name, err, bound, float(want.abs().max()), rel[name]))
        assert err <= bound, name


def test_sdf_term_fit_lowers_the_objective(sdf_setup):
    dec, specs, model, pose = sdf_setup
    layer = mano.ManoLayer(model, ncomps=NCOMPS, center_idx=0)
    res = mano_fit.fit_mano(layer, torch.from_numpy(pose).cuda(), torch.zeros(1, 10, device="cuda"), decoder=dec, head="hand",
                            scale_factor=specs["SdfScaleFactor"], steps=31, lr=0.02)
    print("sdf term fit: mean |f| %.4e -> %.4e after 30 steps" % (res.losses[0], res.losses[30]))
    assert np.isfinite(res.losses).all() and res.losses[30] < res.losses[0]


def test_flow_writes_both_directories_and_evaluate_mano_reads_them(tmp_path):
    from alignsdf_amd import evaluate
    from alignsdf_amd.deep_sdf.metrics.chamfer import load_mesh
    specs, module = syn.specs_for(TAG), gc.module_for(TAG)
    model = mano.ManoModel.synthetic(mano_cases.MODEL_SEED, 778)
    codes, exp, data = tmp_path / "codes", tmp_path / "exp", tmp_path / "data"
    for d in (codes, data / "mesh_hand", data / "meta"):
        os.makedirs(d)
    names = ["00000007", "00000011"]
    for i, name in enumerate(names):
        latent, _, obj_in = syn.sample_inputs(TAG, i)
        pose = (0.2 * syn.normal((1, 3 + NCOMPS), 57100 + i)).astype(np.float32)
        shape = (0.5 * syn.normal((1, 10), 57200 + i)).astype(np.float32)
        np.savez(codes / (name + ".npz"), latent=latent, mano_pose=pose, mano_shape=shape, obj_trans=obj_in["obj_trans"])
        # a "ground truth" next to it: the hand of slightly different parameters (obman stores it with y and z flipped)
        with torch.no_grad():
            v, j = mano.mano_torch(model, torch.from_numpy(pose) + 0.05, torch.from_numpy(shape), center_idx=0)[:2]
        with open(data / "mesh_hand" / (name + ".obj"), "w") as f:
            f.write("".join("v %.8f %.8f %.8f\n" % tuple(r) for r in v[0].tolist()))
            f.write("".join("f %d %d %d\n" % tuple(int(k) + 1 for k in r) for r in model.faces.tolist()))
        flip = np.diag([1.0, -1.0, -1.0])
        with open(data / "meta" / (name + ".pkl"), "wb") as f:
            pickle.dump({"coords_3d": j[0].numpy() @ flip, "verts_3d": v[0].numpy() @ flip}, f)
    out_root = exp / "Eval_obman"
    records = mano_fit.run(specs, module, model, str(codes), str(out_root), steps=5, lr=0.01)
    assert [r["name"] for r in records] == names and all(np.isfinite([r["first"], r["last"]]).all() for r in records)
    for name in names:
        for sub in ("pred_mano", "optim_mano"):
            rec = json.load(open(out_root / sub / (name + ".json")))
            assert set(rec) == {"joints", "vertices", "shape", "pose"}
            assert np.shape(rec["joints"]) == (21, 3) and np.shape(rec["vertices"]) == (778, 3)
            assert np.shape(rec["shape"]) == (10,) and np.shape(rec["pose"]) == (45,)
            pv, pf = load_mesh(str(out_root / sub / (name + ".ply")))
            assert np.allclose(pv, np.array(rec["vertices"]), atol=1e-6) and np.array_equal(pf, model.faces)
    for optim_mano in (False, True):
        rows, n_pred, path = evaluate.evaluate_mano(str(exp), str(data), "obman", optim_mano=optim_mano)
        assert n_pred == 2 and sorted(r[0] for r in rows) == names
        assert np.isfinite([r[1:] for r in rows]).all() and all(r[1] > 0 and 0 < r[2] < 0.05 and 0 < r[3] < 0.05 for r in rows)
        text = open(path).read()
        assert os.path.basename(path) == "chamfer_mano.txt" and "mean joints error:" in text and "nan" not in text


def test_flow_takes_the_module_path_where_the_gradient_kernel_refuses(tmp_path):
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    specs, module = syn.specs_for("comb3"), gc.module_for("comb3")
    native = HipSdfDecoder(module)
    assert native.grad_refusal() is not None
    picked = mano_fit.gradient_decoder(native, module, specs)
    assert isinstance(picked, TorchModuleDecoder) and mano_fit.gradient_decoder(picked, module, specs) is picked
    with pytest.raises(NotImplementedError, match="nn.Module"):
        mano_fit.gradient_decoder(native, None, specs)
    native.close()
    model = mano.ManoModel.synthetic(mano_cases.MODEL_SEED, 70)
    os.makedirs(tmp_path / "codes")
    np.savez(tmp_path / "codes" / "s.npz", latent=syn.sample_inputs("comb3", 0)[0], mano_pose=(0.2 * syn.normal((1, 9), 57300)).astype(np.float32),
             mano_shape=np.zeros((1, 10), np.float32))
    records = mano_fit.run(specs, module, model, str(tmp_path / "codes"), str(tmp_path / "out"), steps=2, lr=0.01)
    assert len(records) == 1 and np.isfinite([records[0]["first"], records[0]["last"]]).all()
    assert all(os.path.exists(tmp_path / "out" / sub / ("s" + ext)) for sub in ("pred_mano", "optim_mano") for ext in (".json", ".ply"))
