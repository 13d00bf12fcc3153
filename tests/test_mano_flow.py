"""The host side of the MANO flow: codes files with MANO parameters, the files mano_fit writes, evaluate_mano's columns and summary
(Chamfer stubbed: the GPU routine is exercised in test_gpu_mano_fit.py), and the pickle converter on a pickle of the official file's
structure written here (chumpy objects included, without chumpy)."""
import importlib.util
import json
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

from tests import mano_cases
from alignsdf_amd import code_sources, evaluate, mano, mano_fit
from alignsdf_amd import synthetic as syn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def model():
    return mano.ManoModel.synthetic(mano_cases.MODEL_SEED, 70)


def test_code_source_with_mano_parameters_equals_the_one_with_their_matrices(tmp_path, model):
    a, b = tmp_path / "params", tmp_path / "matrices"
    os.makedirs(a), os.makedirs(b)
    latent, _, obj = syn.sample_inputs("both9", 1)
    pose = (0.4 * syn.normal((1, 9), 58001)).astype(np.float32)
    shape = syn.normal((1, 10), 58002).astype(np.float32)
    with torch.no_grad():
        _, _, _, gt, center = mano.mano_torch(model, torch.from_numpy(pose), torch.from_numpy(shape), center_idx=0)
    np.savez(a / "s.npz", latent=latent, mano_pose=pose, mano_shape=shape, obj_trans=obj["obj_trans"])
    np.savez(b / "s.npz", latent=latent, global_trans=gt.numpy(), rot_center=center.numpy(), obj_trans=obj["obj_trans"])
    from_params = code_sources.npz_code_source(str(a), mano_model=model)("s", 0)
    for source in (code_sources.npz_code_source(str(b)), code_sources.npz_code_source(str(b), mano_model=model)):      # old files: as ever
        from_matrices = source("s", 0)
        assert torch.equal(from_params[0], from_matrices[0])
        for x, y in zip(from_params[1:], from_matrices[1:]):
            assert set(x) == set(y) and all(torch.equal(x[k], y[k]) and x[k].dtype == torch.float32 and not x[k].is_cuda for k in x)
    assert from_params[1]["global_trans"].shape == (1, 16, 4, 4) and from_params[1]["rot_center"].shape == (1, 1, 3)
    with pytest.raises(ValueError, match="mano_model"):
        code_sources.npz_code_source(str(a))("s", 0)


def test_written_hand_has_the_reference_keys(tmp_path, model):
    layer = mano.ManoLayer(model, ncomps=6, center_idx=0)
    pose, shape = torch.from_numpy((0.3 * syn.normal((1, 9), 58003)).astype(np.float32)), torch.zeros(1, 10)
    res = mano.mano_results(layer, pose, shape)
    mano_fit.write_mano(str(tmp_path / "pred_mano"), "x", res["verts"][0], res["joints"][0], shape, res["pose"][0], model.faces)
    rec = json.load(open(tmp_path / "pred_mano" / "x.json"))
    assert set(rec) == {"joints", "vertices", "shape", "pose"}
    assert np.shape(rec["joints"]) == (21, 3) and np.shape(rec["vertices"]) == (70, 3) and len(rec["shape"]) == 10 and len(rec["pose"]) == 45
    assert np.allclose(rec["vertices"], res["verts"][0].numpy(), atol=1e-7)
    from alignsdf_amd.ply import read_ply
    v, f = read_ply(str(tmp_path / "pred_mano" / "x.ply"))
    assert np.allclose(v, res["verts"][0].numpy(), atol=1e-7) and np.array_equal(f, model.faces)


def test_fit_mano_refuses_what_it_cannot_fit(model):
    layer = mano.ManoLayer(model, ncomps=6, center_idx=None)
    with pytest.raises(ValueError, match="nothing to fit"):
        mano_fit.fit_mano(layer, torch.zeros(1, 9), torch.zeros(1, 10), steps=1, lr=0.01)
    with pytest.raises(ValueError, match="center_idx"):
        mano_fit.fit_mano(layer, torch.zeros(1, 9), torch.zeros(1, 10), decoder=object(), scale_factor=6.2, steps=1, lr=0.01)


def test_evaluate_mano_columns_and_summary(tmp_path, monkeypatch):
    exp, data = tmp_path / "exp", tmp_path / "data"
    for sub in ("pred_mano", "optim_mano"):
        os.makedirs(exp / "Eval_obman" / sub)
    os.makedirs(data / "mesh_hand"), os.makedirs(data / "meta")
    rng = lambda seed, n: syn.normal((n, 3), seed)
    flip = np.diag([1.0, -1.0, -1.0])
    want = {}
    for i, name in enumerate(("a1", "b2", "c3")):
        gt_j, gt_v = rng(59000 + i, 21), rng(59010 + i, 30)
        off_j, off_v = 0.01 * (i + 1) * rng(59020 + i, 21), 0.02 * (i + 1) * rng(59030 + i, 30)
        off_j[0] = 0.0
        shift = np.array([0.3, -0.2, 0.5])                   # (root-relative: a common shift of the prediction does not count)
        for sub, scale in (("pred_mano", 1.0), ("optim_mano", 0.5)):
            rec = {"joints": (gt_j + scale * off_j + shift).tolist(), "vertices": (gt_v + scale * off_v + shift).tolist(),
                   "shape": [0.0] * 10, "pose": [0.0] * 45}
            json.dump(rec, open(exp / "Eval_obman" / sub / (name + ".json"), "w"))
            open(exp / "Eval_obman" / sub / (name + ".ply"), "w").write("ply")
            want[(sub, name)] = (np.linalg.norm(scale * off_j, axis=1).mean(), np.linalg.norm(scale * off_v, axis=1).mean())
        if name != "c3":                                     # c3 has no ground-truth mesh: a failure, like the reference counts them
            open(data / "mesh_hand" / (name + ".obj"), "w").write("obj")
        pickle.dump({"coords_3d": gt_j @ flip, "verts_3d": gt_v @ flip}, open(data / "meta" / (name + ".pkl"), "wb"))
    calls = []

    def chamfer(gt, pred, optim, rot, seed=0):
        calls.append((os.path.basename(gt), pred))
        return 2.0 if "a1" in pred else 1.0
    monkeypatch.setattr(evaluate, "compute_trimesh_chamfer", chamfer)
    for optim_mano, sub in ((False, "pred_mano"), (True, "optim_mano")):
        rows, n_pred, path = evaluate.evaluate_mano(str(exp), str(data), "obman", optim_mano=optim_mano)
        assert n_pred == 3 and [r[0] for r in rows] == ["a1", "b2"] and all(os.sep + sub + os.sep in c[1] for c in calls[-2:])
        for name, ch, j, v in rows:
            assert np.isclose(j, want[(sub, name)][0], rtol=1e-12) and np.isclose(v, want[(sub, name)][1], rtol=1e-12)
        lines = open(path).read().splitlines()
        assert os.path.basename(path) == "chamfer_mano.txt" and lines[0] == "summary of chamfer_dist"
        assert lines[1].startswith("a1, 2.0, ") and lines[2].startswith("b2, 1.0, ")          # sorted by decreasing Chamfer distance
        assert np.isclose(float(lines[1].split(", ")[2]), 1000 * want[(sub, "a1")][0])
        assert lines[3] == "mean chamfer distance:1.5" and lines[4] == "median chamfer distance:1.5"
        # (the two means in millimetres, like the rows and like the reference's evaluate.py:308-309)
        assert np.isclose(float(lines[5].split(":")[1]), 1000 * np.mean([want[(sub, n)][0] for n in ("a1", "b2")]))
        assert np.isclose(float(lines[6].split(":")[1]), 1000 * np.mean([want[(sub, n)][1] for n in ("a1", "b2")]))
        assert lines[7] == "failure count:1"
    # a task whose camera frame is the data's own: no flip, so the flipped ground truth no longer matches
    pred_json, meta = str(exp / "Eval_obman" / "pred_mano" / "a1.json"), str(data / "meta" / "a1.pkl")
    assert np.isclose(evaluate.mano_errors(pred_json, meta, "obman")[0], want[("pred_mano", "a1")][0])
    assert evaluate.mano_errors(pred_json, meta, "dexycb")[0] > 10 * want[("pred_mano", "a1")][0]
    # what existed before stays as it was
    with pytest.raises(NotImplementedError):
        evaluate.evaluate_queue(None, str(exp), str(data), 0, None, False, True, False, False, False, False, "obman")


def test_pickle_converter_round_trips(tmp_path, model):
    import scipy.sparse
    spec = importlib.util.spec_from_file_location("mano_pkl_to_npz", os.path.join(ROOT, "tools", "mano_pkl_to_npz.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    full = mano.ManoModel.synthetic(mano_cases.MODEL_SEED, 778)
    # stand-ins for the two chumpy classes the official file holds, pickled under chumpy's module names
    fake = {"chumpy": types.ModuleType("chumpy"), "chumpy.ch": types.ModuleType("chumpy.ch"),
            "chumpy.reordering": types.ModuleType("chumpy.reordering")}
    Ch = type("Ch", (), {"__module__": "chumpy.ch"})
    Select = type("Select", (), {"__module__": "chumpy.reordering"})
    fake["chumpy.ch"].Ch, fake["chumpy.reordering"].Select = Ch, Select

    def ch(array):
        o = Ch()
        o.x = np.asarray(array, np.float64)
        return o
    shapedirs = Select()
    padded = np.concatenate([full.shapedirs.astype(np.float64), np.full((778, 3, 2), 9.0)], 2)       # the file selects 10 of more
    shapedirs.a, shapedirs.preferred_shape = ch(padded), (778, 3, 10)
    shapedirs.idxs = np.arange(padded.size).reshape(padded.shape)[:, :, :10].ravel()
    data = {"hands_components": full.comps.astype(np.float64), "f": full.faces.astype(np.uint32),
            "J_regressor": scipy.sparse.csc_matrix(full.J_regressor.astype(np.float64)), "kintree_table": np.array(
                [[4294967295, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14], list(range(16))], dtype=np.uint32),
            "weights": ch(full.weights), "posedirs": ch(full.posedirs), "hands_mean": full.hands_mean.astype(np.float64),
            "v_template": ch(full.v_template), "shapedirs": shapedirs, "bs_style": "lbs", "bs_type": "lrotmin"}
    sys.modules.update(fake)
    try:
        with open(tmp_path / "MANO_RIGHT.pkl", "wb") as f:
            pickle.dump(data, f, protocol=2)
    finally:
        for k in fake:
            del sys.modules[k]
    assert "chumpy" not in sys.modules
    tool.main([str(tmp_path / "MANO_RIGHT.pkl"), str(tmp_path / "m.npz")])
    back = mano.ManoModel.from_npz(str(tmp_path / "m.npz"))
    for k in mano.ARRAYS[:-1] + ("faces",):
        assert np.array_equal(getattr(back, k), getattr(full, k)), k
    assert tuple(back.tips) == mano.RIGHT_TIPS
    tool.main([str(tmp_path / "MANO_RIGHT.pkl"), str(tmp_path / "flat.npz"), "--flat_hand_mean"])
    assert not mano.ManoModel.from_npz(str(tmp_path / "flat.npz")).hands_mean.any()
