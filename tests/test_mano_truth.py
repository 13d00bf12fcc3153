"""mano_torch - the MANO rule as a torch statement, the module path of the kernels and, in fp64, their truth - against the reference's
own layer (tests/golden/ref_mano_layer.npz, written by make_mano_goldens.py from manopth/manolayer.py on the host).

Per case and quantity the fixture holds the reference's fp32 result and E_ref, the distance of that result from the same layer's
fp64 result.  Two checks:
  fp32  mano_torch in fp32 against the reference's fp32 result.  mano_torch keeps the reference's order of operations, so every output
        and d_pose are held to EQUALITY (difference 0 - a later reordering of the statement shows here); d_shape, whose two paths
        autograd adds up in an order of its own, is held to E_ref (observed 3.7e-9 .. 6.0e-8 against E_ref 1.2e-8 .. 1.5e-7).
  fp64  mano_torch in fp64 lies E_ref from the reference's fp32 result - it is the reference's fp64 side (to fp64 rounding, for which
        the bound gets 1e-12 of room).
Then a known-answer fit on mano_torch alone: the rule is differentiable well enough to recover a pose from vertices.
"""
import os

import numpy as np
import pytest
import torch

from tests import mano_cases
from alignsdf_amd import mano

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mano_layer.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


run_statement = mano_cases.statement


@pytest.mark.parametrize("case", mano_cases.CASES, ids=lambda c: c.name)
def test_statement_matches_the_reference_layer(golden, case):
    r32, r64 = run_statement(case, torch.float32), run_statement(case, torch.float64)
    names = [k for k in mano_cases.OUTPUTS + mano_cases.GRADS if "%s.%s" % (case.name, k) in golden]
    assert set(names) == set(r32) and ("center" in names) == (case.trans is None and case.center_idx is not None)
    for k in names:
        ref, e_ref = golden["%s.%s" % (case.name, k)].astype(np.float64), float(golden["%s.E_ref.%s" % (case.name, k)])
        d32, d64 = np.abs(r32[k] - ref).max(), np.abs(r64[k] - ref).max()
        print("%s %s: fp32 vs reference fp32 %.3e, fp64 vs reference fp32 %.3e, E_ref %.3e" % (case.name, k, d32, d64, e_ref))
        assert r32[k].shape == ref.shape
        if k == "d_shape":
            assert d32 <= e_ref, (k, d32, e_ref)
        else:           # the order of operations is the reference's: its fp32 bits
            assert d32 == 0, (k, d32)
        assert d64 <= e_ref * (1 + 1e-6) + 1e-12, (k, d64, e_ref)


def test_zero_pose_is_finite_and_differentiable():
    case = mano_cases.BY_NAME["zero778"]
    r = run_statement(case, torch.float32)
    assert all(np.isfinite(v).all() for v in r.values())
    eye = np.broadcast_to(np.eye(3), (1, 16, 3, 3))
    assert np.abs(r["global_trans"][:, :, :3, :3] - eye).max() < 1e-6 and np.abs(r["d_pose"]).max() > 0


def test_synthetic_model_is_hand_sized_and_normalised():
    for V in (778, 70):
        m = mano.ManoModel.synthetic(mano_cases.MODEL_SEED, V)
        extent = (m.v_template.max(0) - m.v_template.min(0)).max()
        assert 0.05 < extent < 0.2
        assert (m.J_regressor >= 0).all() and np.allclose(m.J_regressor.sum(1), 1, atol=1e-5)
        assert (m.weights >= 0).all() and np.allclose(m.weights.sum(1), 1, atol=1e-5)
        assert m.tips.min() >= 0 and m.tips.max() < V and len(set(m.tips.tolist())) == 5
        again = mano.ManoModel.synthetic(mano_cases.MODEL_SEED, V)
        assert all(np.array_equal(getattr(m, k), getattr(again, k)) for k in mano.ARRAYS)


def test_layer_on_host_tensors_is_the_statement_and_npz_round_trips(tmp_path):
    case = mano_cases.BY_NAME["moderate6_70"]
    model = mano_cases.model_of(case)
    model.save_npz(tmp_path / "m.npz")
    layer = mano.ManoLayer(mano.ManoModel.from_npz(tmp_path / "m.npz"), ncomps=case.ncomps, center_idx=case.center_idx)
    pose, shape = torch.from_numpy(case.pose), torch.from_numpy(case.shape)
    got = layer(pose, shape)
    want = mano.mano_torch(model, pose, shape, center_idx=case.center_idx)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    res = mano.mano_results(layer, pose, shape, mano_root=torch.tensor([[0.1, 0.2, 0.3]]))
    assert set(res) == {"verts", "joints", "shape", "pcas", "pose", "center3d", "global_trans", "rot_center"}
    assert torch.equal(res["verts"], res["center3d"] + want[0]) and torch.equal(res["rot_center"], want[4])
    assert res["global_trans"].shape == (1, 16, 4, 4) and res["rot_center"].shape == (1, 1, 3)


def test_known_answer_fit_on_the_statement():
    from alignsdf_amd import mano_fit
    model, _, _, target, start = mano_cases.fit_problem()
    layer = mano.ManoLayer(model, ncomps=mano_cases.FIT_NCOMPS, center_idx=0)
    res = mano_fit.fit_mano(layer, start, torch.zeros(1, 10, dtype=torch.float64), verts_target=target, steps=mano_cases.FIT_STEPS,
                            lr=mano_cases.FIT_LR)
    rms = lambda v: float(((v - target) ** 2).sum(-1).mean().sqrt())
    with torch.no_grad():
        first = rms(layer(start, torch.zeros(1, 10, dtype=torch.float64))[0])
        last = rms(layer(res.pose, res.shape)[0])
    print("known-answer fit, fp64 statement: rms %.3e -> %.3e (bound %.3e)" % (first, last, mano_cases.FIT_RMS_BOUND))
    assert first > 1e-2 and last <= mano_cases.FIT_RMS_BOUND
    assert res.losses.shape == (mano_cases.FIT_STEPS,) and res.losses[-1] < res.losses[0]
