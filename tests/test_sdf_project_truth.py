"""The projection rule on the CPU (alignsdf_amd.project.project_lockstep, the torch statement of asdf_project_points):

  1. analytic fields with known answers - sphere, plane, zero gradient, non-finite points, max_iters = 0, the trust box
  2. the conditions of the GPU sets, asserted on the reference alone: the rule over the fp32 oracle chain (sdf_grad_cases.grad_truth in
     fp32), judged by the fp64 truth"""
import numpy as np
import pytest
import torch

from alignsdf_amd import project as pj
from tests import sdf_project_cases as pc


def _sphere(r, centre=(0.0, 0.0, 0.0)):
    c = torch.tensor(centre, dtype=torch.float32)

    def grad_of(p):
        d = p - c
        n = torch.linalg.vector_norm(d, dim=1)
        return n - r, d / n[:, None]
    return grad_of


def _plane(normal, offset):
    n = torch.tensor(normal, dtype=torch.float32)

    def grad_of(p):
        return p @ n - offset, n.expand(p.shape[0], 3)
    return grad_of


def _points(M, seed, lo=0.3, hi=1.5):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(M, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy((d * rng.uniform(lo, hi, (M, 1))).astype(np.float32))


def test_a_sphere_is_reached_in_one_step():
    pts = _points(200, 1)
    r = pj.project_lockstep(_sphere(0.8), pts, max_iters=8, tol=1e-6, max_move=2.0)
    assert (r["status"] == pj.CONVERGED).all()
    assert int(r["evals"].max()) <= 3 and float((r["evals"] == 2).float().mean()) > 0.9
    radius = torch.linalg.vector_norm(r["xyz_out"].double(), dim=1)
    assert float((radius - 0.8).abs().max()) <= 1e-6 + 4 * np.finfo(np.float32).eps
    # along the ray through the centre, and the returned sdf / grad / sdf_in belong to the returned / the input point
    unit = pts.double() / torch.linalg.vector_norm(pts.double(), dim=1, keepdim=True)
    assert float((r["xyz_out"].double() - 0.8 * unit).abs().max()) <= 1e-6
    f, g = _sphere(0.8)(r["xyz_out"])
    assert torch.equal(r["sdf"], f) and torch.equal(r["grad"], g)
    assert torch.equal(r["sdf_in"], _sphere(0.8)(pts)[0])


def test_a_plane_is_reached_along_its_normal():
    normal, offset = (0.6, 0.0, 0.8), 0.25
    pts = _points(100, 2)
    r = pj.project_lockstep(_plane(normal, offset), pts, max_iters=4, tol=1e-6, max_move=4.0)
    assert (r["status"] == pj.CONVERGED).all() and int(r["evals"].max()) <= 3
    n = torch.tensor(normal, dtype=torch.float64)
    want = pts.double() - ((pts.double() @ n) - offset)[:, None] * n
    assert float((r["xyz_out"].double() - want).abs().max()) <= 1e-6
    # a field scaled by 3: f / |g|^2 still lands on the plane
    scaled = lambda p: tuple(3.0 * v for v in _plane(normal, offset)(p))
    r3 = pj.project_lockstep(scaled, pts, max_iters=4, tol=1e-6, max_move=4.0)
    assert float((r3["xyz_out"].double() - want).abs().max()) <= 2e-6


def test_zero_and_nan_gradients_stall_and_the_point_stays():
    pts = _points(9, 3)
    flat = lambda p: (torch.full((p.shape[0],), 0.5), torch.zeros(p.shape[0], 3))
    r = pj.project_lockstep(flat, pts)
    assert (r["status"] == pj.STALLED).all() and (r["evals"] == 1).all() and torch.equal(r["xyz_out"], pts)
    nan = lambda p: (torch.full((p.shape[0],), 0.5), torch.full((p.shape[0], 3), float("nan")))
    r = pj.project_lockstep(nan, pts)
    assert (r["status"] == pj.STALLED).all() and torch.equal(r["xyz_out"], pts)
    # |f| <= tol is asked first: a point on the level is CONVERGED whatever its gradient
    on = lambda p: (torch.zeros(p.shape[0]), torch.zeros(p.shape[0], 3))
    assert (pj.project_lockstep(on, pts)["status"] == pj.CONVERGED).all()


def test_non_finite_points_are_bad_without_an_evaluation():
    pts = _points(8, 4)
    pts[2, 1], pts[5, 0], pts[6, 2] = float("nan"), float("inf"), float("-inf")
    seen = []

    def grad_of(p):
        seen.append(p.clone())
        return _sphere(0.8)(p)
    r = pj.project_lockstep(grad_of, pts, max_move=2.0)
    bad = torch.tensor([False, False, True, False, False, True, True, False])
    assert torch.equal(r["status"] == pj.BAD, bad)
    assert (r["evals"][bad] == 0).all() and (r["evals"][~bad] >= 1).all()
    assert (r["sdf"][bad] == 0).all() and (r["grad"][bad] == 0).all() and (r["sdf_in"][bad] == 0).all()
    assert torch.equal(r["xyz_out"][bad].isnan(), pts[bad].isnan()) and torch.equal(r["xyz_out"][bad].isinf(), pts[bad].isinf())
    assert all(torch.isfinite(p).all() for p in seen)          # (they feed the origin of the space)
    assert (r["status"][~bad] == pj.CONVERGED).all()
    # nothing but BAD points: no evaluation at all
    seen.clear()
    r = pj.project_lockstep(grad_of, pts[bad], max_move=2.0)
    assert not seen and (r["status"] == pj.BAD).all()


def test_max_iters_zero_is_one_evaluation_judged_by_f_alone():
    pts = torch.cat([_points(20, 5), torch.tensor([[0.8, 0.0, 0.0], [0.0, -0.8, 0.0]])])
    r = pj.project_lockstep(_sphere(0.8), pts, max_iters=0, tol=1e-6, max_move=1.0)
    assert (r["evals"] == 1).all() and torch.equal(r["xyz_out"], pts)
    f = _sphere(0.8)(pts)[0]
    assert torch.equal(r["status"] == pj.CONVERGED, f.abs() <= 1e-6) and torch.equal(r["status"] == pj.SPENT, f.abs() > 1e-6)
    assert (r["status"][-2:] == pj.CONVERGED).all() and (r["status"][:-2] == pj.SPENT).any()


@pytest.mark.parametrize("max_iters", [1, 3, 8])
def test_a_small_trust_box_pins_the_result_to_its_face(max_iters):
    pts = torch.tensor([[1.5, 0.0, 0.0], [0.0, -1.5, 0.0], [0.0, 0.0, 0.2], [0.81, 0.0, 0.0]])
    r = pj.project_lockstep(_sphere(0.8), pts, max_iters=max_iters, tol=1e-6, max_move=0.05)
    lo, hi = pts - torch.tensor(0.05), pts + torch.tensor(0.05)
    assert torch.equal(r["xyz_out"][0], torch.stack([lo[0, 0], pts[0, 1], pts[0, 2]]))
    assert torch.equal(r["xyz_out"][1, 1], hi[1, 1]) and torch.equal(r["xyz_out"][2, 2], hi[2, 2])
    assert (r["status"][:3] == pj.SPENT).all() and (r["evals"][:3] == max_iters + 1).all()
    assert r["status"][3] == pj.CONVERGED                       # (inside the box: reached)
    assert ((r["xyz_out"] >= lo) & (r["xyz_out"] <= hi)).all()
    assert int(r["evals"].max()) <= max_iters + 1


def test_bad_rules_and_the_empty_list():
    pts = _points(3, 6)
    for bad in ({"max_iters": -1}, {"tol": -1e-6}, {"tol": float("nan")}, {"max_move": 0.0}, {"min_grad2": 0.0}, {"max_move": float("nan")}):
        with pytest.raises(ValueError):
            pj.project_lockstep(_sphere(0.8), pts, **bad)
    r = pj.project_lockstep(_sphere(0.8), pts[:0])
    assert r["xyz_out"].shape == (0, 3) and r["status"].shape == (0,) and r["status"].dtype == torch.int32


def _box_slack(pts):
    """What fp32 adds to a distance from the input: the box faces x0 -+ max_move and the difference taken here are rounded once each."""
    return 2 * np.finfo(np.float32).eps * float(np.abs(pts).max() + 1.0)


# ---- 2. the GPU sets, on the reference alone ---------------------------------------------------------------------------------------------
def test_the_vertex_sets_are_the_ones_the_figures_were_taken_on():
    for key, count in pc.VERTEX_COUNTS.items():
        v = pc.vertices(*key)
        N, lo, hi = pc.LATTICES[key]
        assert v.shape == (count, 3) and v.dtype == np.float32 and (v >= lo).all() and (v <= hi).all()


@pytest.mark.parametrize("label", pc.TRUTH_LABELS)
def test_every_point_of_the_sets_converges_on_the_reference(label):
    _, tag, head, pts = next(s for s in pc.truth_sets() if s[0] == label)
    r = pc.reference(label)
    before, after = np.abs(pc.sdf64(tag, pc.SAMPLE, pts)[head]), np.abs(pc.sdf64(tag, pc.SAMPLE, r["xyz_out"])[head])
    print("SDFPROJECT reference %s: CONVERGED %d of %d, evals mean %.2f max %d, fp64 |sdf| before median %.3g max %.3g, after median %.3g "
          "max %.3g" % (label, (r["status"] == pj.CONVERGED).sum(), len(pts), r["evals"].mean(), r["evals"].max(), np.median(before),
                        before.max(), np.median(after), after.max()))
    assert (r["status"] == pj.CONVERGED).all()
    assert r["evals"].max() <= 9 and (np.abs(r["sdf"]) <= pc.TOL).all()
    assert np.abs(r["xyz_out"] - pts).max() <= pc.voxel(tag, head) + _box_slack(pts)
    # fp64 truth at the returned points: the tolerance plus the fp32 chain's own error there
    assert after.max() <= pc.TOL + np.abs(r["sdf"].astype(np.float64) - pc.sdf64(tag, pc.SAMPLE, r["xyz_out"])[head]).max()
    assert np.median(before) >= 100 * np.median(after)


@pytest.mark.parametrize("rule", ["3/1", "8/0.1"])
def test_the_short_and_the_clamped_variant_hold_both_outcomes(rule):
    label = pc.TRUTH_LABELS[0]
    r = pc.reference(label, rule)
    n = np.bincount(r["status"], minlength=4)
    print("SDFPROJECT reference %s rule %s: CONVERGED %d SPENT %d STALLED %d BAD %d" % (label, rule, *n))
    assert n[pj.CONVERGED] > 0 and n[pj.SPENT] > 0 and n[pj.STALLED] == 0 and n[pj.BAD] == 0
    rl = pc.rules()[rule]
    assert r["evals"].max() <= rl["max_iters"] + 1
    assert np.abs(r["xyz_out"] - pc.truth_sets()[0][3]).max() <= rl["max_move"] + _box_slack(pc.truth_sets()[0][3])
