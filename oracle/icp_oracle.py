"""CPU restatement of the reference's eval-mode translate+scale ICP.  TEST INFRASTRUCTURE ONLY.

Follows deep_sdf/metrics/icp_trans_scale.py step by step (ICP_T_S.sample_mesh :19-31 without the random sampling,
run_icp_f :33-113, get_trans_scale :188-191, export_source_mesh :193-196) in float64, with scipy's cKDTree in place of
sklearn's KDTree (both return the exact nearest neighbour) and the 4-unknown least-squares system solved in closed
form instead of np.linalg.lstsq (same minimiser).  Pinned by tests/test_oracle_icp.py against
tests/golden/ref_icp.npz, which is produced by the reference class itself (tests/golden/make_icp_goldens.py).
"""
import numpy as np
from scipy.spatial import cKDTree


def normalise_source(points_source, points_target):
    """sample_mesh's normalisation (:25-31): move / scale the source samples onto the target's centroid and RMS radius."""
    ps, pt = np.asarray(points_source, np.float64), np.asarray(points_target, np.float64)
    offset_s = ps.mean(0)
    scale_s = np.sqrt(((ps - offset_s) ** 2).sum() / len(ps))
    offset_t = pt.mean(0)
    scale_t = np.sqrt(((pt - offset_t) ** 2).sum() / len(pt))
    return (ps - offset_s) / scale_s * scale_t + offset_t, dict(offset_source=offset_s, scale_source=scale_s,
                                                                 offset_target=offset_t, scale_target=scale_t)


def solve_scale_trans(X, Y):
    """argmin_{s,t} sum |s X_i + t - Y_i|^2  (the system of :76-107)."""
    n = len(X)
    xm, ym = X.mean(0), Y.mean(0)
    s = ((X * Y).sum() - n * (xm * ym).sum()) / ((X * X).sum() - n * (xm * xm).sum())
    return s, ym - s * xm


def nearest_first_min(queries, refs, chunk_pairs=1 << 15):
    """Exhaustive nearest neighbour with the brute-force kernel's arithmetic and tie rule: per pair d = d0*d0 + d1*d1 + d2*d2 in
    that order in fp64 (the library is built with -ffp-contract=off: the same roundings), and argmin over the reference index,
    so of several equal minima the FIRST - the lowest index - wins.  cKDTree returns the same distances but an arbitrary one of
    tied neighbours.  Plain numpy, chunked over the queries (about `chunk_pairs` distances at a time: cache-sized, 30 000 x
    30 000 in about three seconds).  Returns (d2 [nq], idx [nq])."""
    q, r = np.asarray(queries, np.float64).reshape(-1, 3), np.asarray(refs, np.float64).reshape(-1, 3)
    r0, r1, r2 = (np.ascontiguousarray(r[:, a])[None, :] for a in range(3))
    d2, idx = np.empty(len(q)), np.empty(len(q), np.int64)
    step = max(1, chunk_pairs // max(1, len(r)))
    for lo in range(0, len(q), step):
        c = q[lo:lo + step]
        d = c[:, 0:1] - r0
        d *= d
        for col, ra in ((1, r1), (2, r2)):
            t = c[:, col:col + 1] - ra
            t *= t
            d += t
        k = d.argmin(1)
        idx[lo:lo + step] = k
        d2[lo:lo + step] = d[np.arange(len(c)), k]
    return d2, idx


def run_icp_f(points_source, points_target, max_iter=100, stop_error=1e-3, stop_improvement=1e-5, nearest=None):
    """ICP_T_S.run_icp_f on already normalised source samples.  Returns (scale, trans[3], iterations, errors).
    `nearest` (optional): a function (queries, refs) -> (squared distances, indices) that replaces the two KD-tree queries -
    nearest_first_min where the choice among exactly tied neighbours matters."""
    ps, pt = np.asarray(points_source, np.float64), np.asarray(points_target, np.float64)
    if nearest is None:
        tree_t, tree_s = cKDTree(pt), cKDTree(ps)
        nn_t, nn_s = (lambda q: tree_t.query(q)[1]), (lambda q: tree_s.query(q)[1])
    else:
        nn_t, nn_s = (lambda q: nearest(q, pt)[1]), (lambda q: nearest(q, ps)[1])
    scale, trans = 1.0, np.zeros(3)
    previous, errors, it = 1e8, [], 0
    for it in range(max_iter):
        q_s = ps * scale + trans
        idx_t = nn_t(q_s)
        ct = pt[idx_t]
        idx_s = nn_s((pt - trans) / scale)
        cs = ps[idx_s] * scale + trans
        error = np.sqrt((((q_s - ct) ** 2).sum() + ((pt - cs) ** 2).sum()) / (len(ps) + len(pt)))
        errors.append(error)
        if previous - error < stop_improvement:
            break
        previous = error
        if error < stop_error:
            break
        scale, trans = solve_scale_trans(np.concatenate([ps, ps[idx_s]]), np.concatenate([ct, pt]))
    return scale, trans, it + 1, errors


def icp_trans_scale(points_source, points_target, vertices, max_iter=100, nearest=None):
    """sample_mesh normalisation + run_icp_f + get_trans_scale + the vertex transform of export_source_mesh."""
    ps, n = normalise_source(points_source, points_target)
    scale, trans, iters, errors = run_icp_f(ps, points_target, max_iter, nearest=nearest)
    all_scale = n["scale_target"] * scale / n["scale_source"]
    all_trans = trans + n["offset_target"] * scale - n["offset_source"] * n["scale_target"] * scale / n["scale_source"]
    v = (np.asarray(vertices, np.float64) - n["offset_source"]) / n["scale_source"] * n["scale_target"] + n["offset_target"]
    return dict(scale=scale, trans=trans, iterations=iters, errors=errors, all_scale=all_scale, all_trans=all_trans,
                vertices=v * scale + trans)


def chamfer_sum(points_source, points_target):
    """The distance part of compute_trimesh_chamfer (deep_sdf/metrics/chamfer.py:217-229) with the same scipy cKDTree
    the reference imports: (gt_to_gen, gen_to_gt) mean squared nearest-neighbour distances; the metric is their sum."""
    ps, pt = np.asarray(points_source, np.float64), np.asarray(points_target, np.float64)
    one_distances, _ = cKDTree(ps).query(pt)
    gt_to_gen = np.mean(np.square(one_distances))
    two_distances, _ = cKDTree(pt).query(ps)
    gen_to_gt = np.mean(np.square(two_distances))
    return gt_to_gen, gen_to_gt
