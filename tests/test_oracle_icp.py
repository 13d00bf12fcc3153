"""Pin the ICP oracle against the reference's own ICP_T_S (tests/golden/ref_icp.npz), its first-minimum neighbour search against
cKDTree and its own definition, and the host restatement of the grid's cell choice (tests/icp_edge_cases.py)."""
import numpy as np
import pytest

from oracle import icp_oracle
from tests import icp_edge_cases as ec


@pytest.mark.parametrize("case", ["small", "noisy", "full30k"])
def test_icp_matches_reference_class(case, golden_dir):
    g = np.load(golden_dir + "/ref_icp.npz")
    r = icp_oracle.icp_trans_scale(g[case + ".src"], g[case + ".tgt"], g[case + ".verts"])
    assert abs(r["scale"] - g[case + ".scale"][0]) <= 1e-9
    assert np.abs(r["trans"] - g[case + ".trans"]).max() <= 1e-9
    assert abs(r["all_scale"] - g[case + ".all_scale"][0]) <= 1e-9
    assert np.abs(r["all_trans"] - g[case + ".all_trans"]).max() <= 1e-9
    assert np.abs(r["vertices"] - g[case + ".verts_out"]).max() <= 1e-9
    assert 2 <= r["iterations"] <= 100 and r["errors"][-1] < 0.01


def test_nearest_first_min_distances_equal_the_kd_tree():
    """The exhaustive first-minimum search returns cKDTree's nearest distances (the two roundings of a squared distance and its
    root apart) on random sets: sizes below, at and above its chunk, a single reference point."""
    from scipy.spatial import cKDTree
    for nq, nr, seed in ((1, 1, 1), (700, 1, 2), (513, 1100, 3), (3000, 4097, 4), (5, 40000, 5)):
        q, r = ec.syn.normal((nq, 3), 300 + seed) * 0.7, ec.syn.normal((nr, 3), 310 + seed) * 0.7 + 0.1
        d2, idx = icp_oracle.nearest_first_min(q, r)
        want, _ = cKDTree(r).query(q)
        assert d2.shape == (nq,) and idx.shape == (nq,) and idx.min() >= 0 and idx.max() < nr
        assert np.abs(np.sqrt(d2) - want).max() <= 4e-16 * max(1.0, want.max())
        assert np.array_equal(d2, ((q - r[idx]) ** 2).sum(1))          # the index is the point the distance belongs to
        assert np.array_equal(icp_oracle.nearest_first_min(q, r, chunk_pairs=1)[1], idx)


def test_nearest_first_min_takes_the_lowest_tied_index():
    """On the tie lattice every query's answer is the lowest index among the reference points at exactly the nearest distance,
    for both directions, and for a reference set that holds every point twice (the first copy wins)."""
    a, b = ec.tie_lattice()
    for q, r in ((a, b), (b, a), (a, np.concatenate([b, b])), (a, np.repeat(b, 2, axis=0))):
        d2, idx = icp_oracle.nearest_first_min(q, r)
        d = ((q[:, None, :] - r[None, :, :]) ** 2).sum(-1)
        assert np.array_equal(d2, d.min(1))
        lowest = np.array([np.flatnonzero(row == m)[0] for row, m in zip(d, d2)])
        assert np.array_equal(idx, lowest)
        assert ec.tied_queries(q, r, d2) > 1000
    assert ec.tied_queries(a, np.concatenate([b, b]), icp_oracle.nearest_first_min(a, np.concatenate([b, b]))[0]) == len(a)


@pytest.mark.parametrize("case", ["small", "noisy", "full30k"])
def test_icp_with_first_minimum_search_matches_reference_class(case, golden_dir):
    """run_icp_f(nearest=nearest_first_min) reproduces the reference class' goldens like the KD-tree form does: sampled surfaces
    have no exact ties, so the two searches pick the same neighbours."""
    g = np.load(golden_dir + "/ref_icp.npz")
    r = icp_oracle.icp_trans_scale(g[case + ".src"], g[case + ".tgt"], g[case + ".verts"], nearest=icp_oracle.nearest_first_min)
    assert abs(r["scale"] - g[case + ".scale"][0]) <= 1e-9
    assert np.abs(r["trans"] - g[case + ".trans"]).max() <= 1e-9
    assert abs(r["all_scale"] - g[case + ".all_scale"][0]) <= 1e-9
    assert np.abs(r["all_trans"] - g[case + ".all_trans"]).max() <= 1e-9
    assert np.abs(r["vertices"] - g[case + ".verts_out"]).max() <= 1e-9


def test_grid_cell_restatement_for_the_scan_boundaries():
    """tests/icp_edge_cases.grid_cells (grid_bbox_kernel's cell choice on the host) for the sets the GPU tests steer the cell scan
    with: cubes of 1024 / 1200 / 1500 points give 15^3 / 16^3 = one scan round exactly / 17^3 = a round and a tail of 817 cells
    (817 % 4 == 1), a 1 x 0.5 x 0.25 box of 30 000 points 47 x 24 x 12, 76 000 points the capped 64^3; degenerate boxes one cell
    along every axis without extent."""
    for n, res in ec.CUBES.items():
        assert ec.grid_cells(ec.box_points(n, n))[2:] == ((res, res, res), res ** 3)
    assert 16 ** 3 == ec.SCAN_ROUND and 17 ** 3 == ec.SCAN_ROUND + 817 and 17 ** 3 % 4 == 1
    assert ec.grid_cells(ec.box_points(30000, 5, (1.0, 0.5, 0.25)))[2] == (47, 24, 12)
    assert ec.grid_cells(ec.box_points(76000, 6))[2:] == ((64, 64, 64), 64 ** 3)
    flat = ec.box_points(1000, 7)
    flat[:, 2] = 0.25
    assert ec.grid_cells(flat)[2] == (15, 15, 1)
    flat[:, 1] = -0.5
    assert ec.grid_cells(flat)[2] == (15, 1, 1)
    assert ec.grid_cells(np.full((1000, 3), 0.3))[1:] == (1.0 + 1e-9, (1, 1, 1), 1)
    assert ec.grid_cells(np.zeros((1, 3)))[0] == 4 and ec.grid_cells(np.zeros((1, 3)))[3] == 1
