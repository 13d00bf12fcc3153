"""K7 (csrc/icp.hip: brute-force and uniform-grid nearest neighbours, ICP update / solve, Chamfer reduction, grid build, the
continuation of a run) and K9's normalisation against host truths at their edges: runs longer than the first batch, the search
mode a run remembers, cell counts at the scan's round boundaries and at the resolution cap, boxes without extent, shell walks
through empty cells, queries outside the box, exact ties against the first-minimum rule on the host, reduction sizes at the
workgroup and grid-cap boundaries.  Every test asserts the premise it is about (iterations, restated cell counts, tied queries,
boundary sizes), so a changed generator cannot quietly turn it into a benign case.

Truths: oracle/icp_oracle.py (cKDTree where no exact ties exist, nearest_first_min where they do); the cell counts come from
tests/icp_edge_cases.grid_cells, pinned on the CPU in tests/test_oracle_icp.py."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import icp_oracle
from tests import icp_edge_cases as ec

pytestmark = pytest.mark.gpu

BRUTE, GRID = 1, 2
_seen = {}


def _report(group, value, bar):
    """Print a deviation next to its bar (pytest -s shows it) and keep the largest per group for the summary line."""
    _seen[group] = (max(_seen.get(group, (0.0, bar))[0], float(value)), bar)
    print("[icp-edges] %s: %.3g (bar %g)" % (group, value, bar))


@pytest.fixture(scope="module", autouse=True)
def _largest_deviations():
    yield
    for group, (value, bar) in sorted(_seen.items()):
        print("[icp-edges] largest %s: %.3g (bar %g)" % (group, value, bar))


class _search:
    """asdf_icp_set_search(mode) for a block; mode 0 again afterwards, whatever happened inside."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from alignsdf_amd import _native
        _native.check(_native.lib().asdf_icp_set_search(self.mode), "asdf_icp_set_search")

    def __exit__(self, *exc):
        from alignsdf_amd import _native
        _native.lib().asdf_icp_set_search(0)


def _workspace_bytes(na, nb):
    from alignsdf_amd import _native
    nbytes = ctypes.c_size_t()
    _native.check(_native.lib().asdf_icp_workspace_bytes(na, nb, ctypes.byref(nbytes)), "asdf_icp_workspace_bytes")
    return nbytes.value


def _chamfer(a, b, mode, ws=None):
    """(a -> b, b -> a) mean squared nearest distances through asdf_chamfer under a search mode; a fresh workspace of exactly the
    reported size unless one is handed in."""
    from alignsdf_amd import _native
    L = _native.lib()
    with _search(mode):
        A, B = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        if ws is None:
            ws = torch.empty(_workspace_bytes(len(a), len(b)), dtype=torch.uint8, device="cuda")
        out = (ctypes.c_double * 2)()
        _native.check(L.asdf_chamfer(A.data_ptr(), len(a), B.data_ptr(), len(b), ws.data_ptr(), ws.numel(), out,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "asdf_chamfer")
        return out[0], out[1]


def _check_chamfer(a, b):
    """Both modes against cKDTree at the bar of tests/test_gpu_chamfer.py, and bit-equal to each other."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    b_to_a, a_to_b = icp_oracle.chamfer_sum(a, b)                 # (source = a: gen_to_gt is a -> b)
    got = {mode: _chamfer(a, b, mode) for mode in (GRID, BRUTE)}
    pairs = [(x, want) for mode in (GRID, BRUTE) for x, want in zip(got[mode], (a_to_b, b_to_a))]
    _report("chamfer / max(1, truth)", max(abs(x - want) / max(1.0, want) for x, want in pairs), 1e-12)
    _report("chamfer / truth", max(abs(x - want) / want if want > 0.0 else abs(x) for x, want in pairs), 1e-12)
    for x, want in pairs:
        assert abs(x - want) <= 1e-12 * max(1.0, want), (x, want, got)
    assert got[GRID] == got[BRUTE], got
    return got[GRID]


# ---- 2. runs longer than the first batch ---------------------------------------------------------------------------------------

LONG_RUNS = ((1025, 1100, 3, 25), (2048, 1024, 6, 22), (3000, 1500, 10, 19))        # (ns, nt, seed, the oracle's iterations)
_long_truth = {}


def _long_run(ns, nt, seed):
    """(src, tgt, verts, oracle result), computed once per case."""
    key = (ns, nt, seed)
    if key not in _long_truth:
        src, tgt, verts = ec.icp_pair(ns, nt, seed)
        _long_truth[key] = (src, tgt, verts, icp_oracle.icp_trans_scale(src, tgt, verts))
    return _long_truth[key]


def _assert_against_oracle(r, ref):
    from alignsdf_amd.icp import FIRST_BATCH
    assert r["iterations"] == ref["iterations"] and r["iterations"] > FIRST_BATCH, (r["iterations"], ref["iterations"])
    dev = max(abs(r["scale"] - ref["scale"]), np.abs(r["trans"] - ref["trans"]).max(), abs(r["all_scale"] - ref["all_scale"]),
              np.abs(r["all_trans"] - ref["all_trans"]).max(), np.abs(r["vertices"] - ref["vertices"]).max())
    _report("icp transform and vertices", dev, 1e-9)
    _report("icp error", abs(r["error"] - ref["errors"][-1]), 1e-12)
    assert abs(r["scale"] - ref["scale"]) <= 1e-9 and np.abs(r["trans"] - ref["trans"]).max() <= 1e-9
    assert abs(r["all_scale"] - ref["all_scale"]) <= 1e-9 and np.abs(r["all_trans"] - ref["all_trans"]).max() <= 1e-9
    assert np.abs(r["vertices"] - ref["vertices"]).max() <= 1e-9
    assert abs(r["error"] - ref["errors"][-1]) <= 1e-12


def _same_run(r, one_shot):
    """A start_icp / finish_icp result against run_icp_f's (scale, trans, iterations, error): the same bits."""
    return (r["scale"] == one_shot[0] and np.array_equal(r["trans"], one_shot[1]) and r["iterations"] == one_shot[2]
            and r["error"] == one_shot[3])


def _same_result(r, q):
    return (r["scale"] == q["scale"] and np.array_equal(r["trans"], q["trans"]) and r["iterations"] == q["iterations"]
            and r["error"] == q["error"] and r["all_scale"] == q["all_scale"] and np.array_equal(r["all_trans"], q["all_trans"])
            and np.array_equal(r["vertices"], q["vertices"]))


@pytest.mark.parametrize("ns,nt,seed,iterations", LONG_RUNS)
def test_grid_run_continued_past_the_first_batch(ns, nt, seed, iterations):
    """finish_icp continues a run that has not converged after FIRST_BATCH iterations on a side stream
    (asdf_icp_ts_enqueue_range with first_iter > 0 attaching to the grids the first batch built).  Both sets have at least 1024
    points: the runs take the grid.  Against the oracle at the bars of tests/test_gpu_icp.py, and bit-equal to the one-shot
    asdf_icp_ts on the same normalised source (both enqueue the same two kernels per iteration in the same order)."""
    from alignsdf_amd.icp import FIRST_BATCH, icp_trans_scale, normalise_source, run_icp_f
    src, tgt, verts, ref = _long_run(ns, nt, seed)
    assert min(ns, nt) >= ec.FORCE_GRID_BELOW and ref["iterations"] == iterations > FIRST_BATCH
    r = icp_trans_scale(src, tgt, verts)
    _assert_against_oracle(r, ref)
    one_shot = run_icp_f(normalise_source(src, tgt)[0], tgt)
    assert _same_run(r, one_shot), (r, one_shot)


def test_grid_run_from_device_samples_continued_past_the_first_batch():
    """The same through start_icp_device (K9's normalisation in front): the oracle's iterations and transform, the one-shot run on
    the source K9 wrote bit for bit, K9's statistics against normalise_source at that function's 1e-12."""
    from alignsdf_amd.icp import finish_icp, normalise_source, run_icp_f, start_icp_device
    ns, nt, seed, _ = LONG_RUNS[2]
    src, tgt, verts, ref = _long_run(ns, nt, seed)
    job = start_icp_device(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda())
    r = finish_icp(job, verts)
    _assert_against_oracle(r, ref)
    moved = job.src.cpu().numpy()
    assert _same_run(r, run_icp_f(moved, tgt))
    want, (os_, ss, ot, st) = normalise_source(src, tgt)
    assert np.allclose(job.host[0].numpy(), np.concatenate([os_, [ss], ot, [st]]), rtol=1e-12, atol=1e-15)
    assert np.abs(moved - want).max() <= 1e-12


def test_continuation_keeps_the_search_mode_its_run_began_with():
    """A run begun under brute force with a workspace of exactly the size reported then, continued after asdf_icp_set_search(2):
    it must go on as a brute-force run (the all-brute result bit for bit).  Were the mode read again at the continuation, the grid
    layout would not fit the workspace and the library would refuse with ASDF_ENOSPC - an error from finish_icp, never a walk
    over grids nobody built.  And the reverse: begun on the grid, continued under mode 1, equal to the all-grid run."""
    from alignsdf_amd.icp import FIRST_BATCH, finish_icp, icp_trans_scale, start_icp
    ns, nt, seed, _ = LONG_RUNS[1]
    src, tgt, verts, ref = _long_run(ns, nt, seed)
    whole = {}
    for mode in (BRUTE, GRID):
        with _search(mode):
            whole[mode] = icp_trans_scale(src, tgt, verts)
            _assert_against_oracle(whole[mode], ref)
    assert _same_result(whole[BRUTE], whole[GRID])
    from alignsdf_amd import _native
    L = _native.lib()
    for begin, later in ((BRUTE, GRID), (GRID, BRUTE)):
        try:
            _native.check(L.asdf_icp_set_search(begin), "asdf_icp_set_search")
            begun_bytes = _workspace_bytes(ns, nt)
            job = start_icp(src, tgt)
            assert job.ws.numel() == begun_bytes
            _native.check(L.asdf_icp_set_search(later), "asdf_icp_set_search")
            later_bytes = _workspace_bytes(ns, nt)
            assert (later_bytes > begun_bytes) == (later == GRID) and later_bytes != begun_bytes
            r = finish_icp(job, verts)
        finally:
            L.asdf_icp_set_search(0)
        assert r["iterations"] == ref["iterations"] > FIRST_BATCH
        assert _same_result(r, whole[begin]), (begin, later)


# ---- 3. grid construction at its boundaries ------------------------------------------------------------------------------------

def _queries(n, seed):
    """Uniform points of a cube a tenth larger on every side than the unit cube: most inside the reference box, some outside."""
    return np.ascontiguousarray(ec.syn.uniform((n, 3), seed, -0.1, 1.1))


@pytest.mark.parametrize("n", sorted(ec.CUBES))
def test_grid_cell_count_at_the_scan_round(n):
    """grid_scan_kernel is one workgroup scanning 4096 cells per round with 16-byte loads: 15^3 cells stay under one round, 16^3
    are one round exactly, 17^3 a round and a tail whose last vector straddles the cell count."""
    res = ec.CUBES[n]
    ref = ec.box_points(n, n)
    assert ec.grid_cells(ref)[2:] == ((res, res, res), res ** 3)
    assert res ** 3 == {1024: 3375, 1200: ec.SCAN_ROUND, 1500: ec.SCAN_ROUND + 817}[n] and 817 % 4 == 1
    _check_chamfer(_queries(1100, 900 + n), ref)
    _check_chamfer(ref, ec.box_points(1300, 901 + n))            # the other argument order, both sets span the cube


def test_grid_of_a_flat_box():
    ref = ec.box_points(30000, 5, (1.0, 0.5, 0.25))
    assert ec.grid_cells(ref)[2] == (47, 24, 12)
    _check_chamfer(_queries(4000, 41) * np.array([1.0, 0.5, 0.25]), ref)


def test_grid_at_the_resolution_cap():
    ref = ec.box_points(76000, 6)
    assert ec.grid_cells(ref)[0] == ec.GRID_MAX_RES and ec.grid_cells(ref)[2:] == ((64, 64, 64), 64 ** 3)
    _check_chamfer(_queries(3000, 42), ref)


@pytest.mark.parametrize("case", ["equal", "planar", "collinear", "one_point", "five_points"])
def test_grid_of_a_box_without_extent(case):
    """All reference points equal (h = 1, one cell), exactly planar and exactly collinear sets (one cell along the flat axes), a
    single reference point and five of them with the grid forced.  cKDTree's distances are exact whatever the ties."""
    ref = ec.box_points(1000, 7)
    if case == "equal":
        ref[:] = [0.3, -0.2, 0.7]
        cells = (1, 1, 1)
    elif case == "planar":
        ref[:, 2] = 0.25
        cells = (15, 15, 1)
    elif case == "collinear":
        ref[:, 1], ref[:, 2] = -0.5, 0.25
        cells = (15, 1, 1)
    elif case == "one_point":
        ref, cells = ref[5:6].copy(), (1, 1, 1)
    else:
        ref, cells = ref[5:10].copy(), None
    if cells is not None:
        assert ec.grid_cells(ref)[2] == cells
    else:
        assert len(ref) == 5 and ec.grid_cells(ref)[0] == 4
    _check_chamfer(_queries(700, 43), ref)
    _check_chamfer(ref, ref)


def test_grid_walk_through_a_hollow_interior():
    """Queries in the hollow of a sphere of reference points: the shell walk doubles r = 1, 2, 4, ... through empty cells (the
    sphere is 20 cells away), then the box of the distance found leaves the block scanned and is scanned as a whole.  The other
    direction: 20 000 queries far outside the small box of the 4000."""
    ref = ec.sphere_points(20000, 44, 0.4)
    res, h, g, _ = ec.grid_cells(ref)
    assert 0.4 / h > 16 and min(g) >= res - 1                    # more than four doublings from the centre to the surface
    inner = np.concatenate([ec.syn.uniform((2000, 3), 45, -0.02 / np.sqrt(3.0), 0.02 / np.sqrt(3.0)), ec.sphere_points(2000, 46, 0.05)])
    assert np.linalg.norm(inner[:2000], axis=1).max() <= 0.02
    _check_chamfer(inner, ref)


@pytest.mark.parametrize("shift", [(3.0, 0.0, 0.0), (0.0, 3.0, 0.0), (0.0, 0.0, 3.0), (3.0, 3.0, 3.0), (-3.0, 0.0, 0.0)])
def test_grid_queries_outside_the_box(shift):
    """Queries three box lengths outside along one axis only (their cell is clamped along that axis alone) and along all three."""
    ref = ec.box_points(1500, 1500)
    assert ec.grid_cells(ref)[2] == (17, 17, 17)
    _check_chamfer(ec.box_points(1200, 1200) + np.array(shift), ref)


def test_one_workspace_reused_across_runs_and_modes():
    """One buffer sized for the largest case: a grid run, a smaller brute-force run, the grid run again - each the result of a fresh
    workspace bit for bit (counts are zeroed per run, nothing of the previous layout is read)."""
    big = (ec.box_points(1500, 1500), _queries(1300, 47))
    small = (_queries(300, 48), ec.box_points(1024, 1024)[:500])
    fresh_big, fresh_small = _chamfer(*big, GRID), _chamfer(*small, BRUTE)
    with _search(GRID):
        nbytes = _workspace_bytes(len(big[0]), len(big[1]))
    with _search(BRUTE):
        assert nbytes > _workspace_bytes(len(small[0]), len(small[1]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ws.fill_(0xff)                                               # (nothing may rely on a zeroed buffer either)
    assert _chamfer(*big, GRID, ws=ws) == fresh_big
    assert _chamfer(*small, BRUTE, ws=ws) == fresh_small
    assert _chamfer(*big, GRID, ws=ws) == fresh_big
    assert _chamfer(*small, GRID, ws=ws) == fresh_small


# ---- 4. the tie rule against the host ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["lattice", "duplicates"])
def test_tie_rule_is_the_first_minimum_of_the_host_scan(case):
    """Lattice points against the lattice shifted by half a cell: every coordinate, difference and squared distance is exact, an
    interior query has eight tied neighbours, and the rule is the brute-force scan's - the lowest index.  Two ICP iterations
    (stopping rules off) against oracle.run_icp_f(nearest=nearest_first_min): any other tied neighbour moves sum Y by a lattice
    step per query, far outside 1e-9.  `duplicates`: every reference point present twice."""
    from alignsdf_amd.icp import run_icp_f
    a, b = ec.tie_lattice()
    assert len(a) == 1728
    if case == "duplicates":
        b = np.ascontiguousarray(np.concatenate([b, b[::-1]]))    # the second copy in reverse order: index order is not lattice order
    d2 = icp_oracle.nearest_first_min(a, b)[0]
    tied = ec.tied_queries(a, b, d2)
    assert tied > 1000 and (case == "lattice" or tied == len(a)), tied
    want = icp_oracle.run_icp_f(a, b, max_iter=2, stop_error=0.0, stop_improvement=-1.0, nearest=icp_oracle.nearest_first_min)
    assert want[2] == 2
    got = {}
    for mode in (BRUTE, GRID):
        with _search(mode):
            got[mode] = run_icp_f(a, b, max_iter=2, stop_error=0.0, stop_improvement=-1.0)
        s, t, iters, error = got[mode]
        _report("icp transform on exact ties", max(abs(s - want[0]), np.abs(t - want[1]).max()), 1e-9)
        assert iters == 2 and abs(s - want[0]) <= 1e-9 and np.abs(t - want[1]).max() <= 1e-9, (mode, s, t, want)
        assert abs(error - want[3][-1]) <= 1e-12
    assert got[BRUTE][0] == got[GRID][0] and np.array_equal(got[BRUTE][1], got[GRID][1]) and got[BRUTE][2:] == got[GRID][2:]


# ---- 5. reduction boundaries ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("total,mode", [(255, 0), (256, 0), (257, 0), (16383, 0), (16384, 0), (16385, 0),
                                        (16383, BRUTE), (16384, BRUTE), (16385, BRUTE)])
def test_icp_update_at_the_workgroup_and_grid_cap_boundaries(total, mode):
    """icp_update_kernel: one workgroup per 256 queries up to 64 workgroups, grid-stride beyond, a 64-lane butterfly over the block
    sums.  ns + nt one below, at and one above 256 (one block) and 64 * 256 (the cap), split unevenly; the large totals on the
    grid (mode 0 with both sets >= 1024) and under brute force."""
    from alignsdf_amd.icp import icp_trans_scale
    ns = total // 3
    nt = total - ns
    edge = ec.UPDATE_THREADS if total < 1000 else ec.UPDATE_THREADS * ec.UPDATE_GRID
    assert abs(total - edge) <= 1 and ns != nt and (total < 1000 or min(ns, nt) >= ec.FORCE_GRID_BELOW)
    src, tgt, verts = ec.icp_pair(ns, nt, 20)
    ref = icp_oracle.icp_trans_scale(src, tgt, verts, max_iter=3)
    with _search(mode):
        r = icp_trans_scale(src, tgt, verts, max_iter=3)
    assert r["iterations"] == ref["iterations"]
    dev = max(abs(r["scale"] - ref["scale"]), np.abs(r["trans"] - ref["trans"]).max(), abs(r["all_scale"] - ref["all_scale"]),
              np.abs(r["all_trans"] - ref["all_trans"]).max(), np.abs(r["vertices"] - ref["vertices"]).max())
    _report("icp transform and vertices", dev, 1e-9)
    _report("icp error", abs(r["error"] - ref["errors"][-1]), 1e-12)
    assert dev <= 1e-9
    assert abs(r["error"] - ref["errors"][-1]) <= 1e-12


@pytest.mark.parametrize("na,nb", [(256, 256), (512, 257), (255, 1), (1, 255)])
def test_chamfer_reduction_at_block_boundaries(na, nb):
    """chamfer_reduce_kernel gives blocks [0, ceil(na / 256)) to the a -> b queries: na a multiple of 256 (no partial block before
    the boundary), one point over, and single-point sets on either side."""
    a = ec.syn.normal((na, 3), 500 + na) * 7.0
    b = ec.syn.normal((nb, 3), 600 + nb) * 7.0 + 0.5
    _check_chamfer(a, b)


# ---- 6. K9's normalisation below and around its workgroup ----------------------------------------------------------------------

@pytest.mark.parametrize("ns,nt", [(2, 3), (1023, 1025), (1024, 7), (5000, 1024)])
def test_device_normalisation_below_and_around_its_workgroup(ns, nt):
    """asdf_icp_normalise is one 1024-thread workgroup: sets smaller than it, one under / over, unequal sizes.  The bars of
    tests/test_gpu_icp.py::test_device_normalisation_equals_the_host_normalisation."""
    from alignsdf_amd.icp import finish_icp, normalise_source, start_icp_device
    ps = ec.syn.normal((ns, 3), 700 + ns) * [0.3, 0.2, 0.5] + [0.1, -0.2, 0.05]
    pt = ec.syn.normal((nt, 3), 710 + nt) * [0.4, 0.25, 0.6] + [0.5, -0.1, -0.25]
    want, (os_, ss, ot, st) = normalise_source(ps, pt)
    runs = []
    for _ in range(2):
        job = start_icp_device(torch.from_numpy(ps).cuda(), torch.from_numpy(pt).cuda(), max_iter=1)
        finish_icp(job, ps[:2])
        runs.append((job.src.cpu().numpy(), job.host[0].numpy().copy()))
    got, stats = runs[0]
    assert got.shape == (ns, 3)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    truth = np.concatenate([os_, [ss], ot, [st]])
    _report("normalisation statistics, relative", np.abs(stats / truth - 1.0).max(), 1e-12)
    _report("normalised points / coordinate magnitude", np.abs(got - want).max() / np.abs(want).max(), 1e-12)
    assert np.allclose(stats, truth, rtol=1e-12, atol=1e-15)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
