"""Pin the case tables of tests/mc_edge_cases.py, not the kernel: every branch of csrc/mc33.hip's layout machinery that
tests/test_gpu_mc_edges.py is written for must be reached by a listed shape (through the host restatement of mc_layout), and every
listed volume must give the sequential oracle a mesh worth comparing - so a later edit of the shapes cannot quietly stop reaching
a branch, or turn a case into an empty one."""
import numpy as np
import pytest

from oracle import mc33
from tests import mc_edge_cases as ec


def _mesh_ok(v, f):
    """Non-empty, every vertex used, every face index valid."""
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.ndim == 2 and v.shape[1] == 3 and f.shape[1] == 3
    assert len(v) > 0 and len(f) > 0
    assert f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)


def _same(a, b):
    return a[0].shape == b[0].shape and a[1].shape == b[1].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the layout restatement itself ------------------------------------------------------------------------------------------------

def test_layout_restates_the_documented_figures():
    """The figures csrc/mc33.hip and the project's records state for known shapes: 256^3 has 16 320 blocks in super-blocks of 128,
    the two long-super-block shapes have 4125 and 4152 blocks."""
    L = ec.layout((256, 256, 256))
    assert (L["cx"], L["cxp"], L["groups_per_row"]) == (255, 256, 64) and L["nslots"] == 256 * 255 * 255
    assert L["nblocks"] == 16257 and L["sb_shift"] == 7 and L["nsuper"] == 128 and L["vec"] and not L["has_tail"]
    assert ec.layout((2, 2, 2)) == {"cx": 1, "cy": 1, "cz": 1, "cxp": 4, "nslots": 4, "nblocks": 1, "sb_shift": 0, "nsuper": 1,
                                    "groups_per_row": 1, "vec": False, "has_tail": False}
    assert [ec.layout(s)["nblocks"] for s in ec.LONG_SUPER_SHAPES] == [4125, 4152]
    assert ec.CHUNK == ec.CLASSIFY_THREADS * ec.CELLS_PER_THREAD


# ---- every branch is reached by a listed shape ------------------------------------------------------------------------------------

def test_row_tail_shapes_reach_every_row_form():
    shapes = ec.ROW_TAIL_SHAPES
    assert len(shapes) == len(set(shapes)) == 21
    L = {s: ec.layout(s) for s in shapes}
    # each residue of the row length: the float4 path, the scalar path with the fifth-element tail, the two scalar paths whose last
    # group is partly outside the row
    for r in range(4):
        assert any(s[2] % 4 == r for s in shapes), r
    assert any(L[s]["vec"] for s in shapes) and any(L[s]["has_tail"] for s in shapes)
    # a vector row whose group count does not divide the wave: lane 63 falls inside a row and loads its own fifth value, and the
    # phase between rows and waves drifts from row to row
    assert any(L[s]["vec"] and ec.WAVE % L[s]["groups_per_row"] != 0 and L[s]["groups_per_row"] > ec.WAVE for s in shapes)
    assert any(L[s]["vec"] and L[s]["groups_per_row"] == ec.WAVE for s in shapes)               # ... and one that does, as 256^3
    assert any(L[s]["vec"] and L[s]["groups_per_row"] == ec.WAVE + 1 for s in shapes)           # ... and one group over
    # a row longer than one block, on the vector path
    assert any(L[s]["cxp"] > ec.CHUNK and L[s]["vec"] for s in shapes)
    assert any(L[s]["cxp"] > ec.CHUNK and L[s]["cxp"] % ec.CHUNK != 0 for s in shapes)          # (block edges drift through the rows)
    # one cell along each axis
    assert any(L[s]["cy"] == 1 for s in shapes) and any(L[s]["cz"] == 1 for s in shapes) and any(L[s]["cx"] == 1 for s in shapes)
    # more than one block, and a last block that is only partly filled
    assert any(L[s]["nblocks"] > 1 and L[s]["nslots"] % ec.CHUNK != 0 for s in shapes)
    # padding groups: rows whose last group holds no cell at all do not exist (cxp - cx <= 3), but groups with 1, 2, 3 cells do
    assert {L[s]["cx"] - (L[s]["cxp"] - 4) for s in shapes} == {1, 2, 3, 4}


def test_misaligned_shapes_would_take_the_vector_path():
    for s in ec.MISALIGNED_SHAPES:
        assert ec.layout(s)["vec"] and s in ec.ROW_TAIL_SHAPES, s        # (the same shapes are compared on the vector path in group A)
    assert sorted(ec.MISALIGNED_OFFSETS) == [1, 2, 3]                    # every residue of a 4-byte-aligned pointer modulo 16
    assert any(ec.layout(s)["nblocks"] > 1 for s in ec.MISALIGNED_SHAPES)
    assert sorted(ec.PERMUTATION) == [0, 1, 2] and tuple(ec.PERMUTATION) != (0, 1, 2)


def test_long_super_block_shapes_take_two_rounds_of_the_strided_sum():
    """block_first_ids adds the totals of the blocks in front of a block inside its super-block, 64 per round: more than one round
    needs super-blocks of more than 64 blocks, sb_shift >= 7, on both paths of mc_classify."""
    L = [ec.layout(s) for s in ec.LONG_SUPER_SHAPES]
    assert [l["sb_shift"] for l in L] == [7, 7] and [l["vec"] for l in L] == [True, False]
    for l in L:
        assert (1 << l["sb_shift"]) > ec.EMIT_WAVE and l["nblocks"] > (1 << l["sb_shift"]) + ec.EMIT_WAVE
        assert 1 < l["nsuper"] <= ec.FINALIZE_THREADS                    # (mc_finalize's second round is out of reach: 2^30 slots)
        assert l["nblocks"] % (1 << l["sb_shift"]) != 0                  # the last super-block is a partial one
    assert L[0]["cxp"] > 64 * ec.CHUNK                                   # rows of more than 64 blocks
    # the smallest: one block fewer than 4097 would be sb_shift 6
    assert all(ec.layout((9, 9, nx))["sb_shift"] == 6 for nx in (65000, 65536)) and ec.layout((161, 161, 161))["sb_shift"] == 6


def test_extreme_positions_cover_every_gathered_row():
    """mc_classify gathers min / max from row 0 of every thread plus rows 1 / 2 / 3 next to the last row / slice, and the fifth
    element at a row tail: the positions put the extreme on each of them, for every residue of the row length."""
    assert {s[2] % 4 for s in ec.EXTREME_SHAPES} == {0, 1, 2, 3}
    assert any(ec.layout(s)["cy"] == 1 and ec.layout(s)["cz"] == 1 for s in ec.EXTREME_SHAPES)
    assert any(ec.layout(s)["cx"] == 1 for s in ec.EXTREME_SHAPES)
    assert any(ec.layout(s)["vec"] and ec.layout(s)["groups_per_row"] > 1 for s in ec.EXTREME_SHAPES)
    for s in ec.EXTREME_SHAPES:
        pos = ec.extreme_positions(s)
        labels = [p[0] for p in pos]
        assert len(set(labels)) == len(pos) == int(np.prod([min(n, 3) for n in s]))
        assert len(pos) == 27 or min(s) == 2
        cells = {p[1] for p in pos}
        for z in (0, s[0] - 1):
            for y in (0, s[1] - 1):
                for x in (0, s[2] - 1):
                    assert (z, y, x) in cells                                # all eight corners of the volume
        for label, p in pos:
            for value in (1.0, -1.0):
                vol = ec.extreme_noise(s, p, value)
                assert (vol == value).sum() == 1 and (vol.max() if value > 0 else vol.min()) == value
                assert np.abs(np.delete(vol.reshape(-1), np.ravel_multi_index(p, s))).max() <= 0.5


def test_workspace_and_dense_block_shapes():
    for s in ec.WORKSPACE_SHAPES:
        assert ec.layout(s)["nblocks"] >= 2
    assert [ec.layout(s)["vec"] for s in ec.WORKSPACE_SHAPES] == [True, False]
    # blocks whose active cells need several rounds of the emit wave, the carried base between the rounds included
    for name, s in ec.DENSE_BLOCK_CASES:
        vol = ec.dense_block_volume(name, s)
        active = ec.cell_triangle_counts(vol, 0.0, mc33.marching_cubes_raw) > 0 if np.prod(s) < 5000 else None
        if active is not None:
            assert active.sum() > 4 * ec.EMIT_WAVE
    assert any(ec.layout(s)["nslots"] >= ec.CHUNK for _, s in ec.DENSE_BLOCK_CASES)


# ---- the oracle over every case ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ec.FIELDS))
def test_oracle_meshes_of_the_row_tail_shapes(name):
    for s in ec.ROW_TAIL_SHAPES:
        vol, level = ec.field(name, s)
        assert vol.shape == s and vol.dtype == np.float32 and np.isfinite(vol).all()
        _mesh_ok(*mc33.marching_cubes_raw(vol, level))
    vol = ec.dense(ec.PERMUTED_SHAPE, ec.shape_seed(ec.PERMUTED_SHAPE))
    moved = np.transpose(vol, ec.PERMUTATION)
    assert not moved.flags["C_CONTIGUOUS"]
    _mesh_ok(*mc33.marching_cubes_raw(moved, 0.0))
    assert not _same(mc33.marching_cubes_raw(moved, 0.0), mc33.marching_cubes_raw(vol, 0.0))


@pytest.mark.parametrize("shape", ec.LONG_SUPER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_meshes_of_the_long_super_block_shapes(shape):
    """smooth_noise has surface in blocks of every super-block; two_ends in the first and the last block only, one corner each."""
    L = ec.layout(shape)
    vol, level = ec.long_super_volume("smooth_noise", shape)
    v, f = mc33.marching_cubes_raw(vol, level)
    _mesh_ok(v, f)
    # vertices beyond the first super-block's cells and in the last one's: their bases come from mc_finalize and block_first_ids
    slots_per_super = ec.CHUNK << L["sb_shift"]
    slot = (np.floor(v[:, 0]) * L["cy"] + np.floor(v[:, 1])) * L["cxp"] + np.floor(v[:, 2])
    supers = np.unique((slot // slots_per_super).astype(np.int64))
    assert supers.min() == 0 and supers.max() >= L["nsuper"] - 1 and len(supers) >= L["nsuper"]
    vol, level = ec.long_super_volume("two_ends", shape)
    v, f = mc33.marching_cubes_raw(vol, level)
    _mesh_ok(v, f)
    assert (len(v), len(f)) == (12, 16)                                  # two octahedra
    first = ((0 * L["cy"] + 0) * L["cxp"] + 0) // ec.CHUNK
    last = (((shape[0] - 2) * L["cy"] + shape[1] - 2) * L["cxp"] + shape[2] - 2) // ec.CHUNK
    assert first == 0 and last == L["nblocks"] - 1


def test_oracle_meshes_of_the_one_corner_volumes():
    for s in ec.EXTREME_SHAPES:
        for label, p in ec.extreme_positions(s):
            got = {}
            for value in (1.0, -1.0):
                v, f = got[value] = mc33.marching_cubes_raw(ec.one_corner(s, p, value), 0.0)
                _mesh_ok(v, f)
                inside = sum(1 for c, n in zip(p, s) if 0 < c < n - 1)
                assert len(v) == 3 + inside and len(f) == (1, 2, 4, 8)[inside], (s, label)
            # the same surface from either side (the order of first reference, hence of the vertices, may differ)
            assert np.array_equal(np.unique(got[1.0][0], axis=0), np.unique(got[-1.0][0], axis=0))


def test_level_edge_volumes_give_different_meshes():
    """Levels on different sides of a voxel value give different sign patterns, hence different faces; levels on the same side
    differ by an ulp of a double in (value - level), which moves vertices between voxels that are both within 2 float ulps of the
    level.  The one pair that cannot differ is +0.0 against -0.0 (c > level is the same set and |c - level| the same number); the
    smallest positive double gives the same active cells as 0.0 but turns corners at exactly 0 into negative ones for the MC33
    deciders."""
    vol = ec.ulp_volume()
    assert vol.shape == ec.LEVEL_SHAPE_ULP and len(np.unique(vol)) == 9
    levels = ec.ulp_levels()
    assert len({l for _, l in levels}) == len(levels) == 6
    b = float(ec.B32)
    assert all((l < b) == (n in ec.ULP_LEVELS_BELOW_B) for n, l in levels) and 0.3 < b
    meshes = {n: mc33.marching_cubes_raw(vol, l) for n, l in levels}
    negated = {n: mc33.marching_cubes_raw(-vol, -l) for n, l in levels}
    for n, l in levels:
        _mesh_ok(*meshes[n])
        _mesh_ok(*negated[n])
        assert not np.array_equal(meshes[n][1], negated[n][1]) or meshes[n][1].shape != negated[n][1].shape
    for n, _ in levels:
        for m, _ in levels:
            if (n in ec.ULP_LEVELS_BELOW_B) != (m in ec.ULP_LEVELS_BELOW_B):
                assert meshes[n][1].shape != meshes[m][1].shape or not np.array_equal(meshes[n][1], meshes[m][1]), (n, m)
                assert negated[n][1].shape != negated[m][1].shape or not np.array_equal(negated[n][1], negated[m][1]), (n, m)
            elif n < m:
                assert not _same(meshes[n], meshes[m]), (n, m)
    vol = ec.zero_volume()
    assert vol.shape == ec.LEVEL_SHAPE_ZERO and vol.dtype == np.float32
    assert sorted(np.unique(vol.view(np.uint32)).tolist()) == sorted(ec.ZERO_BITS.tolist())      # +-0 and the denormals survived
    assert np.array_equal(ec.ZERO_BITS.view(np.float32)[[2, 4, 6]], np.array([1e-45, 1e-38, 1.0], np.float32))
    assert 0.0 < ec.ZERO_BITS.view(np.float32)[4] < np.finfo(np.float32).tiny
    meshes = {n: mc33.marching_cubes_raw(vol, l) for n, l in ec.ZERO_LEVELS}
    for n in meshes:
        _mesh_ok(*meshes[n])
    assert _same(meshes["+0"], meshes["-0"])
    assert not _same(meshes["+0"], meshes["+denorm"])                    # (a corner at 0 - 2^-1074 < 0 steers the MC33 deciders)
    assert not _same(meshes["+0"], meshes["-denorm"]) and not _same(meshes["+denorm"], meshes["-denorm"])
    assert meshes["-denorm"][1].shape != meshes["+0"][1].shape or not np.array_equal(meshes["-denorm"][1], meshes["+0"][1])


def test_range_volume_outcomes_of_the_oracle():
    vol = ec.range_volume()
    lo, hi = float(vol.min()), float(vol.max())
    with pytest.raises(RuntimeError, match="No surface found"):
        mc33.marching_cubes_raw(vol, hi)
    _mesh_ok(*mc33.marching_cubes_raw(vol, lo))
    for level in (np.nextafter(hi, np.inf), np.nextafter(lo, -np.inf)):
        with pytest.raises(ValueError, match="Surface level must be within volume data range"):
            mc33.marching_cubes_raw(vol, float(level))


def test_checkerboard_holds_cells_of_twelve_triangles():
    """Every cell of a checkerboard is MC33 case 13; its sub-cases run from 4 to 12 triangles, and the 12-triangle ones (13.4, 13.5
    with its interior vertex) are the maximum the cell code's 4-bit count and the three 64-bit tiling words must hold."""
    for name, s in ec.DENSE_BLOCK_CASES[:2]:
        vol = ec.dense_block_volume(name, s)
        above = vol > 0
        assert (above[1:] != above[:-1]).all() and (above[:, 1:] != above[:, :-1]).all() and (above[:, :, 1:] != above[:, :, :-1]).all()
        v, f = mc33.marching_cubes_raw(vol, 0.0)
        _mesh_ok(v, f)
        per_cell = ec.cell_triangle_counts(vol, 0.0, mc33.marching_cubes_raw)
        assert per_cell.min() >= 4 and per_cell.max() == 12 and per_cell.sum() == len(f)
        assert len(v) > len(np.unique(np.floor(v), axis=0))                  # more vertices than cells own on edges alone
    for _, vol in ec.bounded_volumes()[1:]:
        assert ec.cell_triangle_counts(vol, 0.0, mc33.marching_cubes_raw).max() == 12


def test_oracle_meshes_of_the_remaining_cases():
    for name, vol in ec.bounded_volumes():
        v, f = mc33.marching_cubes_raw(vol, 0.0)
        _mesh_ok(v, f)
        assert len(v) > ec.BOUNDED_SLACK_ROWS and len(f) > ec.BOUNDED_SLACK_ROWS
        assert ec.caps(len(v)) == [0, 1, len(v) - 1, len(v), len(v) + 1]
    for s in ec.WORKSPACE_SHAPES:
        seq = ec.workspace_sequence(s)
        assert [n for n, _ in seq] == ["dense", "two_ends", "checkerboard", "dense_again"]
        meshes = [mc33.marching_cubes_raw(vol, 0.0) for _, vol in seq]
        for m in meshes:
            _mesh_ok(*m)
        assert _same(meshes[0], meshes[3]) and len(meshes[1][1]) == 16 and len(meshes[2][1]) > len(meshes[0][1])
    for name, s in ec.DENSE_BLOCK_CASES:
        _mesh_ok(*mc33.marching_cubes_raw(ec.dense_block_volume(name, s), 0.0))
    for d in ec.BAD_DIMS:
        assert min(d) < 2
    assert int(np.prod(ec.TOO_MANY_VOXELS, dtype=np.int64)) > 2 ** 31
