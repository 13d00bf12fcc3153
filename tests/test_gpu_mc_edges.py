"""K3-K6 (csrc/mc33.hip: mc_classify, mc_finalize, mc_emit_verts, mc_emit_faces) and alignsdf_amd/marching_cubes.py against the
sequential oracle (oracle/mc33.py, itself pinned to skimage bit for bit by tests/test_oracle_mc.py) at the edges of the layout
wrapped around the cells: row tails and the scalar fall-back, a misaligned base pointer, the long sum over a super-block's blocks,
the voxels the min / max gather takes from rows 1 - 3 and from the fifth element, levels next to and between voxel values, the
bounded emit at its capacities, workspaces reused across volumes, blocks full of active cells, the ABI's refusals.

The assertion is the project's for marching cubes everywhere: arrays of equal shape, np.array_equal on faces and on vertices.
There is no tolerance in this file.  The shapes and volumes live in tests/mc_edge_cases.py; tests/test_mc_edge_cases.py pins on
the CPU that they reach the branches named here.

Out of reach of any test: the second round of mc_finalize's loop over super-blocks (more than 1024 super-blocks, i.e. more than
2^30 cell slots).  Out of scope: NaN or +-inf voxels, which are not part of skimage's contract; every input here is finite."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import mc33
from tests import mc_edge_cases as ec

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC = -1, -5
_truth = {}


def _oracle(key, vol, level):
    """The oracle's (verts, faces) for a volume, computed once per key."""
    if key not in _truth:
        _truth[key] = mc33.marching_cubes_raw(vol, level)
    return _truth[key]


def _device(vol):
    return torch.as_tensor(np.ascontiguousarray(vol, dtype=np.float32)).cuda()


def _assert_equal(got, want, what=None):
    v, f = got
    rv, rf = want
    assert v.shape == rv.shape and f.shape == rf.shape, (what, v.shape, rv.shape, f.shape, rf.shape)
    assert v.dtype == rv.dtype and f.dtype == rf.dtype, what
    assert np.array_equal(f, rf), what
    assert np.array_equal(v, rv), what


def _hip_mc(vol, level):
    from alignsdf_amd.marching_cubes import marching_cubes_lewiner
    return marching_cubes_lewiner(vol if isinstance(vol, torch.Tensor) else _device(vol), level)


def _id(shape):
    return "x".join(str(n) for n in shape)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _workspace_bytes(shape):
    from alignsdf_amd import _native
    nbytes = ctypes.c_size_t()
    _native.check(_native.lib().asdf_mc_workspace_bytes(shape[0], shape[1], shape[2], ctypes.byref(nbytes)), "asdf_mc_workspace_bytes")
    return nbytes.value


def _key_float(k):
    """key_float of csrc/mc33.hip restated: the float whose order-preserving key is k."""
    k = int(k) & 0xFFFFFFFF
    b = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)
    return float(np.array([b], np.uint32).view(np.float32)[0])


def _count(vol_t, level, ws, record=None):
    """asdf_mc_count_enqueue into `ws`; returns the pinned record (V, F, min key, max key) as uint32 after a synchronisation."""
    from alignsdf_amd import _native
    if record is None:
        record = torch.zeros(4, dtype=torch.int32).pin_memory()
    s = vol_t.shape
    _native.check(_native.lib().asdf_mc_count_enqueue(vol_t.data_ptr(), s[0], s[1], s[2], ctypes.c_double(level), ws.data_ptr(),
                                                      ws.numel(), record.data_ptr(), _stream()), "asdf_mc_count_enqueue")
    torch.cuda.synchronize()
    return record.numpy().view(np.uint32).copy()


# ---- A. row tails and thin shapes -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ec.FIELDS))
@pytest.mark.parametrize("shape", ec.ROW_TAIL_SHAPES, ids=_id)
def test_row_tails_and_thin_shapes(shape, name):
    """mc_classify's loads (mc33.hip: the float4 rows + the neighbour lane's first value by DPP, `own5` for lane 63 and a row's
    last group, the scalar rows when nx % 4 != 0), `ncell` of a row's last group, cell_coords' reciprocal division, rows that span
    blocks."""
    vol, level = ec.field(name, shape)
    _assert_equal(_hip_mc(vol, level), _oracle(("A", name, shape), vol, level))


# ---- B. misaligned base pointer ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", ec.MISALIGNED_OFFSETS)
@pytest.mark.parametrize("shape", ec.MISALIGNED_SHAPES, ids=_id)
def test_misaligned_base_pointer(shape, offset):
    """A contiguous view `offset` floats into a larger buffer: nx % 4 == 0 but ((size_t)vol & 15) != 0, so mc_classify must take its
    scalar rows (`vec` false) - marching_cubes_begin keeps the view, .contiguous() is a no-op on it."""
    from alignsdf_amd.marching_cubes import marching_cubes_begin, marching_cubes_finish
    for name in sorted(ec.FIELDS):
        host, level = ec.field(name, shape)
        n = host.size
        buf = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")      # (a read outside the view would meet NaN)
        assert buf.data_ptr() % 16 == 0
        buf[offset:offset + n] = torch.from_numpy(host.reshape(-1)).cuda()
        vol = buf[offset:offset + n].view(shape)
        assert vol.is_contiguous() and vol.data_ptr() % 16 == 4 * offset != 0
        ticket = marching_cubes_begin(vol, level)
        assert ticket[0].data_ptr() == vol.data_ptr()                                     # no copy was made
        v, f = marching_cubes_finish(ticket)
        _assert_equal((v.cpu().numpy(), f.cpu().numpy()), _oracle(("A", name, shape), host, level), (name, offset))


def test_permuted_view():
    """A non-contiguous view is copied by marching_cubes_begin: the mesh of the permuted array, not of its storage."""
    host = ec.dense(ec.PERMUTED_SHAPE, ec.shape_seed(ec.PERMUTED_SHAPE))
    vol = _device(host).permute(*ec.PERMUTATION)
    assert not vol.is_contiguous()
    moved = np.transpose(host, ec.PERMUTATION)
    _assert_equal(_hip_mc(vol, 0.0), _oracle(("B", "permuted"), moved, 0.0))


# ---- C. long super-blocks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ec.LONG_SUPER_FIELDS)
@pytest.mark.parametrize("shape", ec.LONG_SUPER_SHAPES, ids=_id)
def test_long_super_blocks(shape, name):
    """sb_shift == 7: super-blocks of 128 blocks, so block_first_ids' 64-strided sum over the blocks in front of a block takes two
    rounds, mc_finalize sums 128 block records per super-block and the last super-block is a partial one; on the vector path (rows
    of more than 64 blocks) and on the scalar one.  two_ends: everything between the first and the last block is empty."""
    L = ec.layout(shape)
    assert L["sb_shift"] == 7 and L["nblocks"] > 4096
    vol, level = ec.long_super_volume(name, shape)
    _assert_equal(_hip_mc(vol, level), _oracle(("C", name, shape), vol, level))


# ---- D. where the extreme value sits ----------------------------------------------------------------------------------------------

EXTREME_CASES = [pytest.param(s, p, id="%s-%s" % (_id(s), label)) for s in ec.EXTREME_SHAPES for label, p in ec.extreme_positions(s)]
_workspaces = {}


def _workspace(shape):
    if shape not in _workspaces:
        _workspaces.clear()
        _workspaces[shape] = torch.empty(_workspace_bytes(shape), dtype=torch.uint8, device="cuda")
    return _workspaces[shape]


@pytest.mark.parametrize("shape,pos", EXTREME_CASES)
def test_min_max_record_wherever_the_extreme_sits(shape, pos):
    """mc_classify gathers min / max from elements 0..3 of row 0 of every thread, rows 1 / 2 / 3 of the threads next to the last row
    / slice, and the fifth element at a row tail; mc_finalize reduces the block records.  The record of asdf_mc_count_enqueue must
    decode to the volume's min and max exactly, with the only maximum (then the only minimum) at `pos`."""
    ws = _workspace(shape)
    for value in (1.0, -1.0):
        host = ec.extreme_noise(shape, pos, value)
        rec = _count(_device(host), 0.0, ws)
        lo, hi = _key_float(rec[2]), _key_float(rec[3])
        print("[mc-edges] %s %s %+g: min %r (volume %r) max %r (volume %r)" % (_id(shape), pos, value, lo, float(host.min()), hi,
                                                                               float(host.max())))
        assert lo == float(host.min()) and hi == float(host.max()), (value, lo, hi, float(host.min()), float(host.max()))


@pytest.mark.parametrize("shape,pos", EXTREME_CASES)
def test_one_corner_surface_wherever_it_sits(shape, pos):
    """-1 everywhere and +1 at `pos` (and the negation), level 0: a voxel the gather missed would turn the oracle's one-corner mesh
    into ValueError - the form in which it would reach a user."""
    for value in (1.0, -1.0):
        host = ec.one_corner(shape, pos, value)
        _assert_equal(_hip_mc(host, 0.0), _oracle(("D", shape, pos, value), host, 0.0), value)


# ---- E. levels --------------------------------------------------------------------------------------------------------------------

def test_levels_next_to_and_between_voxel_values():
    """`level_f`, the largest float <= level that mc_classify compares in fp32 in place of the double comparison, for levels that
    are a voxel value, lie between two adjacent floats, or next to a float among the doubles; and the emit's (double)c - level."""
    host = ec.ulp_volume()
    for sign in (1.0, -1.0):
        vol = _device(sign * host)
        for name, level in ec.ulp_levels():
            _assert_equal(_hip_mc(vol, sign * level), _oracle(("E", "ulp", sign, name), sign * host, sign * level), (sign, name))


def test_levels_around_zero_with_signed_zeros_and_denormals():
    """+-0 and fp32 denormals in the volume, +-0 and the smallest doubles as levels: no flush to zero anywhere on the way (the
    volume is built from bit patterns), level_f = -2^-149 for the level -2^-1074."""
    host = ec.zero_volume()
    vol = _device(host)
    assert np.array_equal(vol.cpu().numpy().view(np.uint32), host.view(np.uint32))
    for name, level in ec.ZERO_LEVELS:
        _assert_equal(_hip_mc(vol, level), _oracle(("E", "zero", name), host, level), name)


def _outcome(run):
    try:
        return ("mesh", run())
    except (ValueError, RuntimeError) as e:
        return (type(e), str(e))


def test_levels_at_and_beyond_the_data_range():
    """asdf_mc_result_status: level == max has no surface (RuntimeError), level == min has one, one double ulp outside either is
    ValueError - type and message of the oracle's outcome."""
    host = ec.range_volume()
    vol = _device(host)
    lo, hi = float(host.min()), float(host.max())
    expected = {"max": RuntimeError, "min": "mesh", "above_max": ValueError, "below_min": ValueError}
    levels = {"max": hi, "min": lo, "above_max": float(np.nextafter(hi, np.inf)), "below_min": float(np.nextafter(lo, -np.inf))}
    for name, level in levels.items():
        want, got = _outcome(lambda: mc33.marching_cubes_raw(host, level)), _outcome(lambda: _hip_mc(vol, level))
        assert want[0] == expected[name] and got[0] == want[0], (name, got, want)
        if want[0] == "mesh":
            _assert_equal(got[1], want[1], name)
        else:
            assert got[1] == want[1], (name, got, want)


# ---- F. bounded emit --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", [0, 1], ids=[n for n, _ in ec.bounded_volumes()])
def test_bounded_emit_writes_nothing_past_its_capacity(which):
    """mc_emit_verts' `id < cap_verts` and mc_emit_faces' `tri0 + ... >= cap_faces` guards, with buffers 64 rows longer than the
    true counts and pre-filled with a sentinel: rows below the capacity are the oracle's, every row from min(capacity, count) on
    still holds the sentinel.  With both capacities at or above the counts: asdf_mc_emit's result."""
    from alignsdf_amd import _native
    L = _native.lib()
    name, host = ec.bounded_volumes()[which]
    rv, rf = _oracle(("F", name), host, 0.0)
    V, F = len(rv), len(rf)
    vol = _device(host)
    s = vol.shape
    ws = torch.empty(_workspace_bytes(s), dtype=torch.uint8, device="cuda")
    rec = _count(vol, 0.0, ws)
    assert (int(rec[0]), int(rec[1])) == (V, F)
    rows_v, rows_f = V + ec.BOUNDED_SLACK_ROWS, F + ec.BOUNDED_SLACK_ROWS
    verts = torch.empty((rows_v, 3), dtype=torch.float32, device="cuda")
    faces = torch.empty((rows_f, 3), dtype=torch.int32, device="cuda")
    plain_v, plain_f = torch.empty((V, 3), dtype=torch.float32, device="cuda"), torch.empty((F, 3), dtype=torch.int32, device="cuda")
    _native.check(L.asdf_mc_emit(vol.data_ptr(), s[0], s[1], s[2], ctypes.c_double(0.0), ws.data_ptr(), ws.numel(), plain_v.data_ptr(),
                                 plain_f.data_ptr(), _stream()), "asdf_mc_emit")
    plain = (plain_v.cpu().numpy(), plain_f.cpu().numpy())
    _assert_equal(plain, (rv, rf), "asdf_mc_emit")
    for cap_v in ec.caps(V):
        for cap_f in ec.caps(F):
            verts.view(torch.int32).fill_(ec.VERT_SENTINEL)
            faces.fill_(ec.FACE_SENTINEL)
            _native.check(L.asdf_mc_emit_bounded(vol.data_ptr(), s[0], s[1], s[2], ctypes.c_double(0.0), ws.data_ptr(), ws.numel(),
                                                 verts.data_ptr(), cap_v, faces.data_ptr(), cap_f, _stream()), "asdf_mc_emit_bounded")
            v, f = verts.cpu().numpy(), faces.cpu().numpy()
            kv, kf = min(cap_v, V), min(cap_f, F)
            assert np.array_equal(v[:kv], rv[:kv]) and np.array_equal(f[:kf], rf[:kf]), (cap_v, cap_f)
            assert (v[kv:].view(np.uint32) == ec.VERT_SENTINEL).all(), (cap_v, cap_f, np.flatnonzero(v[kv:].view(np.uint32) != ec.VERT_SENTINEL)[:8])
            assert (f[kf:] == ec.FACE_SENTINEL).all(), (cap_v, cap_f, np.flatnonzero(f[kf:] != ec.FACE_SENTINEL)[:8])
            if cap_v >= V and cap_f >= F:
                _assert_equal((v[:V], f[:F]), plain, (cap_v, cap_f))


# ---- G. one workspace, many volumes -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ec.WORKSPACE_SHAPES, ids=_id)
def test_one_workspace_serves_many_volumes(shape):
    """One shape, one slot: dense, two_ends, checkerboard, dense again.  The compacted list, the id table and the block records of
    an earlier volume stay in the workspace; none of them may be read (block_seg's counts bound the list, every id an emitted face
    looks up was written by the same volume's mc_emit_verts).  Then the same through both slots, interleaved."""
    from alignsdf_amd.marching_cubes import marching_cubes_begin, marching_cubes_finish
    seq = ec.workspace_sequence(shape)
    want = {name: _oracle(("G", shape, name), vol, 0.0) for name, vol in seq}
    vols = {name: _device(vol) for name, vol in seq}
    for name, _ in seq:
        _assert_equal(_hip_mc(vols[name], 0.0), want[name], name)
    order = [name for name, _ in seq]
    for a, b in zip(order, order[1:] + order[:1]):
        t0 = marching_cubes_begin(vols[a], 0.0, slot=0)
        t1 = marching_cubes_begin(vols[b], 0.0, slot=1)
        assert t0[2].data_ptr() != t1[2].data_ptr()
        for name, t in ((a, t0), (b, t1)):
            v, f = marching_cubes_finish(t)
            _assert_equal((v.cpu().numpy(), f.cpu().numpy()), want[name], (a, b, name))


# ---- H. dense blocks --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", ec.DENSE_BLOCK_CASES, ids=["%s-%s" % (n, _id(s)) for n, s in ec.DENSE_BLOCK_CASES])
def test_blocks_full_of_active_cells(name, shape):
    """Blocks with up to 1024 active cells: 16 rounds of the emit wave with the carried base (wave_excl_scan), cells of 12 triangles
    and 13 owned vertices (the 4-bit counts of the cell code, all three tiling words, the cell-centre vertex), mc_classify's
    compaction with every thread holding four active cells."""
    vol = ec.dense_block_volume(name, shape)
    _assert_equal(_hip_mc(vol, 0.0), _oracle(("H", name, shape), vol, 0.0))


# ---- I. ABI edges -----------------------------------------------------------------------------------------------------------------

def test_abi_edges():
    """mc_layout's refusals (a dimension below 2, more than 2^31 voxels), a workspace one byte short (refused before anything is
    launched: the result record stays as it was), and the synchronous asdf_mc_count against the enqueue form's record."""
    from alignsdf_amd import _native
    L = _native.lib()
    nbytes = ctypes.c_size_t(12345)
    for dims in ec.BAD_DIMS + [ec.TOO_MANY_VOXELS]:
        assert L.asdf_mc_workspace_bytes(dims[0], dims[1], dims[2], ctypes.byref(nbytes)) == EINVAL, dims
        assert nbytes.value == 12345
    name, host = ec.bounded_volumes()[0]
    vol = _device(host)
    s = vol.shape
    total = _workspace_bytes(s)
    ws = torch.empty(total, dtype=torch.uint8, device="cuda")
    record = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32).pin_memory()
    rc = L.asdf_mc_count_enqueue(vol.data_ptr(), s[0], s[1], s[2], ctypes.c_double(0.0), ws.data_ptr(), total - 1, record.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == ENOSPC and (record.numpy() == 0x5A5A5A5A).all()
    for dims in ec.BAD_DIMS:
        assert L.asdf_mc_count_enqueue(vol.data_ptr(), dims[0], dims[1], dims[2], ctypes.c_double(0.0), ws.data_ptr(), total,
                                       record.data_ptr(), _stream()) == EINVAL, dims
    torch.cuda.synchronize()
    assert (record.numpy() == 0x5A5A5A5A).all()
    # the final check, the one launch of this test: both forms of the count phase give the oracle's sizes
    rec = _count(vol, 0.0, ws, record)
    nv, nf = ctypes.c_uint32(), ctypes.c_uint32()
    _native.check(L.asdf_mc_count(vol.data_ptr(), s[0], s[1], s[2], ctypes.c_double(0.0), ws.data_ptr(), total, ctypes.byref(nv),
                                  ctypes.byref(nf), _stream()), "asdf_mc_count")
    rv, rf = _oracle(("F", name), host, 0.0)
    assert (nv.value, nf.value) == (int(rec[0]), int(rec[1])) == (len(rv), len(rf))
    assert _key_float(rec[2]) == float(host.min()) and _key_float(rec[3]) == float(host.max())
