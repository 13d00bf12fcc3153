"""The record schedule of the W-form split-half kernel (csrc/sdf_mlp_f16w_kernel.h: stage16w) must not show in any value.

A record's six MFMAs carry the deferred epilogue of the previous tile in steps (accumulator reads, plane split, running maximum),
the LDS-DMA piece of the ring's refill and ONE explicit wait for the record's two A fragments.  A step cut at the wrong place, a
record paired with the wrong operands or a wait placed too late gives values that depend on where a voxel sits - its lane, its
tile's position in the sweep - or that change from run to run.  So, on the flagship's decoder (nerf3, both heads):

* the full sweep (sdf_mlp_f16w_kernel) against the voxel-list form (sdf_mlp_f16w_subset_kernel), bit for bit, at N = 8 (4 whole
  tiles) and N = 12 (1 728 voxels: 13 tiles and a half-filled one);
* the W form against the 32-wide form and the fp32 chain on the same lattices;
* the same N = 16 sweep twice.

The voxel lists.  The library's only entry to the list form is the band sweep (asdf_decode_grid_band): its list is the set of
voxels the allowance tau marks, in lattice order, followed - audit on - by voxels drawn at random.  There is no entry that takes a
caller's order and none that takes an allowance of 0.5 or more, so "every voxel, shuffled" is covered by what the entry can do: the
largest allowance (0.499) lists every voxel of a cell that reaches inside |sdf| < 0.499 (the lengths reached are printed), smaller
allowances give lists in which a voxel sits in another lane and another tile than in the full sweep, the audit's picks ride
behind them at random positions, and on a lattice off the surfaces
the allowance is steered to the list nearest to 130 voxels - one full tile plus two lanes - that unions of whole cells can reach."""
import numpy as np
import pytest
import torch

from alignsdf_amd import _native
from alignsdf_amd import synthetic as syn
from tests.test_gpu_split_half_fp64 import _band_marks, _taus_for

pytestmark = pytest.mark.gpu
REF = _native.GRID_REFERENCE
WG_PTS = 128


def _decoder(refine=0.0):
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    specs = syn.specs_for("nerf3")
    hip = HipSdfDecoder(syn.full_state_dict("nerf3"), 256, specs["PointFeatSize"], specs["EncodeStyle"])
    if refine is not None:
        hip.set_refine(refine)                  # 0: the arithmetic itself, not the near-level repair
    hip.set_sample(torch.from_numpy(syn.latent_code(0).reshape(-1)))
    return hip


@pytest.fixture
def mfma_shape():
    L = _native.lib()
    before = L.asdf_get_mfma_shape()
    yield lambda shape: L.asdf_set_mfma_shape(int(shape))
    L.asdf_set_mfma_shape(before)


def _cube(N):
    return [-1.0, -1.0, -1.0], 2.0 / (N - 1)


def _band(hip, N, origin, vs, tau):
    rec, bh, bo = hip._one_plane_launch(hip._L.asdf_decode_grid_band, "asdf_decode_grid_band", N, origin, vs, REF, True, True, tau)
    r = rec.cpu().numpy()
    assert r[7] == 0 and r[15] == 0, (r[7], r[15])
    return r, bh.cpu().numpy().reshape(-1), bo.cpu().numpy().reshape(-1)


def _one_plane(hip, N, origin, vs):
    """The one-plane values of the lattice: the scratch volumes of a box sweep with next to no candidates."""
    _, uh, uo = hip._one_plane_launch(hip._L.asdf_decode_grid_box, "asdf_decode_grid_box", N, origin, vs, REF, True, True, 1e-7)
    return uh.cpu().numpy().reshape(-1), uo.cpu().numpy().reshape(-1)


@pytest.mark.parametrize("N", [8, 12])
def test_full_sweep_is_the_list_form_bit_for_bit(N):
    hip = _decoder()
    assert hip.split_half_instance() == "sdf_mlp_f16w_kernel" and hip.split_half_instance(subset=True) == "sdf_mlp_f16w_subset_kernel"
    hip.set_audit(0)
    origin, vs = _cube(N)
    P = N ** 3
    assert (P % WG_PTS == 0) == (N == 8) and (N != 12 or P == 13 * WG_PTS + 64)
    vh, vo, bbox = hip.decode_grid(N, origin, vs, REF)
    assert hip.math == "f16x3"
    full = (vh.cpu().numpy().reshape(-1), vo.cpu().numpy().reshape(-1))
    # the longest list the entry takes (tau < 0.5): every voxel of a cell with a corner inside |sdf| < 0.499
    one_plane = _one_plane(hip, N, origin, vs)
    reached = []
    r, bh, bo = _band(hip, N, origin, vs, 0.499)
    for h, (band, exact) in enumerate(zip((bh, bo), full)):
        mark = _band_marks([one_plane[h]], N, 0.499).reshape(-1)
        assert int(mark.sum()) == int(r[33 + h]) > P // 4, (N, h, int(mark.sum()), r[33 + h])
        bad = np.flatnonzero((band.view(np.int32) != exact.view(np.int32)) & mark)
        assert bad.size == 0, (N, h, bad[:8], bad % 32, bad // WG_PTS)
        reached.append(int(mark.sum()))
    # shorter lists: the same voxels in other lanes and other tiles
    for h in (0, 1):
        for tau, count in _taus_for([one_plane[h]], N, (1, 130, 3 * WG_PTS + 2, P // 2)):
            r, bh, bo = _band(hip, N, origin, vs, tau)
            mark = _band_marks([one_plane[h]], N, tau).reshape(-1)
            assert int(mark.sum()) == count == int(r[33 + h]), (tau, count, r[33], r[34])
            band = (bh, bo)[h]
            assert np.array_equal(band[mark].view(np.int32), full[h][mark].view(np.int32)), (N, h, count)
            assert np.array_equal(band[~mark].view(np.int32), one_plane[h][~mark].view(np.int32)), (N, h, count)
            reached.append(count)
    print("N = %d: list lengths %s and %d" % (N, sorted(set(reached)), P))
    assert any(c % 32 for c in reached) and any(c > WG_PTS for c in reached), reached
    # audit on: its picks are unmarked voxels at random, evaluated behind the marked ones - every voxel of the delivered volume is
    # the full sweep's value (marked or picked) or the one-plane value, and picks were evaluated
    hip.set_audit(1 << 16, seed=4242)
    tau, count = _taus_for([one_plane[0]], N, (1,))[0]
    r, bh, bo = _band(hip, N, origin, vs, tau)
    assert int(r[37]) > 0, r[37]
    for h, band in enumerate((bh, bo)):
        same = band.view(np.int32) == full[h].view(np.int32)
        assert np.all(same | (band.view(np.int32) == one_plane[h].view(np.int32))), (N, h)
        assert np.all(same[_band_marks([one_plane[h]], N, tau).reshape(-1)]), (N, h)
    hip.close()


def test_list_of_one_tile_and_two_lanes():
    """A lattice off both surfaces (values grow away from a lattice corner), where the allowance steers the list length in steps of
    a few voxels: the list nearest to 130 voxels - more than one 128-point tile, less than a tile and a wave - against the full sweep."""
    hip = _decoder()
    hip.set_audit(0)
    N, origin, vs = 12, [0.56, 0.31, 0.21], 0.025
    vh, vo, _ = hip.decode_grid(N, origin, vs, REF)
    full = (vh.cpu().numpy().reshape(-1), vo.cpu().numpy().reshape(-1))
    one_plane = _one_plane(hip, N, origin, vs)
    lengths = []
    for h in (0, 1):
        tau, count = _taus_for([one_plane[h]], N, (130,))[0]
        r, bh, bo = _band(hip, N, origin, vs, tau)
        mark = _band_marks([one_plane[h]], N, tau).reshape(-1)
        assert int(mark.sum()) == count == int(r[33 + h])
        band = (bh, bo)[h]
        assert np.array_equal(band[mark].view(np.int32), full[h][mark].view(np.int32)), (h, count)
        lengths.append(count)
    print("lists nearest to 130 voxels: hand %d, object %d" % tuple(lengths))
    assert any(WG_PTS < c < WG_PTS + 32 for c in lengths), lengths
    hip.close()


@pytest.mark.parametrize("N", [8, 12])
def test_w_form_against_the_32_wide_form_and_the_fp32_chain(N, mfma_shape):
    hip = _decoder(refine=None)                 # the product's sweeps: near-level repair on, as wherever the boxes are used
    origin, vs = _cube(N)
    assert hip.split_half_instance() == "sdf_mlp_f16w_kernel"
    wh, wo, wbox = hip.decode_grid(N, origin, vs, REF)
    mfma_shape(32)
    assert hip.split_half_instance() == "sdf_mlp_f16_kernel"
    nh, no, nbox = hip.decode_grid(N, origin, vs, REF)
    mfma_shape(16)
    assert hip.math == "f16x3"
    hip.set_math("f32")
    fh, fo, _ = hip.decode_grid(N, origin, vs, REF)
    hip.set_math("f16x3")
    d32 = max(float((wh - nh).abs().max()), float((wo - no).abs().max()))
    df = max(float((wh - fh).abs().max()), float((wo - fo).abs().max()))
    print("N = %d: W form against the 32-wide form %.3g, against the fp32 chain %.3g" % (N, d32, df))
    assert d32 <= 2e-6, d32
    assert df <= 1e-5, df
    wb, nb = wbox.cpu().numpy(), nbox.cpu().numpy()
    assert wb[6] > 0 and wb[14] > 0 and wb[7] == 0 and wb[15] == 0
    assert np.array_equal(wb[0:7], nb[0:7]) and np.array_equal(wb[8:15], nb[8:15]), (wb, nb)
    hip.close()


def test_same_sweep_twice_is_bit_equal():
    """A wait placed too late shows as a run-to-run difference in values fed from LDS."""
    hip = _decoder()
    N = 16
    origin, vs = _cube(N)
    ah, ao, abox = hip.decode_grid(N, origin, vs, REF)
    bh, bo, bbox = hip.decode_grid(N, origin, vs, REF)
    assert hip.math == "f16x3" and hip.split_half_instance() == "sdf_mlp_f16w_kernel"
    assert torch.equal(ah.view(torch.int32), bh.view(torch.int32)) and torch.equal(ao.view(torch.int32), bo.view(torch.int32))
    assert torch.equal(abox, bbox)
    assert bool(torch.isfinite(ah).all()) and bool(torch.isfinite(ao).all())
    hip.close()
