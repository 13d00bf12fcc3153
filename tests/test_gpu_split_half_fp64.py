"""Every split-half decoder kernel held to an fp64 truth on every voxel, at the lattice edges where tiled kernels go wrong.

The split-half kernels (two fp16 planes per operand, three fp16 MFMAs per product sum, fp32 accumulation) are the default arithmetic
of every grid sweep.  Their error against fp64 is a few 1e-7 - far inside the 1e-5 bar the other value tests use - so a subtle
arithmetic fault (a dropped lo x hi term in one K-block, a wrong bias slot in one feature half, the second 16-point group reading the
first group's operands in a partial tile) would pass those.  Here the yardsticks are the fp64 evaluation of the same weights
(oracle/sdf_oracle.py decode_points(..., dtype=torch.float64)), the fp32 MFMA chain of the same library ("f32") and the fp32 CPU
oracle, and the criterion is the one of tests/test_gpu_split_half_adversarial.py, on every lattice:

    e16 <= 3 max(e32, eor) + 5e-7        (e = largest |value - fp64| over every voxel of both heads)

on lattices of 4096 voxels or more also rms16 <= 1.5 max(rms32, rmsor) (the same errors' root mean square: 0.86-0.94 on the
shipped library), and, for the shipped decoders, <= 1e-5 against the fp32 oracle on every voxel.  The near-level repair is off (set_refine(0)), and
the range words and hip.math are checked, so neither the fp32 chain nor the repair can stand in for the kernel under test.

Instantiations (hip.split_half_instance(), csrc/k1h_kernels.hip k1h_launch / k1h_subset_launch): the W form sdf_mlp_f16w_kernel
(SeparateDecoder, affine point features, the default shape), the 32x32x16 form sdf_mlp_f16_kernel on the same decoders
(asdf_set_mfma_shape(32)), sdf_mlp_f16_combined_kernel (CombinedDecoder, two outputs), sdf_mlp_f16_nerf9_kernel /
sdf_mlp_f16_nerf15_kernel (NeRF features, KP 5 / 8), and their voxel-list (subset) forms.

Lattice sizes: a workgroup is 4 waves of kWavePts = 32 points (csrc/sdf_layout.h kWgPts = kWavePts * kWaves = 128, launched with
256 threads by k1h_kernels.hip / k1hw_kernels.hip), and the W form splits each wave's 32 points into two groups of 16
(csrc/sdf_mlp_f16w_kernel.h).  N^3 for N = 2, 3, 5, 17, 33, 65 is odd - a partial 16-point group in the last tile - and N = 8
(512 = 4 x 128) is the control without one."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from alignsdf_amd import _native
from alignsdf_amd import synthetic as syn
from tests import split_half_cases as cases

pytestmark = pytest.mark.gpu
REF, INT = _native.GRID_REFERENCE, _native.GRID_INTEGER
GROUP_PTS = 16
RMS_FACTOR = 1.5

# (N, grid mode, origin, voxel size)
LATTICES = (
    (2, REF, (-1.0, -1.0, -1.0), 2.0),                 # 8 voxels: a lone partial group
    (3, INT, (-0.7, -0.6, -0.5), 0.55),                # 27
    (5, REF, (-0.9, -0.75, -0.8), 0.41),               # 125: three short of one workgroup
    (8, INT, (-1.0, -1.0, -1.0), 2.0 / 7),             # 512 = 4 x 128: the control
    (17, REF, (-0.95, -0.9, -0.85), 0.115),            # 4913 = 38 x 128 + 49
    (33, INT, (-1.0, -1.0, -1.0), 2.0 / 32),           # 35937 = 280 x 128 + 97
)
SMALL = LATTICES[:1] + LATTICES[4:5] + ((21, INT, (-0.8, -0.7, -0.75), 0.08),)   # 21^3 = 9261 = 72 x 128 + 45
AFFINE = ["nerf3", "both9", "hand6", "hand51", "obj6"]
WIDE_ONLY = {"comb3": "sdf_mlp_f16_combined_kernel", "nerf9": "sdf_mlp_f16_nerf9_kernel", "nerf15": "sdf_mlp_f16_nerf15_kernel"}


def _layout_constant(name):
    path = os.path.join(os.path.dirname(__file__), "..", "alignsdf_amd", "csrc", "sdf_layout.h")
    return int(re.search(r"constexpr int %s = (\w+);" % name, open(path).read()).group(1))


WAVE_PTS = _layout_constant("kWavePts")
WG_PTS = WAVE_PTS * _layout_constant("kWaves")


def test_lattice_sizes_straddle_the_tiles():
    assert (WAVE_PTS, WG_PTS) == (32, 128)
    for N, *_ in LATTICES + SMALL + ((65, REF, None, None),):
        P = N ** 3
        assert (P % WG_PTS == 0) == (N == 8) and (P % GROUP_PTS == 0) == (N == 8), N


@pytest.fixture
def mfma_shape():
    """Sets the process-wide shape for a test and puts the previous one back."""
    L = _native.lib()
    before = L.asdf_get_mfma_shape()
    yield lambda shape: L.asdf_set_mfma_shape(int(shape))
    L.asdf_set_mfma_shape(before)


def _pose():
    m, o = syn.pose_inputs(0)
    return {k: torch.from_numpy(v) for k, v in m.items()}, {k: torch.from_numpy(v) for k, v in o.items()}


def _weights(tag, name):
    """(state dict, latent [L] fp32) of a shipped decoder (name None) or an adversarial variant of it."""
    if name is None:
        return syn.full_state_dict(tag), syn.latent_code(0).reshape(-1)
    return cases.variant(name, tag)


def _coords(N, mode, origin, vs):
    from oracle import sdf_oracle as orc
    return orc.grid_coords(N, vs, list(origin), integer_mode=mode == INT)


@functools.lru_cache(maxsize=None)
def _truth(tag, name, lat_key):
    """(fp64 hand, fp64 obj, fp32-oracle hand, fp32-oracle obj) as flat numpy arrays on one lattice (lat_key: (N, mode, origin, vs),
    vs a python float - or the 0-dim fp32 tensor of a zoom cube, as the reference's pass 2 passes it)."""
    from oracle import sdf_oracle as orc
    sd, lat = _weights(tag, name)
    specs = syn.specs_for(tag)
    mano, obj = _pose() if specs["EncodeStyle"] != "nerf" else (None, None)
    N, mode, origin, vs = lat_key
    pts = _coords(N, mode, origin, vs)
    t = orc.decode_points(sd, lat, pts, specs, mano, obj, dtype=torch.float64)
    f = orc.decode_points(sd, lat, pts, specs, mano, obj)
    return tuple(x.numpy() for x in t + f)


def _decoder(tag, name):
    from alignsdf_amd.hip_decoder import HipSdfDecoder, kinematic_affine
    sd, lat = _weights(tag, name)
    specs = syn.specs_for(tag)
    hip = HipSdfDecoder(sd, 256, specs["PointFeatSize"], specs["EncodeStyle"])
    hip.set_refine(0.0)                        # the arithmetic itself, not the near-level repair
    emb = None
    if specs["EncodeStyle"] != "nerf":
        mano, obj = _pose()
        emb = kinematic_affine(specs["PointFeatSize"], specs["EncodeStyle"], specs["SdfScaleFactor"], mano, obj, hip.combined)
    hip.set_sample(torch.from_numpy(lat), emb)
    return hip


def _err(vols, refs):
    """(largest, rms) |value - fp64| over every voxel of the evaluated heads."""
    d = np.concatenate([np.asarray(v.cpu().numpy() if torch.is_tensor(v) else v, np.float64).reshape(-1) - r
                        for v, r in zip(vols, refs) if v is not None and r is not None])
    return float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))


def _check(hip, label, lat_key, truth, shipped, hand=True, obj=True, lattice_dev=None, instance=None):
    """One sweep on the split-half kernel and one on the fp32 chain of the same lattice, against fp64 and the fp32 oracle."""
    N, mode, origin, vs = lat_key
    t_h, t_o, o_h, o_o = truth
    want = [t_h if (hand or hip.combined) else None, t_o if (obj or hip.combined) else None]
    orac = [o_h, o_o]
    assert hip.math == "f16x3"
    if instance is not None:
        assert hip.split_half_instance() == instance, (hip.split_half_instance(), instance)
    args = (N, origin, vs, mode) if lattice_dev is None else (N, None, None, mode)
    vh, vo, bbox = hip.decode_grid(*args, hand=hand, obj=obj, lattice=lattice_dev)
    # a range violation or a silent fall-back to the fp32 chain would make this another kernel's number
    assert hip.math == "f16x3", (label, "fell back to the fp32 chain")
    b = bbox.cpu().numpy()
    assert b[7] == 0 and b[15] == 0, (label, b[7], b[15])
    vols16 = [vh, vo]
    e16, r16 = _err(vols16, want)
    hip.set_math("f32")
    fh, fo, _ = hip.decode_grid(*args, hand=hand, obj=obj, lattice=lattice_dev)
    hip.set_math("f16x3")
    e32, r32 = _err([fh, fo], want)
    eor, ror = _err(orac, want)
    print("%-44s N=%-3d %s: e16 %.2e  e32 %.2e  eor %.2e | rms %.2e %.2e %.2e" % (
        label, N, "ref" if mode == REF else "int", e16, e32, eor, r16, r32, ror))
    assert e16 <= 3.0 * max(e32, eor) + 5e-7, (label, N, e16, e32, eor)
    # The largest error of a few 1e-7 is the fp32 accumulation's, shared with the fp32 chain: a fault that adds errors of that size
    # everywhere (low planes carried with 7 instead of 10 bits: ~1e-6 largest, ~1.7e-7 rms) hides under the bound above, but not
    # in the rms over a lattice of thousands of voxels.
    if N ** 3 >= 4096:
        assert r16 <= RMS_FACTOR * max(r32, ror), (label, N, r16, r32, ror)
    if shipped:
        d = max(float(np.abs(v.cpu().numpy().reshape(-1) - o).max()) for v, o in zip(vols16, orac) if v is not None)
        assert d <= 1e-5, (label, N, d)
    return e16


# ---- shipped decoders, every instantiation, every lattice ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [16, 32])
@pytest.mark.parametrize("tag", AFFINE)
def test_affine_decoders_both_shapes(tag, shape, mfma_shape):
    hip = _decoder(tag, None)
    mfma_shape(shape)
    inst = "sdf_mlp_f16w_kernel" if shape == 16 else "sdf_mlp_f16_kernel"
    assert hip.split_half_kernel == inst
    for key in LATTICES:
        _check(hip, "%s %s" % (tag, inst), key, _truth(tag, None, key), True, instance=inst)
    hip.close()


@pytest.mark.parametrize("tag", sorted(WIDE_ONLY))
def test_two_out_and_nerf_decoders(tag):
    hip = _decoder(tag, None)
    assert hip.split_half_kernel == "sdf_mlp_f16_kernel"
    for key in LATTICES:
        _check(hip, "%s %s" % (tag, WIDE_ONLY[tag]), key, _truth(tag, None, key), True, instance=WIDE_ONLY[tag])
    hip.close()


def test_w_form_at_n65():
    """The largest lattice the fp64 truth is computed on: 65^3 = 274 625 = 2145 x 128 + 65, sheared (reference) indices."""
    hip = _decoder("nerf3", None)
    key = (65, REF, (-1.0, -1.0, -1.0), 2.0 / 64)
    _check(hip, "nerf3 sdf_mlp_f16w_kernel", key, _truth("nerf3", None, key), True, instance="sdf_mlp_f16w_kernel")
    hip.close()


@pytest.mark.parametrize("shape", [16, 32])
@pytest.mark.parametrize("tag", ["both9", "nerf3"])
def test_single_head_sweeps(tag, shape, mfma_shape):
    hip = _decoder(tag, None)
    mfma_shape(shape)
    inst = "sdf_mlp_f16w_kernel" if shape == 16 else "sdf_mlp_f16_kernel"
    for key in (LATTICES[2], LATTICES[4]):
        for hand, obj in ((True, False), (False, True)):
            _check(hip, "%s %s %s only" % (tag, inst, "hand" if hand else "obj"), key, _truth(tag, None, key), True, hand=hand, obj=obj,
                   instance=inst)
    hip.close()


@pytest.mark.parametrize("tag", ["both9", "comb3", "nerf9"])
def test_pass2_zoom_lattice_on_the_device(tag):
    """A real pass-2 lattice: the zoom cube of a coarse sweep's boxes (zoom_cube_from_bboxes), handed to the sweep in device memory
    (asdf_decode_grid_dev, the path of a sample enqueued in one go), sheared reference indices."""
    from alignsdf_amd.utils.mesh import zoom_cube_from_bboxes
    hip = _decoder(tag, None)
    N, vs1 = 33, 2.0 / 32
    _, _, bbox = hip.decode_grid(N, [-1.0, -1.0, -1.0], vs1)
    b = bbox.cpu().numpy()
    assert b[6] > 0 and b[14] > 0
    nvs, norg = zoom_cube_from_bboxes([(b[0:3], b[3:6], int(b[6])), (b[8:11], b[11:14], int(b[14]))], N, vs1)
    assert 0.0 < float(nvs) < vs1
    lattice = torch.cat([norg.float(), nvs.reshape(1).float()]).cuda()
    key = (N, REF, tuple(float(v) for v in norg), nvs)
    inst = hip.split_half_instance()
    _check(hip, "%s %s zoom" % (tag, inst), key, _truth(tag, None, key), True, lattice_dev=lattice, instance=inst)
    hip.close()


# ---- adversarial decoders ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,name,shape", [
    ("hand6", "spread1e4", 16), ("hand6", "tiny", 16), ("hand6", "spread1e4", 32),
    ("comb3", "spread1e4", 32), ("comb3", "tiny", 32), ("comb3", "huge", 32),
    ("nerf9", "spread1e4", 32), ("nerf9", "tiny", 32), ("nerf9", "huge", 32),
])
def test_adversarial_variants(tag, name, shape, mfma_shape):
    hip = _decoder(tag, name)
    mfma_shape(shape)
    inst = WIDE_ONLY.get(tag, "sdf_mlp_f16w_kernel" if shape == 16 else "sdf_mlp_f16_kernel")
    for key in SMALL:
        _check(hip, "%s/%s %s" % (tag, name, inst), key, _truth(tag, name, key), False, instance=inst)
    hip.close()


# ---- the voxel-list (subset) forms: bit-identical to the ordinary sweep at the listed voxels ------------------------------------------
def _band_marks(vols, N, tau):
    """csrc/decoder.hip band_mark_kernel on the host: the 8 corners of every cell that is not certainly positive (all corners >= tau)
    and not certainly negative (all < -tau) in any of `vols`."""
    t = np.float32(tau)
    mark = np.zeros((N, N, N), bool)
    for v in vols:
        v = v.reshape(N, N, N)
        cells = None
        for b in (v >= t, v < -t):
            a = np.ones((N - 1,) * 3, bool)
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        a &= b[dz:N - 1 + dz, dy:N - 1 + dy, dx:N - 1 + dx]
            cells = a if cells is None else cells | a
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    mark[dz:N - 1 + dz, dy:N - 1 + dy, dx:N - 1 + dx] |= ~cells
    return mark


def _taus_for(vols, N, targets):
    """Allowances whose band lists are as close to each target length as the lattice allows (a cell is marked at tau iff
    tau > its smallest corner and tau >= -its largest: every tau in between two cells' thresholds gives the same list)."""
    lo = np.full((N - 1,) * 3, np.inf, np.float32)
    hi = np.full((N - 1,) * 3, -np.inf, np.float32)
    for v in vols:
        v = v.reshape(N, N, N)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    c = v[dz:N - 1 + dz, dy:N - 1 + dy, dx:N - 1 + dx]
                    lo, hi = np.minimum(lo, c), np.maximum(hi, c)
    thr = np.maximum(np.nextafter(lo, np.float32(np.inf)), -hi).reshape(-1)
    thr = np.unique(thr[(thr > 1e-6) & (thr < 0.45)])[:600]
    counts = np.array([int(_band_marks(vols, N, t).sum()) for t in thr])
    out = []
    for target in targets:
        k = int(np.argmin(np.abs(counts - target) * 2 + (counts < target)))
        out.append((float(thr[k]), int(counts[k])))
    return out


BAND_TARGETS = (1, 15, 16, 17, 31, 33, 100, 200)


@pytest.mark.parametrize("tag,shape,inst", [
    ("nerf3", 16, "sdf_mlp_f16w_subset_kernel"), ("nerf3", 32, "sdf_mlp_f16_subset_kernel"),
    ("comb3", 16, "sdf_mlp_f16_subset_combined_kernel"), ("nerf9", 16, "sdf_mlp_f16_subset_nerf9_kernel"),
])
def test_voxel_list_forms_are_the_ordinary_sweep(tag, shape, inst, mfma_shape):
    """The band sweep (asdf_decode_grid_band) evaluates the corners of the cells that can be active through the subset form of the
    split-half kernel; everything else keeps its one-plane value.  The list length is steered with the allowance tau on a lattice
    off the surfaces, from the one-plane values of the same lattice (a box sweep with a 1e-7 allowance): every marked voxel must be
    the ordinary sweep's value bit for bit, every other one the one-plane value, and the record must count exactly the host's
    marks.  Lists are unions of whole cells' 8 corners, so they grow in steps of 8, 12, 16, 18, ... voxels: a list of 1, 15, 17, 31 or
    33 cannot be made this way.  The nearest reachable lengths are taken and printed, and the lengths reached must include one below
    a 16-point group, one between a group and a 32-point wave, one between a wave and a 128-point workgroup that is not a multiple
    of 16, and one beyond a workgroup."""
    hip = _decoder(tag, None)
    mfma_shape(shape)
    assert hip.split_half_instance(subset=True) == inst
    hip.set_audit(0)                           # no audit picks behind the marked voxels
    N, vs = 9, 0.025
    heads = [(True, True)] if hip.combined else [(True, False), (False, True)]
    reached = set()
    # two 9^3 lattices off both shapes: one whose values grow away from a lattice corner (lists of 8, 12, 16, ...), one away from a face
    for origin, (hand, obj) in [(o, h) for o in ((0.56, 0.31, 0.21), (-0.2, 0.55, -0.1)) for h in heads]:
        want = hip.decode_grid(N, origin, vs, REF, hand=hand, obj=obj)
        _, uh, uo = hip._one_plane_launch(hip._L.asdf_decode_grid_box, "asdf_decode_grid_box", N, origin, vs, REF, hand, obj, 1e-7)
        one_plane = [u.cpu().numpy() if u is not None else None for u in (uh, uo)]
        for tau, count in _taus_for([u for u in one_plane if u is not None], N, BAND_TARGETS):
            rec, bh, bo = hip._one_plane_launch(hip._L.asdf_decode_grid_band, "asdf_decode_grid_band", N, origin, vs, REF, hand, obj, tau)
            r = rec.cpu().numpy()
            mark = _band_marks([u for u in one_plane if u is not None], N, tau).reshape(-1)
            assert int(mark.sum()) == count
            assert int(r[33] if (hand or hip.combined) else r[34]) == count, (tau, count, r[33], r[34])
            assert r[7] == 0 and r[15] == 0
            for band, exact, u in zip((bh, bo), want[:2], one_plane):
                if band is None:
                    continue
                band, exact = band.cpu().numpy().reshape(-1), exact.cpu().numpy().reshape(-1)
                assert np.array_equal(band[mark], exact[mark]), (inst, count, np.abs(band[mark] - exact[mark]).max())
                assert np.array_equal(band[~mark], u.reshape(-1)[~mark])
            reached.add(count)
    print("%s %s: list lengths %s" % (tag, inst, sorted(reached)))
    reached = sorted(reached)
    assert any(0 < c < GROUP_PTS for c in reached) and any(GROUP_PTS < c < WAVE_PTS for c in reached), reached
    assert any(WAVE_PTS < c < WG_PTS and c % GROUP_PTS for c in reached) and any(c > WG_PTS for c in reached), reached
    hip.close()
