"""The native pixel-aligned decoder kernel (csrc/k1pa_kernels.hip, the PA branches of csrc/sdf_mlp_kernel.h, pixel_project_kernel /
channel_mean_kernel / asdf_decoder_set_sample_pixel) held to an fp64 truth on every point it evaluates.

It is the only decoder kernel with per-point address arithmetic into a per-sample buffer: an in-kernel camera projection, an inclusive
in / out decision, 16 clamped bicubic taps into P = W_lat . F, a workspace indexed by blockIdx.x and a projection launch of
ceil(H W / 64) blocks.  tests/test_gpu_pixel_align.py holds it to 1e-5 on smooth maps; the fp32 chain's real error is a few 1e-7, so a
swapped tap, a border tap that keeps its weight or a stale pixel of P can pass there.  Yardsticks here, as in
tests/test_gpu_split_half_fp64.py:

    t     the fp64 truth, oracle/sdf_oracle.py decode_points_pixel(..., dtype=torch.float64, inside=the fp32 op-for-op mask of
          tests/pixel_align_cases.project): everything in fp64 except the in / out decision, which is the one the kernel has to take
    e_pa  largest |native - t| over EVERY point of both heads
    e_mod the same for the module path (TorchModuleDecoder: the reference's arithmetic on the GPU), e_or for the fp32 oracle on the
          CPU - both over the CLEAR points only (fp32 and fp64 masks agree, ||u| - 1| and ||v| - 1| > 1e-4, |z_cam| > 1e-3), since torch
          may fuse or reorder the projection and decide a borderline point the other way

    e_pa <= 3 max(e_mod, e_or) + 5e-7,   on 4096 points or more also rms_pa <= 1.5 max(rms_mod, rms_or),   blob maps: <= 1e-5 against
    the fp32 oracle (tests/test_gpu_split_half_adversarial.py's criterion; measured values per case: profiles/pixel_align_fp64_errors.txt)

The clear share is a condition: at least 99.9 % of every lattice.  Border-point sets (adjacent floats that straddle u, v = +-1 under an
inexact camera) are exempt from it by construction and carry the absolute bound |native - t| <= 1e-5 max(1, max |t|) per point - the
maps they run on make a wrong decision cost 1e-3 or more (asserted on the CPU, tests/test_pixel_align_fold.py).

Every case is a valid call; every line printed with the prefix PAFP64 is one case's measured errors."""
import ctypes

import numpy as np
import pytest
import torch

from alignsdf_amd import _native
from alignsdf_amd import synthetic as syn
from tests import pixel_align_cases as pc
from tests.test_gpu_split_half_fp64 import LATTICES, WG_PTS

pytestmark = pytest.mark.gpu
REF, INT = _native.GRID_REFERENCE, _native.GRID_INTEGER
N65 = (65, REF, (-1.0, -1.0, -1.0), 2.0 / 64)           # tests/test_gpu_split_half_fp64.py test_w_form_at_n65
RMS_FACTOR, RMS_MIN_POINTS = 1.5, 4096
LIMIT_SIZES = [(256, 256), (256, 1)]                    # once each, on one decoder: test_every_pixel_at_the_size_limit
SMALL_SIZES = [s for s in pc.SIZES if s not in LIMIT_SIZES]


class Sample:
    """One PixelAlign sample: feature map [1, C, H, W], camera [1, 3, 4], root joint [3], ImageSize[0], SdfScaleFactor (numpy)."""

    def __init__(self, feat, cam, root, image=256, scale=None):
        self.feat, self.cam, self.root = np.ascontiguousarray(feat, np.float32), np.asarray(cam, np.float32), np.asarray(root, np.float32)
        self.image, self.scale = image, BASE_SPECS["SdfScaleFactor"] if scale is None else scale
        self.specs = dict(BASE_SPECS, SdfScaleFactor=self.scale, ImageSize=[image, image])
        self.mano = {"joints": np.tile(self.root.reshape(1, 1, 3), (1, 21, 1))}

    def project(self, pts, dtype=np.float32):
        return pc.project(pts, self.cam, self.root, self.image, self.scale, dtype)


BASE_SPECS, _, STATE_DICT, _, _, _, _ = syn.variant_config("pixelalign")


def edge_sample(feat):
    return Sample(feat, pc.EDGE_CAM, pc.EDGE_ROOT, pc.EDGE_IMAGE, pc.EDGE_SCALE)


def blob_sample(seed=0, H=64, W=64, focal=None):
    """synthetic.pixel_align_sample: the inexact camera a user has (focal 420, root 0.55 m).  `focal` replaces both focal lengths."""
    feat, mano, cam = syn.pixel_align_sample(seed, H, W)
    if focal is not None:
        cam = cam.copy()
        cam[0, 0, 0] = cam[0, 1, 1] = focal
    return Sample(feat, cam, mano["joints"][0, 0])


def skew_sample(feat):
    return Sample(feat, pc.SKEW_CAM, pc.SKEW_ROOT)


# ---- the evaluators -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def module_dec():
    """The nn.Module of the PixelAlign variant (the module path calls it; the native decoders are packed from it)."""
    from alignsdf_amd.networks import model as arch
    dec = getattr(arch, "SeparateDecoder")(BASE_SPECS["LatentSize"], BASE_SPECS["PointFeatSize"], BASE_SPECS["EncodeStyle"],
                                           **BASE_SPECS["NetworkSpecs"]).eval()
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in STATE_DICT.items()})
    return dec


def _native_decoder(weights):
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    hip = HipSdfDecoder(weights, 256, 3, "nerf", pixel_align=True) if isinstance(weights, dict) else HipSdfDecoder(weights, pixel_align=True)
    assert hip.pixel_align and hip.math == "f32"
    return hip


@pytest.fixture
def native(module_dec):
    hip = _native_decoder(module_dec)
    yield hip
    hip.close()


def _bind(hip, s):
    hip.set_sample_pixel(torch.from_numpy(s.feat).cuda(), s.cam, s.root, s.image, s.scale)


def _module_path(module_dec, s):
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    from alignsdf_amd.utils.utils import bind_sample, decoder_for
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    mod = decoder_for(module_dec, s.specs, t(s.mano), pixel_align="module")
    assert isinstance(mod, TorchModuleDecoder)
    bind_sample(mod, s.specs, torch.from_numpy(s.feat).cuda(), t(s.mano), None, torch.from_numpy(s.cam))
    return mod


def _np(v):
    return None if v is None else v.detach().cpu().numpy().reshape(-1)


# ---- the truth and the criterion ------------------------------------------------------------------------------------------------------
def _truth(s, pts):
    """(in32, clear, (t_hand, t_obj) fp64 with the fp32 decision, (f_hand, f_obj) the fp32 oracle with the same decision)."""
    from oracle import sdf_oracle as orc
    pts = np.asarray(pts, np.float32)
    _, in32 = s.project(pts, np.float32)
    uv64, in64 = s.project(pts, np.float64)
    zc = pts[:, 2].astype(np.float64) * 2.0 / s.scale + float(s.root[2])
    with np.errstate(invalid="ignore"):
        clear = (in32 == in64) & (np.abs(np.abs(uv64) - 1.0) > 1e-4).all(1) & (np.abs(zc) > 1e-3)
    t = orc.decode_points_pixel(STATE_DICT, s.feat, pts, s.specs, s.mano, s.cam, dtype=torch.float64, inside=in32)
    f = orc.decode_points_pixel(STATE_DICT, s.feat, pts, s.specs, s.mano, s.cam, inside=in32)
    return in32, clear, tuple(x.numpy() for x in t), tuple(x.numpy().astype(np.float64) for x in f)


def _err(vals, refs, keep=None):
    d = np.concatenate([(np.asarray(v, np.float64) - r)[slice(None) if keep is None else keep] for v, r in zip(vals, refs)
                        if v is not None])
    if d.size == 0:
        return 0.0, 0.0
    return float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))


def _check(label, truth, got, mod, blob, min_clear=0.0):
    """The criterion of the module docstring on one point set.  got / mod: (hand, obj) flat numpy values of the native and the
    module path, None for a head that was switched off."""
    in32, clear, t, f = truth
    assert clear.mean() >= min_clear, (label, clear.mean())
    assert clear.any(), label
    M = len(in32)
    heads = [k for k in (0, 1) if got[k] is not None]
    sel = lambda x: [x[k] for k in heads]
    assert all(np.isfinite(got[k]).all() for k in heads), label
    e_pa, r_pa = _err(sel(got), sel(t))
    e_mod, r_mod = _err(sel(mod), sel(t), clear)
    e_or, r_or = _err(sel(f), sel(t), clear)
    print("PAFP64 %-58s M=%-7d in %5.1f%% clear %6.2f%%: e_pa %.2e e_mod %.2e e_or %.2e | rms %.2e %.2e %.2e" % (
        label, M, 100.0 * in32.mean(), 100.0 * clear.mean(), e_pa, e_mod, e_or, r_pa, r_mod, r_or))
    assert e_pa <= 3.0 * max(e_mod, e_or) + 5e-7, (label, e_pa, e_mod, e_or)
    if M >= RMS_MIN_POINTS:
        assert r_pa <= RMS_FACTOR * max(r_mod, r_or), (label, r_pa, r_mod, r_or)
    if blob:
        d, _ = _err(sel(got), sel(f))
        assert d <= 1e-5, (label, d)


def _check_points(label, hip, module_dec, s, pts, blob=False, min_clear=0.0):
    """decode_points of `pts` on the bound native decoder against the truth; returns the native values."""
    x = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
    h, o = hip.decode_points(x)
    mh, mo = _module_path(module_dec, s).decode_points(x)
    got = (_np(h), _np(o))
    _check(label, _truth(s, pts), got, (_np(mh), _np(mo)), blob, min_clear)
    return got


def _box_of_volume(vol, N):
    """asdf_neg_bbox of a device volume: the stand-alone box kernel, as the module path uses it."""
    L = _native.lib()
    rec = torch.empty(_native.BOX_WORDS, dtype=torch.int32, device="cuda")
    _native.check(L.asdf_neg_bbox(vol.data_ptr(), N, N, N, rec.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "asdf_neg_bbox")
    return rec.cpu().numpy()[:_native.BOX_STRIDE]


EMPTY_BOX = np.array([0x7fffffff] * 3 + [-1] * 3 + [0, 0], np.int32)


def _check_lattice(label, hip, module_dec, s, key, hand=True, obj=True, lattice_dev=None):
    from oracle import sdf_oracle as orc
    N, mode, origin, vs = key
    pts = orc.grid_coords(N, vs, list(origin), integer_mode=mode == INT).numpy()
    truth = _truth(s, pts)
    share = truth[0].mean()
    if N <= 3:
        assert 0 < truth[0].sum() < N ** 3, (label, share)
    else:
        assert 0.10 <= share <= 0.90, (label, share)
    args = (N, origin, vs, mode) if lattice_dev is None else (N, None, None, mode)
    vh, vo, rec = hip.decode_grid(*args, hand=hand, obj=obj, lattice=lattice_dev)
    assert (vh is None) == (not hand) and (vo is None) == (not obj)
    mh, mo, mrec = _module_path(module_dec, s).decode_grid(N, origin, float(vs), mode, hand=hand, obj=obj)
    got, mod = (_np(vh), _np(vo)), (_np(mh), _np(mo))
    _check(label, truth, got, mod, True, min_clear=0.999)
    # the fused box record: the module path's record on the same lattice, word for word (as test_native_against_the_module_path
    # asserts it), and the stand-alone box kernel's on the kernel's own values; a sign may differ from the module path's only where
    # that is within 2e-6 of the level
    rec, mrec = rec.cpu().numpy(), mrec.cpu().numpy()
    S = _native.BOX_STRIDE
    assert np.array_equal(rec[:2 * S], mrec[:2 * S]), (label, rec, mrec)
    for k, (vol, g, m) in enumerate(((vh, got[0], mod[0]), (vo, got[1], mod[1]))):
        if vol is None:
            assert np.array_equal(rec[S * k:S * k + S], EMPTY_BOX), (label, k, rec)
            continue
        own = _box_of_volume(vol, N)
        assert np.array_equal(rec[S * k:S * k + S - 1], own[:S - 1]) and rec[S * k + S - 1] == 0, (label, k, rec, own)
        differ = (g < 0) != (m < 0)
        assert np.all(np.abs(m[differ]) <= 2e-6), (label, k, int(differ.sum()))
    return got


def _lattice_sample(N):
    """The sample camera leaves 29-63 % of every lattice of N >= 3 inside the image; the corners of the 2^3 lattice need a wider
    view (focal 200) to have a voxel on either side."""
    return blob_sample(0, focal=200.0 if N == 2 else None)


# ---- 1. lattices ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [REF, INT], ids=["ref", "int"])
@pytest.mark.parametrize("key", LATTICES + (N65,), ids=lambda k: "N%d" % k[0])
def test_lattice_sweeps(key, mode, native, module_dec):
    N, _, origin, vs = key
    assert (N ** 3 % WG_PTS == 0) == (N == 8)
    s = _lattice_sample(N)
    _bind(native, s)
    _check_lattice("lattice blob64", native, module_dec, s, (N, mode, origin, vs))


@pytest.mark.parametrize("hand", [True, False], ids=["hand_only", "obj_only"])
def test_single_head_sweeps(hand, native, module_dec):
    s = _lattice_sample(5)
    _bind(native, s)
    for key in (LATTICES[2], LATTICES[4], LATTICES[5]):
        assert key[0] in (5, 17, 33)
        got = _check_lattice("lattice blob64 %s" % ("hand only" if hand else "obj only"), native, module_dec, s, key, hand=hand, obj=not hand)
        # the head that runs alone gives the bits it gives beside the other one
        vh, vo, _ = native.decode_grid(*key[:1], key[2], key[3], key[1])
        assert np.array_equal(got[0 if hand else 1], _np(vh if hand else vo)), key[0]


@pytest.mark.parametrize("N", [17, 33])
def test_pass2_zoom_lattice_on_the_device(N, native, module_dec):
    """A real pass-2 lattice: the cube get_higher_res_cube makes of a coarse sweep's boxes, with its fp32 voxel size, handed over in
    device memory.  (On these coarse lattices the boxes span nearly the whole cube, so the "zoom" cube is the larger one - index span
    + 4 over N - 1 - and part of it lies outside [-1, 1]^3: a pass-2 lattice all the same, 22 % / 28 % of it inside the image.)"""
    from alignsdf_amd.utils.mesh import zoom_cube_from_bboxes
    s = _lattice_sample(N)
    _bind(native, s)
    vs1 = 2.0 / (N - 1)
    _, _, rec = native.decode_grid(N, [-1.0, -1.0, -1.0], vs1)
    b = rec.cpu().numpy()
    assert b[6] > 0 and b[14] > 0
    nvs, norg = zoom_cube_from_bboxes([(b[0:3], b[3:6], int(b[6])), (b[8:11], b[11:14], int(b[14]))], N, vs1)
    assert 0.0 < float(nvs) != np.float32(vs1) and nvs.dtype == torch.float32
    lattice = torch.cat([norg.float(), nvs.reshape(1).float()]).cuda()
    key = (N, REF, tuple(float(v) for v in norg), nvs)
    got = _check_lattice("zoom lattice (device) blob64", native, module_dec, s, key, lattice_dev=lattice)
    # the same lattice by value gives the same bits
    vh, vo, _ = native.decode_grid(N, key[2], float(nvs), REF)
    assert np.array_equal(got[0], _np(vh)) and np.array_equal(got[1], _np(vo))


# ---- 2. point lists -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 31, 32, 33, 127, 128, 129, 4097, 70001])
def test_point_lists(M, native, module_dec):
    """Partial waves, one workgroup, many workgroups (more than one per compute unit at 70001); mixed inside / outside."""
    s = blob_sample(0)
    _bind(native, s)
    pts = syn.uniform((M, 3), 7700 + M, -1.0, 1.0).astype(np.float32)
    if M == 1:
        pts[0] = (0.1, -0.2, 0.3)
    in32 = s.project(pts)[1]
    assert M < 31 or 0 < in32.sum() < M
    a = _check_points("point list blob64", native, module_dec, s, pts, blob=True)
    b = native.decode_points(torch.from_numpy(pts).cuda())
    assert np.array_equal(a[0], _np(b[0])) and np.array_equal(a[1], _np(b[1]))


def test_a_lattice_as_a_point_list_gives_the_sweeps_bits(native):
    """The sweep computes its coordinates with the device function the oracle's lattice equals bit for bit (test_gpu_grid_coords.py);
    from there on a list and a sweep run the same instructions."""
    from oracle import sdf_oracle as orc
    s = blob_sample(0)
    _bind(native, s)
    N, mode, origin, vs = LATTICES[4]
    assert N == 17
    vh, vo, _ = native.decode_grid(N, origin, vs, mode)
    h, o = native.decode_points(orc.grid_coords(N, vs, list(origin)).cuda())
    assert np.array_equal(_np(vh), _np(h)) and np.array_equal(_np(vo), _np(o))


# ---- 3. every pixel of P, every size ------------------------------------------------------------------------------------------------
def _every_pixel(H, W, native, module_dec):
    s = edge_sample(pc.signed_wide(H, W))
    _bind(native, s)
    pts = pc.pixel_centre_points(H, W)
    assert len(pts) == H * W + (H - 1) * (W - 1)
    _check_points("every pixel signed_wide %dx%d" % (H, W), native, module_dec, s, pts)
    return s


@pytest.mark.parametrize("H,W", SMALL_SIZES)
def test_every_pixel(H, W, native, module_dec):
    _every_pixel(H, W, native, module_dec)


def test_every_pixel_at_the_size_limit(native, module_dec):
    """256 x 256 (a 512 MiB P) and then, on the same decoder, 256 x 1: once each, with the edge points of case 5 on the map bound."""
    assert set(SMALL_SIZES) | set(LIMIT_SIZES) == set(pc.SIZES)
    for H, W in LIMIT_SIZES:
        s = _every_pixel(H, W, native, module_dec)
        _check_points("edge points signed_wide %dx%d" % (H, W), native, module_dec, s, pc.edge_points(W, H=H))


# ---- 4. tap indexing ----------------------------------------------------------------------------------------------------------------
def impulse_pixels(H, W):
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (1, 1),
            (H - 2, W - 2), (H // 2 - 1, W // 2)]


@pytest.mark.parametrize("H,W", [(9, 5), (5, 9)])
def test_impulse_maps(H, W, native, module_dec):
    """One non-zero pixel: a point's value depends on the one tap that hits it - its row, its column, its weight."""
    for pixel in impulse_pixels(H, W):
        s = edge_sample(pc.impulse(H, W, pixel))
        _bind(native, s)
        _check_points("impulse %dx%d at %s" % (H, W, pixel), native, module_dec, s, pc.impulse_probe_points(H, W, pixel))


@pytest.mark.parametrize("H,W", [(8, 8), (5, 9), (63, 17), (64, 64)])
def test_ramp_map_at_the_border_taps(H, W, native, module_dec):
    """Points within a pixel of each of the four edges (rows from H, columns from W), where zero padding cuts taps off."""
    s = edge_sample(pc.ramp(H, W))
    _bind(native, s)
    _check_points("ramp %dx%d edge points" % (H, W), native, module_dec, s, pc.edge_points(W, H=H))


# ---- 5. the decision ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", ["sample", "skew"])
@pytest.mark.parametrize("H,W", [(64, 64), (63, 17)])
def test_border_points_under_an_inexact_camera(H, W, camera, native):
    """Adjacent floats either side of u, v = +-1, and points exactly on it, where fp32 and fp64 often decide differently.  On the blob
    maps: there a wrong decision costs 2.9e-3 or more at every such point (tests/test_pixel_align_fold.py) and the fp32 oracle is
    within 7e-7 of the truth, so the 1e-5 bound separates the two.  (On signed_wide the fp32 oracle itself is 2e-5 off at these
    points - channels of order 1e2 - and the bound would measure the map, not the decision.)"""
    s = blob_sample(0 if H == 64 else 1, H, W)
    if camera == "skew":
        s = skew_sample(s.feat)
    pts, kind = pc.border_points(s.cam, s.root, s.image, s.scale, 16)
    in32, _, t, _ = _truth(s, pts)
    assert in32[kind != 1].all() and not in32[kind == 1].any()
    _bind(native, s)
    h, o = native.decode_points(torch.from_numpy(pts).cuda())
    bound = 1e-5 * max(1.0, float(np.abs(np.concatenate(t)).max()))
    d = np.maximum(np.abs(_np(h) - t[0]), np.abs(_np(o) - t[1]))
    in64 = s.project(pts, np.float64)[1]
    print("PAFP64 %-58s M=%-7d fp32 != fp64 decisions %d: largest |native - t| %.2e (bound %.1e)" % (
        "border points %s camera blob %dx%d" % (camera, H, W), len(pts), int((in32 != in64).sum()), d.max(), bound))
    assert (d <= bound).all(), (camera, int((d > bound).sum()), d.max(), kind[d > bound])


@pytest.mark.parametrize("H,W", SMALL_SIZES)
def test_exact_edge_points_every_size(H, W, native, module_dec):
    """u / v exactly +-1, one step outside, z_cam = 0, behind the camera: the decision where fp32 and fp64 agree by construction
    (256 x 256 and 256 x 1: in test_every_pixel_at_the_size_limit, on the maps bound there)."""
    s = edge_sample(pc.signed_wide(H, W))
    _bind(native, s)
    pts = pc.edge_points(W, H=H)
    in32, in64 = s.project(pts)[1], s.project(pts, np.float64)[1]
    assert np.array_equal(in32, in64)
    _check_points("edge points signed_wide %dx%d" % (H, W), native, module_dec, s, pts)


# ---- 6. re-binding ------------------------------------------------------------------------------------------------------------------
def _probe(hip):
    """A sweep with a partial last tile and a list with a partial wave, as bits."""
    N, mode, origin, vs = LATTICES[4]
    vh, vo, rec = hip.decode_grid(N, origin, vs, mode)
    h, o = hip.decode_points(torch.from_numpy(syn.uniform((129, 3), 7801, -1.0, 1.0).astype(np.float32)).cuda())
    return [_np(vh).copy(), _np(vo).copy(), rec.cpu().numpy().copy(), _np(h).copy(), _np(o).copy()]


def _rebind_samples():
    a = blob_sample(1, 8, 8)
    b = blob_sample(2, 64, 64)
    c = Sample(pc.signed_wide(8, 8), a.cam, a.root)
    d = blob_sample(3, 65, 64)
    e = skew_sample(d.feat)
    return [("8x8", a), ("64x64 (grows)", b), ("8x8 other content (stale tail)", c), ("65x64 (grows)", d), ("65x64 new camera", e),
            ("8x8 again", a)]


def test_rebinding_one_decoder(native, module_dec):
    """8 x 8 -> 64 x 64 -> 8 x 8 -> 65 x 64 -> a new camera on that map -> the first sample again: every result is the one a fresh
    decoder gives on that sample, bit for bit; the last one is also held to the truth."""
    fresh = []
    for _, s in _rebind_samples():
        hip = _native_decoder(module_dec)
        _bind(hip, s)
        fresh.append(_probe(hip))
        hip.close()
    assert not np.array_equal(fresh[0][0], fresh[2][0]) and not np.array_equal(fresh[3][0], fresh[4][0])
    for (name, s), want in zip(_rebind_samples(), fresh):
        _bind(native, s)
        got = _probe(native)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), name
    _check_lattice("lattice after six binds blob8", native, module_dec, _rebind_samples()[-1][1], LATTICES[4])


def test_two_decoders_alternate_on_one_stream(module_dec):
    """Two decoders with different weights, each with its own P and constants, bound and swept in turn on one stream."""
    sd2 = {k: (v * np.float32(0.9) if k.endswith("weight_g") else v) for k, v in STATE_DICT.items()}
    sa, sb = blob_sample(0), blob_sample(2, 63, 17)
    want = []
    for w, s in ((module_dec, sa), (sd2, sb)):
        hip = _native_decoder(w)
        _bind(hip, s)
        want.append(_probe(hip))
        hip.close()
    assert not np.array_equal(want[0][0], want[1][0])
    one, two = _native_decoder(module_dec), _native_decoder(sd2)
    _bind(one, sa)
    _bind(two, sb)
    for _ in range(2):
        for hip, w in ((one, want[0]), (two, want[1])):
            for g, x in zip(_probe(hip), w):
                assert np.array_equal(g, x)
    _bind(two, sa)
    _bind(one, sb)
    _bind(one, sa)
    for g, x in zip(_probe(one), want[0]):
        assert np.array_equal(g, x)
    one.close()
    two.close()
