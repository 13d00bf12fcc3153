"""Shared pieces of the mesh signed distance tests (tests/test_mesh_sdf_truth.py on the CPU, tests/test_gpu_mesh_sdf.py on the GPU): THE
RULE of include/alignsdf_hip.h (asdf_mesh_sdf_*) in numpy, written from the header's words and not from the kernels - `rule(...,
np.float64)` is the truth (plain sums), `rule(..., np.float32)` the model: fp32 without contraction, the winding sum per chunk of
CHUNK faces from +0 and the chunk sums in chunk order from +0 -, the mesh builders, the query sets and the measured bounds.

The numpy rule walks the faces in a Python loop with every query at once: about 10^6 pairs a second, so every case keeps M T <= 2 10^6.
"""
import functools

import numpy as np

from alignsdf_amd import _native
from alignsdf_amd import synthetic as syn

BLOCK = _native.MESH_SDF_BLOCK_FACES
CHUNK = _native.MESH_SDF_CHUNK_FACES

# Measured by tests/test_mesh_sdf_truth.py over every case below (profiles/mesh_sdf_fp64_errors.txt): the largest |d_model - d_truth| and
# - over the queries that are not ON the surface (truth d >= ON_SURFACE, where w jumps by 1/2 per face through p) - |w_model - w_truth| of
# the fp32 model against the fp64 truth, rounded up to two digits.  The GPU's bounds are 4 x these: its sqrt, division and atan2 are
# not numpy's.
ON_SURFACE = 1e-6
MODEL_MAX_D = 2.1e-7
MODEL_MAX_W = 1.7e-6
D_BOUND = 4.0 * MODEL_MAX_D
W_BOUND = 4.0 * MODEL_MAX_W
W_CLEAR = 0.05               # signs are compared where ||w| - 0.5| >= W_CLEAR and d >= D_BOUND in the truth
MAX_LEFT_OUT = 0.01          # of a case's queries


# ---- the rule

def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _closest_on_triangle(a, b, c, P):
    ab, ac, bc = b - a, c - a, c - b
    ap, bp, cp = P - a, P - b, P - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    M = len(P)
    dt = P.dtype
    num, den = np.zeros(M, dt), np.ones(M, dt)
    base, dirn = np.tile(a, (M, 1)), np.tile(ab, (M, 1))
    free = np.ones(M, bool)

    def region(cond, n=None, d=None, bs=None, dr=None):
        nonlocal free
        m = free & cond
        if n is not None:
            num[m], den[m] = n[m], d[m]
        if bs is not None:
            base[m] = bs
        if dr is not None:
            dirn[m] = dr
        free = free & ~m

    region((d1 <= 0) & (d2 <= 0), bs=a)
    region((d3 >= 0) & (d4 <= d3), bs=b)
    region((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, d1 - d3)
    region((d6 >= 0) & (d5 <= d6), bs=c)
    region((vb <= 0) & (d2 >= 0) & (d6 <= 0), d2, d2 - d6, dr=ac)
    region((va <= 0) & (e43 >= 0) & (e56 >= 0), e43, e43 + e56, bs=b, dr=bc)
    q = base + (num / den)[:, None] * dirn
    s = (va + vb) + vc
    q_in = (a + (vb / s)[:, None] * ab) + (vc / s)[:, None] * ac
    q[free] = q_in[free]
    return q


def _closest_on_segment(base, e, P):
    ee = _dot(e, e)
    t = np.zeros(len(P), P.dtype)
    if ee > 0:
        t = np.minimum(np.maximum(_dot(P - base, e) / ee, P.dtype.type(0)), P.dtype.type(1))
    return base + t[:, None] * e


def _closest_on_flat(a, b, c, P):
    q = _closest_on_segment(a, b - a, P)
    r = P - q
    d2 = _dot(r, r)
    for base, e in ((b, c - b), (c, a - c)):
        q1 = _closest_on_segment(base, e, P)
        r = P - q1
        d21 = _dot(r, r)
        m = d21 < d2
        d2 = np.where(m, d21, d2)
        q[m] = q1[m]
    return q, d2


def _half_solid_angle(a, b, c, P):
    A, B, C = a - P, b - P, c - P
    la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
    x = np.stack([B[:, 1] * C[:, 2] - B[:, 2] * C[:, 1], B[:, 2] * C[:, 0] - B[:, 0] * C[:, 2], B[:, 0] * C[:, 1] - B[:, 1] * C[:, 0]], 1)
    det = _dot(A, x)
    den = (((la * lb) * lc + _dot(A, B) * lc) + _dot(B, C) * la) + _dot(C, A) * lb
    return np.arctan2(det, den)


def face_state(verts, faces, dtype):
    """0 a face, 1 a zero-area face, 2 an absent one - per face, by the header's words in `dtype`."""
    V = len(verts)
    v = np.asarray(verts, np.float32).astype(dtype)
    out = np.zeros(len(faces), np.int64)
    for t, f in enumerate(np.asarray(faces, np.int64).reshape(-1, 3)):
        if (f < 0).any() or (f >= V).any() or not np.isfinite(v[f]).all():
            out[t] = 2
            continue
        f = index_order(f)[0]
        ab, ac = v[f[1]] - v[f[0]], v[f[2]] - v[f[0]]
        n = np.array([ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]])
        out[t] = 1 if not n.any() else 0
    return out


def index_order(face):
    """(the face's corners in the order of their vertex indices, sigma = +1 / -1 for an even / odd permutation)."""
    f = [int(i) for i in face]
    order = sorted(range(3), key=lambda k: (f[k], k))
    return [f[k] for k in order], (1 if tuple(order) in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) else -1)


def face_distance2(verts, face, P):
    """(closest [M, 3], d2 [M]) of ONE face at the queries P [M, 3] (P's dtype): the header's region rule or its zero-area rule."""
    v = np.asarray(verts, np.float32).astype(P.dtype)
    face = index_order(face)[0]
    a, b, c = v[face[0]], v[face[1]], v[face[2]]
    ab, ac = b - a, c - a
    n = np.array([ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]])
    with np.errstate(all="ignore"):
        if not n.any():
            return _closest_on_flat(a, b, c, P)
        q = _closest_on_triangle(a, b, c, P)
        r = P - q
        return q, _dot(r, r)


def rule(verts, faces, xyz, dtype=np.float64, chunk=None):
    """The rule at xyz [M, 3] (fp32 values, taken to `dtype`): {"sdf", "d", "d2", "w", "face", "closest", "skipped", "zero_area"}.
    dtype float32 sums the winding number as the header defines it (chunk = CHUNK); float64 sums plainly."""
    dt = np.dtype(dtype)
    chunk = CHUNK if chunk is None else chunk
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    P = np.asarray(xyz, np.float32).reshape(-1, 3).astype(dt)
    M = len(P)
    state = face_state(verts, faces, dt)
    best = np.full(M, np.inf, dt)
    face = np.full(M, -1, np.int64)
    closest = np.full((M, 3), np.nan, dt)
    S = np.zeros(M, dt)
    v = np.asarray(verts, np.float32).astype(dt)
    with np.errstate(all="ignore"):
        for c0 in range(0, len(faces), chunk):
            part = np.zeros(M, dt)
            for t in range(c0, min(c0 + chunk, len(faces))):
                if state[t] == 2:
                    continue
                q, d2 = face_distance2(verts, faces[t], P)
                m = d2 < best
                best[m], face[m] = d2[m], t
                closest[m] = q[m]
                if state[t] == 0:
                    (i, j, k), sigma = index_order(faces[t])
                    part = part + dt.type(sigma) * _half_solid_angle(v[i], v[j], v[k], P)
            S = S + part
        w = S / dt.type(2.0 * np.pi)
        d = np.sqrt(best)
        sdf = np.where(np.abs(w) >= 0.5, -d, d)
    bad = ~np.isfinite(P).all(1)
    sdf[bad], w[bad], d[bad], face[bad], closest[bad] = np.nan, np.nan, np.nan, -1, np.nan
    return {"sdf": sdf, "d": d, "d2": best, "w": w, "face": face, "closest": closest,
            "skipped": int((state == 2).sum()), "zero_area": int((state == 1).sum())}


# ---- meshes: (verts float32 [V, 3], faces int32 [T, 3])

BOX_HALF = (0.5, 0.375, 0.25)          # (dyadic: the lattice below hits its planes, edges and corners exactly)


def box(half=BOX_HALF):
    h = np.asarray(half, np.float32)
    verts = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32) * h
    quads = ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3))          # outward
    faces = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return verts, np.asarray(faces, np.int32)


def torus(nu, nv, R=0.55, r=0.22, inward=False):
    """2 nu nv faces, closed, genus 1; tilted so that nothing is axis-aligned."""
    u = 2.0 * np.pi * np.arange(nu) / nu
    v = 2.0 * np.pi * np.arange(nv) / nv
    uu, vv = np.meshgrid(u, v, indexing="ij")
    pts = np.stack([(R + r * np.cos(vv)) * np.cos(uu), (R + r * np.cos(vv)) * np.sin(uu), r * np.sin(vv)], -1).reshape(-1, 3)
    rot = syn._rot((0.3, 1.0, 0.2), 0.6)
    pts = pts @ rot.T + np.array([0.03, -0.02, 0.05])
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces += [(a, b, c), (a, c, d)]
    faces = np.asarray(faces, np.int32)
    if inward:
        faces = faces[:, ::-1].copy()
    return pts.astype(np.float32), faces


def torus_open(nu, nv, seed=7):
    """The torus with a seeded 10 % of its faces removed."""
    verts, faces = torus(nu, nv)
    keep = syn.uniform((len(faces),), 41000 + seed) >= 0.1
    return verts, faces[keep]


def box_with_flat_faces():
    """The box plus appended zero-area faces: three collinear corners (a segment off the box) and three equal corners (a point)."""
    verts, faces = box()
    extra = np.array([[1.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.25]], np.float32)
    n = len(verts)
    flat = np.array([[n, n + 2, n + 1], [n + 3, n + 3, n + 3], [n, n, n + 2]], np.int32)
    return np.concatenate([verts, extra]), np.concatenate([faces, flat])


# ---- queries (float32 [M, 3])

def uniform_queries(verts, count, seed, grow=0.25):
    lo, hi = np.asarray(verts, np.float64).min(0), np.asarray(verts, np.float64).max(0)
    pad = grow * (hi - lo)
    return (lo - pad + syn.uniform((count, 3), 42000 + seed) * (hi - lo + 2 * pad)).astype(np.float32)


def feature_queries(verts, faces):
    """Every vertex the faces use, every edge midpoint and every face centroid (fp32 arithmetic: ON the mesh to rounding)."""
    v = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    used = v[np.unique(f)]
    mids = np.concatenate([(v[f[:, i]] + v[f[:, (i + 1) % 3]]) * np.float32(0.5) for i in range(3)])
    cent = (v[f[:, 0]] + v[f[:, 1]] + v[f[:, 2]]) / np.float32(3.0)
    return np.concatenate([used, np.unique(mids, axis=0), cent])


def box_lattice(half=BOX_HALF, per_axis=9):
    """per_axis^3 points at multiples of half / 2 per axis, -2 .. 2: planes, edges and corners of the box are hit exactly."""
    k = np.arange(per_axis) - per_axis // 2
    ax = [np.float32(h) * np.float32(0.5) * k.astype(np.float32) for h in half]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


LIST_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 4097)
FACE_COUNTS = (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
TORUS_EDGE = (10, 13)          # 260 faces >= 2 CHUNK + 3: the face-count cases are its first T faces (open meshes)
assert 2 * TORUS_EDGE[0] * TORUS_EDGE[1] >= max(FACE_COUNTS)


@functools.lru_cache(maxsize=None)
def box_pool():
    """4097 queries of the box: lattice, features, then seeded uniform points - shuffled (seeded), so that every prefix mixes them."""
    verts, faces = box()
    q = np.concatenate([box_lattice(), feature_queries(verts, faces)])
    q = np.concatenate([q, uniform_queries(verts, max(LIST_LENGTHS) - len(q), 1)])
    return q[np.argsort(syn.uniform((len(q),), 43000), kind="stable")]


@functools.lru_cache(maxsize=None)
def case(name):
    """(verts, faces, xyz) of a named case.  The box and the prefix cases take EVERY vertex, edge midpoint and face centroid as queries;
    the three 576-face torus cases take every seventh of their feature points (a plain stride over vertices, midpoints and
    centroids alike) beside 2 048 uniform points, which keeps M T within what the numpy truth manages."""
    if name == "box":
        v, f = box()
        return v, f, box_pool()
    if name.startswith("prefix"):
        T = int(name[6:])
        v, f = torus(*TORUS_EDGE)
        f = f[:T]
        # (grown by 1: far from an open patch |w| is small, and the 1 % that may be left out is for the neighbourhood of its rim)
        return v, f, np.concatenate([feature_queries(v, f), uniform_queries(v[np.unique(f)], 600, T, grow=1.0)])
    if name in ("torus", "torus_inward"):
        v, f = torus(18, 16)                                         # 576 faces; the same queries for both orientations
        xyz = np.concatenate([feature_queries(v, f)[::7], uniform_queries(v, 2048, 3)])
        return v, (f[:, ::-1].copy() if name == "torus_inward" else f), xyz
    if name == "torus_open":
        v, f = torus_open(18, 16)
        return v, f, np.concatenate([feature_queries(v, f)[::7], uniform_queries(v, 2048, 4, grow=1.0)])
    if name == "box_flat":
        v, f = box_with_flat_faces()
        extra = np.array([[1.25, 0.0, 0.0], [2.5, 0.0, 0.0], [1.5, 0.25, 0.0], [0.0, 1.0, 0.25], [0.0, 1.125, 0.25], [0.75, 0.0, 0.0]], np.float32)
        return v, f, np.concatenate([extra, box_pool()[:1024]])
    raise KeyError(name)


CASES = ("box",) + tuple("prefix%d" % T for T in FACE_COUNTS) + ("torus", "torus_inward", "torus_open", "box_flat")


@functools.lru_cache(maxsize=None)
def truth(name):
    v, f, xyz = case(name)
    return rule(v, f, xyz, np.float64)


@functools.lru_cache(maxsize=None)
def model(name):
    v, f, xyz = case(name)
    return rule(v, f, xyz, np.float32)


def clear_sign(tr):
    """Queries whose sign the truth decides: off the surface by the distance bound and |w| not within W_CLEAR of 1/2."""
    return (tr["d"] >= D_BOUND) & (np.abs(np.abs(tr["w"]) - 0.5) >= W_CLEAR)


def off_surface(tr):
    return tr["d"] >= ON_SURFACE


def compare(name, got, who, take=None):
    """Hold `got` ({"sdf", "w", "face", "closest"} as numpy arrays) to the truth of case `name` (`take`: of these of its queries, an
    index or a slice) by the yardsticks above; returns (max |d| error, max |w| error off the surface, queries left out of the sign
    comparison)."""
    v, f, xyz = case(name)
    tr = truth(name)
    if take is not None:
        xyz, tr = xyz[take], {k: (a[take] if isinstance(a, np.ndarray) else a) for k, a in tr.items()}
    M = len(xyz)
    sdf, w, face, closest = (np.asarray(got[k], np.float64 if k != "face" else np.int64) for k in ("sdf", "w", "face", "closest"))
    if M == 0:
        return 0.0, 0.0, 0
    e_d = np.abs(np.abs(sdf) - tr["d"]).max()
    off = off_surface(tr)
    e_w = np.abs(w - tr["w"])[off].max() if off.any() else 0.0
    assert e_d <= D_BOUND, (who, name, "d", e_d)
    assert e_w <= W_BOUND, (who, name, "w", e_w)
    clear = clear_sign(tr)
    left_out = int((off & ~clear).sum())
    assert left_out <= MAX_LEFT_OUT * M, (who, name, "left out", left_out, M)
    assert np.array_equal(np.signbit(sdf[clear]), np.signbit(tr["sdf"][clear])), (who, name, "sign")
    # face by value: the truth's distance to the returned face is the truth's minimum within the bound; closest lies on that face
    # (the truth's distance from it to the face is within the bound) and at |sdf| from the query
    assert ((face >= 0) & (face < len(f))).all(), (who, name, "face range")
    P = xyz.astype(np.float64)
    d_face, d_cl = np.empty(M), np.empty(M)
    for t in np.unique(face):
        m = face == t
        d_face[m] = np.sqrt(face_distance2(v, f[t], P[m])[1])
        d_cl[m] = np.sqrt(face_distance2(v, f[t], closest[m])[1])
    assert np.abs(d_face - tr["d"]).max() <= D_BOUND, (who, name, "face value", np.abs(d_face - tr["d"]).max())
    assert d_cl.max() <= D_BOUND, (who, name, "closest on its face", d_cl.max())
    gap = np.abs(np.linalg.norm(P - closest, axis=1) - np.abs(sdf)).max()
    assert gap <= D_BOUND, (who, name, "closest at |sdf|", gap)
    return float(e_d), float(e_w), left_out


# ---- the fit to (xyz, sdf) samples of ground-truth meshes (fit.fit_sample's sdf_hand / sdf_obj)

FIT_N, FIT_NEAR, FIT_UNIFORM, FIT_SEED = 24, 384, 128, 5
# fit_reference_fp64() on the CPU: loss 3.627e-2 -> 8.520e-3 in 40 steps, ratio 0.235 (0.215 at lr 5e-3).  The GPU fits are held to this
# plus the margin tests/test_gpu_sdf_vjp.py's fit test leaves above its own fp64 reference (0.25 - 0.055), for fp32 and clamp / ReLU
# mask flips along the trajectory
FIT_REFERENCE_RATIO = 0.235
FIT_RATIO_BOUND = FIT_REFERENCE_RATIO + (0.25 - 0.055)


@functools.lru_cache(maxsize=None)
def fit_meshes():
    """((verts, faces) hand, (verts, faces) obj): the ground-truth meshes of the fit - the CPU oracle's marching cubes of the analytic
    scene (synthetic.grasp_sdf) that sdf_vjp_cases.FIT_TAG's decoder was trained on, sample FIT_SAMPLE, on the FIT_N^3 lattice of
    [-1, 1]^3, in the decoder's normalised space."""
    from oracle import mc33
    from tests import sdf_vjp_cases as vc
    voxel = 2.0 / (FIT_N - 1)
    idx = np.stack(np.meshgrid(*[np.arange(FIT_N, dtype=np.float64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    out = []
    for values in syn.grasp_sdf(idx * voxel - 1.0, vc.FIT_SAMPLE):
        v, f = mc33.marching_cubes_raw(values.astype(np.float32).reshape(FIT_N, FIT_N, FIT_N), 0.0)
        out.append(((np.asarray(v, np.float64) * voxel - 1.0).astype(np.float32), np.asarray(f, np.int32)))
    return tuple(out)


def fit_points(head):
    """The sample positions of head 0 / 1: mesh_sdf.sample_points of its mesh (host arithmetic, the same on every machine)."""
    from alignsdf_amd.mesh_sdf import sample_points
    return sample_points(*fit_meshes()[head], FIT_NEAR, FIT_UNIFORM, seed=FIT_SEED + head)


def fit_start():
    """(z0 [L] float32, E0 two [pf_head, 4] float32): the start of sdf_vjp_cases.fit_scenario - the code moved by 0.3 |z| along a
    seeded direction, the two heads shifted by FIT_START_SHIFTS - made without a GPU."""
    import torch
    from alignsdf_amd.fit import kinematic_affine_torch, shift_embed
    from tests import sdf_vjp_cases as vc
    specs = syn.specs_for(vc.FIT_TAG)
    latent, mano, obj = syn.sample_inputs(vc.FIT_TAG, vc.FIT_SAMPLE)
    t = lambda d: None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}
    z = torch.from_numpy(latent).reshape(-1).double()
    n = torch.from_numpy(np.random.default_rng(11).standard_normal(z.numel()))
    z0 = (z + 0.3 * z.norm() * n / n.norm()).float()
    E = kinematic_affine_torch(specs["PointFeatSize"], specs["EncodeStyle"], specs["SdfScaleFactor"], t(mano), t(obj))
    return z0, tuple(shift_embed(e, torch.tensor(s, dtype=torch.float64)).float() for e, s in zip(E, vc.FIT_START_SHIFTS))


def fit_reference_fp64(steps=40, lr=2e-3, prior=1e-3, clamp=0.05):
    """fit_sample's loss with sdf_hand / sdf_obj alone, step for step, in fp64 on the CPU: the package's nn.Module in float64, the
    targets valued by the fp64 rule.  Returns the history of the data term."""
    import torch
    from alignsdf_amd.fit import shift_embed
    from tests import sdf_grad_cases as gc
    from tests import sdf_vjp_cases as vc
    module = gc.module_for(vc.FIT_TAG, torch.float64)
    pf = int(syn.specs_for(vc.FIT_TAG)["PointFeatSize"])
    a = torch.arange(pf)
    cols = (a[:-3], torch.cat([a[:3], a[-3:]]))                       # the (pf 9, "both") heads' feature columns
    z0, E0 = fit_start()
    z0, E0 = z0.double(), [e.double() for e in E0]
    pts = [torch.from_numpy(fit_points(h)).double() for h in range(2)]
    tgt = [torch.from_numpy(rule(*fit_meshes()[h], pts[h].numpy().astype(np.float32))["sdf"]).clamp(-clamp, clamp) for h in range(2)]
    z = z0.clone().requires_grad_()
    shifts = torch.zeros(2, 3, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([z, shifts], lr=lr)
    history = []
    for _ in range(steps):
        opt.zero_grad()
        data = torch.zeros((), dtype=torch.float64)
        for h in range(2):
            E = shift_embed(E0[h], shifts[h])
            q = torch.zeros(len(pts[h]), pf, dtype=torch.float64).index_copy(1, cols[h], pts[h] @ E[:, :3].t() + E[:, 3])
            f = module(torch.cat([z.reshape(1, -1).expand(len(q), -1), q], 1))[h].reshape(-1)
            data = data + (f.clamp(-clamp, clamp) - tgt[h]).abs().mean()
        (data + prior * ((z - z0) ** 2).mean()).backward()
        history.append(float(data.detach()))
        opt.step()
    return history
