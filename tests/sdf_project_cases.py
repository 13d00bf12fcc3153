"""Shared pieces of the projection tests (tests/test_sdf_project_truth.py on the CPU, tests/test_gpu_sdf_project.py on the GPU): the
point sets - edge-crossing vertices of the fp64 truth on a small lattice, i.e. what marching cubes would hand the projection - the
rule variants, and the fp32 / fp64 references built on tests/sdf_grad_cases.grad_truth."""
import functools

import numpy as np
import torch

from alignsdf_amd import synthetic as syn
from tests import sdf_grad_cases as gc

SAMPLE = gc.SAMPLE
LIST_LENGTHS = gc.LIST_LENGTHS      # edges of the 8-per-wave / 32-per-workgroup tiling
TOL = 1e-6
# (tag, head) -> (N, lo, hi) of the lattice its vertices come from, and the number of vertices it has
LATTICES = {("both9", "hand"): (32, -1.0, 1.0), ("both9", "obj"): (32, -1.0, 1.0), ("grasp3", "hand"): (48, -0.6, 0.6)}
TRUTH_LABELS = ("both9 hand M=4097 jittered", "both9 obj M=1024 jittered", "grasp3 hand 3258")      # of truth_sets()
VERTEX_COUNTS = {("both9", "hand"): 354, ("both9", "obj"): 118, ("grasp3", "hand"): 3258}


def voxel(tag, head):
    N, lo, hi = LATTICES[(tag, head)]
    return (hi - lo) / (N - 1)


def rules(tag="both9", head="hand"):
    """The three rule variants of the GPU sets: (max_iters, max_move) = (8, 1 voxel), (3, 1 voxel), (8, 0.1 voxel)."""
    v = voxel(tag, head)
    base = {"tol": TOL, "min_grad2": 1e-12}
    return {"8/1": dict(base, max_iters=8, max_move=v), "3/1": dict(base, max_iters=3, max_move=v),
            "8/0.1": dict(base, max_iters=8, max_move=0.1 * v)}


def sdf64(tag, sample, pts, chunk=1 << 15):
    """{"hand" / "obj": sdf [M]} of the oracle's decode chain in fp64 (values only: the lattices are too big to differentiate)."""
    from oracle import sdf_oracle as orc
    dtype = torch.float64
    sd, specs = gc.state_dict(tag), syn.specs_for(tag)
    latent, mano, obj = syn.sample_inputs(tag, sample)
    cast = lambda d: None if d is None else {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}
    mano, obj = cast(mano), cast(obj)
    hp, op = orc.effective_head_params(sd, "h", dtype), orc.effective_head_params(sd, "o", dtype)
    lat = torch.as_tensor(latent).to(dtype).reshape(1, -1)
    x = torch.as_tensor(np.array(pts, np.float32)).to(dtype)
    out = {"hand": [], "obj": []}
    with torch.no_grad():
        for i in range(0, len(x), chunk):
            h, o = orc.decode_sdf_multi_output(hp, op, lat, orc.point_features(x[i:i + chunk], specs, mano, obj), specs)
            out["hand"].append(h.reshape(-1).numpy())
            out["obj"].append(o.reshape(-1).numpy())
    return {k: np.concatenate(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _lattice_sdf(tag, N, lo, hi):
    axis = np.linspace(lo, hi, N).astype(np.float32).astype(np.float64)
    grid = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    vals = sdf64(tag, SAMPLE, grid)
    return axis, {k: v.reshape(N, N, N) for k, v in vals.items()}


@functools.lru_cache(maxsize=None)
def vertices(tag, head):
    """[V, 3] float32: on every lattice edge whose ends differ in sign in the fp64 truth of head `head`, the vertex of the linear
    interpolation (edges along axis 0 first, then 1, then 2, each in index order)."""
    N, lo, hi = LATTICES[(tag, head)]
    axis, vols = _lattice_sdf(tag, N, lo, hi)
    vol = vols[head]
    out = []
    for a in range(3):
        sl0 = [slice(None)] * 3
        sl1 = [slice(None)] * 3
        sl0[a], sl1[a] = slice(0, N - 1), slice(1, N)
        f0, f1 = vol[tuple(sl0)], vol[tuple(sl1)]
        idx = np.argwhere((f0 < 0) != (f1 < 0))
        t = f0[tuple(idx.T)] / (f0[tuple(idx.T)] - f1[tuple(idx.T)])
        p = axis[idx]                              # [E, 3]: the edge's lower end
        p[:, a] = p[:, a] + t * (axis[idx[:, a] + 1] - axis[idx[:, a]])
        out.append(p)
    v = np.concatenate(out).astype(np.float32)
    v.setflags(write=False)
    return v


def list_set(M, tag="both9", head="hand", seed=None):
    """[M, 3] float32: the head's vertices cycled to length M plus a seeded jitter of +-0.25 voxel per axis."""
    v = vertices(tag, head)
    rng = np.random.default_rng(1000 + M if seed is None else seed)
    base = v[np.arange(M) % len(v)].astype(np.float64)
    return (base + rng.uniform(-0.25, 0.25, (M, 3)) * voxel(tag, head)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def truth_sets():
    """((label, tag, head, points)) of the three sets the convergence claims are made on."""
    sets = ((TRUTH_LABELS[0], "both9", "hand", list_set(4097, "both9", "hand")),
            (TRUTH_LABELS[1], "both9", "obj", list_set(1024, "both9", "obj")),
            (TRUTH_LABELS[2], "grasp3", "hand", np.array(vertices("grasp3", "hand"))))
    for s in sets:
        s[3].setflags(write=False)
    return sets


def mixed_set(M, head):
    """list_set(M) of both9 with two non-finite rows and a few far-field points (sdf_grad_cases.points) mixed in where M allows."""
    pts = list_set(M, "both9", head).copy()
    if M >= 9:
        pts[3] = (np.nan, 0.1, 0.2)
        pts[M - 2] = (0.3, np.inf, -0.1)
        far = gc.points(4, 77)
        pts[5:7] = far[:2]
        if M >= 33:
            pts[M // 2: M // 2 + 2] = far[2:]
    return pts


def oracle_grad_of(tag, head, dtype=torch.float32):
    """points (tensor [M, 3]) -> (sdf, grad) tensors of grad_truth in `dtype` on the CPU: the fp32 oracle chain the rule runs over in
    the CPU tests."""
    def grad_of(points):
        r = gc.grad_truth(tag, SAMPLE, points.detach().cpu().numpy(), dtype)[head]
        return torch.from_numpy(np.ascontiguousarray(r["sdf"])), torch.from_numpy(np.ascontiguousarray(r["grad"]))
    return grad_of


@functools.lru_cache(maxsize=None)
def reference(label, rule="8/1"):
    """project_lockstep over the fp32 oracle chain on one of truth_sets(), as numpy arrays."""
    from alignsdf_amd.project import project_lockstep
    _, tag, head, pts = next(s for s in truth_sets() if s[0] == label)
    res = project_lockstep(oracle_grad_of(tag, head), torch.from_numpy(np.array(pts)), **rules(tag, head)[rule])
    return {k: v.numpy() for k, v in res.items()}
