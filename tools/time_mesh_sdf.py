"""Time the mesh signed distance kernels (csrc/mesh_sdf.hip) against the same rule written in torch on the same GPU - what a user
would write today - and the ground-truth interaction flow per sample.  Writes profiles/mesh_sdf.txt (--out).

    python tools/time_mesh_sdf.py [--out profiles/mesh_sdf.txt] [--repeats 5]

Per shape (M queries, T faces): the kernel row is one MeshField.at call - its output allocations and the size query included, as the
torch statement's are - so the smallest shape, two launches over 1.2 M pairs, is partly host time.  Both are warmed up, then timed
alternately between device events; the medians, the pair rate M T / t and the ratio are reported, and the largest differences between the two results (the torch statement sums the winding number in
torch's own order, so w differs in the last bits).  The torch statement is chunked over the queries to 2^22 pairs a piece.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from alignsdf_amd import synthetic as syn  # noqa: E402
from alignsdf_amd.mesh_sdf import MeshField  # noqa: E402
from tests import mesh_sdf_cases as mc  # noqa: E402  (its torus builder)

SHAPES = ((778, 1538), (30000, 1538), (30000, 20480), (262144, 20480))
PAIRS_PER_PIECE = 1 << 22


def mesh_of(T):
    """T faces: the closed 80 x 128 torus (20 480), or the first T faces of the 24 x 33 one (1 538 - a hand mesh's count)."""
    v, f = mc.torus(80, 128) if T == 20480 else mc.torus(24, 33)
    assert len(f) >= T
    return v, f[:T]


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def torch_rule(verts, faces, xyz):
    """(sdf [M], w [M]) of the rule of include/alignsdf_hip.h as a user writes it in torch: all pairs of a piece at once."""
    f = faces.long().sort(1).values                      # corners in index order, as the rule words it
    flip = ((faces[:, 0] < faces[:, 1]).int() + (faces[:, 1] < faces[:, 2]).int() + (faces[:, 2] < faces[:, 0]).int()) == 1
    sigma = torch.where(flip, -1.0, 1.0).to(verts.dtype)
    a, b, c = (verts[f[:, k]][None] for k in range(3))
    ab, ac, bc = b - a, c - a, c - b
    out_sdf, out_w = [], []
    step = max(1, PAIRS_PER_PIECE // max(1, len(faces)))
    for first in range(0, len(xyz), step):
        P = xyz[first:first + step][:, None, :]
        ap, bp, cp = P - a, P - b, P - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        s = (va + vb) + vc
        q = (a + (vb / s)[..., None] * ab) + (vc / s)[..., None] * ac
        # the regions in reverse order, so that the first match of the rule is the last one written
        for cond, point in (((va <= 0) & (e43 >= 0) & (e56 >= 0), lambda: b + (e43 / (e43 + e56))[..., None] * bc),
                            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), lambda: a + (d2 / (d2 - d6))[..., None] * ac),
                            ((d6 >= 0) & (d5 <= d6), lambda: c.expand_as(q)),
                            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), lambda: a + (d1 / (d1 - d3))[..., None] * ab),
                            ((d3 >= 0) & (d4 <= d3), lambda: b.expand_as(q)),
                            ((d1 <= 0) & (d2 <= 0), lambda: a.expand_as(q))):
            q = torch.where(cond[..., None], point(), q)
        r = P - q
        dist = torch.sqrt(_dot(r, r).min(1).values)
        A, B, C = -ap, -bp, -cp
        la, lb, lc = torch.sqrt(_dot(A, A)), torch.sqrt(_dot(B, B)), torch.sqrt(_dot(C, C))
        det = _dot(A, torch.cross(B, C, dim=-1))
        den = (((la * lb) * lc + _dot(A, B) * lc) + _dot(B, C) * la) + _dot(C, A) * lb
        w = (sigma * torch.atan2(det, den)).sum(1) / (2.0 * np.pi)
        out_sdf.append(torch.where(w.abs() >= 0.5, -dist, dist))
        out_w.append(w)
    return torch.cat(out_sdf), torch.cat(out_w)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def kernel_rows(repeats, emit):
    for M, T in SHAPES:
        v, f = mesh_of(T)
        field = MeshField(v, f)
        lo, hi = v.min(0), v.max(0)
        xyz = torch.from_numpy((lo - 0.1 + syn.uniform((M, 3), 46000 + T) * (hi - lo + 0.2)).astype(np.float32)).cuda()
        vd, fd = field.verts, field.faces
        kernel = lambda: field.at(xyz, winding=True)
        statement = lambda: torch_rule(vd, fd, xyz)
        k, t = kernel(), statement()                       # warm-up of both, and the comparison of their results
        kernel(), torch.cuda.synchronize()
        d_sdf = (k.sdf.abs() - t[0].abs()).abs().max().item()
        d_w = (k.winding - t[1]).abs().max().item()
        signs = int(((k.sdf < 0) != (t[0] < 0)).sum())
        tk, tt = [], []
        for _ in range(repeats):                           # alternated
            tk.append(timed(kernel)[0])
            tt.append(timed(statement)[0])
        mk, mt = float(np.median(tk)), float(np.median(tt))
        emit("M=%d T=%d kernel %.3f ms (%.2f G pairs/s; runs %s) | torch statement %.2f ms (%.3f G pairs/s; runs %s) | kernel %.1f x the "
             "statement | results: max ||sdf| difference| %.2e, max |w difference| %.2e, signs that differ %d" % (
                 M, T, mk, M * T / mk / 1e6, " ".join("%.3f" % x for x in tk), mt, M * T / mt / 1e6, " ".join("%.1f" % x for x in tt),
                 mt / mk, d_sdf, d_w, signs))


def flow_rows(repeats, emit, N=64, samples=(0, 1, 2, 3)):
    """gt_interaction.run on synthetic grasps written as OBJ (marching cubes of synthetic.grasp_sdf at N^3; file units = normalised
    units, taken as 0.1 m each: --unit_m 0.1, so the 2 mm lattice is 0.02 units)."""
    from alignsdf_amd import gt_interaction as gi
    from alignsdf_amd.marching_cubes import marching_cubes_device
    from alignsdf_amd.utils.mesh import lattice_points
    origin, voxel = [-1.0, -1.0, -1.0], 2.0 / (N - 1)
    idx = np.stack(np.meshgrid(*[np.arange(N, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = lattice_points(torch.from_numpy(idx), origin, voxel).numpy()
    with tempfile.TemporaryDirectory() as tmp:
        sizes = []
        for s in samples:
            for part, values in zip(("mesh_hand", "mesh_obj"), syn.grasp_sdf(pts, s)):
                verts, faces = marching_cubes_device(torch.from_numpy(values.astype(np.float32).reshape(N, N, N)).cuda(), 0.0)
                verts, faces = lattice_points(verts, origin, voxel).cpu().numpy(), faces.cpu().numpy()
                os.makedirs(os.path.join(tmp, "data", "obman", "test", part), exist_ok=True)
                with open(os.path.join(tmp, "data", "obman", "test", part, "grasp%d.obj" % s), "w") as fh:
                    fh.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in verts.tolist()))
                    fh.write("".join("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1) for t in faces.tolist()))
                sizes.append((len(verts), len(faces)))
        run = lambda: gi.run(os.path.join(tmp, "exp"), "obman", os.path.join(tmp, "data"), unit_m=0.1)
        run()                                              # warm-up
        times = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, summary, _ = run()
            times.append((time.perf_counter() - t0) * 1e3 / len(samples))      # (every record has crossed to the host: the flow has ended)
        emit("gt_interaction flow, %d synthetic grasps (N=%d marching cubes; vertices / faces per mesh: %s): %.1f ms per sample with "
             "reading the OBJ files (runs %s)" % (len(samples), N, " ".join("%d/%d" % s for s in sizes), float(np.median(times)),
                                                  " ".join("%.1f" % x for x in times)))
        emit("  " + str(summary))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sdf.txt"))
    p.add_argument("--repeats", type=int, default=5)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("a GPU is needed: nothing here is measured without one")
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    emit("# Mesh signed distance kernels (csrc/mesh_sdf.hip, alignsdf_amd/mesh_sdf.py): tools/time_mesh_sdf.py on one MI355X")
    prop = torch.cuda.get_device_properties(0)
    emit("# %s, %s, %d CUs, %.0f GiB | torch %s | device events, warm-up, median of %d alternated runs; cost model M x T pairs, no culling" % (
        prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, torch.__version__, a.repeats))
    emit("# (a kernel row is one MeshField.at call with its allocations: the M=778 row, two launches over 1.2 M pairs, is partly host time)")
    kernel_rows(a.repeats, emit)
    flow_rows(a.repeats, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
