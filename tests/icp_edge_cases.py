"""Point sets for the edges of the ICP / Chamfer neighbour search (K7, csrc/icp.hip) and a host restatement of the cell choice
of its uniform grid.  TEST INFRASTRUCTURE ONLY: shared by tests/test_oracle_icp.py (CPU pins) and tests/test_gpu_icp_edges.py."""
import numpy as np

from alignsdf_amd import synthetic as syn

GRID_MAX_RES = 64          # kGridMaxRes
SCAN_ROUND = 4096          # cells per round of grid_scan_kernel's one workgroup (1024 threads x one int4)
UPDATE_THREADS = 256       # kIcpThreads
UPDATE_GRID = 64           # kIcpUpdateGrid
FORCE_GRID_BELOW = 1024    # use_grid(): mode 0 takes the grid when both sets have at least this many points


def grid_cells(points):
    """grid_bbox_kernel's choice for a reference set, restated: the resolution from the point count alone, the cell edge h from
    the longest extent, g[a] = floor(ext_a / h) + 1 cells per axis.  Returns (res, h, (g0, g1, g2), ncell)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(p)
    res = int(1.5 * np.cbrt(float(n)) + 0.5)
    res = 4 if res < 4 else (GRID_MAX_RES if res > GRID_MAX_RES else res)
    ext_a = p.max(0) - p.min(0)
    ext = max(0.0, float(ext_a.max()))
    h = ext / res if ext > 0.0 else 1.0
    h *= 1.0 + 1e-9
    inv_h = 1.0 / h
    g = tuple(min(max(int(np.floor(e * inv_h)) + 1, 1), res + 1) for e in ext_a)
    return res, h, g, g[0] * g[1] * g[2]


def box_points(n, seed, box=(1.0, 1.0, 1.0)):
    """n uniform points in [0, box] that include the two opposite corners, so the bounding box is the box exactly."""
    p = syn.uniform((n, 3), seed) * np.asarray(box, np.float64)
    p[n // 3] = 0.0
    p[(2 * n) // 3] = box
    return np.ascontiguousarray(p)


# the three cubes whose cell counts steer grid_scan_kernel: under one round, exactly one round, one round and a tail that is no
# multiple of the four cells a thread loads at once
CUBES = {1024: 15, 1200: 16, 1500: 17}


def icp_pair(ns, nt, seed):
    """The generator of tests/test_gpu_icp.py::test_icp_iteration_count_and_ragged_sizes."""
    tgt = syn.normal((nt, 3), 50 + seed) * np.array([0.1, 0.06, 0.04]) + 0.3
    src = (syn.normal((ns, 3), 60 + seed) * np.array([0.1, 0.06, 0.04]) + 0.3 - 0.02) / 1.1
    return src, tgt, syn.normal((40, 3), 70 + seed)


def tie_lattice(m=12):
    """(a, b): b = the lattice arange(m)/8 cubed, a = b + 1/16.  Coordinates, differences and squared distances are exact in fp64;
    an interior query of `a` has the eight corners of its lattice cell of `b` at the same distance."""
    g = np.stack(np.meshgrid(*[np.arange(m) / 8.0] * 3, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(g + 1.0 / 16.0), np.ascontiguousarray(g)


def tied_queries(queries, refs, d2):
    """How many queries have more than one reference point at exactly their nearest squared distance `d2` (fp64, the kernels'
    expression)."""
    q, r = np.asarray(queries, np.float64), np.asarray(refs, np.float64)
    count = 0
    for lo in range(0, len(q), 128):
        d = q[lo:lo + 128, None, :] - r[None, :, :]
        d = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        count += int(((d == d2[lo:lo + 128, None]).sum(1) > 1).sum())
    return count


def sphere_points(n, seed, radius, centre=(0.0, 0.0, 0.0)):
    u = syn.normal((n, 3), seed)
    return np.ascontiguousarray(u / np.linalg.norm(u, axis=1, keepdims=True) * radius + np.asarray(centre, np.float64))
