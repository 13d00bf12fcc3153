"""Volumes and shapes for the layout edges of the marching-cubes chain (K3-K6, csrc/mc33.hip) and a host restatement of the layout
that mc_layout picks for a shape.  TEST INFRASTRUCTURE ONLY: shared by tests/test_mc_edge_cases.py (CPU pins of the case tables)
and tests/test_gpu_mc_edges.py.  numpy only."""
import numpy as np

from alignsdf_amd import synthetic as syn

CLASSIFY_THREADS = 256     # kMcThreads
CELLS_PER_THREAD = 4       # kMcCellsPerThread: one thread of mc_classify takes a group of 4 x-consecutive cell slots
CHUNK = 1024               # kMcChunk = kMcThreads * kMcCellsPerThread: cell slots per workgroup of mc_classify, per block of the emit
EMIT_WAVE = 64             # kEmitThreads: one wave per block in mc_emit_verts / mc_emit_faces; the stride of block_first_ids' sum
WAVE = 64                  # lanes of a wave of mc_classify: lane 63 never has a neighbour lane for its fifth value
FINALIZE_THREADS = 1024    # super-blocks per round of mc_finalize's one workgroup


def layout(shape):
    """mc_layout restated for an (nz, ny, nx) volume.  `vec`: mc_classify takes the float4 path when the base pointer is 16-byte
    aligned; `has_tail`: a row's last value is the fifth element of its last group (nx % 4 == 1)."""
    nz, ny, nx = (int(n) for n in shape)
    assert min(nz, ny, nx) >= 2
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    cxp = (cx + 3) & ~3
    nslots = cxp * cy * cz
    nblocks = (nslots + CHUNK - 1) // CHUNK
    sb_shift = 0
    while (1 << (2 * sb_shift)) < nblocks:
        sb_shift += 1
    nsuper = (nblocks + (1 << sb_shift) - 1) >> sb_shift
    return {"cx": cx, "cy": cy, "cz": cz, "cxp": cxp, "nslots": nslots, "nblocks": nblocks, "sb_shift": sb_shift, "nsuper": nsuper,
            "groups_per_row": cxp // CELLS_PER_THREAD, "vec": nx % 4 == 0, "has_tail": nx % 4 == 1}


# ---- volume builders (float32, C order) -------------------------------------------------------------------------------------------

def shape_seed(shape):
    return 40000 + 10007 * shape[0] + 101 * shape[1] + shape[2]


def dense(shape, seed):
    """Uniform noise in [-1, 1]: nearly every cell is active, most sign patterns occur."""
    return syn.uniform(shape, seed, -1.0, 1.0).astype(np.float32)


def smooth_noise(shape, seed, noise=0.3):
    """The field of tests/test_gpu_mc.py::test_large_volumes_vs_oracle: a smooth surface plus noise (ambiguous cells)."""
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij"), -1)
    smooth = np.sin(4.0 * g[..., 0]) * np.cos(3.0 * g[..., 1]) + 0.5 * np.sin(6.0 * g[..., 2] + 1.0)
    return (smooth + noise * syn.uniform(shape, seed, -1.0, 1.0)).astype(np.float32)


def checkerboard(shape, seed):
    """Sign (-1)^(x + y + z) times a magnitude in [0.1, 1]: every cell has the sign pattern 0x5A or 0xA5 (MC33 case 13), the cells
    with the most triangles, the most owned vertices and the cell-centre vertex."""
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    sign = 1.0 - 2.0 * ((x + y + z) & 1)
    return (sign * syn.uniform(shape, seed, 0.1, 1.0)).astype(np.float32)


def two_ends(shape):
    """-1 everywhere, +1 at voxel (1, 1, 1) and at (nz - 2, ny - 2, nx - 2): surface in the first and in the last block only."""
    vol = np.full(shape, -1.0, np.float32)
    vol[1, 1, 1] = 1.0
    vol[shape[0] - 2, shape[1] - 2, shape[2] - 2] = 1.0
    return vol


FIELDS = {"dense": (dense, 0.0), "smooth_noise": (smooth_noise, 0.05)}        # name -> (builder, level)


def field(name, shape):
    """(volume, level) of one of FIELDS on `shape`, seeded by the shape."""
    build, level = FIELDS[name]
    return build(shape, shape_seed(shape)), level


# ---- A. row tails and thin shapes -------------------------------------------------------------------------------------------------
ROW_TAIL_SHAPES = ([(3, 5, nx) for nx in range(2, 10)]
                   + [(2, 9, 2), (9, 2, 2), (2, 3, 4), (3, 2, 4), (2, 3, 5)]
                   + [(3, 3, nx) for nx in range(256, 261)]             # 64 / 65 groups per row: a wave's last lane inside a row
                   + [(5, 4, 1028), (3, 3, 4100)]                       # rows longer than one block's 1024 slots
                   + [(17, 33, 64)])

# ---- B. misaligned base pointer ---------------------------------------------------------------------------------------------------
MISALIGNED_SHAPES = [(3, 5, 8), (3, 3, 260), (17, 33, 64)]
MISALIGNED_OFFSETS = [1, 2, 3]                                          # floats
PERMUTED_SHAPE, PERMUTATION = (5, 8, 12), (2, 0, 1)

# ---- C. long super-blocks ---------------------------------------------------------------------------------------------------------
LONG_SUPER_SHAPES = [(9, 9, 66000), (162, 162, 162)]
LONG_SUPER_FIELDS = ["smooth_noise", "two_ends"]


def long_super_volume(name, shape):
    if name == "two_ends":
        return two_ends(shape), 0.0
    return field(name, shape)


# ---- D. where the extreme value sits ----------------------------------------------------------------------------------------------
EXTREME_SHAPES = [(5, 6, 8), (5, 6, 9), (5, 6, 10), (5, 6, 11), (2, 2, 9), (9, 2, 2), (4, 4, 64)]


def extreme_positions(shape):
    """The positions whose every coordinate is the first, a middle or the last of its axis, as (label, (z, y, x)): 27 of them, fewer
    where an axis has two voxels (its middle is its last)."""
    axes = []
    for n in shape:
        named = {0: "first", n // 2: "mid", n - 1: "last"}              # (later names win: on an axis of 2, index 1 is `last`)
        axes.append(sorted(named.items()))
    return [("%s-%s-%s" % (lz, ly, lx), (z, y, x)) for z, lz in axes[0] for y, ly in axes[1] for x, lx in axes[2]]


def extreme_noise(shape, pos, value):
    """Uniform noise in [-0.5, 0.5] with the voxel `pos` set to `value` (+1 or -1): the volume's only maximum / minimum."""
    vol = syn.uniform(shape, shape_seed(shape) + 7, -0.5, 0.5).astype(np.float32)
    vol[pos] = value
    return vol


def one_corner(shape, pos, value):
    """-value everywhere, `value` at `pos`: the surface is the one corner around that voxel."""
    vol = np.full(shape, -value, np.float32)
    vol[pos] = value
    return vol


# ---- E. levels --------------------------------------------------------------------------------------------------------------------
LEVEL_SHAPE_ULP, LEVEL_SHAPE_ZERO, LEVEL_SHAPE_RANGE = (7, 10, 13), (6, 7, 9), (6, 6, 6)
B32 = np.float32(0.3)


def _pick(shape, seed, values):
    idx = np.minimum((syn.uniform(shape, seed) * len(values)).astype(np.int64), len(values) - 1)
    return np.asarray(values)[idx]


def ulp_volume():
    """Values from {b - 2 ulp .. b + 2 ulp, 0.29, 0.31, -1, 1} around b = float32(0.3)."""
    up1 = np.nextafter(B32, np.float32(np.inf))
    dn1 = np.nextafter(B32, np.float32(-np.inf))
    values = np.array([np.nextafter(dn1, np.float32(-np.inf)), dn1, B32, up1, np.nextafter(up1, np.float32(np.inf)),
                       0.29, 0.31, -1.0, 1.0], np.float32)
    return np.ascontiguousarray(_pick(LEVEL_SHAPE_ULP, 51001, values), np.float32)


def ulp_levels():
    """(name, level) around b: b itself, the double midpoints to its float neighbours, the double 0.3 (below b: float32(0.3) is
    0.3 rounded up), the doubles next to b.  `below_b` tells on which side of the voxel value b the level lies: c > level holds
    for c = b exactly at the levels below it."""
    b = float(B32)
    up, dn = float(np.nextafter(B32, np.float32(np.inf))), float(np.nextafter(B32, np.float32(-np.inf)))
    return [("b", b), ("mid_below", 0.5 * (dn + b)), ("mid_above", 0.5 * (b + up)), ("double_0.3", 0.3),
            ("double_below_b", float(np.nextafter(b, -np.inf))), ("double_above_b", float(np.nextafter(b, np.inf)))]


ULP_LEVELS_BELOW_B = ("mid_below", "double_0.3", "double_below_b")

# bit patterns: +0, -0, +-2^-149 (the float nearest 1e-45), +-float32(1e-38) (a denormal), +-1
ZERO_BITS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x006CE3EE, 0x806CE3EE, 0x3F800000, 0xBF800000], np.uint32)
ZERO_LEVELS = [("+0", 0.0), ("-0", -0.0), ("+denorm", 5e-324), ("-denorm", -5e-324)]


def zero_volume():
    """Values from {+-0, +-1e-45, +-1e-38, +-1}, built from their bit patterns."""
    return np.ascontiguousarray(_pick(LEVEL_SHAPE_ZERO, 51002, ZERO_BITS).astype(np.uint32)).view(np.float32)


def range_volume():
    return dense(LEVEL_SHAPE_RANGE, 51003)


# ---- F. bounded emit --------------------------------------------------------------------------------------------------------------
BOUNDED_SLACK_ROWS = 64
VERT_SENTINEL, FACE_SENTINEL = 0x7FC5A5A5, 0x5A5A5A5A                   # a quiet NaN with a payload / no valid vertex id


def bounded_volumes():
    return [("dense12", dense((12, 12, 12), 52001)), ("checker6x6x64", checkerboard((6, 6, 64), 52002))]


def caps(count):
    return [0, 1, count - 1, count, count + 1]


# ---- G. one workspace, many volumes -----------------------------------------------------------------------------------------------
WORKSPACE_SHAPES = [(6, 6, 64), (7, 9, 30)]                             # vector / scalar path, two blocks each


def workspace_sequence(shape):
    """dense, two_ends, checkerboard, dense again: many active cells, then almost none, then the most, then the first again."""
    first = dense(shape, shape_seed(shape) + 1)
    return [("dense", first), ("two_ends", two_ends(shape)), ("checkerboard", checkerboard(shape, shape_seed(shape) + 2)),
            ("dense_again", first)]


# ---- H. dense blocks --------------------------------------------------------------------------------------------------------------
DENSE_BLOCK_CASES = [("checkerboard", (8, 9, 12)), ("checkerboard", (6, 6, 64)), ("dense", (4, 4, 1028))]


def dense_block_volume(name, shape):
    if name == "checkerboard":
        return checkerboard(shape, shape_seed(shape) + 3)
    return dense(shape, shape_seed(shape) + 3)


# ---- I. ABI edges -----------------------------------------------------------------------------------------------------------------
BAD_DIMS = [(1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (4, 4, -3)]
TOO_MANY_VOXELS = (2048, 2048, 513)


def cell_triangle_counts(volume, level, oracle):
    """Triangles of every cell of `volume`, each cell run through `oracle` (marching_cubes_raw) as its own 2 x 2 x 2 volume; 0 for
    a cell without surface."""
    nz, ny, nx = volume.shape
    out = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for z in range(nz - 1):
        for y in range(ny - 1):
            for x in range(nx - 1):
                try:
                    out[z, y, x] = len(oracle(volume[z:z + 2, y:y + 2, x:x + 2], level)[1])
                except (ValueError, RuntimeError):
                    pass
    return out
