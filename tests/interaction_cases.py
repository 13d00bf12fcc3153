"""Shared pieces of the interaction tests (tests/test_interaction_host.py on the CPU, tests/test_gpu_interaction.py on the GPU): numpy
statements of the two records of csrc/interaction.hip, worded from include/alignsdf_hip.h and not from the kernels; the volumes and value
lists they are compared on; the CPU oracle's fine volumes of the grasp9 samples and the table of their both-negative counts."""
import functools

import numpy as np
import torch

from alignsdf_amd import synthetic as syn

INT_MAX = 0x7fffffff
INF_BITS = 0x7f800000
TAG = "grasp9"
# both-negative voxels of oracle.sdf_oracle.two_pass_volumes (fp32, CPU) on grasp9, samples 0..3: the grasps are built to
# interpenetrate (synthetic.grasp_scene), so the intersection is never empty
ORACLE_BOTH_NEGATIVE = {32: (23, 6, 19, 14), 48: (106, 40, 71, 38)}
NEAR_LEVEL = 4e-6          # the refinement threshold of the sweeps (include/alignsdf_hip.h: asdf_decoder_set_refine)

LATTICE_SHAPES = ((1, 1, 1), (2, 3, 5), (7, 1, 129), (33, 33, 33), (64, 64, 64))
LIST_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 4097)


def overlap_statement(vol_hand, vol_obj):
    """OVERLAP record, int32[16]: [0] voxels with hand < 0, [1] with obj < 0, [2] with both, [3] where either is NaN, [4..6] / [7..9]
    smallest / largest index per axis of the both-negative voxels (INT_MAX / -1 when there is none), rest 0."""
    a, b = np.asarray(vol_hand, np.float32), np.asarray(vol_obj, np.float32)
    assert a.ndim == 3 and a.shape == b.shape
    rec = np.zeros(16, np.int32)
    both = (a < 0) & (b < 0)
    rec[0], rec[1], rec[2], rec[3] = (a < 0).sum(), (b < 0).sum(), both.sum(), (np.isnan(a) | np.isnan(b)).sum()
    where = np.argwhere(both)
    rec[4:7] = where.min(0) if len(where) else INT_MAX
    rec[7:10] = where.max(0) if len(where) else -1
    return rec


def contact_statement(values, tau, count=None):
    """CONTACT record, int32[8], over the first n = min(max(count, 0), len) values (count None: all): [0] n, [1] f < 0, [2] f <= tau,
    [3] NaN, [4] bits of the smallest non-NaN value (-0.0 below +0.0; +inf when there is none), [5] the lowest index that holds it
    (-1 when none), rest 0."""
    f = np.asarray(values, np.float32).reshape(-1)
    n = len(f) if count is None else min(max(int(count), 0), len(f))
    f = f[:n]
    rec = np.zeros(8, np.int32)
    nan = np.isnan(f)
    rec[0], rec[1], rec[2], rec[3] = n, (f < 0).sum(), (f <= np.float32(tau)).sum(), nan.sum()
    cand = np.flatnonzero(~nan)
    if len(cand):
        sub = f[cand]
        first = cand[np.lexsort((cand, ~np.signbit(sub), sub))[0]]      # by value, then -0.0 before +0.0, then by index
        rec[4], rec[5] = f[first:first + 1].view(np.int32)[0], first
    else:
        rec[4], rec[5] = INF_BITS, -1
    return rec


SPECIALS = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, -1e-40, -1.4e-45, 1e-40], np.float32)      # (with negative denormals)


def mixed_values(M, seed):
    """[M] float32: seeded normal values around zero with -0.0, +0.0, NaN, +-inf and denormals mixed in (about one in six)."""
    rng = np.random.default_rng(seed)
    v = (0.05 * rng.standard_normal(M)).astype(np.float32)
    pick = rng.random(M) < 1.0 / 6.0
    v[pick] = SPECIALS[rng.integers(0, len(SPECIALS), int(pick.sum()))]
    return v


def mixed_volume(shape, seed):
    return mixed_values(int(np.prod(shape)), seed).reshape(shape)


def _t(d):
    return None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def oracle_volumes(sample, N=32):
    """(vol_hand, vol_obj, voxel_size, origin) of the CPU oracle's fine pass (fp32) for grasp9 sample `sample`: computed once, shared,
    read-only."""
    from oracle import sdf_oracle as orc
    latent, mano, obj = syn.sample_inputs(TAG, sample)
    r = orc.two_pass_volumes(syn.full_state_dict(TAG), torch.from_numpy(latent), syn.specs_for(TAG), N, _t(mano), _t(obj))
    vh, vo = (np.ascontiguousarray(r[k].numpy(), np.float32) for k in ("vol_hand2", "vol_obj2"))
    vh.setflags(write=False)
    vo.setflags(write=False)
    return vh, vo, float(r["new_voxel_size"]), [float(v) for v in r["new_origin"]]


def near_level_voxels(sample, N=32):
    """Oracle voxels with |value| < NEAR_LEVEL in either fine volume: where a sign may legitimately differ between two fp32 evaluations."""
    vh, vo, _, _ = oracle_volumes(sample, N)
    return int(((np.abs(vh) < NEAR_LEVEL) | (np.abs(vo) < NEAR_LEVEL)).sum())
