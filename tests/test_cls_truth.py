"""The fp64 truth of the label pass (oracle.sdf_oracle.classify_points(dtype=torch.float64)), checked without a GPU: against an
independent formulation - the package's nn.Module in fp64 - against the fp32 oracle, and for the share of points whose label the GPU
tests (tests/test_gpu_cls_fp64.py) may leave out."""
import numpy as np
import pytest
import torch

from oracle import sdf_oracle as orc
from tests import cls_cases as cc


def _module_fp64(tag, pts):
    """Scores of build_decoder(...).double() on orc.point_features in fp64: the module's own forward (weight-norm hook, head slices,
    classifier_head), not the oracle's _run_head."""
    specs = cc.specs_for(tag)
    lat, mano, obj = cc.sample_inputs(tag, 0)
    cast = lambda d: None if d is None else {k: torch.as_tensor(v).double() for k, v in d.items()}
    x = torch.from_numpy(pts).double()
    feats = orc.point_features(x, specs, cast(mano), cast(obj))
    dec = cc.module_for(tag, cc.STD, torch.float64)
    with torch.no_grad():
        scores = dec(torch.cat([torch.from_numpy(lat).double().expand(len(x), -1), feats], 1))[2]
    assert scores.dtype == torch.float64
    return scores.numpy()


@pytest.mark.parametrize("tag", cc.CONFIGS)
def test_fp64_truth(tag):
    pts = cc.points(cc.FULL)
    truth, oracle32, _ = cc.references(tag, cc.FULL)
    assert truth.dtype == np.float64 and truth.shape == (cc.FULL, 6) and oracle32.dtype == np.float32
    tmax = float(np.abs(truth).max())
    # 1. an independent formulation in fp64
    d_mod = float(np.abs(_module_fp64(tag, pts) - truth).max())
    # 2. the fp32 oracle against it
    e_or, r_or = cc.err(oracle32, truth)
    # 3. the label rule of the GPU tests on the reference alone: e = the fp32 oracle's own error
    bound = cc.rule_bound(e_or, e_or, tmax)
    gap = cc.top_two_gap(truth)
    left_out = int((gap <= 2.0 * bound).sum())
    print("CLSTRUTH %-6s M=%d max|truth| %.2f: module fp64 %.2e | fp32 oracle e %.2e rms %.2e | margin %.2e smallest gap %.2e left out %d" % (
        tag, cc.FULL, tmax, d_mod, e_or, r_or, 2.0 * bound, float(gap.min()), left_out))
    assert d_mod <= 1e-12, (tag, d_mod)
    assert e_or <= cc.TOL, (tag, e_or)
    assert left_out <= cc.MAX_LEFT_OUT, (tag, left_out)
    keep = gap > 2.0 * bound
    assert np.array_equal(cc.first_argmax(oracle32)[keep], cc.first_argmax(truth)[keep]), tag


def test_default_dtype_is_the_fp32_oracle():
    """classify_points without `dtype` returns fp32 scores and int64 labels, and dtype=torch.float32 the same bits."""
    tag = "both9"
    lat, mano, obj = cc.sample_inputs(tag, 0)
    args = (cc.state_dict(tag), lat, cc.points(129), cc.specs_for(tag), cc._t(mano), cc._t(obj))
    s, l = orc.classify_points(*args)
    s32, l32 = orc.classify_points(*args, dtype=torch.float32)
    assert s.dtype == torch.float32 and l.dtype == torch.int64 and torch.equal(s, s32) and torch.equal(l, l32)
    s64, l64 = orc.classify_points(*args, dtype=torch.float64)
    assert s64.dtype == torch.float64 and l64.dtype == torch.int64 and float((s64 - s.double()).abs().max()) <= cc.TOL


def test_kernel_table_covers_every_instantiation():
    """The ten configurations reach all six kernels of csrc/k1_cls_kernels.hip, and ONE_PER_KERNEL names one of each."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alignsdf_amd", "csrc", "k1_cls_kernels.hip")).read()
    built = set(re.findall(r"void (sdf_mlp_\w*cls_kernel)\(", src))
    assert len(built) == 6 and built == {v[0] for v in cc.KERNEL_OF.values()}
    assert {cc.KERNEL_OF[t][0] for t in cc.ONE_PER_KERNEL} == built and set(cc.KERNEL_OF) == set(cc.CONFIGS)
