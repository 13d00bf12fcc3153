"""Shared pieces of the auto-decode tests (tests/test_fit_code_truth.py on the CPU, tests/test_gpu_fit_code.py on the GPU): the fp64
statements of the fit's two rules - the clamped-L1 weight and the Adam step - written out independently of alignsdf_amd.fit, and the
target lists of the device tests."""
import functools

import numpy as np

from tests import sdf_vjp_cases as vc

TAG, SAMPLE, OTHER_SAMPLE = "both9", vc.SAMPLE, vc.SAMPLE + 1
CLAMP = 0.06                      # the synthetic fields have |f| around 0.05: a clamp that cuts a share of the points, not all
STEP_TOL = 16 * 2.0 ** -24        # per Adam step, relative, on z - z_prev (see test_fit_code_truth)
VARIANTS = ("hand", "obj", "both", "disjoint")


def loss_rule_f64(f, t, c, n):
    """(l, w) of the loss form in numpy fp64: r = clip(f) - clip(t), l = |r| (0 where t is NaN), w = 0 where t is NaN or f is outside
    [-c, c], else sign(r) / n."""
    f, t = np.asarray(f, np.float64), np.asarray(t, np.float64)
    out = np.isnan(t)
    r = np.clip(f, -c, c) - np.clip(np.where(out, 0.0, t), -c, c)
    l = np.where(out, 0.0, np.abs(r))
    w = np.where(out | (f < -c) | (f > c), 0.0, np.sign(r) * (1.0 / n if n else 0.0))
    return l, w


def adam_f64(z, m, v, d, z0, k_prior, lr_k, k, b1, b2, eps):
    """One Adam step on g = d + k_prior (z - z0) in fp64, the textbook way: the bias corrections applied to m and v, eps added to
    sqrt(v_hat).  Returns (z, m, v)."""
    g = d + k_prior * (z - z0)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    m_hat, v_hat = m / (1.0 - b1 ** (k + 1)), v / (1.0 - b2 ** (k + 1))
    return z - lr_k * m_hat / (np.sqrt(v_hat) + eps), m, v


def long_list(num_cus):
    """A list length above 128 num_cus: some workgroup of the persistent grid takes a second tile."""
    return 128 * int(num_cus) + 77


@functools.lru_cache(maxsize=None)
def targets(M, variant, seed=5):
    """(t_hand, t_obj, n_hand, n_obj) float32 / None for a list of M points: uniform in [-0.09, 0.09] (some beyond the clamp).
    "disjoint": the hand owns the head of the list and the object the rest, cut at a tile edge where there is one - the last tile is
    all NaN for the hand."""
    rng = np.random.default_rng(seed + M)
    raw = [rng.uniform(-0.09, 0.09, M).astype(np.float32) for _ in range(2)]
    if variant == "hand":
        return raw[0], None, M, 0
    if variant == "obj":
        return None, raw[1], 0, M
    if variant == "both":
        return raw[0], raw[1], M, M
    cut = ((M - 1) // 128) * 128 if M > 128 else (M + 1) // 2
    th, to = raw[0].copy(), raw[1].copy()
    th[cut:], to[:cut] = np.nan, np.nan
    return th, to, cut, M - cut


@functools.lru_cache(maxsize=None)
def truth_case(M=4097):
    """The fp64 one-step case on both9: points, the targets (the field of ANOTHER sample's code, so f - t is generically far from 0),
    the clear masks and the fp64 weights.  A point is clear for a head when every ReLU pre-activation, |f - t| and ||f| - c| are more
    than CLEAR_EPS from their kinks in fp64; the weights are 0 elsewhere.  Returns {"pts", "t": {head}, "clear": {head}, "w64": {head}}."""
    pts = vc.list_points(M)
    here, there = vc.vjp_truth(TAG, SAMPLE, pts, {}), vc.vjp_truth(TAG, OTHER_SAMPLE, pts, {})
    out = {"pts": pts, "t": {}, "clear": {}, "w64": {}}
    for name in vc.HEADS:
        f, t = here["sdf"][name], there["sdf"][name].astype(np.float32).astype(np.float64)
        clear = (here["minz"][name] > vc.CLEAR_EPS) & (np.abs(f - t) > vc.CLEAR_EPS) & (np.abs(np.abs(f) - CLAMP) > vc.CLEAR_EPS)
        _, w = loss_rule_f64(f, t, CLAMP, M)
        out["t"][name], out["clear"][name], out["w64"][name] = t.astype(np.float32), clear, np.where(clear, w, 0.0)
    return out
