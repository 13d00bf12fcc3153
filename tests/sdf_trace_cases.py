"""Shared pieces of the ray-tracing tests (tests/test_sdf_trace_truth.py on the CPU, tests/test_gpu_sdf_trace.py on the GPU): the ray
sets, `march` - the rule of asdf_trace_rays (include/alignsdf_hip.h) as a numpy float32 state machine over any evaluator - and
`trace_truth`, the same rule over oracle.sdf_oracle's decoder in fp64 (or fp32).

Positions and t are fp32 everywhere: the rule is an fp32 rule, and only the decoder changes precision.  A MARCH sample whose |f| is
within rounding of 0 may legitimately take either sign in fp32, and a different sign is a different path (a bracket one step later,
or another surface altogether).  So comparisons against the fp64 truth run over the DECIDED rays of a head: those whose smallest |f|
over their MARCH samples exceeds DECIDE_EPS.  The share of decided rays is a condition of every set (test_sdf_trace_truth.py asserts
it on the truth alone)."""
import functools
import os
import re

import numpy as np
import torch

from alignsdf_amd import synthetic as syn
from tests.sdf_grad_cases import _head_slices, state_dict

MISS, HIT, INSIDE, EXHAUSTED = 0, 1, 2, 3
DECIDE_EPS = 1e-5
MIN_DECIDED_SHARE = 0.90
MIN_HITS = 50
SAMPLE = 1
ORIGIN = (0.1, -0.2, -1.6)
BOX = ((-0.6, -0.6, -0.6), (0.6, 0.6, 0.6))
RULE = {"max_steps": 64, "refine_steps": 6, "step_scale": 1.0, "min_step": 1e-3, "max_step": 0.05}
LIST_LENGTHS = (1, 31, 32, 33, 127, 128, 129, 257, 1000)       # edges of the 32-per-wave / 128-per-workgroup slots, on both9
TRUTH_SETS = (("both9", 1000), ("grasp9", 768), ("grasp3", 768))      # the sets whose DECIDED share and HIT count are conditions
VIEW = {"tag": "grasp9", "H": 48, "W": 32}                     # the render_view test: a 48 x 32 view of the same box
F = np.float32
ERRORS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "sdf_trace_fp64_errors.txt")


def recorded(kind, ray_set_name, head):
    """The max_dt figure of THE `<kind> <set> <head> ... max_dt <x>` line of profiles/sdf_trace_fp64_errors.txt (kind "cpu" / "gpu", set
    a tag or "view"): exactly one such line, or the file is not to be trusted as a bound."""
    with open(ERRORS_FILE) as fh:
        found = re.findall(r"^%s %s %s .*max_dt (\S+)$" % (kind, ray_set_name, head), fh.read(), re.M)
    assert len(found) == 1, "%d `%s %s %s` lines in profiles/sdf_trace_fp64_errors.txt, one expected" % (len(found), kind, ray_set_name, head)
    return float(found[0])


def record(lines):
    """Put figure lines (`<kind> <set> <head> ...`) into the file, each in place of the line with the same first three words."""
    with open(ERRORS_FILE) as fh:
        old = fh.read().splitlines()
    keys = {tuple(l.split()[:3]) for l in lines}
    kept = [l for l in old if tuple(l.split()[:3]) not in keys]
    last = max([k for k, l in enumerate(kept) if l.split()[:1] in (["cpu"], ["gpu"])], default=len(kept) - 1)
    with open(ERRORS_FILE, "w") as fh:
        fh.write("\n".join(kept[:last + 1] + list(lines) + kept[last + 1:]) + "\n")


def slab(o, d, lo, hi):
    """(t0, t1) of the rays o + t d against the box, fp64; every direction component non-zero."""
    ta, tb = (np.asarray(lo) - o) / d, (np.asarray(hi) - o) / d
    return np.maximum(np.minimum(ta, tb).max(1), 0.0), np.maximum(ta, tb).min(1)


def ray_set(M, seed=None):
    """[M, 8] float32 (o, d, t0, t1): from ORIGIN towards targets uniform in [-0.45, 0.45]^3, unit directions, clipped to BOX."""
    rng = np.random.default_rng(200 + M if seed is None else seed)
    targets = rng.uniform(-0.45, 0.45, (M, 3))
    o = np.broadcast_to(np.asarray(ORIGIN, np.float64), (M, 3))
    d = targets - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t0, t1 = slab(o, d, *BOX)
    return np.concatenate([o, d, t0[:, None], t1[:, None]], 1).astype(np.float32)


def view_camera():
    """(cam_intr [3, 3], root_joint [3]) of the render_view test: the wrist 0.5 m in front of a 48 x 32 view."""
    return np.array([[60.0, 0.0, 16.0], [0.0, 60.0, 24.0], [0.0, 0.0, 1.0]]), np.array([0.01, -0.02, 0.5])


def view_rays():
    """The rays render_view marches for VIEW ([M, 8] float32, in ray order) and the camera_rays record they come from."""
    from alignsdf_amd.render import camera_rays
    cam, root = view_camera()
    cr = camera_rays(cam, root, syn.specs_for(VIEW["tag"])["SdfScaleFactor"], VIEW["H"], VIEW["W"], *BOX)
    return np.concatenate([cr["origins"], cr["dirs"], cr["t0"][:, None], cr["t1"][:, None]], 1), cr


def march(f, rays, max_steps=64, refine_steps=6, step_scale=1.0, min_step=1e-3, max_step=0.05, full=False):
    """The rule, ray by ray.  `f(points [K, 3] float32) -> sdf [K]` (any float dtype) is called once per step with the points of the
    rays that are still live (full=True: with one row per ray, zeros for the rays that are done - for an evaluator whose rounding may
    depend on the shape of the batch).  Signs are read from f's own values; everything the rule computes with is float32.  Returns {"t" [M]
    float32, "status" [M] int32, "bracket" [M, 4] float32 (zeros unless HIT), "evals" [M] int32, "min_abs" [M] float64: the smallest
    |f| over the ray's MARCH samples (inf without one)}."""
    rays = np.ascontiguousarray(rays, np.float32)
    M = len(rays)
    o, d, t1 = rays[:, 0:3], rays[:, 3:6], rays[:, 7]
    t = rays[:, 6].copy()
    scale, lo_step, hi_step, half = F(step_scale), F(min_step), F(max_step), F(0.5)
    out_t = np.full(M, np.inf, np.float32)
    status = np.zeros(M, np.int32)
    bracket = np.zeros((M, 4), np.float32)
    evals = np.zeros(M, np.int32)
    min_abs = np.full(M, np.inf, np.float64)
    tlo, flo, thi, fhi = (np.zeros(M, np.float32) for _ in range(4))
    count = np.zeros(M, np.int64)
    phase = np.where(np.isfinite(rays).all(1) & ~(rays[:, 6] > t1), 1, 0)

    def done(i, code, value):
        status[i], out_t[i], phase[i] = code, value, 0

    def finish(i):
        w = flo[i] / (flo[i] - fhi[i])
        x = tlo[i] + (thi[i] - tlo[i]) * w
        x = x if x > tlo[i] else tlo[i]
        x = x if x < thi[i] else thi[i]
        bracket[i] = (tlo[i], thi[i], flo[i], fhi[i])
        done(i, HIT, x)

    def next_midpoint(i):
        tm = half * (tlo[i] + thi[i])
        if count[i] == 0 or tm == tlo[i] or tm == thi[i]:
            finish(i)
        else:
            t[i] = tm

    with np.errstate(all="ignore"):
        while True:
            live = np.nonzero(phase)[0]
            if not len(live):
                break
            points = o[live] + t[live, None] * d[live]
            if full:
                every = np.zeros((M, 3), np.float32)
                every[live] = points
                raw = np.asarray(f(every)).reshape(-1)[live]
            else:
                raw = np.asarray(f(points)).reshape(-1)
            assert len(raw) == len(live)
            val = raw.astype(np.float32)
            evals[live] += 1
            for k, i in enumerate(live):
                ti, fi, neg = t[i], val[k], bool(raw[k] <= 0)
                if phase[i] == 1:
                    min_abs[i] = min(min_abs[i], abs(float(raw[k])))
                    if neg:
                        if evals[i] == 1:
                            done(i, INSIDE, ti)
                        else:
                            thi[i], fhi[i], count[i], phase[i] = ti, fi, refine_steps, 2
                            next_midpoint(i)
                    else:
                        tlo[i], flo[i] = ti, fi
                        if ti == t1[i]:
                            done(i, MISS, np.inf)
                            continue
                        count[i] += 1
                        if count[i] == max_steps:
                            done(i, EXHAUSTED, ti)
                            continue
                        s = scale * fi
                        s = s if s > lo_step else lo_step
                        s = s if s < hi_step else hi_step
                        tn = ti + s
                        t[i] = tn if tn < t1[i] else t1[i]
                else:
                    if neg:
                        thi[i], fhi[i] = ti, fi
                    else:
                        tlo[i], flo[i] = ti, fi
                    count[i] -= 1
                    next_midpoint(i)
    return {"t": out_t, "status": status, "bracket": bracket, "evals": evals, "min_abs": min_abs}


def oracle_heads(tag, sample, dtype):
    """{"hand" / "obj": f(points float32 [K, 3]) -> sdf [K] numpy `dtype`}: one head of the oracle's SeparateDecoder chain at a time
    (point_features, effective_head_params, _run_head: what oracle.sdf_oracle.decode_points runs for both)."""
    from oracle import sdf_oracle as orc
    sd, specs = state_dict(tag), syn.specs_for(tag)
    latent, mano, obj = syn.sample_inputs(tag, sample)
    cast = lambda d: None if d is None else {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}
    mano, obj = cast(mano), cast(obj)
    lat = torch.as_tensor(latent).to(dtype).reshape(1, -1)
    out = {}
    for k, (name, letter) in enumerate((("hand", "h"), ("obj", "o"))):
        params = orc.effective_head_params(sd, letter, dtype)

        def f(points, k=k, params=params):
            x = torch.as_tensor(np.asarray(points, np.float32)).to(dtype)
            with torch.no_grad():
                feats = orc.point_features(x, specs, mano, obj)
                inputs = torch.cat([lat.expand(x.shape[0], -1), feats], 1)
                cols = torch.as_tensor(_head_slices(specs["EncodeStyle"], lat.shape[1], feats.shape[1])[k])
                xin = inputs[:, cols]
                return orc._run_head(params, xin, xin)[:, 0].numpy()
        out[name] = f
    return out


def _truth(tag, sample, rays, dtype, rule):
    heads = oracle_heads(tag, sample, dtype)
    return {name: march(heads[name], rays, **rule) for name in ("hand", "obj")}


@functools.lru_cache(maxsize=None)
def _truth_cached(tag, sample, key, dtype):
    rays = view_rays()[0] if key == "view" else ray_set(key)
    return _truth(tag, sample, rays, dtype, RULE)


def trace_truth(tag, sample, rays, dtype=torch.float64, rule=None):
    """{"hand" / "obj": march(...)} of synthetic sample `sample` of configuration `tag`: the rule in fp32, the decoder (the oracle's) in
    `dtype`.  `rays` an [M, 8] array, or the key of a standard set (an int M: ray_set(M); "view": view_rays()) - those are computed
    once per process under RULE and must be left unchanged."""
    if isinstance(rays, (int, str)):
        assert rule is None
        return _truth_cached(tag, sample, rays, dtype)
    return _truth(tag, sample, rays, dtype, dict(RULE, **(rule or {})))


def decided(truth_head, eps=DECIDE_EPS):
    return truth_head["min_abs"] > eps


def module_for(tag):
    from tests.sdf_grad_cases import module_for as grad_module_for
    return grad_module_for(tag)
