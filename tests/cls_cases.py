"""Shared pieces of the label-pass truth tests (tests/test_cls_truth.py on the CPU, tests/test_gpu_cls_fp64.py on the GPU): the ten
decoder configurations with a part classifier, their point lists, the fp64 truth of `oracle.sdf_oracle.classify_points` beside the fp32
yardsticks, the error rule, and the kernel of csrc/k1_cls_kernels.hip each configuration must reach.

A classifier is named by a hashable `variant`:
    ("std", C, seed)     synthetic.classifier_state_dict(C, seed)
    ("tie", C, a, b)     the same with row b (weights and bias) a copy of row a: two bit-equal score columns, label b never wins
                         (with seed 0 row 2 is never the largest of 8 on the lists used here and row 0 often is: (2, 4) checks the columns,
                         (0, 6) the first-maximum rule)
    ("same", C)          every row a copy of row 0: every label is 0
    ("high", 8)          8 classes with +10 added to the biases of classes 5 to 7: every label lies in 5..7"""
import functools

import numpy as np
import torch

from alignsdf_amd import synthetic as syn

CONFIGS = ("nerf3", "both9", "comb3", "nerf9", "nerf15", "comb9", "comb15", "hand6", "hand51", "obj6")
STD = ("std", 6, 0)
TOL = 2e-5                       # the fp32 parity bar of tests/test_oracle_cls.py / tests/test_gpu_cls.py
LIST_LENGTHS = (1, 31, 32, 33, 127, 128, 129, 257)        # edges of kWavePts = 32 and kWgPts = 128
FULL = 4096
RMS_FACTOR, RMS_MIN_POINTS = 1.5, 4096
MAX_LEFT_OUT = 4                 # of 4096 points: those whose top-two gap is within 2 * bound

# configuration -> (kernel of k1_cls_kernels.hip, hip.nerf_features, hip.combined, point-feature size): KP = 2 for xyz and every affine
# embedding (folded into the constants block), 5 / 8 for the NeRF encoding of 9 / 15 features; `combined` selects the two-row form
KERNEL_OF = {
    "nerf3": ("sdf_mlp_cls_kernel", False, False, 3),
    "both9": ("sdf_mlp_cls_kernel", False, False, 9),
    "hand6": ("sdf_mlp_cls_kernel", False, False, 6),
    "hand51": ("sdf_mlp_cls_kernel", False, False, 51),
    "obj6": ("sdf_mlp_cls_kernel", False, False, 6),
    "comb3": ("sdf_mlp_combined_cls_kernel", False, True, 3),
    "nerf9": ("sdf_mlp_nerf9_cls_kernel", True, False, 9),
    "nerf15": ("sdf_mlp_nerf15_cls_kernel", True, False, 15),
    "comb9": ("sdf_mlp_combined_nerf9_cls_kernel", True, True, 9),
    "comb15": ("sdf_mlp_combined_nerf15_cls_kernel", True, True, 15),
}
ONE_PER_KERNEL = ("nerf3", "comb3", "nerf9", "nerf15", "comb9", "comb15")


def kernel_reached(tag, hip):
    """The kernel k1_cls_launch selects for this decoder (by KP and the number of MLPs), after asserting that the decoder has the
    properties the selection rests on - a refactor that routes `nerf9` elsewhere fails here."""
    name, nerf, combined, pf = KERNEL_OF[tag]
    assert hip.nerf_features == nerf and hip.combined == combined and hip.point_feat_size == pf, (
        tag, hip.nerf_features, hip.combined, hip.point_feat_size)
    kp = (pf + 1) // 2 if nerf else 2
    derived = "sdf_mlp_%s%scls_kernel" % ("combined_" if combined else "", {2: "", 5: "nerf9_", 8: "nerf15_"}[kp])
    assert derived == name, (tag, derived, name)
    return name


def classifier(variant):
    kind, C = variant[0], variant[1]
    sd = syn.classifier_state_dict(C, variant[2] if kind == "std" else 0)
    w, b = sd["classifier_head.weight"].copy(), sd["classifier_head.bias"].copy()
    if kind == "tie":
        w[variant[3]], b[variant[3]] = w[variant[2]], b[variant[2]]
    elif kind == "same":
        w[:], b[:] = w[0], b[0]
    elif kind == "high":
        b[5:8] += np.float32(10.0)
    elif kind != "std":
        raise ValueError(variant)
    return {"classifier_head.weight": w, "classifier_head.bias": b}


@functools.lru_cache(maxsize=None)
def state_dict(tag, variant=STD):
    """The configuration's decoder plus the classifier `variant` (numpy float32).  comb9 / comb15: a CombinedDecoder over the NeRF
    encoding, built as tests/test_gpu_nerf_one_plane.py::_state_dict builds it."""
    if tag in ("comb9", "comb15"):
        pf = int(tag[4:])
        sd = syn.combined_hidden_state_dict(256, pf, 0)
        last = syn.load_last_layers("nerf%d" % pf)
        w, b = last["linh4.weight"], last["linh4.bias"]
        sd["lin4.weight"] = np.concatenate([w, w], axis=0).astype(np.float32)
        sd["lin4.bias"] = np.concatenate([b, b + np.float32(0.04)]).astype(np.float32)
    else:
        sd = dict(syn.full_state_dict(tag))
    sd.update(classifier(variant))
    return sd


def specs_for(tag, num_class=6):
    if tag in ("comb9", "comb15"):
        specs = syn.specs_for("comb3")
        specs["PointFeatSize"] = int(tag[4:])
    else:
        specs = syn.specs_for(tag)
    specs["ClassifierBranch"] = True
    specs["NetworkSpecs"]["num_class"] = num_class
    return specs


def sample_inputs(tag, sample):
    """(latent [1, 256], mano_results or None, obj_results or None), numpy: tests/test_gpu_decoder.py::_setup for any sample."""
    mano, obj = syn.pose_inputs(sample) if specs_for(tag)["EncodeStyle"] != "nerf" else (None, None)
    return syn.latent_code(sample), mano, obj


def points(M, seed=None):
    return syn.uniform((M, 3), 4321 + M if seed is None else seed, -1.0, 1.0).astype(np.float32)


def _t(d):
    return None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def native_decoder(tag, variant=STD):
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    specs = specs_for(tag)
    return HipSdfDecoder(state_dict(tag, variant), 256, specs["PointFeatSize"], specs["EncodeStyle"], device="cuda:0")


def bind(hip, tag, sample):
    from alignsdf_amd.hip_decoder import kinematic_affine
    specs = specs_for(tag)
    lat, mano, obj = sample_inputs(tag, sample)
    emb = None
    if specs["EncodeStyle"] != "nerf":
        emb = kinematic_affine(specs["PointFeatSize"], specs["EncodeStyle"], specs["SdfScaleFactor"], _t(mano), _t(obj))
    hip.set_sample(torch.from_numpy(lat), emb)


@functools.lru_cache(maxsize=None)
def module_for(tag, variant=STD, dtype=torch.float32):
    from alignsdf_amd.networks.model import build_decoder
    sd = {k: torch.from_numpy(v) for k, v in state_dict(tag, variant).items()}
    return build_decoder(specs_for(tag, variant[1]), sd).to(dtype).eval()


def module_scores(tag, pts, sample=0, variant=STD):
    """TorchModuleDecoder.classify_points on the GPU (the module on PyTorch-ROCm), or None on a host without one."""
    if not torch.cuda.is_available():
        return None
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    mod = TorchModuleDecoder(module_for(tag, variant), specs_for(tag, variant[1]), "yardstick of the label-pass truth tests")
    lat, mano, obj = sample_inputs(tag, sample)
    mod.set_sample(torch.from_numpy(lat), _t(mano), _t(obj))
    scores = mod.classify_points(torch.from_numpy(pts).cuda())[2].cpu().numpy()
    mod.close()
    return scores


@functools.lru_cache(maxsize=None)
def references(tag, M, sample=0, variant=STD, seed=None):
    """(fp64 truth [M, C], fp32 CPU oracle [M, C], module scores on the GPU [M, C] or None) of the point list points(M, seed), numpy.
    Computed once per case and never modified (the arrays are read-only)."""
    from oracle import sdf_oracle as orc
    pts = points(M, seed)
    lat, mano, obj = sample_inputs(tag, sample)
    args = (state_dict(tag, variant), lat, pts, specs_for(tag, variant[1]), _t(mano), _t(obj))
    truth = orc.classify_points(*args, dtype=torch.float64)[0].numpy()
    oracle32 = orc.classify_points(*args)[0].numpy()
    out = (truth, oracle32, module_scores(tag, pts, sample, variant))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sdf_truth(tag, M, sample=0, seed=None):
    """fp64 (hand [M], obj [M]) of oracle.sdf_oracle.decode_points on the same list."""
    from oracle import sdf_oracle as orc
    lat, mano, obj = sample_inputs(tag, sample)
    h, o = orc.decode_points(state_dict(tag), lat, points(M, seed), specs_for(tag), _t(mano), _t(obj), dtype=torch.float64)
    return h.numpy(), o.numpy()


def err(a, truth):
    """(largest |a - truth|, rms of a - truth)."""
    d = np.asarray(a, np.float64) - truth
    return float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))


def rule_bound(e_mod, e_or, tmax):
    """The right-hand side of the project's rule (tests/test_gpu_sdf_grad.py, tests/test_gpu_sdf_vjp.py)."""
    return 3.0 * max(e_mod, e_or) + 5e-7 * max(1.0, tmax)


def top_two_gap(scores):
    if scores.shape[1] < 2:
        return np.full(scores.shape[0], np.inf)
    top2 = np.sort(scores, axis=1)[:, -2:]
    return top2[:, 1] - top2[:, 0]


def first_argmax(scores):
    """argmax with the first index on ties (numpy's rule, torch.argmax's, and the kernel's strict `>`)."""
    return np.asarray(scores).argmax(axis=1)
