"""Decoders chosen to break the split-half arithmetic, and their fp64 evaluation: shared by tests/test_gpu_split_half_adversarial.py,
tests/test_gpu_split_half_fp64.py and tests/test_oracle_fp64.py (a plain helper module, like tests/kernel_emulator.py).

`plain_weights(tag)` is a synthetic decoder with its weight norm folded (plain `.weight` keys), `variant(name, tag)` one of the
adversarial restatements of it, `forward64` the stand-alone fp64 evaluation of a PointFeatSize-3 SeparateDecoder (the oracle's
decode_points(..., dtype=torch.float64) must equal it) and `lattice` the integer-mode lattice of the adversarial test."""
import numpy as np

from alignsdf_amd import synthetic as syn

N = 24
ORIGIN, VS = [-0.9, -0.8, -0.85], 1.7 / (N - 1)


def prefixes(sd):
    """The MLPs of a state dict: ("lin",) for a CombinedDecoder, ("linh", "lino") for a SeparateDecoder."""
    return ("lin",) if "lin0.bias" in sd else ("linh", "lino")


def plain_weights(tag="nerf3"):
    from oracle import sdf_oracle as orc
    base, sd = syn.full_state_dict(tag), {}
    if "lin0.bias" in base:
        for layer, (w, b) in enumerate(orc.combined_params(base)):
            sd["lin%d.weight" % layer], sd["lin%d.bias" % layer] = w.numpy().copy(), b.numpy().copy()
        return sd
    for head in "ho":
        for layer, (w, b) in enumerate(orc.effective_head_params(base, head)):
            sd["lin%s%d.weight" % (head, layer)], sd["lin%s%d.bias" % (head, layer)] = w.numpy().copy(), b.numpy().copy()
    return sd


def forward64(sd, latent, pts):
    """fp64 evaluation of both heads (networks/model.py:285-350, PointFeatSize 3)."""
    x0 = np.concatenate([np.repeat(latent.reshape(1, -1).astype(np.float64), len(pts), 0), pts.astype(np.float64)], 1)
    out, peaks = [], []
    for head in "ho":
        W = [sd["lin%s%d.weight" % (head, k)].astype(np.float64) for k in range(5)]
        b = [sd["lin%s%d.bias" % (head, k)].astype(np.float64) for k in range(5)]
        h0 = np.maximum(x0 @ W[0].T + b[0], 0)
        h1 = np.maximum(h0 @ W[1].T + b[1], 0)
        h2 = np.maximum(np.concatenate([h1, x0], 1) @ W[2].T + b[2], 0)
        h3 = np.maximum(h2 @ W[3].T + b[3], 0)
        out.append(np.tanh(h3 @ W[4].T + b[4])[:, 0])
        peaks.append((h0.max(), h1.max(), h2.max(), h3.max()))
    return out[0], out[1], peaks


def lattice(n=N, origin=ORIGIN, vs=VS):
    """Integer-mode lattice (idx * vs + origin, fp32) in sweep order."""
    idx = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return idx * np.float32(vs) + np.array(origin, np.float32)


def rescale_last_layer(sd, latent, target=0.08):
    """Keep the pre-tanh outputs of an altered network of order 0.1 (where the 1e-5 bar means something).  PointFeatSize 3."""
    pts = syn.uniform((2000, 3), 55, -1.0, 1.0).astype(np.float32)
    x0 = np.concatenate([np.repeat(latent.reshape(1, -1).astype(np.float64), len(pts), 0), pts.astype(np.float64)], 1)
    for head in "ho":
        W = [sd["lin%s%d.weight" % (head, k)].astype(np.float64) for k in range(5)]
        b = [sd["lin%s%d.bias" % (head, k)].astype(np.float64) for k in range(5)]
        h = np.maximum(x0 @ W[0].T + b[0], 0)
        h = np.maximum(h @ W[1].T + b[1], 0)
        h = np.maximum(np.concatenate([h, x0], 1) @ W[2].T + b[2], 0)
        h = np.maximum(h @ W[3].T + b[3], 0)
        pre = h @ W[4].T
        k = target / max(float(np.std(pre)), 1e-30)
        sd["lin%s4.weight" % head] = (W[4] * k).astype(np.float32)
        sd["lin%s4.bias" % head] = np.float32([-float(np.mean(pre)) * k])
    return sd


def variant(name, tag="nerf3"):
    """(state dict, latent [L] fp32) of adversarial variant `name` of the synthetic decoder `tag`.  spread1e4 / huge / tiny are
    function-preserving re-parametrisations (ReLU is positively homogeneous) and apply to every family - the layer-2 input is
    [h1, head input] in each, so its first n1 = rows(layer 1) columns consume h1; the others rescale the last layer of a
    PointFeatSize-3 SeparateDecoder and are nerf3 only."""
    sd, lat = plain_weights(tag), syn.latent_code(3).reshape(-1)
    rng = np.random.RandomState(7)
    heads = prefixes(sd)
    if name == "spread1e4":                    # h0 x 100, h1 x 0.01, h2 x 100
        for p in heads:
            n1 = sd["%s1.weight" % p].shape[0]
            sd["%s0.weight" % p] *= np.float32(100.0); sd["%s0.bias" % p] *= np.float32(100.0)
            sd["%s1.weight" % p] *= np.float32(1e-4); sd["%s1.bias" % p] *= np.float32(1e-2)
            sd["%s2.weight" % p][:, :n1] *= np.float32(1e4); sd["%s2.weight" % p][:, n1:] *= np.float32(100.0)
            sd["%s2.bias" % p] *= np.float32(100.0)
            sd["%s3.weight" % p] *= np.float32(1e-2)
    elif name == "huge":                       # activations of order 1e4: beyond the default scale's fp16 range
        for p in heads:
            sd["%s0.weight" % p] *= np.float32(4096.0); sd["%s0.bias" % p] *= np.float32(4096.0)
            sd["%s1.weight" % p] /= np.float32(4096.0)
    elif name == "tiny":                       # activations of order 1e-4: low planes subnormal at the default scale
        for p in heads:
            sd["%s0.weight" % p] /= np.float32(16384.0); sd["%s0.bias" % p] /= np.float32(16384.0)
            sd["%s1.weight" % p] *= np.float32(16384.0)
    elif tag != "nerf3":
        raise ValueError("variant %r is defined for nerf3 only" % name)
    elif name == "heavy_tails":                # log-normal multipliers on every hidden weight: a few weights dominate their rows
        for head in "ho":
            for k in range(4):
                sd["lin%s%d.weight" % (head, k)] *= np.exp(1.2 * rng.randn(*sd["lin%s%d.weight" % (head, k)].shape)).astype(np.float32)
        sd = rescale_last_layer(sd, lat)
    elif name == "gain30":                     # weight_g = 30 instead of 1.5 / 3 on every normed layer
        for head in "ho":
            for k, g in enumerate((3.0, 1.5, 1.5, 1.5)):
                sd["lin%s%d.weight" % (head, k)] *= np.float32(30.0 / g)
        sd = rescale_last_layer(sd, lat)
    elif name == "latent_x10":
        lat = lat * np.float32(10.0)
        sd = rescale_last_layer(sd, lat)
    else:
        raise ValueError(name)
    return sd, lat.astype(np.float32)
