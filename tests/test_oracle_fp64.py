"""The fp64 evaluation of the CPU oracle (oracle/sdf_oracle.py decode_points(..., dtype=torch.float64)): the truth the split-half
GPU kernels are held to in tests/test_gpu_split_half_fp64.py.  It must be the same function as the fp32 oracle (which
tests/test_oracle_decoder.py pins to the reference) and the same number as the stand-alone fp64 evaluation of the adversarial test
(tests/split_half_cases.py forward64): one fp64 truth, not two."""
import numpy as np
import pytest
import torch

from alignsdf_amd import synthetic as syn
from oracle import sdf_oracle as orc
from tests import split_half_cases as cases

TAGS = ["nerf3", "both9", "comb3", "nerf9", "nerf15", "hand6", "hand51", "obj6"]


def _inputs(tag):
    specs, sd = syn.specs_for(tag), syn.full_state_dict(tag)
    lat = torch.from_numpy(syn.latent_code(0))
    mano = obj = None
    if specs["EncodeStyle"] != "nerf":
        m, o = syn.pose_inputs(0)
        mano = {k: torch.from_numpy(v) for k, v in m.items()}
        obj = {k: torch.from_numpy(v) for k, v in o.items()}
    return specs, sd, lat, mano, obj


@pytest.mark.parametrize("tag", TAGS)
def test_fp64_oracle_is_the_fp32_oracle_and_the_reference(tag, golden_dir):
    g = np.load("%s/ref_decoder_%s.npz" % (golden_dir, tag))
    specs, sd, lat, mano, obj = _inputs(tag)
    pts = torch.from_numpy(g["rand_pts"])
    h64, o64 = orc.decode_points(sd, lat, pts, specs, mano, obj, dtype=torch.float64)
    assert h64.dtype == torch.float64 and o64.dtype == torch.float64
    h32, o32 = orc.decode_points(sd, lat, pts, specs, mano, obj)
    assert h32.dtype == torch.float32
    d32 = max((h64 - h32.double()).abs().max().item(), (o64 - o32.double()).abs().max().item())
    # a real fp64 evaluation: close to the fp32 one, yet not its values rounded back
    assert 0.0 < d32 <= 1e-6, (tag, d32)
    dref = max(np.abs(h64.numpy() - g["rand_hand"]).max(), np.abs(o64.numpy() - g["rand_obj"]).max())
    assert dref <= 1e-5, (tag, dref)


@pytest.mark.parametrize("tag", TAGS)
def test_fp64_chain_has_no_fp32_step(tag):
    """Every stage of the fp64 path stays in fp64: weight-norm fold, point features, both decoders."""
    specs, sd, lat, mano, obj = _inputs(tag)
    pts = torch.from_numpy(syn.uniform((64, 3), 91, -1.0, 1.0))
    params = orc.combined_params(sd, torch.float64) if tag == "comb3" else orc.effective_head_params(sd, "h", torch.float64)
    assert all(w.dtype == torch.float64 and b.dtype == torch.float64 for w, b in params)
    if mano is not None:
        mano = {k: v.double() for k, v in mano.items()}
        obj = {k: v.double() for k, v in obj.items()}
    assert orc.point_features(pts, specs, mano, obj).dtype == torch.float64
    # the fold in fp64 is the fp32 fold to fp32 rounding, not bit for bit (it is computed, not cast)
    if tag != "comb3":
        w64, w32 = params[0][0], orc.effective_head_params(sd, "h")[0][0]
        assert torch.allclose(w64, w32.double(), rtol=1e-6, atol=0) and not torch.equal(w64, w32.double())


@pytest.mark.parametrize("name", ["spread1e4", "huge", "tiny", "heavy_tails", "gain30", "latent_x10"])
def test_fp64_oracle_is_forward64_on_the_adversarial_variants(name):
    sd, lat = cases.variant(name)
    pts = cases.lattice(9)
    t_h, t_o, _ = cases.forward64(sd, lat, pts)
    h, o = orc.decode_points(sd, lat, pts, syn.specs_for("nerf3"), dtype=torch.float64)
    d = max(np.abs(h.numpy() - t_h).max(), np.abs(o.numpy() - t_o).max())
    assert d <= 1e-12, (name, d)


@pytest.mark.parametrize("tag", ["hand6", "comb3", "nerf9"])
@pytest.mark.parametrize("name", ["spread1e4", "huge", "tiny"])
def test_restated_variants_are_the_same_function(tag, name):
    """The function-preserving variants restated on the other families' weights (SeparateDecoder heads of every input width,
    the CombinedDecoder's single MLP): the fp64 function is unchanged up to the fp32 rounding of the rescaled weights (1e-4 and
    1e-2 are not powers of two), only its internal magnitudes move - a wrong split of the layer-2 columns would change it by O(1)."""
    specs, _, _, mano, obj = _inputs(tag)
    base, lat = cases.plain_weights(tag), syn.latent_code(3).reshape(-1)
    sd, vlat = cases.variant(name, tag)
    assert np.array_equal(vlat, lat)
    pts = torch.from_numpy(syn.uniform((256, 3), 92, -1.0, 1.0))
    want = orc.decode_points(base, lat, pts, specs, mano, obj, dtype=torch.float64)
    got = orc.decode_points(sd, lat, pts, specs, mano, obj, dtype=torch.float64)
    for a, b in zip(want, got):
        assert (a - b).abs().max().item() <= 1e-6, (tag, name)
    changed = [k for k in base if not np.array_equal(base[k], sd[k])]
    assert len(changed) >= 3 * len(cases.prefixes(sd)), changed          # every MLP of the decoder restated
