"""The rules of the device auto-decode (alignsdf_amd.fit: adam_step_host, clamped_l1_rule; alignsdf_amd.autodecode) held to
statements written independently of them, on the CPU: the Adam step against fp64 and torch.optim.Adam, the loss rule against the
autograd of fit_sample's expression at the rule's own edges, the fp64 reference of the device test against its own cap, and the host
logic of the flow with a stub in place of the fit."""
import json
import os

import numpy as np
import pytest
import torch

from alignsdf_amd import autodecode as ad
from alignsdf_amd import fit
from alignsdf_amd import synthetic as syn
from tests import fit_code_cases as fc
from tests import sdf_vjp_cases as vc

L = 256


# ---- the Adam rule ---------------------------------------------------------------------------------------------------------------------------
def test_adam_step_host_against_fp64_and_torch_adam():
    """50 steps on random gradients, lr 5e-3 decayed by 0.5 every 10 steps, prior 1e-3.

    Per step the fp32 step is compared with the fp64 statement (fit_code_cases.adam_f64: the textbook update with the bias corrections
    on m and v) started from the SAME fp32 state, on the increment dz = z - z_prev.  The bound is derived, not measured: the step is
    thirteen fp32 operations - three for g, three for m, four for v, and sqrt, product, sum, quotient, product for the increment -
    each correctly rounded (2^-24 relative) and none of them a cancelling difference of the vector as a whole (g is dominated by
    d_latent, m and v are averages of it), plus the two table entries rounded once: 16 * 2^-24 relative to the largest increment of
    the step.  On top of it the last operation, z - q, rounds z itself: half an ulp of z, which is not part of the increment's error.
    The constants of both statements are the fp32 values (b1, b2, eps as floats; 1 - b1 and 1 - b2 are exact differences).

    The fp64 statement in turn is torch.optim.Adam's in fp64 fed the same gradients - over the whole trajectory, to the same bound
    (not in bits: torch's own operation order varies by version)."""
    rng = np.random.default_rng(3)
    steps, lr, decay, every, prior = 50, 5e-3, 0.5, 10, 1e-3
    b1, b2, eps = (float(np.float32(v)) for v in (fit.ADAM_B1, fit.ADAM_B2, fit.ADAM_EPS))
    table32, table64 = fit.adam_step_table(steps, lr, decay, every), fit.adam_step_table(steps, lr, decay, every, dtype=np.float64)
    kp = fit.prior_factor(prior, L)
    assert kp == np.float32(2.0 * float(np.float32(prior)) / L) and table32.dtype == np.float32 and table32.shape == (steps, 2)
    z = rng.standard_normal(L).astype(np.float32)
    z0 = rng.standard_normal(L).astype(np.float32)
    m, v = np.zeros(L, np.float32), np.zeros(L, np.float32)
    # the fp64 trajectory and torch's, on the same gradients
    zt = torch.from_numpy(z.astype(np.float64)).requires_grad_()
    z64, m64, v64 = z.astype(np.float64), np.zeros(L), np.zeros(L)
    worst = worst_entry = 0.0
    for k in range(steps):
        d = rng.standard_normal(L).astype(np.float32)
        lr_k = lr * decay ** (k // every)
        assert abs(table64[k, 0] - lr_k / (1.0 - b1 ** (k + 1))) <= 1e-13 * table64[k, 0] and abs(table64[k, 1] - (1.0 - b2 ** (k + 1)) ** -0.5) <= 1e-13 * table64[k, 1]
        # (a) one fp32 step against the fp64 statement from the same state
        want = fc.adam_f64(*(a.astype(np.float64) for a in (z, m, v, d, z0)), float(kp), lr_k, k, b1, b2, eps)
        got = fit.adam_step_host(z, m, v, d, z0, kp, table32[k, 0], table32[k, 1])
        assert all(a.dtype == np.float32 for a in got)
        dz, dz64 = got[0].astype(np.float64) - z, want[0] - z
        err = np.abs(dz - dz64) - 2.0 ** -24 * np.abs(got[0])
        worst = max(worst, float(err.max() / np.abs(dz64).max()))
        assert (err <= fc.STEP_TOL * np.abs(dz64).max()).all(), (k, float(err.max()), float(np.abs(dz64).max()))
        # ... and ELEMENTWISE, relative to the entry's own increment, wherever the one sum of the rule that can cancel does not: the
        # entries whose b1 m and (1 - b1) g have one sign (|b1 m| + |(1 - b1) g| = |m_new|: condition number 1; v is a sum of squares
        # and g is d_latent plus a prior term 1e-5 of it).  There every operation's rounding reaches the increment with a factor of
        # at most 1, sqrt's with 1/2: within the same sixteen roundings
        same = np.sign(m.astype(np.float64)) * np.sign(d.astype(np.float64) + float(kp) * (z.astype(np.float64) - z0)) >= 0
        assert same.mean() >= 0.3, (k, float(same.mean()))
        assert (err[same] <= fc.STEP_TOL * np.abs(dz64[same])).all(), (k, float((err[same] / np.abs(dz64[same])).max() / 2.0 ** -24))
        worst_entry = max(worst_entry, float((err[same] / np.abs(dz64[same])).max()))
        assert np.abs(got[1] - want[1]).max() <= 4 * 2.0 ** -24 * np.abs(want[1]).max() and np.abs(got[2] - want[2]).max() <= 5 * 2.0 ** -24 * np.abs(want[2]).max()
        z, m, v = got
        # (b) the fp64 trajectories: torch.optim.Adam with this step's rate (a fresh optimizer per rate would lose m and v: the rate is set)
        if k == 0:
            opt = torch.optim.Adam([zt], lr=lr_k, betas=(b1, b2), eps=eps)
        opt.param_groups[0]["lr"] = lr_k
        before = zt.detach().numpy().copy()
        zt.grad = torch.from_numpy(d.astype(np.float64)) + float(kp) * (zt.detach() - torch.from_numpy(z0.astype(np.float64)))
        opt.step()
        new64 = fc.adam_f64(z64, m64, v64, d.astype(np.float64), z0.astype(np.float64), float(kp), lr_k, k, b1, b2, eps)
        assert np.abs(z64 - before).max() <= 1e-12
        inc_t, inc_64 = zt.detach().numpy() - before, new64[0] - z64
        assert np.abs(inc_t - inc_64).max() <= fc.STEP_TOL * np.abs(inc_64).max(), k
        z64, m64, v64 = new64
    print("FITCODE adam_step_host: worst per-step error %.2f x 2^-24 of the step's largest increment, %.2f x 2^-24 of an entry's own "
          "increment where m's sum does not cancel (bound 16)" % (worst / 2.0 ** -24, worst_entry / 2.0 ** -24))
    # the fp64 form of the same function is the fp64 statement
    z64b = fit.adam_step_host(z64, m64, v64, np.ones(L), z0.astype(np.float64), float(kp), table64[0, 0], table64[0, 1], b1, b2, eps)[0]
    assert z64b.dtype == np.float64
    assert np.abs(z64b - fc.adam_f64(z64, m64, v64, np.ones(L), z0.astype(np.float64), float(kp), lr, 0, b1, b2, eps)[0]).max() <= 1e-14


# ---- the loss rule at its own edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0.05, float("inf")])
def test_loss_rule_is_the_autograd_of_fit_samples_term(c):
    """f == t, f == +-c exactly, |f| > c, t outside the clamp, t = NaN, c = inf, and a head with n = 0 - the numpy / torch statement
    against the autograd of (f.clamp(-c, c) - s.clamp(-c, c)).abs().mean() over the head's own points, in weights and in value."""
    c = float(np.float32(c))                      # (the clamp is an fp32 number: the C ABI carries it as a float)
    cc = float(np.float32(0.05)) if np.isinf(c) else c
    f = np.array([0.01, 0.02, cc, -cc, 0.07, -0.2, 0.03, -0.01, 0.04, 0.0, np.nextafter(np.float32(cc), np.float32(1)), -0.03], np.float32)
    t = np.array([0.01, 0.03, 0.01, 0.0, 0.01, -0.01, 0.09, -0.5, np.nan, np.nan, 0.02, -0.03], np.float32)
    own = ~np.isnan(t)
    n = int(own.sum())
    for dtype in (torch.float32, torch.float64):
        ft, tt = torch.from_numpy(f).to(dtype), torch.from_numpy(t).to(dtype)
        l, w = fit.clamped_l1_rule(ft, tt, c, n)
        x = ft[torch.from_numpy(own)].clone().requires_grad_()
        term = (x.clamp(-c, c) - tt[torch.from_numpy(own)].clamp(-c, c)).abs().mean()
        term.backward()
        inv_n = torch.tensor(1.0 / n, dtype=torch.float64).to(dtype)
        assert l.dtype == dtype and w.dtype == dtype
        # the weights are sign / n exactly; autograd's are the same numbers
        assert torch.equal(w[torch.from_numpy(own)], x.grad) and not w[torch.from_numpy(~own)].any() and not l[torch.from_numpy(~own)].any()
        assert set(np.unique(w.numpy())) <= {-float(inv_n), 0.0, float(inv_n)}
        assert abs(float(l.double().sum()) / n - float(term.detach())) <= 1e-6 * float(term.detach())
        l64, w64 = fc.loss_rule_f64(ft.double().numpy(), tt.double().numpy(), c, n)
        assert np.array_equal(np.sign(w.numpy()), np.sign(w64)) and np.abs(l.numpy() - l64).max() <= 1e-7
        wn = w.numpy()
        assert wn[0] == 0 and wn[11] == 0                                    # f == t: sign(0) = 0
        assert wn[2] > 0 and wn[3] < 0                                       # f == +-c passes the inclusive mask (also without a clamp)
        assert (wn[4] == 0 and wn[5] == 0 and wn[10] == 0) == (not np.isinf(c))          # |f| > c: off - unless there is no clamp
        assert wn[6] < 0 and wn[7] > 0                                       # t outside the clamp still says which way
    # a head with an empty set: nothing, and no division by zero
    l, w = fit.clamped_l1_rule(torch.from_numpy(f), torch.full((len(f),), float("nan")), c, 0)
    assert not l.any() and not w.any() and bool(torch.isfinite(w).all())


def test_fit_targets_build_one_nan_masked_list():
    class Dev:
        device = torch.device("cpu")
    xh, xo, sh = np.ones((3, 3), np.float32), 2 * np.ones((2, 3), np.float32), 3 * np.ones((4, 3), np.float32)
    xyz, th, to, nh, no = fit.fit_targets(Dev(), sdf_hand=(xh, np.array([0.1, 0.2, 0.3])), sdf_obj=(xo, np.array([-0.1, -0.2])), surface_hand=sh)
    assert tuple(xyz.shape) == (9, 3) and (nh, no) == (7, 2)
    assert int((~torch.isnan(th)).sum()) == 7 and int((~torch.isnan(to)).sum()) == 2
    assert torch.equal(th[3:7], torch.zeros(4)) and torch.isnan(th[7:]).all() and torch.equal(to[7:], torch.tensor([-0.1, -0.2]))
    xyz, th, to, nh, no = fit.fit_targets(Dev(), sdf_obj=(xo, np.zeros(2)))
    assert th is None and (nh, no) == (0, 2)
    with pytest.raises(ValueError):
        fit.fit_targets(Dev())


# ---- the fp64 reference of the device test stays within its own cap ---------------------------------------------------------------------------
def test_truth_case_leaves_out_no_more_than_the_cap():
    case = fc.truth_case()
    M = len(case["pts"])
    for name in vc.HEADS:
        share = float(case["clear"][name].mean())
        w = case["w64"][name]
        print("FITCODE truth case %s: %.4f of %d points clear, %d of them inside the clamp" % (name, share, M, int((w != 0).sum())))
        assert share >= vc.MIN_CLEAR_SHARE, (name, share)
        assert (w != 0).sum() >= 0.2 * M and set(np.unique(np.abs(w))) <= {0.0, 1.0 / M}
        assert not np.isnan(case["t"][name]).any()


# ---- the flow's host logic ------------------------------------------------------------------------------------------------------------------
def test_frame_map_is_the_writers_placement():
    """to_decoder_frame / from_decoder_frame invert each other, and from_decoder_frame is utils.mesh.place_vertices - the arithmetic
    sample_writer places a written mesh with - for scale = 2 / (SdfScaleFactor unit_m) and offset = centre / unit_m."""
    from alignsdf_amd.utils.mesh import place_vertices
    rng = np.random.default_rng(0)
    sf, unit_m, centre = syn.SDF_SCALE_OBMAN, 0.001, np.array([0.02, -0.1, 0.4])
    v = torch.from_numpy(rng.uniform(0, 63, (50, 3)))
    origin, voxel = [-1.0, -1.0, -1.0], 2.0 / 63
    _, _, placed = place_vertices(v, torch.zeros(1, 3, dtype=torch.int64), origin, voxel, offset=centre / unit_m, scale=2.0 / (sf * unit_m))
    x = np.asarray(origin) + v.numpy() * voxel
    files = ad.from_decoder_frame(x, unit_m, centre, sf)
    assert np.abs(files - placed).max() <= 1e-9 * np.abs(placed).max()
    assert np.abs(ad.to_decoder_frame(files, unit_m, centre, sf) - x).max() <= 1e-12
    assert np.abs(ad.to_decoder_frame([[0.5, 0.0, 0.0]], 1.0, [0.5, 0, 0], 2.0)).max() == 0.0


def _tree(root, names, only_hand=()):
    for sub, which in (("mesh_hand", names + list(only_hand)), ("mesh_obj", names)):
        os.makedirs(os.path.join(root, "obman", "test", sub), exist_ok=True)
        for n in which:
            with open(os.path.join(root, "obman", "test", sub, n + ".obj"), "w") as fh:
                fh.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")


def test_flow_with_a_stub_fit(tmp_path):
    from alignsdf_amd.code_sources import npz_code_source
    names = ["00000005", "00000001", "00000009", "00000003"]
    data, poses, init = str(tmp_path / "data"), str(tmp_path / "poses"), str(tmp_path / "init")
    _tree(data, names, only_hand=["00000007"])
    os.makedirs(poses), os.makedirs(init)
    lat0, mano, obj = syn.sample_inputs("both9", 1)
    for i, n in enumerate(names):
        np.savez(os.path.join(poses, n + ".npz"), global_trans=mano["global_trans"], rot_center=mano["rot_center"] + i, obj_trans=obj["obj_trans"],
                 unrelated=np.zeros(3))
        np.savez(os.path.join(init, n + ".npz"), latent=np.full((1, L), float(i), np.float32))
    seen = []

    def stub(name, hand_path, obj_path, pose, start):
        assert hand_path.endswith(os.path.join("mesh_hand", name + ".obj")) and obj_path.endswith(os.path.join("mesh_obj", name + ".obj"))
        seen.append((name, float(start[0]), sorted(pose)))
        return start + 0.5, {"first": 2.0, "last": 1.0, "steps": 7, "mesh_info": {"hand": {"skipped": 0, "zero_area": 0}}}

    specs = syn.specs_for("both9")
    # a pose-aligned decoder without poses: an error before any work
    with pytest.raises(ValueError, match="poses"):
        ad.run(specs, stub, "obman", data, str(tmp_path / "never"))
    assert not seen and not os.path.exists(str(tmp_path / "never"))
    out = str(tmp_path / "codes")
    path, records = ad.run(specs, stub, "obman", data, out, poses, init, start=1, end=3)
    # discovery: pairs only, sorted; [start, end) of them
    assert [s[0] for s in seen] == ["00000003", "00000005"] and [r["name"] for r in records] == ["00000003", "00000005"]
    assert seen[0][1] == 3.0 and seen[1][1] == 0.0 and seen[0][2] == ["global_trans", "obj_trans", "rot_center"]
    body = json.load(open(path))
    assert path == os.path.join(out, "autodecode.json") and body["samples"][0] == dict({"name": "00000003"}, **stub("00000003", "mesh_hand/00000003.obj", "mesh_obj/00000003.obj", {}, np.zeros(1))[1])
    assert sorted(os.listdir(out)) == ["00000003.npz", "00000005.npz", "autodecode.json"]
    source = npz_code_source(out)
    lat, m, o = source("00000003", 0)
    assert tuple(lat.shape) == (1, L) and float(lat[0, 0]) == 3.5
    assert np.array_equal(m["global_trans"].numpy(), mano["global_trans"]) and np.array_equal(m["rot_center"].numpy(), mano["rot_center"] + 3)
    assert np.array_equal(o["obj_trans"].numpy(), obj["obj_trans"]) and "unrelated" not in np.load(os.path.join(out, "00000003.npz")).files
    assert "2 samples, 7 steps" in ad.summary_line(records) and "no mesh pairs" in ad.summary_line([])
    # a poses file that lacks one of the three arrays: an error that names the file, before the sample is fitted
    np.savez(os.path.join(poses, "00000009.npz"), global_trans=mano["global_trans"], rot_center=mano["rot_center"])
    seen.clear()
    with pytest.raises(ValueError, match=r"00000009\.npz.*obj_trans"):
        ad.run(specs, stub, "obman", data, str(tmp_path / "partial"), poses, start=3)
    assert not seen
    # without --init the start is the zero code; a decoder that is not pose-aligned needs no poses and writes the latent alone
    seen.clear()
    _, records = ad.run(syn.specs_for("nerf3"), stub, "obman", data, str(tmp_path / "plain"))
    assert len(records) == 4 and all(s[1] == 0.0 and s[2] == [] for s in seen)
    assert np.load(os.path.join(str(tmp_path / "plain"), "00000001.npz")).files == ["latent"]
    assert ad.pose_aligned(specs) and not ad.pose_aligned(syn.specs_for("nerf3")) and not ad.pose_aligned(syn.specs_for("nerf9"))


def test_abi_bookkeeping():
    from alignsdf_amd import _native
    assert "asdf_fit_code" in _native.EXPORTS and _native.ABI_VERSION == 132
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "alignsdf_hip.h")) as fh:
        text = fh.read()
    assert "int asdf_fit_code(" in text and "#define ASDF_FIT_STATE_BYTES %d" % _native.FIT_STATE_BYTES in text
