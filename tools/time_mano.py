"""Cost of the MANO kernels (csrc/mano.hip) against the torch statement (mano.mano_torch, stock PyTorch-ROCm launches and autograd) on
the same GPU, and of the fits built on them.

  1. B in {1, 8, 64}, V = 778, ncomps 15, by device events, warmed up, the two paths alternated in one call:
       forward (all five outputs), and forward + reverse (cotangents of verts, joints and global_trans);
  2. a 300-step vertex-target fit (the known-answer problem of tests/mano_cases.py), both ways: wall time and final rms;
  3. a 300-step SDF-term fit on the synthetic pose-aligned decoder "both9", both ways.
  "statement" below is mano_torch on device tensors: a ManoLayer stand-in whose call is the torch graph.

    python tools/time_mano.py >> profiles/mano.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.environ.get("ASDF_TREE", "."))
from alignsdf_amd import mano, mano_fit  # noqa: E402
from alignsdf_amd import synthetic as syn  # noqa: E402

REPS = int(os.environ.get("ASDF_TIMING_REPS", "15"))
NCOMPS = 15


class StatementLayer:
    """ManoLayer's call by the torch statement, whatever the device."""

    def __init__(self, model, ncomps, center_idx=0):
        self.model, self.ncomps, self.center_idx = model, ncomps, center_idx

    def __call__(self, pose, shape, trans=None):
        return mano.mano_torch(self.model, pose, shape, trans, center_idx=self.center_idx)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    model = mano.ManoModel.synthetic(3, 778)
    layer, statement = mano.ManoLayer(model, ncomps=NCOMPS, center_idx=0), StatementLayer(model, NCOMPS)
    dm = layer.device_model("cuda")
    print("# %s | synthetic model, V = 778, ncomps %d, median of %d alternated runs, device events" % (
        torch.cuda.get_device_name(0), NCOMPS, REPS))
    for B in (1, 8, 64):
        pose = torch.from_numpy((0.5 * syn.normal((B, 3 + NCOMPS), 60000 + B)).astype(np.float32)).cuda()
        shape = torch.from_numpy(syn.normal((B, 10), 60100 + B).astype(np.float32)).cuda()
        cv, cj, cg = (torch.from_numpy(syn.normal((B,) + s, 60200 + i).astype(np.float32)).cuda()
                      for i, s in enumerate(((778, 3), (21, 3), (16, 4, 4))))
        d_out = (torch.empty(B, 3 + NCOMPS, device="cuda"), torch.empty(B, 10, device="cuda"))

        def kernels_both():
            dm.forward(pose, shape, None, 0)
            dm.backward(pose, shape, None, 0, cv, cj, cg, None, out=d_out)

        def statement_forward():
            with torch.no_grad():
                statement(pose, shape)

        def statement_both():
            p, s = pose.detach().requires_grad_(True), shape.detach().requires_grad_(True)
            v, j, _, g, _ = statement(p, s)
            torch.autograd.grad((v * cv).sum() + (j * cj).sum() + (g * cg).sum(), (p, s))
        forms = {"kernels fwd": lambda: dm.forward(pose, shape, None, 0), "statement fwd": statement_forward,
                 "kernels fwd+rev": kernels_both, "statement fwd+rev": statement_both}
        for fn in forms.values():
            for _ in range(3):
                fn()
        times = {k: [] for k in forms}
        for _ in range(REPS):
            for k, fn in forms.items():
                times[k].append(events(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("B=%-3d forward: kernels %.3f ms | statement %.3f ms | %.1f x     forward + reverse: kernels %.3f ms | statement %.3f ms | %.1f x"
              % (B, med["kernels fwd"], med["statement fwd"], med["statement fwd"] / med["kernels fwd"], med["kernels fwd+rev"],
                 med["statement fwd+rev"], med["statement fwd+rev"] / med["kernels fwd+rev"]))

    from tests.mano_cases import FIT_LR, FIT_NCOMPS, FIT_STEPS, fit_problem
    fmodel, _, _, target, start = fit_problem(torch.float32, "cuda")
    zero = torch.zeros(1, 10, device="cuda")
    for name, lay in (("kernels", mano.ManoLayer(fmodel, ncomps=FIT_NCOMPS, center_idx=0)), ("statement", StatementLayer(fmodel, FIT_NCOMPS))):
        mano_fit.fit_mano(lay, start, zero, verts_target=target, steps=3, lr=FIT_LR)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = mano_fit.fit_mano(lay, start, zero, verts_target=target, steps=FIT_STEPS, lr=FIT_LR)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        rms = float(((res.verts - target) ** 2).sum(-1).mean().sqrt())
        print("vertex fit %-9s %d steps in %.1f ms (wall, %.3f ms per step): rms -> %.3e" % (name, FIT_STEPS, ms, ms / FIT_STEPS, rms))

    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.networks.model import build_decoder
    from alignsdf_amd.utils.utils import bind_sample
    specs = syn.specs_for("both9")
    module = build_decoder(specs, {k: torch.from_numpy(v) for k, v in syn.full_state_dict("both9").items()}).eval()
    dec = HipSdfDecoder(module)
    latent, mano_in, obj_in = syn.sample_inputs("both9", 0)
    t = lambda d: {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}
    bind_sample(dec, specs, torch.from_numpy(latent), t(mano_in), t(obj_in))
    pose = (0.2 * syn.normal((1, 3 + NCOMPS), 57001)).astype(np.float32)
    pose[0, :3] = 0.0
    pose = torch.from_numpy(pose).cuda()
    for name, lay in (("kernels", layer), ("statement", statement)):
        kw = dict(decoder=dec, head="hand", scale_factor=specs["SdfScaleFactor"], lr=0.02)
        mano_fit.fit_mano(lay, pose, zero, steps=3, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = mano_fit.fit_mano(lay, pose, zero, steps=300, **kw)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        print("SDF-term fit %-9s 300 steps in %.1f ms (wall, %.3f ms per step): mean |f| %.4e -> %.4e" % (
            name, ms, ms / 300, res.losses[0], res.losses[-1]))
    dec.close()


if __name__ == "__main__":
    main()
