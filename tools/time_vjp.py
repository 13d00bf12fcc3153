"""Cost of the reverse-mode decoder kernel (HipSdfDecoder.decode_points_vjp, csrc/k1v_kernels.hip) and the fit built on it.

  1. P in {1024, 65536} points, both heads, by device events, interleaved on one box:
       the native VJP call (forward + reverse chain + the two small reduction kernels),
       decode_points under math "f32" on the same list - the floor: the reverse chain issues the same MFMAs again -
       and the module-path VJP (TorchModuleDecoder.decode_points_vjp: torch autograd through the module);
     the three times and the two ratios native / floor and module / native.
  2. the fit scenario of tests/test_gpu_sdf_vjp.py (grasp9 sample 3, fit_sample's defaults) on the native and the module path: the
     loss history, its ratio last / first, and the wall time of the 40 steps.

    python tools/time_vjp.py [--tag grasp9] >> profiles/sdf_vjp.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.environ.get("ASDF_TREE", "."))
from alignsdf_amd import synthetic as syn  # noqa: E402
from alignsdf_amd.networks.model import build_decoder  # noqa: E402

REPS = int(os.environ.get("ASDF_TIMING_REPS", "7"))


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tag", default="grasp9")
    p.add_argument("--label", default="this tree")
    args = p.parse_args()
    from alignsdf_amd.fit import fit_sample
    from alignsdf_amd.hip_decoder import HipSdfDecoder
    from alignsdf_amd.torch_decoder import TorchModuleDecoder
    from alignsdf_amd.utils.utils import bind_sample
    tag = args.tag
    specs = syn.specs_for(tag)
    module = build_decoder(specs, {k: torch.from_numpy(v) for k, v in syn.full_state_dict(tag).items()}).eval()
    t = lambda d: None if d is None else {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}
    latent, mano, obj = syn.sample_inputs(tag, 3)
    hip = HipSdfDecoder(module)
    mod = TorchModuleDecoder(module, specs, "timed against the reverse-mode kernel")
    for dec in (hip, mod):
        bind_sample(dec, specs, torch.from_numpy(latent), t(mano), t(obj))
    print("# %s | %s | %s sample 3, hand + object, median of %d interleaved runs, device events" % (
        args.label, torch.cuda.get_device_name(0), tag, REPS))
    before = hip.math
    hip.set_math("f32")
    for P in (1024, 65536):
        rng = np.random.default_rng(P)
        x = torch.from_numpy(rng.uniform(-1, 1, (P, 3)).astype(np.float32)).cuda()
        wh, wo = (torch.from_numpy(rng.standard_normal(P).astype(np.float32)).cuda() for _ in range(2))
        forms = {"native vjp": lambda: hip.decode_points_vjp(x, wh, wo), "decode_points f32": lambda: hip.decode_points(x),
                 "module vjp": lambda: mod.decode_points_vjp(x, wh, wo)}
        for fn in forms.values():
            fn()
        times = {k: [] for k in forms}
        for _ in range(REPS):
            for k, fn in forms.items():
                times[k].append(events(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("P=%-6d native vjp %.3f ms | decode_points (f32, the floor) %.3f ms | module vjp %.3f ms | native / floor %.2f x | "
              "module / native %.2f x" % (P, med["native vjp"], med["decode_points f32"], med["module vjp"],
                                          med["native vjp"] / med["decode_points f32"], med["module vjp"] / med["native vjp"]))
    hip.set_math(before)

    from tests.sdf_vjp_cases import fit_scenario
    z0, E0, sh, so = fit_scenario(hip)
    for name, dec in (("native", hip), ("module", mod)):
        fit_sample(dec, z0, E0, sh, so, steps=2)          # (first use: the optimizer's and autograd's own set-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, shifts, history = fit_sample(dec, z0, E0, sh, so)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        print("fit %-6s %d + %d targets, 40 steps in %.1f ms (wall): loss %.3e -> %.3e, ratio %.3f | history %s" % (
            name, len(sh), len(so), ms, history[0], history[-1], history[-1] / history[0], " ".join("%.2e" % v for v in history)))
    hip.close()


if __name__ == "__main__":
    main()
