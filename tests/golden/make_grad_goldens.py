"""Generate tests/golden/ref_sdf_grad.npz by RUNNING THE REFERENCE (zerchen/AlignSDF at /root/reference): the fp32 values of its own
SeparateDecoder and their torch autograd gradients with respect to the query points, 257 points each of "nerf3" and "both9" (sample 1
of tests/sdf_grad_cases.py).  Runs only in the build container (the reference tree does not travel to the GPU box); the reference
modules are imported with the stubs of make_ref_goldens.py.

    python tests/golden/make_grad_goldens.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ref_goldens import import_reference, syn  # noqa: E402

from tests import sdf_grad_cases as gc  # noqa: E402

M = 257


def main():
    arch, um, uu, dm = import_reference()
    gold = {}
    for tag in ("nerf3", "both9"):
        specs = syn.specs_for(tag)
        dec = arch.SeparateDecoder(256, specs["PointFeatSize"], specs["EncodeStyle"], **specs["NetworkSpecs"], use_classifier=False).eval()
        dec.load_state_dict({k: torch.from_numpy(v) for k, v in syn.full_state_dict(tag).items()})
        latent, mano, obj = syn.sample_inputs(tag, gc.SAMPLE)
        t = lambda d: None if d is None else {k: torch.from_numpy(v) for k, v in d.items()}
        mano, obj, latent = t(mano), t(obj), torch.from_numpy(latent)
        pts = gc.list_points(M)
        x = torch.from_numpy(pts).requires_grad_()
        q = x
        if specs["PointFeatSize"] > 3:
            q = uu.kinematic_embedding(x, mano, M, specs["PointFeatSize"], specs["SdfScaleFactor"], obj, specs["EncodeStyle"])
        h, o, _ = uu.decode_sdf_multi_output(dec, latent, q, mano, None, specs)
        gold[tag + ".pts"] = pts
        for name, v in (("hand", h), ("obj", o)):
            g, = torch.autograd.grad(v.sum(), x, retain_graph=True)
            gold["%s.sdf_%s" % (tag, name)] = v.detach().reshape(-1).numpy()
            gold["%s.grad_%s" % (tag, name)] = g.numpy()
        print(tag, "max |grad|", float(np.abs(gold[tag + ".grad_hand"]).max()), float(np.abs(gold[tag + ".grad_obj"]).max()))
    np.savez_compressed(os.path.join(HERE, "ref_sdf_grad.npz"), **gold)


if __name__ == "__main__":
    main()
