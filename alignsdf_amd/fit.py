"""Fitting a sample's latent code and pose to surface points, on the reverse-mode decoder kernel.

`sdf_at_points` makes the bound quantities of a decoder - the latent code and the per-head point embedding - differentiable torch
inputs: its backward is one `decode_points_vjp` launch (csrc/k1v_kernels.hip) on a HipSdfDecoder and plain autograd through the module
on a TorchModuleDecoder.  `kinematic_affine_torch` carries an embedding gradient further, to the pose the embedding was built from, and
`fit_sample` is the usual test-time refinement of an SDF auto-decoder on top: Adam over the code and one rigid shift per head.
"""
import numpy as np
import torch


def kinematic_affine_torch(point_feat_size, encode_style, scale_factor, mano_results, obj_results, combined=False):
    """hip_decoder.kinematic_affine as a differentiable fp64 torch graph: the same arguments, the same per-head E [pf_head, 4] (feat =
    E[:, :3] xyz + E[:, 3]) - tensors that carry gradients back to mano_results["global_trans"], mano_results["rot_center"] and
    obj_results["obj_trans"].  NeRF style (no pose enters): identity embeddings."""
    sf = float(scale_factor)
    a = 2.0 / sf
    f64 = lambda t: torch.as_tensor(t).to(torch.float64)
    eye = torch.eye(3, dtype=torch.float64)
    rows_hand, rows_obj_tail = [], []
    if encode_style in ("hand", "both"):
        rc = f64(mano_results["rot_center"]).reshape(3)
        rows_hand.append(torch.cat([eye, (rc * sf / 2.0)[:, None]], 1))
        G = f64(mano_results["global_trans"]).reshape(16, 4, 4)
        joints = 1 if ((point_feat_size == 6 and encode_style == "hand") or (point_feat_size == 9 and encode_style == "both")) else 16
        for j in range(joints):
            Gi = torch.linalg.inv(G[j])
            w = Gi[3, :3] @ rc + Gi[3, 3]
            lin = Gi[:3, :3] * a / w
            off = (Gi[:3, :3] @ rc + Gi[:3, 3]) / w
            rows_hand.append(torch.cat([lin * sf / 2.0, (off * sf / 2.0)[:, None]], 1))
    if encode_style in ("obj", "both"):
        Ti = torch.linalg.inv(f64(obj_results["obj_trans"]).reshape(4, 4))
        w = Ti[3, 3]
        rows_obj_tail.append(torch.cat([Ti[:3, :3] * a / w * sf / 2.0, (Ti[:3, 3] / w * sf / 2.0)[:, None]], 1))
    ident = torch.cat([eye, torch.zeros(3, 1, dtype=torch.float64)], 1)
    if encode_style == "nerf":
        return (ident,) if combined else (ident, ident.clone())
    if combined:
        if encode_style == "hand":
            return (torch.cat(rows_hand, 0),)
        if encode_style == "obj":
            return (torch.cat([ident] + rows_obj_tail, 0),)
        return (torch.cat(rows_hand + rows_obj_tail, 0),)
    if encode_style == "hand":
        return torch.cat(rows_hand, 0), rows_hand[0]
    if encode_style == "obj":
        return ident, torch.cat([ident] + rows_obj_tail, 0)
    return torch.cat(rows_hand, 0), torch.cat([rows_hand[0]] + rows_obj_tail, 0)


def shift_embed(E, t):
    """The embedding of the field moved by t (its value at x is the old value at x - t): E'[:, :3] = E[:, :3], E'[:, 3] = E[:, 3] -
    E[:, :3] t.  E [pf, 4], t [3]; a torch graph in both."""
    t = t.to(E.dtype).to(E.device)
    return torch.cat([E[:, :3], (E[:, 3] - E[:, :3] @ t)[:, None]], 1)


class _NativeSdf(torch.autograd.Function):
    """(sdf_hand, sdf_obj) of a HipSdfDecoder as a function of (latent, hand E, obj E, xyz)."""

    @staticmethod
    def forward(ctx, decoder, latent, e_hand, e_obj, xyz):
        ctx.decoder = decoder
        ctx.save_for_backward(latent, e_hand, e_obj, xyz)
        ctx.bound = _bind(decoder, latent, e_hand, e_obj)
        # the values the backward differentiates are the fp32 chain's, whatever arithmetic the decoder's sweeps are set to
        before = decoder.math
        decoder.set_math("f32")
        try:
            return decoder.decode_points(xyz)
        finally:
            decoder.set_math(before)

    @staticmethod
    def backward(ctx, g_hand, g_obj):
        decoder = ctx.decoder
        latent, e_hand, e_obj, xyz = ctx.saved_tensors
        if getattr(decoder, "_bound", None) is not ctx.bound:      # (another sample was bound in between)
            _bind(decoder, latent, e_hand, e_obj)
        r = decoder.decode_points_vjp(xyz, w_hand=g_hand, w_obj=g_obj, want_sdf=False)
        g_xyz = None
        if ctx.needs_input_grad[4]:
            _, gh, _, go = decoder.decode_points_grad(xyz)
            g_xyz = (g_hand.reshape(-1, 1).to(gh.dtype) * gh + g_obj.reshape(-1, 1).to(go.dtype) * go).to(xyz.dtype)
        return (None, r.d_latent.reshape(latent.shape).to(latent.dtype), r.d_embed[0].to(e_hand.dtype), r.d_embed[1].to(e_obj.dtype), g_xyz)


def _bind(decoder, latent, e_hand, e_obj):
    """set_sample with the embeddings as host arrays (its interface: one device -> host copy of the two small matrices per bind);
    returns the decoder's record of the binding, by whose identity the backward knows whether it still holds."""
    both = torch.cat([e_hand.detach().reshape(-1), e_obj.detach().reshape(-1)]).cpu().numpy()
    n = e_hand.numel()
    decoder.set_sample(latent.detach().reshape(1, -1), embed=(both[:n].reshape(e_hand.shape), both[n:].reshape(e_obj.shape)))
    return decoder._bound


def sdf_at_points(decoder, latent, embed, xyz):
    """(sdf_hand [M], sdf_obj [M]) at xyz [M, 3] for the latent code [L] and the point embeddings `embed` - differentiable in latent,
    embed and xyz.
      HipSdfDecoder: embed = (hand [pf_h, 4], obj [pf_o, 4]).  The forward binds the sample and is decode_points on the fp32 chain,
        the backward is one decode_points_vjp launch (plus decode_points_grad when xyz requires grad).  A decoder whose
        vjp_refusal() names a reason raises NotImplementedError with it: such a decoder is differentiated on the module path -
      TorchModuleDecoder: autograd through the module (decode_embedded), for every variant with a per-sample latent code -
        SeparateDecoder and CombinedDecoder with affine features (embed per head / (E,) / None for plain xyz) and NeRF-encoded
        features (embed None: there is no affine embedding to differentiate)."""
    latent = latent.to(decoder.device)
    xyz = xyz.to(decoder.device, torch.float32)
    if embed is not None:
        embed = tuple(e.to(decoder.device) for e in embed)
    if hasattr(decoder, "decode_embedded"):
        return decoder.decode_embedded(latent, embed, xyz)
    why = decoder.vjp_refusal()
    if why is not None:
        raise NotImplementedError("the reverse-mode kernel does not cover this decoder: %s (sdf_at_points runs on a TorchModuleDecoder "
                                  "of the same module)" % why)
    if embed is None:
        embed = (torch.eye(3, 4, device=decoder.device),) * 2
    return _NativeSdf.apply(decoder, latent, embed[0], embed[1], xyz)


def fit_sample(decoder, latent, embed, surface_hand=None, surface_obj=None, steps=40, lr=2e-3, prior=1e-3, penetration=0.0,
               sdf_hand=None, sdf_obj=None, clamp=0.05):
    """Refine a sample against observed surface points: Adam over the latent code z and one rigid shift per head (shift_embed) on
        mean |f_hand(surface_hand)| + mean |f_obj(surface_obj)| + prior mean((z - z0)^2) + penetration mean(relu(-f_obj(surface_hand)))
    with z0 the code it starts from.  surface_* [n, 3] in the decoder's normalised space (None: that term is absent).
    sdf_hand / sdf_obj: an (xyz [m, 3], sdf [m]) pair each, in the same space (mesh_sdf.sdf_samples makes them): that head gains the
    auto-decoder's own term mean |clip(f, -clamp, clamp) - clip(s, -clamp, clamp)|, which - unlike |f| on the surface - says which
    side is inside.  Returns (latent, embed, shifts, history): the fitted code [L] and embeddings, the two shifts [2, 3] and, per
    step, the data terms of the loss (all but prior and penetration) taken before that step."""
    dev = decoder.device
    z0 = latent.detach().reshape(-1).to(dev, torch.float32)
    z = z0.clone().requires_grad_()
    E0 = [torch.as_tensor(np.asarray(e, np.float64) if not torch.is_tensor(e) else e.detach()).to(dev, torch.float32) for e in embed]
    shifts = torch.zeros(2, 3, dtype=torch.float32, device=dev, requires_grad=True)
    sets = [None if s is None else torch.as_tensor(s).detach().to(dev, torch.float32).reshape(-1, 3) for s in (surface_hand, surface_obj)]
    valued = [None if s is None else (torch.as_tensor(s[0]).detach().to(dev, torch.float32).reshape(-1, 3),
                                      torch.as_tensor(s[1]).detach().to(dev, torch.float32).reshape(-1).clamp(-clamp, clamp))
              for s in (sdf_hand, sdf_obj)]
    if all(s is None for s in sets + valued):
        raise ValueError("fit_sample: no surface points")
    pts = torch.cat([s for s in sets if s is not None] + [s[0] for s in valued if s is not None], 0)
    n_hand = 0 if sets[0] is None else sets[0].shape[0]
    first = [0, 0]                                     # where each head's valued points begin in pts
    first[0] = n_hand + (0 if sets[1] is None else sets[1].shape[0])
    first[1] = first[0] + (0 if valued[0] is None else valued[0][0].shape[0])
    opt = torch.optim.Adam([z, shifts], lr=lr)
    history = []
    for _ in range(steps):
        opt.zero_grad()
        E = (shift_embed(E0[0], shifts[0]), shift_embed(E0[1], shifts[1]))
        f_hand, f_obj = sdf_at_points(decoder, z, E, pts)
        data = torch.zeros((), dtype=torch.float32, device=dev)
        if sets[0] is not None:
            data = data + f_hand[:n_hand].abs().mean()
        if sets[1] is not None:
            data = data + f_obj[n_hand:n_hand + sets[1].shape[0]].abs().mean()
        for f, v, at in ((f_hand, valued[0], first[0]), (f_obj, valued[1], first[1])):
            if v is not None:
                data = data + (f[at:at + v[0].shape[0]].clamp(-clamp, clamp) - v[1]).abs().mean()
        loss = data + prior * ((z - z0) ** 2).mean()
        if penetration and sets[0] is not None:
            loss = loss + penetration * torch.relu(-f_obj[:n_hand]).mean()
        history.append(data.detach())
        loss.backward()
        opt.step()
    E = tuple(shift_embed(E0[h], shifts[h]).detach() for h in range(2))
    return z.detach(), E, shifts.detach(), [float(v) for v in torch.stack(history).cpu()]
