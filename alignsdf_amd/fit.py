"""Fitting a sample's latent code and pose to surface points, on the reverse-mode decoder kernel.

`sdf_at_points` makes the bound quantities of a decoder - the latent code and the per-head point embedding - differentiable torch
inputs: its backward is one `decode_points_vjp` launch (csrc/k1v_kernels.hip) on a HipSdfDecoder and plain autograd through the module
on a TorchModuleDecoder.  `kinematic_affine_torch` carries an embedding gradient further, to the pose the embedding was built from, and
`fit_sample` is the usual test-time refinement of an SDF auto-decoder on top: Adam over the code and one rigid shift per head.
`fit_code` is the auto-decode proper - the code alone against (xyz, sdf) targets - with the whole Adam loop on the device
(HipSdfDecoder.fit_code); `fit_code_lockstep`, `clamped_l1_rule` and `adam_step_host` state its rule on the host.
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


# ---- auto-decode: the code alone, against SDF targets, on the device ----------------------------------------------------------------------
# One rule, one device loop: fit_loop of csrc/decoder.hip (every step a stream of launches over B >= 1 samples) behind both asdf_fit_codes
# and asdf_fit_code, its batch of one.  Beside it the rule stands twice on the host: fit_code_lockstep below (one step at a time, the
# weights made in torch, the step on the host) and - operation by operation - clamped_l1_rule and adam_step_host.
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8


def adam_step_table(steps, lr, decay=1.0, every=1, b1=ADAM_B1, b2=ADAM_B2, dtype=np.float32):
    """[steps, 2] (a_k, s_k) of Adam's step k with its bias corrections folded in: a_k = lr_k / (1 - b1^(k+1)), s_k = 1 / sqrt(1 -
    b2^(k+1)), lr_k = lr decay^(k // every) (DeepSDF's reconstruction schedule; decay = 1: a constant rate) - computed in double and
    rounded once to `dtype`.  b1 and b2 enter with the fp32 values the step itself uses: the corrections are those of the recursion
    that runs."""
    b1, b2 = float(np.float32(b1)), float(np.float32(b2))
    k = np.arange(int(steps), dtype=np.float64)
    lr_k = float(lr) * float(decay) ** np.floor(k / max(int(every), 1))
    a = lr_k / (1.0 - float(b1) ** (k + 1.0))
    s = 1.0 / np.sqrt(1.0 - float(b2) ** (k + 1.0))
    return np.stack([a, s], 1).astype(dtype)


def prior_factor(prior, latent_size, dtype=np.float32):
    """k_prior = 2 prior / L, the factor of (z - z0) in the gradient of prior mean((z - z0)^2): in double from the fp32 value of
    `prior` (the C ABI carries it as a float), rounded once."""
    return np.dtype(dtype).type(2.0 * float(np.float32(prior)) / int(latent_size))


def adam_step_host(z, m, v, d_latent, z0, k_prior, a, s, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """THE DEFINITION of the fit's Adam step, in numpy, in the dtype of z (fp32 in the product; fp64 as the tests' yardstick) - every
    line below is one correctly rounded operation per element, in this order, and the device step (csrc/k1vb_kernels.hip:
    adam_step_batch_kernel) equals it in every bit:
        g = d_latent + k_prior (z - z0)
        m = b1 m + (1 - b1) g
        v = b2 v + ((1 - b2) g) g
        z = z - a (m / (sqrt(v) s + eps))
    (a, s): this step's row of adam_step_table.  Returns the new (z, m, v); the inputs are left as they are."""
    t = np.asarray(z).dtype.type
    z, m, v, d, z0 = (np.asarray(x, dtype=t) for x in (z, m, v, d_latent, z0))
    b1, b2, eps, k_prior, a, s, one = t(b1), t(b2), t(eps), t(k_prior), t(a), t(s), t(1)
    g = z - z0
    g = k_prior * g
    g = d + g
    m = b1 * m
    m = m + (one - b1) * g          # (two operations: the product is rounded before the sum)
    w = (one - b2) * g
    w = w * g
    v = b2 * v
    v = v + w
    den = np.sqrt(v)
    den = den * s
    den = den + eps
    q = m / den
    q = a * q
    return z - q, m, v


def clamped_l1_rule(f, t, clamp, n):
    """The loss form's rule per point, in torch and in the dtype of f: for values f [M], targets t [M] (NaN: the point is not in this
    head's set), the clamp c (inf: unclamped) and the size n of the set,
        r = clip(f, -c, c) - clip(t, -c, c);   l = |r|;   w = (t is NaN or f < -c or f > c) ? 0 : sign(r) (1 / n)
    with 1 / n computed in double and rounded once, sign(0) = 0 and the clamp's mask inclusive (f = +-c passes), as torch.clamp's
    backward: (l, w) are fit_sample's (f.clamp(-c, c) - s.clamp(-c, c)).abs().mean() term by term and its autograd weight.  l = 0
    outside the set.  c is the fp32 value of `clamp` in every dtype (the C ABI carries it as a float).  Returns (l [M], w [M])."""
    c = float(np.float32(clamp))
    t = t.to(f.dtype)
    out = torch.isnan(t)
    r = f.clamp(-c, c) - torch.nan_to_num(t, nan=0.0).clamp(-c, c)
    inv_n = torch.tensor(1.0 / n if n > 0 else 0.0, dtype=torch.float64).to(f.dtype)
    zero = torch.zeros((), dtype=f.dtype, device=f.device)
    l = torch.where(out, zero, r.abs())
    w = torch.where(out | (f < -c) | (f > c), zero, torch.sign(r) * inv_n.to(f.device))
    return l, w


def fit_targets(decoder, sdf_hand=None, sdf_obj=None, surface_hand=None, surface_obj=None):
    """One point list with NaN-masked per-head targets from fit_sample's kinds of input: sdf_* = (xyz [m, 3], sdf [m]) pairs, surface_*
    [n, 3] points (targets 0).  Returns (xyz [M, 3], t_hand [M] or None, t_obj [M] or None, n_hand, n_obj) on the decoder's device."""
    dev = decoder.device
    f32 = lambda a: torch.as_tensor(a).detach().to(dev, torch.float32)
    parts = []            # (head, xyz, targets)
    for head, valued, surface in ((0, sdf_hand, surface_hand), (1, sdf_obj, surface_obj)):
        if valued is not None:
            parts.append((head, f32(valued[0]).reshape(-1, 3), f32(valued[1]).reshape(-1)))
        if surface is not None:
            x = f32(surface).reshape(-1, 3)
            parts.append((head, x, torch.zeros(x.shape[0], dtype=torch.float32, device=dev)))
    if not parts:
        raise ValueError("fit_code: no targets")
    xyz = torch.cat([x for _, x, _ in parts], 0)
    ts, ns = [None, None], [0, 0]
    at = 0
    for head, x, t in parts:
        if ts[head] is None:
            ts[head] = torch.full((xyz.shape[0],), float("nan"), dtype=torch.float32, device=dev)
        ts[head][at:at + x.shape[0]] = t
        if torch.isnan(t).any():
            raise ValueError("fit_code: a NaN target")
        ns[head] += x.shape[0]
        at += x.shape[0]
    return xyz, ts[0], ts[1], ns[0], ns[1]


def _bind_code(decoder, latent, embed):
    """Bind `latent` with the embeddings `embed` (torch or numpy; None: plain xyz) on a HipSdfDecoder."""
    if embed is not None:
        embed = tuple(np.asarray(e.detach().cpu() if torch.is_tensor(e) else e, np.float64) for e in embed)
    decoder.set_sample(latent.detach().reshape(1, -1), embed=embed)


def _module_values_f64(decoder, module64, lat, embed, xyz):
    """decode_embedded's SeparateDecoder branch on a double copy of the module (the fp64 statement of the rule)."""
    cols = decoder._head_columns()
    if cols is None:
        raise NotImplementedError("the fp64 lockstep is written for SeparateDecoder with point features affine in xyz")
    pf = int(decoder.specs["PointFeatSize"])
    if embed is None:
        embed = (torch.eye(3, 4, dtype=torch.float64, device=xyz.device),) * 2
    out = []
    for h, (E, c) in enumerate(zip(embed, cols)):
        E = E.to(xyz.device, torch.float64)
        q = torch.zeros(xyz.shape[0], pf, dtype=torch.float64, device=xyz.device).index_copy(1, c, xyz @ E[:, :3].t() + E[:, 3])
        out.append(module64(torch.cat([lat.reshape(1, -1).expand(xyz.shape[0], -1), q], 1))[h].reshape(-1))
    return tuple(out)


def fit_code_lockstep(decoder, latent, embed, xyz, t_hand, t_obj, n_hand, n_obj, z0=None, steps=800, lr=5e-3, decay=0.1, every=400,
                      prior=1e-4, clamp=0.05, dtype=torch.float32):
    """HipSdfDecoder.fit_code's rule one step at a time, the host in the loop: per step the values (decode_points on the fp32 chain),
    the weights and the data term by clamped_l1_rule in torch, the gradient from decode_points_vjp, the step by adam_step_host.  On a
    HipSdfDecoder the kernel covers this is fit_code's result bit for bit (the history to the rounding of an fp64 sum).  On a
    TorchModuleDecoder - every variant with a per-sample latent code - the values and the gradient come from sdf_at_points and
    autograd; there dtype=torch.float64 runs the whole rule in double on a double copy of the module (SeparateDecoder, affine
    features): the yardstick the fp32 statements are measured against.  Arguments as HipSdfDecoder.fit_code, plus the start `latent`
    and the embeddings `embed` to bind.  Returns (latent [L] in dtype, history [steps] fp64) on the decoder's device."""
    dev = decoder.device
    module_path = hasattr(decoder, "decode_embedded")
    if dtype != torch.float32 and not module_path:
        raise ValueError("fit_code_lockstep: dtype %s on the module path only" % dtype)
    npt = np.float64 if dtype == torch.float64 else np.float32
    xyz = xyz.detach().to(dev, torch.float32)
    ts = [None if (t is None or n == 0) else t.detach().to(dev, torch.float32).reshape(-1) for t, n in ((t_hand, n_hand), (t_obj, n_obj))]
    ns = (int(n_hand), int(n_obj))
    z = latent.detach().reshape(-1).cpu().numpy().astype(npt)
    zc = z.copy() if z0 is None else z0.detach().reshape(-1).cpu().numpy().astype(npt)
    m, v = np.zeros_like(z), np.zeros_like(z)
    table = adam_step_table(steps, lr, decay, every, dtype=npt)
    k_prior = prior_factor(prior, z.size, npt)
    history = torch.zeros(int(steps), dtype=torch.float64, device=dev)
    if embed is not None:
        embed = tuple(torch.as_tensor(e).detach().to(dev) for e in embed)
    module64 = None
    if dtype == torch.float64:
        import copy
        # (old-style weight_norm leaves the effective weight of its last forward on the module as a non-leaf tensor, which deepcopy
        # refuses: it is handed a detached clone, as TorchModuleDecoder.module does - the pre-hook recomputes it on every call)
        memo = {id(val): val.detach().clone() for sub in decoder.module.modules() for val in vars(sub).values()
                if torch.is_tensor(val) and not val.is_leaf}
        module64 = copy.deepcopy(decoder.module, memo).double().eval()
        xyz = xyz.double()
    before = None if module_path else decoder.math
    try:
        for k in range(int(steps)):
            zt = torch.from_numpy(z).to(dev)
            if module_path:
                zt.requires_grad_()
                with torch.enable_grad():
                    f = _module_values_f64(decoder, module64, zt, embed, xyz) if module64 is not None else sdf_at_points(decoder, zt, embed, xyz)
            else:
                _bind_code(decoder, zt, embed)
                decoder.set_math("f32")
                f = decoder.decode_points(xyz)
            ws, data = [None, None], torch.zeros((), dtype=torch.float64, device=dev)
            for h in range(2):
                if ts[h] is not None:
                    l, ws[h] = clamped_l1_rule(f[h].detach(), ts[h], clamp, ns[h])
                    data = data + l.double().sum() * (1.0 / ns[h])
            history[k] = data
            if ws[0] is None and ws[1] is None:
                d = np.zeros_like(z)
            elif module_path:
                d = torch.autograd.grad(sum((f[h] * ws[h]).sum() for h in range(2) if ws[h] is not None), zt)[0].cpu().numpy().astype(npt)
            else:
                d = decoder.decode_points_vjp(xyz, w_hand=ws[0], w_obj=ws[1], want_sdf=False).d_latent.cpu().numpy()
            z, m, v = adam_step_host(z, m, v, d, zc, k_prior, table[k, 0], table[k, 1])
    finally:
        if before is not None:
            decoder.set_math(before)
    out = torch.from_numpy(z).to(dev)
    if not module_path and int(steps) > 0 and xyz.shape[0] > 0:
        _bind_code(decoder, out, embed)
    return out, history


def fit_code(decoder, latent, embed, sdf_hand=None, sdf_obj=None, surface_hand=None, surface_obj=None, z0=None, steps=800, lr=5e-3,
             decay=0.1, every=400, prior=1e-4, clamp=0.05, module=None, specs=None):
    """Auto-decode one sample: Adam over the latent code alone (the embeddings stay; fit_sample keeps the per-head shifts) on
        sum over heads of mean |clip(f, -clamp, clamp) - clip(s, -clamp, clamp)|  +  prior mean((z - z0)^2)
    over fit_sample's kinds of input - sdf_hand / sdf_obj = (xyz [m, 3], sdf [m]) pairs in the decoder's normalised space
    (mesh_sdf.sdf_samples makes them), surface_hand / surface_obj [n, 3] surface points - all in ONE point list with NaN-masked
    per-head targets (fit_targets).  Surface points are targets 0 UNDER THE SAME CLAMP: their term is |clip(f, -clamp, clamp)|, which
    stops pulling where |f| > clamp - unlike fit_sample's unclamped |f| there.  z0: the prior's centre (None: the start code); the rate
    of step k is lr decay^(k // every).
    On a HipSdfDecoder the whole loop is enqueued by one call (HipSdfDecoder.fit_code: nothing is read back, nothing waits) and the
    decoder is left bound to the fitted code.  A TorchModuleDecoder runs the same rule in fit_code_lockstep, one step at a time on the
    module path - and so does a HipSdfDecoder that call refuses (fit_code_refusal: CombinedDecoder, NeRF-encoded features), through a
    TorchModuleDecoder of `module` with `specs` (the nn.Module the decoder was packed from: a HipSdfDecoder does not keep it); without
    them such a decoder raises NotImplementedError with the reason.  Returns (latent [L], history [steps] fp64: the data term before
    each step), device tensors."""
    xyz, t_hand, t_obj, n_hand, n_obj = fit_targets(decoder, sdf_hand, sdf_obj, surface_hand, surface_obj)
    kw = dict(z0=z0, steps=steps, lr=lr, decay=decay, every=every, prior=prior, clamp=clamp)
    latent = latent.detach().reshape(-1).to(decoder.device, torch.float32)
    if hasattr(decoder, "decode_embedded"):
        return fit_code_lockstep(decoder, latent, embed, xyz, t_hand, t_obj, n_hand, n_obj, **kw)
    why = decoder.fit_code_refusal()
    if why is not None:
        if module is None or specs is None:
            raise NotImplementedError("the fit kernel does not cover this decoder: %s (pass module= and specs=, or a TorchModuleDecoder "
                                      "of the same module: fit_code then runs on the module path)" % why)
        from .torch_decoder import TorchModuleDecoder
        fallback = TorchModuleDecoder(module, specs, "fit_code: %s" % why, decoder.device)
        return fit_code_lockstep(fallback, latent, embed, xyz, t_hand, t_obj, n_hand, n_obj, **kw)
    _bind_code(decoder, latent, embed)
    return decoder.fit_code(xyz, t_hand, t_obj, n_hand, n_obj, latent, **kw)


def fit_codes(decoder, items, steps=800, lr=5e-3, decay=0.1, every=400, prior=1e-4, clamp=0.05, module=None, specs=None):
    """fit_code over many samples.  Each item is a dict with fit_code's per-sample inputs: `latent`, `embed` and any of `sdf_hand`,
    `sdf_obj`, `surface_hand`, `surface_obj`, `z0` (absent = None); the rule (steps, lr, decay, every, prior, clamp) is shared.  On a
    HipSdfDecoder the kernel covers, the whole batch is ONE stream of launches (HipSdfDecoder.fit_codes: every step carries all
    samples, nothing is read back, nothing waits), every sample to the bits fit_code gives it alone; the decoder's bound sample is
    left as it was.  On a TorchModuleDecoder - and, with `module` and `specs`, on a HipSdfDecoder the kernel refuses - the items run
    through fit_code one after the other: the results of a loop over fit_code.  Returns (latents [B, L], history [B, steps] fp64),
    device tensors."""
    items = list(items)
    if not items:
        raise ValueError("fit_codes: no items")
    rule = dict(steps=steps, lr=lr, decay=decay, every=every, prior=prior, clamp=clamp)
    kinds = ("sdf_hand", "sdf_obj", "surface_hand", "surface_obj")
    if hasattr(decoder, "decode_embedded") or decoder.fit_codes_refusal() is not None:
        outs = [fit_code(decoder, it["latent"], it.get("embed"), z0=it.get("z0"), module=module, specs=specs,
                         **{k: it.get(k) for k in kinds}, **rule) for it in items]
        return torch.stack([z for z, _ in outs]), torch.stack([h for _, h in outs])
    targets = [fit_targets(decoder, *(it.get(k) for k in kinds)) for it in items]
    latents = torch.stack([it["latent"].detach().reshape(-1).to(decoder.device, torch.float32) for it in items])
    z0s = [it.get("z0") for it in items]
    return decoder.fit_codes([t[0] for t in targets], [t[1] for t in targets], [t[2] for t in targets], [t[3] for t in targets],
                             [t[4] for t in targets], latents, [it.get("embed") for it in items],
                             z0=None if all(c is None for c in z0s) else z0s, **rule)
