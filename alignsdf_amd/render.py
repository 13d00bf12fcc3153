"""One view of a prediction without a mesh: depth, normal and part maps ray-cast straight from the SDF decoder.

A view is one ray per pixel, marched by sphere tracing and refined by bisection - HipSdfDecoder.trace_rays (one kernel:
csrc/k1t_kernels.hip) or, for decoders that kernel does not cover, TorchModuleDecoder.trace_rays (the same rule in torch, all rays in
lockstep: trace_lockstep below).  There is no lattice in it: each hit is a root of the decoder along its own ray.

What sphere tracing cannot promise: a step can jump a feature thinner than the step (min_step bounds the step from below, so a sheet
thinner than min_step can be missed even by a perfect distance field), and a learned field is only approximately a distance - where
it overestimates the distance a step can pass through the surface and come out again without a sample <= 0.  The decoders are trained
as unit-slope distances clamped at +-ClampingDistance, which is why max_step defaults to it.  EXHAUSTED says a ray ran out of steps.

Camera convention (torch_decoder.pixel_alignment, utils/utils.py:538-546): a normalised point x is the camera point
x_cam = x * 2 / scale + root, its pixel (u, v) = (K x_cam)[:2] / (K x_cam)[2] with K the 3 x 3 part of cam_intr; pixel (row i,
column j) of an H x W view has its centre at (u, v) = (j + 0.5, i + 0.5) in the units of cam_intr (a view at another resolution than
the camera's image scales cam_intr: scale_intrinsics)."""
import os

import numpy as np
import torch

MISS, HIT, INSIDE, EXHAUSTED = 0, 1, 2, 3
TRACE_DEFAULTS = {"max_steps": 64, "refine_steps": 6, "step_scale": 1.0, "min_step": 1e-3, "max_step": 0.05}
TILE = (16, 8)           # pixels (wide, tall) of a ray tile: 128 rays, one workgroup's columns


def trace_defaults(specs=None):
    """The trace parameters: max_step is the clamping distance the decoder was trained with."""
    out = dict(TRACE_DEFAULTS)
    if specs is not None:
        out["max_step"] = float(specs.get("ClampingDistance", TRACE_DEFAULTS["max_step"]))
    return out


def pack_rays(origins, dirs, t0, t1, device):
    """[M, 8] fp32 on `device`: origin, direction, t0, t1 (t0 / t1 [M] or scalars)."""
    f32 = lambda v: torch.as_tensor(v).detach().to(device=device, dtype=torch.float32)
    o, d = f32(origins).reshape(-1, 3), f32(dirs).reshape(-1, 3)
    M = o.shape[0]
    if d.shape[0] != M:
        raise ValueError("origins and dirs differ in length")
    rays = torch.empty((M, 8), dtype=torch.float32, device=device)
    rays[:, 0:3], rays[:, 3:6] = o, d
    rays[:, 6], rays[:, 7] = f32(t0).reshape(-1).expand(M), f32(t1).reshape(-1).expand(M)
    return rays


def trace_lockstep(sdf_of, rays, max_steps=64, refine_steps=6, step_scale=1.0, min_step=1e-3, max_step=0.05):
    """The rule of asdf_trace_rays (include/alignsdf_hip.h) in torch fp32 for ONE head: every ray takes its next sample in the same
    call of `sdf_of(points [M, 3]) -> sdf [M]`, finished rays ride along under masks (they feed the origin of the space), and the loop
    ends when no ray is live - one host read per step.  rays [M, 8] fp32.  Returns {"t", "status", "bracket", "evals"} on rays'
    device.  Every operation is one rounded fp32 torch op, so on equal sdf bits the results are the kernel's bit for bit."""
    if max_steps < 1 or refine_steps < 0 or not min_step > 0 or not max_step > 0:
        raise ValueError("max_steps >= 1, refine_steps >= 0, min_step > 0 and max_step > 0 are required")
    dev, M = rays.device, rays.shape[0]
    o, d, t1 = rays[:, 0:3], rays[:, 3:6], rays[:, 7]
    c = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    scale, lo_step, hi_step, inf, zero = c(step_scale), c(min_step), c(max_step), c(float("inf")), c(0.0)
    ok = torch.isfinite(rays).all(1) & ~(rays[:, 6] > t1)
    phase = torch.where(ok, 1, 0).to(torch.int32)
    t = rays[:, 6].clone()
    tlo, flo, thi, fhi = (torch.zeros(M, dtype=torch.float32, device=dev) for _ in range(4))
    count = torch.zeros(M, dtype=torch.int32, device=dev)
    evals = torch.zeros(M, dtype=torch.int32, device=dev)
    t_out = torch.full((M,), float("inf"), dtype=torch.float32, device=dev)
    status = torch.zeros(M, dtype=torch.int32, device=dev)
    bracket = torch.zeros((M, 4), dtype=torch.float32, device=dev)

    for _ in range(max_steps + refine_steps + 1):
        live = phase != 0
        if M == 0 or not bool(live.any()):
            break
        p = torch.where(live[:, None], o + t[:, None] * d, zero)
        f = sdf_of(p).reshape(M).to(torch.float32)
        evals = evals + live.to(torch.int32)
        march, refine, neg = phase == 1, phase == 2, f <= 0
        # MARCH, f <= 0: INSIDE on the first sample, else the bracket is there
        inside = march & neg & (evals == 1)
        found = march & neg & ~inside
        # MARCH, f > 0
        pos = march & ~neg
        tlo, flo = torch.where(pos, t, tlo), torch.where(pos, f, flo)
        ended = pos & (t == t1)
        count = count + (pos & ~ended).to(torch.int32)
        spent = pos & ~ended & (count == max_steps)
        step = scale * f
        step = torch.where(step > lo_step, step, lo_step)
        step = torch.where(step < hi_step, step, hi_step)
        tn = t + step
        tn = torch.where(tn < t1, tn, t1)
        # REFINE: the sample replaces an end
        hi_end, lo_end = found | (refine & neg), refine & ~neg
        thi, fhi = torch.where(hi_end, t, thi), torch.where(hi_end, f, fhi)
        tlo, flo = torch.where(lo_end, t, tlo), torch.where(lo_end, f, flo)
        count = torch.where(found, refine_steps, count - refine.to(torch.int32)).to(torch.int32)
        # the next midpoint, or the end of the refinement
        bisect = found | refine
        tm = 0.5 * (tlo + thi)
        final = bisect & ((count == 0) | (tm == tlo) | (tm == thi))
        hit_t = tlo + (thi - tlo) * (flo / (flo - fhi))
        hit_t = torch.where(hit_t > tlo, hit_t, tlo)
        hit_t = torch.where(hit_t < thi, hit_t, thi)
        # results of the rays that end here
        t_out = torch.where(inside | spent, t, torch.where(final, hit_t, t_out))        # (a MISS keeps +inf)
        status = torch.where(inside, INSIDE, torch.where(spent, EXHAUSTED, torch.where(final, HIT, status))).to(torch.int32)
        bracket = torch.where(final[:, None], torch.stack([tlo, thi, flo, fhi], 1), bracket)
        # where the others go
        t = torch.where(pos & ~ended & ~spent, tn, torch.where(bisect & ~final, tm, t))
        phase = torch.where(inside | ended | spent | final, 0, torch.where(found, 2, phase)).to(torch.int32)
    return {"t": t_out, "status": status, "bracket": bracket, "evals": evals}


def scale_intrinsics(cam_intr, sx, sy=None):
    """cam_intr ([3, 3], [3, 4] or with a leading batch axis of 1) for the same view at sx (sy) times the pixels per axis."""
    k = np.array(cam_intr, dtype=np.float64)
    shape = k.shape
    k = k.reshape(3, -1)
    k[0] *= sx
    k[1] *= sx if sy is None else sy
    return k.reshape(shape)


def _intrinsics(cam_intr):
    k = np.asarray(cam_intr.detach().cpu() if torch.is_tensor(cam_intr) else cam_intr, dtype=np.float64).reshape(3, -1)
    if k.shape[1] == 4:
        if np.any(k[:, 3] != 0):
            raise ValueError("camera_rays needs a camera whose projection is K [R = I | 0]: the fourth column of cam_intr is not zero")
        k = k[:, :3]
    if k.shape != (3, 3):
        raise ValueError("cam_intr must be 3 x 3 or 3 x 4")
    return k


def tile_order(H, W, tile=TILE):
    """(order [H W], inverse [H W]): order[k] is the flat pixel index (i * W + j) of ray k when the pixels are taken tile by tile (tiles of
    tile[0] columns x tile[1] rows, row-major inside a tile and over the tiles), inverse[pixel] the ray of a pixel: maps = per_ray[inverse]."""
    tw, th = int(tile[0]), int(tile[1])
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    key = (((i // th) * ((W + tw - 1) // tw) + (j // tw)) * th + (i % th)) * tw + (j % tw)
    order = np.argsort(key.reshape(-1), kind="stable").astype(np.int64)
    inverse = np.empty(H * W, dtype=np.int64)
    inverse[order] = np.arange(H * W)
    return order, inverse


def camera_rays(cam_intr, root_joint, scale_factor, H, W, box_lo, box_hi, tile=TILE):
    """One ray per pixel centre of an H x W view, in the decoder's normalised space, clipped to the box [box_lo, box_hi] (slab test).
    Returns {"origins" [M, 3], "dirs" [M, 3] (unit: t is a normalised length), "t0", "t1" [M] (t0 > t1: the ray misses the box, or
    the box is behind the camera), "order", "inverse" (tile_order), "z_per_t" [M]: camera-space z in metres per unit of t}, M = H W,
    numpy; origins / dirs / t0 / t1 are fp32 (computed in fp64), rays in tiles of `tile` pixels."""
    k = _intrinsics(cam_intr)
    root = np.asarray(root_joint.detach().cpu() if torch.is_tensor(root_joint) else root_joint, dtype=np.float64).reshape(-1)[:3]
    s = float(scale_factor)
    order, inverse = tile_order(H, W, tile)
    i, j = order // W, order % W
    pix = np.stack([j + 0.5, i + 0.5, np.ones(len(order))], 0)
    d_cam = np.linalg.solve(k, pix).T                           # K^-1 (u, v, 1)
    d = d_cam / np.linalg.norm(d_cam, axis=1, keepdims=True)    # (x = (x_cam - root) s / 2: a positive scale keeps directions)
    o = np.broadcast_to(-root * s / 2.0, d.shape).copy()        # the camera centre
    lo, hi = np.asarray(box_lo, np.float64).reshape(3), np.asarray(box_hi, np.float64).reshape(3)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d
    near, far = np.minimum(ta, tb), np.maximum(ta, tb)
    flat = d == 0                                               # parallel to a slab: inside it for every t, or never
    within = (o >= lo) & (o <= hi)
    near = np.where(flat, np.where(within, -np.inf, np.inf), near)
    far = np.where(flat, np.where(within, np.inf, -np.inf), far)
    t0, t1 = np.maximum(near.max(1), 0.0), far.min(1)
    miss = ~(t0 <= t1) | ~np.isfinite(t0) | ~np.isfinite(t1)
    t0, t1 = np.where(miss, 1.0, t0), np.where(miss, 0.0, t1)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"origins": f32(o), "dirs": f32(d), "t0": f32(t0), "t1": f32(t1), "order": order, "inverse": inverse,
            "z_per_t": f32(d[:, 2] * 2.0 / s)}


def render_view(evaluator, cam_intr, root_joint, scale_factor, H, W, box=((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), normals=True, **trace):
    """Depth, status, part and normal maps of the BOUND sample in the camera (cam_intr, root_joint): `evaluator` is a HipSdfDecoder or
    a TorchModuleDecoder (trace_rays, decode_points_grad), `box` = (lo, hi) the region that is marched, `trace` the parameters of
    trace_rays.  Returns device tensors: depth_hand / depth_obj [H, W] fp32 (camera-space z of the hit in metres, inf without a HIT),
    status_hand / status_obj [H, W] int32, part [H, W] uint8 (0 none, 1 hand, 2 object: the nearer hit), normal [H, W, 3] (unit
    gradient of the visible part's own head at its hit, zeros where nothing is hit; with normals=True), and evals_mean (evaluations per
    ray and head), exhausted_hand / exhausted_obj (ray counts) as 0-dim tensors."""
    from .utils.mesh import unit_normals
    cr = camera_rays(cam_intr, root_joint, scale_factor, H, W, box[0], box[1])
    dev = evaluator.device
    up = lambda a: torch.from_numpy(a).to(dev)
    o, d, zt, inverse = up(cr["origins"]), up(cr["dirs"]), up(cr["z_per_t"]), up(cr["inverse"])
    res = evaluator.trace_rays(o, d, up(cr["t0"]), up(cr["t1"]), hand=True, obj=True, want_evals=True, **trace)
    M = H * W
    out, t_of, evals = {}, {}, []
    for name in ("hand", "obj"):
        r = res.get(name)
        if r is None:                       # (an evaluator without this head)
            r = {"t": torch.full((M,), float("inf"), device=dev), "status": torch.zeros(M, dtype=torch.int32, device=dev)}
        else:
            evals.append(r["evals"].to(torch.float32).mean())
        hit = r["status"] == HIT
        t_of[name] = torch.where(hit, r["t"], torch.full_like(r["t"], float("inf")))
        out["depth_" + name] = torch.where(hit, r["t"] * zt, torch.full_like(r["t"], float("inf")))[inverse].reshape(H, W)
        out["status_" + name] = r["status"][inverse].reshape(H, W)
        out["exhausted_" + name] = (r["status"] == EXHAUSTED).sum()
    out["evals_mean"] = torch.stack(evals).mean() if evals else torch.zeros((), device=dev)
    th, to = t_of["hand"], t_of["obj"]
    part = torch.where(torch.isfinite(th) & (th <= to), 1, torch.where(torch.isfinite(to), 2, 0)).to(torch.uint8)
    out["part"] = part[inverse].reshape(H, W)
    if normals:
        # one list for both heads: every pixel's visible hit (the origin of the space where there is none), the gradient of its own head
        t_vis = torch.where(part == 1, th, to)
        pts = torch.where((part != 0)[:, None], o + torch.where(part != 0, t_vis, torch.zeros_like(t_vis))[:, None] * d, torch.zeros_like(o))
        g = evaluator.decode_points_grad(pts, hand=True, obj=True)
        gh = g[1] if g[1] is not None else torch.zeros_like(pts)
        go = g[3] if g[3] is not None else torch.zeros_like(pts)
        n = unit_normals(torch.where((part == 1)[:, None], gh, go))
        out["normal"] = torch.where((part != 0)[:, None], n, torch.zeros_like(n))[inverse].reshape(H, W, 3)
    return out


def view_evaluator(evaluator, module, specs):
    """The evaluator a view of this decoder is traced on: `evaluator` itself where it can trace - a HipSdfDecoder the kernel covers,
    or the module path - and otherwise (nerf9 / nerf15 / comb3: their sweeps are native, the tracing kernel refuses them) a
    TorchModuleDecoder over `module`, the product path of refused decoders.  NotImplementedError when there is no nn.Module to call."""
    refusal = getattr(evaluator, "trace_refusal", None)
    why = refusal() if callable(refusal) else None
    if why is None:
        return evaluator
    if not isinstance(module, torch.nn.Module):
        raise NotImplementedError("the ray-tracing kernel does not cover this decoder (%s) and there is no nn.Module to trace on the "
                                  "module path" % why)
    from .torch_decoder import TorchModuleDecoder
    return TorchModuleDecoder(module, specs, "ray tracing: " + why, evaluator.device)


VIEW_MAPS = ("depth_hand", "depth_obj", "status_hand", "status_obj", "part", "normal")
VIEW_STATS = ("evals_mean", "exhausted_hand", "exhausted_obj")


def save_view(path, view, H, W, trace):
    """<name>_render.npz: the maps of render_view (host arrays or tensors), H, W, the trace parameters and the three statistics."""
    host = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    data = {k: host(view[k]) for k in VIEW_MAPS + VIEW_STATS if k in view}
    data.update({"H": np.int32(H), "W": np.int32(W)})
    data.update({k: np.asarray(v) for k, v in trace.items()})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **data)


# ---- cameras of the reconstruct flows: camera_source(name, index) -> (cam_intr [3, 3] / [3, 4], root_joint [3])
def npz_camera_source(camera_dir):
    """<camera_dir>/<sample>.npz with `cam_intr` and `root_joint` (what the front end hands to pixel_alignment)."""
    def source(name, index):
        with np.load(os.path.join(camera_dir, name + ".npz")) as z:
            return np.asarray(z["cam_intr"], np.float64), np.asarray(z["root_joint"], np.float64).reshape(-1)[:3]
    return source


def synthetic_camera_source(H, W):
    """One fixed camera for synthetic runs: the wrist 0.6 m in front of it, the normalised cube about three quarters of the view."""
    def source(name, index):
        f = 1.6 * max(H, W)
        return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]]), np.array([0.0, 0.0, 0.6])
    return source


def parse_size(text):
    """"HxW" -> (H, W)."""
    try:
        h, w = (int(v) for v in str(text).lower().split("x"))
    except ValueError:
        raise ValueError("--render takes HxW, e.g. 128x128 (got %r)" % (text,))
    if h < 1 or w < 1:
        raise ValueError("--render takes positive sizes (got %r)" % (text,))
    return h, w
