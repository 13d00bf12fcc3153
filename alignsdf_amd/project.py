"""Newton projection of points onto the zero level of an SDF head.

A marching-cubes vertex sits where a LINEAR interpolation along a lattice edge crosses zero, not where the decoder's field does.  A few
steps x <- x - f grad f / |grad f|^2 move it onto the level set: HipSdfDecoder.project_points (one kernel: csrc/k1p_kernels.hip) or,
for decoders that kernel does not cover, TorchModuleDecoder.project_points (the same rule in torch, all points in lockstep:
project_lockstep below).  The rule is worded in include/alignsdf_hip.h (asdf_project_points).
"""
import numpy as np
import torch

CONVERGED, SPENT, STALLED, BAD = 0, 1, 2, 3        # ASDF_PROJECT_*
STATUS_NAMES = ("converged", "spent", "stalled", "bad")

PROJECT_DEFAULTS = {"max_iters": 8, "tol": 1e-6, "min_grad2": 1e-12}
OUTPUTS = ("xyz_out", "sdf", "grad", "sdf_in", "status", "evals")


def check_rule(max_iters, tol, max_move, min_grad2):
    if max_iters < 0 or not tol >= 0 or not max_move > 0 or not min_grad2 > 0:
        raise ValueError("max_iters >= 0, tol >= 0, max_move > 0 and min_grad2 > 0 are required")


def project_lockstep(grad_of, points, max_iters=8, tol=1e-6, max_move=1.0, min_grad2=1e-12):
    """The rule of asdf_project_points (include/alignsdf_hip.h) in torch fp32 for ONE head: every point takes its next evaluation in
    the same call of `grad_of(points [M, 3]) -> (sdf [M], grad [M, 3])`, finished points ride along frozen under masks (non-finite ones
    feed the origin of the space), and the loop ends when no point is live - one host read per step.  Returns {"xyz_out", "sdf",
    "grad", "sdf_in", "status", "evals"} on points' device.  Every operation is one rounded fp32 torch op, so on equal evaluation bits
    the results are the kernel's bit for bit."""
    check_rule(max_iters, tol, max_move, min_grad2)
    x0 = points.detach().to(torch.float32).reshape(-1, 3)
    dev, M = x0.device, x0.shape[0]
    c = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    tol_, move, floor, zero = c(tol), c(max_move), c(min_grad2), c(0.0)
    lo, hi = x0 - move, x0 + move
    ok = torch.isfinite(x0).all(1)
    live = ok.clone()
    x = x0.clone()
    sdf = torch.zeros(M, dtype=torch.float32, device=dev)
    grad = torch.zeros((M, 3), dtype=torch.float32, device=dev)
    sdf_in = torch.zeros(M, dtype=torch.float32, device=dev)
    status = torch.where(ok, SPENT, BAD).to(torch.int32)
    evals = torch.zeros(M, dtype=torch.int32, device=dev)

    for step in range(max_iters + 1):
        if M == 0 or not bool(live.any()):
            break
        f, g = grad_of(torch.where(ok[:, None], x, zero))
        f, g = f.reshape(M).to(torch.float32), g.reshape(M, 3).to(torch.float32)
        evals = evals + live.to(torch.int32)
        if step == 0:
            sdf_in = torch.where(live, f, sdf_in)
        sdf, grad = torch.where(live, f, sdf), torch.where(live[:, None], g, grad)
        # decide
        sq = g * g
        n2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
        converged = live & (f.abs() <= tol_)
        stalled = live & ~converged & ~(n2 >= floor)
        spent = live & ~converged & ~stalled & (step == max_iters)
        status = torch.where(converged, CONVERGED, torch.where(stalled, STALLED, torch.where(spent, SPENT, status))).to(torch.int32)
        live = live & ~converged & ~stalled & ~spent
        # step
        s = f / n2
        sg = s[:, None] * g
        v = x - sg
        v = torch.where(v > lo, v, lo)
        v = torch.where(v < hi, v, hi)
        x = torch.where(live[:, None], v, x)
    return {"xyz_out": x, "sdf": sdf, "grad": grad, "sdf_in": sdf_in, "status": status, "evals": evals}


def head_index(head):
    """0 / 1 for 0, 1, "hand", "obj"."""
    if head in (0, "hand"):
        return 0
    if head in (1, "obj"):
        return 1
    raise ValueError("head: 0 / \"hand\" or 1 / \"obj\", not %r" % (head,))


def grad_of_head(evaluator, head):
    """points -> (sdf, grad) of one head of a BOUND evaluator with decode_points_grad."""
    h = head_index(head)

    def grad_of(points):
        res = evaluator.decode_points_grad(points, hand=h == 0, obj=h == 1)
        sdf, grad = (res[0], res[1]) if h == 0 else (res[2], res[3])
        if sdf is None:
            raise ValueError("the evaluator has no %s head to project on" % ("hand", "obj")[h])
        return sdf, grad
    return grad_of


def count_record(counts):
    """The five counts of polish_vertices (host array or tensor) as the `polish_<part>` entry of a record: vertices by status, and
    `kept` = how many stayed at their marching-cubes position."""
    c = np.asarray(counts.detach().cpu() if torch.is_tensor(counts) else counts).reshape(-1)
    return dict({name: int(c[k]) for k, name in enumerate(STATUS_NAMES)}, kept=int(c[4]))


def project_refusal_of(evaluator):
    """Why (a string) this evaluator cannot project points, or None: the native kernel covers SeparateDecoder with point features
    affine in xyz (hip_decoder.project_refusal); the module path projects on whatever it differentiates."""
    if not hasattr(evaluator, "project_points"):
        return "%s has no project_points" % type(evaluator).__name__
    refusal = getattr(evaluator, "project_refusal", None)
    return refusal() if callable(refusal) else None


def require_polish(evaluator):
    """Raise before anything is swept or written when `evaluator` cannot project the vertices `polish` moves."""
    why = project_refusal_of(evaluator)
    if why is not None:
        raise NotImplementedError("polish needs the projection onto the zero level, which the native kernel does not cover here: %s" % why)


def polish_vertices(evaluator, verts, origin, voxel_size, part, count=None):
    """Marching-cubes vertices `verts` [V, 3] (lattice units, device) of surface `part` ("hand" / "obj") -> (the vertices on the zero
    level of the part's own head of the BOUND evaluator [V, 3] in lattice units, counts): projected with PROJECT_DEFAULTS and a trust
    box of one voxel per axis; a vertex keeps its marching-cubes position where the status is BAD or STALLED or |sdf| > |sdf_in|.
    `count` (a device scalar, optional): only the first `count` rows hold vertices - the others are projected along and not counted.
    counts = int64 [5] on the device (see count_record).  Nothing here waits for the stream."""
    from .utils.mesh import lattice_points
    voxel_size = float(voxel_size)
    res = evaluator.project_points(lattice_points(verts, origin, voxel_size), part, max_move=voxel_size, **PROJECT_DEFAULTS)
    status = res["status"]
    keep = (status == BAD) | (status == STALLED) | ~(res["sdf"].abs() <= res["sdf_in"].abs())
    moved = res["xyz_out"].clone()
    for a in range(3):
        moved[:, a] -= float(origin[a])
    moved /= voxel_size
    out = torch.where(keep[:, None], verts, moved.to(verts.dtype))
    rows = torch.ones_like(keep) if count is None else torch.arange(verts.shape[0], device=verts.device) < count
    counts = torch.stack([((status == code) & rows).sum() for code in range(4)] + [(keep & rows).sum()])
    return out, counts


class VertexPolish:
    """(verts [V, 3] in lattice units on the device, origin, voxel_size) -> the polished vertices of one surface (polish_vertices on head
    `part` of the BOUND evaluator).  `counts` is count_record of the last call."""

    def __init__(self, evaluator, part):
        require_polish(evaluator)
        self.evaluator, self.part, self.counts = evaluator, part, None

    def __call__(self, verts, origin, voxel_size):
        out, counts = polish_vertices(self.evaluator, verts, origin, voxel_size, self.part)
        self.counts = count_record(counts)
        return out
