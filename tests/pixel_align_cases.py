"""Shared pieces of the PixelAlign tests (test_pixel_align_fold.py, test_gpu_pixel_align.py): an EDGE camera under which the
projection of chosen points is exact in fp32 and fp64 alike (so the inclusive -1 <= u, v <= 1 test decides the same way in both),
the points that probe it, and a numpy emulation of the native path's fold-then-gather arithmetic (csrc/sdf_mlp_kernel.h:
pixel_taps / pixel_prologue, csrc/decoder.hip: pixel_project_kernel)."""
import numpy as np

# cam_intr [1, 3, 4], root joint, SdfScaleFactor, ImageSize[0]: xyz_cam = xyz + (0, 0, 1); u = 2 x / z_cam, v = 2 y / z_cam exactly
EDGE_CAM = np.array([[[256.0, 0.0, 128.0, 0.0], [0.0, 256.0, 128.0, 0.0], [0.0, 0.0, 1.0, 0.0]]], np.float32)
EDGE_ROOT = np.array([0.0, 0.0, 1.0], np.float32)
EDGE_SCALE = 2.0
EDGE_IMAGE = 256


def edge_points(W=64, seed=0, H=None):
    """[M, 3] float32 normalised points under EDGE_CAM: inside the image, on the border taps of a map W wide and H high (H None: W;
    a size of 1 counts as 2), exactly at u / v = +-1, one fp32 step outside, at z_cam = 0 (0 / 0 and x / 0) and behind the camera
    (z_cam < 0, some of which project into the image)."""
    W = max(W, 2)
    H = W if H is None else max(H, 2)
    rng = np.random.default_rng(4400 + seed)
    f = np.float32
    eps = f(2.0 ** -20)
    pts = [rng.uniform(-0.45, 0.45, (64, 3)).astype(np.float32) * np.array([1, 1, 0.6], np.float32)]
    ys = np.array([-0.37, -0.1, 0.0, 0.23, 0.49], np.float32)
    for y in ys:
        pts.append(np.array([[-0.5, y, 0.0], [0.5, y, 0.0], [y, -0.5, 0.0], [y, 0.5, 0.0]], np.float32))             # u or v = +-1
        pts.append(np.array([[-0.5 - eps, y, 0.0], [0.5 + eps, y, 0.0], [y, -0.5 - eps, 0.0], [y, 0.5 + eps, 0.0]], np.float32))
    pts.append(np.array([[sx * 0.5, sy * 0.5, 0.0] for sx in (-1, 1) for sy in (-1, 1)], np.float32))               # corners
    # border taps: ix = (x + 0.5) (W - 1), iy = (y + 0.5) (H - 1) at z_cam = 1 - within one pixel (1.4: two) of either edge
    for t in (0.01, 0.3, 0.5, 0.99, 1.4):
        for sgn in (-1, 1):
            x, y = (f(sgn) * (f(0.5) - f(t / (n - 1))) for n in (W, H))
            pts.append(np.array([[x, 0.11, 0.0], [0.07, y, 0.0]], np.float32))
    pts.append(np.array([[0.0, 0.0, -1.0], [0.3, -0.2, -1.0], [0.0, 0.4, -1.0]], np.float32))                        # z_cam = 0
    pts.append(np.array([[0.2, 0.1, -1.5], [0.1, -0.05, -1.25], [0.9, 0.9, -1.5], [-0.3, 0.25, -1.2]], np.float32))   # behind
    return np.concatenate(pts, 0)


def project(xyz, cam, root, image_size, scale, dtype=np.float32):
    """uv [M, 2] and the in-image mask, op for op as utils/utils.py:538-553 (every operation rounded to `dtype`)."""
    t = lambda a: np.asarray(a, dtype)
    x = t(xyz)
    c = t(cam).reshape(3, 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        xc = x * t(2) / t(scale) + t(root).reshape(1, 3)
        h = [((c[i, 0] * xc[:, 0] + c[i, 1] * xc[:, 1]) + c[i, 2] * xc[:, 2]) + c[i, 3] for i in range(3)]
        uv = np.stack([h[0] / h[2], h[1] / h[2]], 1) / t(image_size) * t(2) - t(1)
    inside = (uv[:, 0] >= -1) & (uv[:, 0] <= 1) & (uv[:, 1] >= -1) & (uv[:, 1] <= 1)
    return uv, inside


def _cubic(tt):
    A = np.float32(-0.75)
    far = lambda x: ((A * x - np.float32(5) * A) * x + np.float32(8) * A) * x - np.float32(4) * A
    near = lambda x: ((A + np.float32(2)) * x - (A + np.float32(3))) * x * x + np.float32(1)
    return [far(tt + np.float32(1)), near(tt), near(np.float32(1) - tt), far(np.float32(2) - tt)]


def fold_gather(F, w_lat, b, xyz, cam, root, image_size, scale):
    """Layer-l pre-activations from the latent columns, the native way: P = W_lat . F per pixel, then per point b + sum over the 16
    bicubic taps (torch grid_sample: align_corners, zero padding, A = -0.75) of w_t P[:, tap] in the image, and the fold of the
    channel mean (F.mean(3).mean(2)) outside.  Projection, mask and tap weights in fp32 op for op; the sums in fp64.
    F [C, H, W], w_lat [R, C], b [R], xyz [M, 3] -> [M, R] float64."""
    C, H, W = F.shape
    P = w_lat.astype(np.float64) @ F.reshape(C, H * W).astype(np.float64)             # [R, H W]
    mean = F.astype(np.float64).mean(2).mean(1)
    out = np.empty((xyz.shape[0], w_lat.shape[0]), np.float64)
    out[:] = w_lat.astype(np.float64) @ mean + b
    uv, inside = project(xyz, cam, root, image_size, scale)
    f = np.float32
    for m in np.nonzero(inside)[0]:
        ix = (uv[m, 0] + f(1)) / f(2) * f(W - 1)
        iy = (uv[m, 1] + f(1)) / f(2) * f(H - 1)
        fx, fy = np.floor(ix), np.floor(iy)
        cx, cy = _cubic(ix - fx), _cubic(iy - fy)
        acc = np.zeros(w_lat.shape[0], np.float64)
        for i in range(4):
            yi = int(fy) - 1 + i
            for j in range(4):
                xj = int(fx) - 1 + j
                if 0 <= xj < W and 0 <= yi < H:
                    acc += float(cy[i] * cx[j]) * P[:, yi * W + xj]
        out[m] = b + acc
    return out, inside


# ---- cases of tests/test_gpu_pixel_align_fp64.py (their conditions are asserted on the CPU in tests/test_pixel_align_fold.py) ----------
# (H, W) of the feature maps: one pixel, one row, one column (W - 1 = 0 / H - 1 = 0), smaller than the 4 x 4 tap window, H != W both
# ways, H W not a multiple of the 64 pixels of a pixel_project_kernel block, the 256 x 256 limit and its one-column form
SIZES = ((1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (5, 3), (8, 8), (63, 17), (17, 63), (64, 64), (65, 64), (256, 256), (256, 1))

# a camera with a skew term, a non-zero fourth column and a third row that is not (0, 0, 1, 0); its root joint
SKEW_CAM = np.array([[[401.3, 3.7, 131.2, 2.1], [-0.9, 397.6, 124.9, -1.6], [0.002, -0.001, 1.0, 0.013]]], np.float32)
SKEW_ROOT = np.array([-0.021, 0.034, 0.61], np.float32)


def impulse(H, W, pixel, C=256):
    """[1, C, H, W]: zero but for `pixel` = (row, col), where channel c holds its own amplitude (both signs, 0.25 .. 1.25)."""
    F = np.zeros((1, C, H, W), np.float32)
    c = np.arange(C)
    F[0, :, pixel[0], pixel[1]] = ((0.25 + ((c * 37) % C) / C) * np.where(c % 3 == 0, -1.0, 1.0)).astype(np.float32)
    return F


def ramp(H, W, C=256, seed=0):
    """[1, C, H, W]: F[c] = a_c col + b_c row + d_c - linear in the pixel index.  Every tap of a point carries a value of its own
    that depends on its row and its column separately, and the sample changes by a known smooth amount from cell to cell except in
    the border cells, where the zero padding cuts taps off: the border handling stands out.  (Cubic convolution with A = -0.75 keeps
    constants, not slopes - unlike A = -0.5 - so the truth is grid_sample's value, not the ramp's.)"""
    rng = np.random.default_rng(5100 + seed)
    a, b, d = (rng.uniform(-1.0, 1.0, (C, 1, 1)) * s for s in (0.6 / max(W - 1, 1), 0.6 / max(H - 1, 1), 0.3))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (a * xx + b * yy + d).astype(np.float32)[None]


def signed_wide(H, W, C=256, seed=0):
    """[1, C, H, W]: independent values of both signs in every pixel, magnitudes log-uniform over 1e-3 .. 1e2 across the CHANNELS
    (a channel keeps its magnitude, within a factor 2, over the map): four channels of order 1e2, four of order 10, the others spread
    over 1e-3 .. 1 - with more large channels the decoder's outputs sit on tanh's plateaus, where an error in the latent is hard to see."""
    rng = np.random.default_rng(5200 + seed + 1000 * H + W)
    c = np.arange(C)
    expo = np.where(c % 64 == 63, 2.0, np.where(c % 64 == 31, 1.0, -3.0 + 3.0 * c / (C - 1)))
    mag = (10.0 ** expo).reshape(C, 1, 1) * rng.uniform(0.5, 1.0, (C, H, W))
    return (mag * rng.choice([-1.0, 1.0], (C, H, W))).astype(np.float32)[None]


def pixel_centre_points(H, W):
    """[H W + (H - 1)(W - 1), 3] float32 points under EDGE_CAM (z_cam = 1: u = 2 x, v = 2 y): one at the centre of every pixel
    (ix = col, iy = row: that pixel is a tap of weight ~1) and one at the centre of every quad of four pixels."""
    def axis(n, half):
        if n == 1:
            return np.zeros(0 if half else 1)
        k = np.arange(n - 1) + 0.5 if half else np.arange(n)
        return (k / (n - 1) - 0.5)                  # u = 2 k / (n - 1) - 1, x = u / 2
    out = []
    for half in (False, True):
        ys, xs = axis(H, half), axis(W, half)
        yy, xx = np.meshgrid(ys, xs, indexing="ij")
        out.append(np.stack([xx.reshape(-1), yy.reshape(-1), np.zeros(xx.size)], 1))
    return np.concatenate(out, 0).astype(np.float32)


def tap_weights(xyz, cam, root, image_size, scale, H, W):
    """For every point the (row, col) of its heaviest in-map tap and that tap's weight (fp32 op for op, as fold_gather); -1 and 0
    for a point outside the image."""
    uv, inside = project(xyz, cam, root, image_size, scale)
    f = np.float32
    with np.errstate(invalid="ignore"):
        ix = np.where(inside, (uv[:, 0] + f(1)) / f(2) * f(W - 1), f(0)).astype(f)
        iy = np.where(inside, (uv[:, 1] + f(1)) / f(2) * f(H - 1), f(0)).astype(f)
    fx, fy = np.floor(ix), np.floor(iy)
    cx, cy = np.stack(_cubic(ix - fx), 1), np.stack(_cubic(iy - fy), 1)            # [M, 4]
    xj = fx.astype(np.int64)[:, None] - 1 + np.arange(4)
    yi = fy.astype(np.int64)[:, None] - 1 + np.arange(4)
    w = (cy[:, :, None] * cx[:, None, :]).astype(np.float64)                         # [M, 4 rows, 4 cols], the fp32 products
    ok = ((yi >= 0) & (yi < H))[:, :, None] & ((xj >= 0) & (xj < W))[:, None, :] & inside[:, None, None]
    w = np.where(ok, w, 0.0).reshape(len(xyz), 16)
    k = w.argmax(1)
    m = np.arange(len(xyz))
    wbest = w[m, k]
    best = np.stack([yi[m, k // 4], xj[m, k % 4]], 1)
    best[wbest <= 0.0] = -1
    return best, wbest


def _solve_axis(cam, root, image_size, scale, axis, target, other, z):
    """fp64: the normalised coordinate on `axis` (0: x for u, 1: y for v) at which u (v) = target, the other in-plane coordinate and z
    given."""
    c = np.asarray(cam, np.float64).reshape(3, 4)
    r = np.asarray(root, np.float64)
    k = (target + 1.0) * image_size / 2.0
    oc = other * 2.0 / scale + r[1 - axis]
    zc = z * 2.0 / scale + r[2]
    row = c[axis] - k * c[2]                         # row . (xc, yc, zc, 1) = 0
    ac = -(row[1 - axis] * oc + row[2] * zc + row[3]) / row[axis]
    return (ac - r[axis]) * scale / 2.0


def border_points(cam, root, image_size, scale, n, seed=0):
    """fp32 points whose neighbours in fp32 straddle the image border under an INEXACT camera: for each of the four borders
    (u = 1, u = -1, v = 1, v = -1) n pairs of ADJACENT floats on one coordinate, found by bisection on the fp32 op-for-op mask of
    `project` - the last point inside and the first outside - and, where one of the eight floats below the flip has it, a point
    whose u (v) is exactly +-1.  Returns (points [M, 3] float32, kind [M]: 0 last inside, 1 first outside, 2 exactly on the border)."""
    rng = np.random.default_rng(6100 + seed)
    f = np.float32
    pts, kind = [], []
    inside = lambda p: bool(project(p.reshape(1, 3), cam, root, image_size, scale)[1][0])
    for axis, sign in ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0)):
        found = 0
        while found < n:
            z = rng.uniform(-0.6, 0.6)
            other_uv = rng.uniform(-0.7, 0.7)
            # the other coordinate such that its own uv is about other_uv at the crossing (one fixed-point step is plenty)
            other = _solve_axis(cam, root, image_size, scale, 1 - axis, other_uv, 0.0, z)
            a_in = _solve_axis(cam, root, image_size, scale, axis, sign * 0.9, other, z)
            a_out = _solve_axis(cam, root, image_size, scale, axis, sign * 1.1, other, z)
            p = np.zeros(3, f)
            p[1 - axis], p[2] = other, z
            lo, hi = p.copy(), p.copy()
            lo[axis], hi[axis] = a_in, a_out
            if not inside(lo) or inside(hi):
                continue
            while np.nextafter(lo[axis], hi[axis]) != hi[axis]:
                mid = lo.copy()
                mid[axis] = f((np.float64(lo[axis]) + np.float64(hi[axis])) / 2)
                if inside(mid):
                    lo = mid
                else:
                    hi = mid
            pts += [lo.copy(), hi.copy()]
            kind += [0, 1]
            q = lo.copy()
            for _ in range(8):
                uv = project(q.reshape(1, 3), cam, root, image_size, scale)[0][0]
                if uv[axis] == f(sign):
                    pts.append(q.copy())
                    kind.append(2)
                    break
                q[axis] = np.nextafter(q[axis], lo[axis] - (hi[axis] - lo[axis]) * f(1e6))
            found += 1
    return np.stack(pts).astype(f), np.array(kind)


def impulse_probe_points(H, W, pixel):
    """[256, 3] points under EDGE_CAM at quarter-pixel spacing over the 4 x 4-pixel neighbourhood of `pixel` (ix from col - 2 to
    col + 1.75), kept inside the image: every tap position of the pixel, at every sub-pixel phase."""
    k = np.arange(16) * 0.25 - 2.0
    ix = np.clip(pixel[1] + k, 0.0, W - 1.0)
    iy = np.clip(pixel[0] + k, 0.0, H - 1.0)
    yy, xx = np.meshgrid(iy / (H - 1) - 0.5, ix / (W - 1) - 0.5, indexing="ij")
    return np.stack([xx.reshape(-1), yy.reshape(-1), np.zeros(256)], 1).astype(np.float32)
