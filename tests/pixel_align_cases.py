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


def edge_points(W=64, seed=0):
    """[M, 3] float32 normalised points under EDGE_CAM: inside the image, on the border taps, exactly at u / v = +-1, one fp32 step
    outside, at z_cam = 0 (0 / 0 and x / 0) and behind the camera (z_cam < 0, some of which project into the image)."""
    rng = np.random.default_rng(4400 + seed)
    f = np.float32
    eps = f(2.0 ** -20)
    pts = [rng.uniform(-0.45, 0.45, (64, 3)).astype(np.float32) * np.array([1, 1, 0.6], np.float32)]
    ys = np.array([-0.37, -0.1, 0.0, 0.23, 0.49], np.float32)
    for y in ys:
        pts.append(np.array([[-0.5, y, 0.0], [0.5, y, 0.0], [y, -0.5, 0.0], [y, 0.5, 0.0]], np.float32))             # u or v = +-1
        pts.append(np.array([[-0.5 - eps, y, 0.0], [0.5 + eps, y, 0.0], [y, -0.5 - eps, 0.0], [y, 0.5 + eps, 0.0]], np.float32))
    pts.append(np.array([[sx * 0.5, sy * 0.5, 0.0] for sx in (-1, 1) for sy in (-1, 1)], np.float32))               # corners
    # border taps: ix = (x + 0.5) (W - 1) at z_cam = 1 - within one pixel of either edge
    for t in (0.01, 0.3, 0.5, 0.99, 1.4):
        for x in (f(t / (W - 1)) - f(0.5), f(0.5) - f(t / (W - 1))):
            pts.append(np.array([[x, 0.11, 0.0], [0.07, x, 0.0]], np.float32))
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
