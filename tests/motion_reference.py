"""The motion texel of UH_HYBRID_MOTION restated in float64, from DESIGN.md section 2 "Motion vectors". Not a test module:
test_motion_cpu.py holds it to known answers on hand-made triangles, test_gpu_motion.py holds the device to it."""
import numpy as np

STATIC, RIGID, DEFORMED, NONE = range(4)


def affine(m3x4, p):
    """m (p, 1) for a row-major 3x4 (12 values) and points (..., 3), float64"""
    m = np.asarray(m3x4, np.float64).reshape(3, 4)
    return np.asarray(p, np.float64) @ m[:, :3].T + m[:, 3]


def inverse3x4(m3x4):
    """the inverse affine map as a row-major 3x4, float64"""
    m = np.asarray(m3x4, np.float64).reshape(3, 4)
    inv = np.linalg.inv(m[:, :3])
    return np.concatenate([inv, (-inv @ m[:, 3])[:, None]], axis=1)


def motion_texel(state, position, corners, bary, prev_o2w):
    """(xyz, w) of one pixel or of N pixels at once. position (..., 3): the position texel's xyz. corners (..., 3, 3): the triangle's
    object-space corners q0, q1, q2 - the PREVIOUS ones for a deformed mesh, the current ones for a rigid one. bary (..., 3): b0 = 1 -
    u - v, b1 = u, b2 = v. prev_o2w: the previous object-to-world 3x4. static and none return the position itself."""
    position = np.asarray(position, np.float64)
    if state == STATIC:
        return position.copy(), 1.0
    if state == NONE:
        return position.copy(), 0.0
    q, b = np.asarray(corners, np.float64), np.asarray(bary, np.float64)
    o = (q[..., 0, :] * b[..., 0:1] + q[..., 1, :] * b[..., 1:2]) + q[..., 2, :] * b[..., 2:3]
    return affine(prev_o2w, o), 1.0


def locate(points, world_corners):
    """for every point (N, 3), the triangle among world_corners (T, 3, 3) it lies on and its barycentrics there, float64: the triangle
    whose plane is nearest among those that contain the point's projection (smallest violation of b >= 0 otherwise). Returns (triangle
    (N,), bary (N, 3), distance (N,))."""
    p = np.asarray(points, np.float64)[:, None, :]
    t = np.asarray(world_corners, np.float64)[None]
    e1, e2 = t[:, :, 1] - t[:, :, 0], t[:, :, 2] - t[:, :, 0]
    n = np.cross(e1, e2)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    d = p - t[:, :, 0]
    dist = np.abs((d * n).sum(-1))
    d11, d12, d22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    p1, p2 = (d * e1).sum(-1), (d * e2).sum(-1)
    det = d11 * d22 - d12 * d12
    u, v = (d22 * p1 - d12 * p2) / det, (d11 * p2 - d12 * p1) / det
    b = np.stack([1.0 - u - v, u, v], axis=-1)
    outside = np.maximum(-b.min(axis=-1), 0.0)
    scale = np.sqrt(np.maximum(d11, d22))
    score = dist + outside * scale
    tri = score.argmin(axis=1)
    k = np.arange(len(tri))
    return tri, b[k, tri], score[k, tri]
