"""Camera matrices with glam 0.20.5 semantics (the reference's utopian/src/camera.rs:90-107).

All arithmetic is float32. Matrices are returned column-major flattened (glam::Mat4 memory
order, the order ViewUniformData stores them in).
"""
import numpy as np

f32 = np.float32


def _normalize(v):
    v = np.asarray(v, dtype=f32)
    return (v / np.sqrt(np.dot(v, v), dtype=f32)).astype(f32)


def look_at_rh(eye, center, up):
    """glam Mat4::look_at_rh(eye, center, up) = look_to_rh(eye, center - eye, up)."""
    eye = np.asarray(eye, dtype=f32)
    f = _normalize(np.asarray(center, dtype=f32) - eye)
    s = _normalize(np.cross(f, np.asarray(up, dtype=f32)).astype(f32))
    u = np.cross(s, f).astype(f32)
    m = np.zeros((4, 4), dtype=f32)  # m[row, col]
    m[0, 0:3] = s
    m[1, 0:3] = u
    m[2, 0:3] = -f
    m[0, 3] = -np.dot(s, eye)
    m[1, 3] = -np.dot(u, eye)
    m[2, 3] = np.dot(f, eye)
    m[3, 3] = 1
    return m


def perspective_rh(fov_y_radians, aspect, z_near, z_far):
    """glam Mat4::perspective_rh: right-handed, depth 0..1, y up (no Vulkan y flip)."""
    fov = f32(fov_y_radians)
    sin_fov, cos_fov = np.sin(f32(0.5) * fov, dtype=f32), np.cos(f32(0.5) * fov, dtype=f32)
    h = f32(cos_fov / sin_fov)
    w = f32(h / f32(aspect))
    r = f32(f32(z_far) / (f32(z_near) - f32(z_far)))
    m = np.zeros((4, 4), dtype=f32)
    m[0, 0] = w
    m[1, 1] = h
    m[2, 2] = r
    m[3, 2] = -1
    m[2, 3] = r * f32(z_near)
    return m


def inverse(m):
    return np.linalg.inv(m.astype(np.float64)).astype(f32)


def jitter_projection(projection, jx, jy, width, height):
    """(projection', inverse(projection')), both 16 floats column-major: the perspective projection (16 floats column-major) whose image
    of every point is moved by (jx, jy) pixels in G-buffer pixel coordinates (x right, y down) of a width x height frame.
    A point's pixel is ((ndc.x * 0.5 + 0.5) * width, (1 - (ndc.y * 0.5 + 0.5)) * height) and ndc = clip.xy / clip.w with clip.w = -z
    (row 3 of perspective_rh is (0, 0, -1, 0)), so adding d to element 8 (row 0, column 2: the factor of z in clip.x) moves ndc.x by
    d z / -z = -d: jx pixels are d = -2 jx / width; y points down, so jy pixels are +2 jy / height on element 9. (0, 0) returns the
    input's bits."""
    p = np.array(projection, dtype=f32).reshape(16).copy()
    p[8] = p[8] + f32(-2.0) * f32(jx) / f32(width)
    p[9] = p[9] + f32(2.0) * f32(jy) / f32(height)
    return p, to_glam(inverse(p.reshape(4, 4).T))


def jitter_clip(matrix, jx, jy, width, height):
    """16 floats column-major: J * matrix, where J moves clip.xy by (-2 jx / width, +2 jy / height) * -clip.w - what jitter_projection does
    to a perspective projection, applied to any matrix that ends in one (a projection * view product: the previous frame's, which a
    jittered frame reprojects through with ITS OWN jitter, so that a camera at rest lands on its own texel)"""
    m = np.array(matrix, dtype=f32).reshape(16).copy()
    dx, dy = f32(-2.0) * f32(jx) / f32(width), f32(2.0) * f32(jy) / f32(height)
    for c in range(4):
        m[4 * c] = m[4 * c] - dx * m[4 * c + 3]
        m[4 * c + 1] = m[4 * c + 1] - dy * m[4 * c + 3]
    return m


def to_glam(m):
    """row/col matrix -> 16 floats column-major."""
    return np.ascontiguousarray(m.T, dtype=f32).reshape(16)


class Camera:
    """utopian::Camera (camera.rs) reduced to what the path needs: the two matrices + position."""

    def __init__(self, position, target, fov_degrees=60.0, aspect_ratio=16.0 / 9.0, z_near=0.01, z_far=1000.0):
        self.position = np.asarray(position, dtype=f32)
        self.target = np.asarray(target, dtype=f32)
        self.fov_degrees, self.aspect_ratio, self.z_near, self.z_far = fov_degrees, aspect_ratio, z_near, z_far

    def get_view(self):
        return look_at_rh(self.position, self.target, (0.0, 1.0, 0.0))

    def get_projection(self):
        return perspective_rh(np.radians(f32(self.fov_degrees), dtype=f32), self.aspect_ratio, self.z_near, self.z_far)

    def get_position(self):
        return self.position
