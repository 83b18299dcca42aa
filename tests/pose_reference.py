"""The arithmetic of uh_pose_mesh ("Posed meshes") restated in numpy float32, vectorised over the vertices, every
operation in the written order and rounded on its own - numpy neither fuses nor reorders elementwise float32 operations, and its float32
sqrt and division are correctly rounded. The only definition the GPU tests compare k_pose against."""
import numpy as np

from rust_renderer_amd.types import VERTEX_DTYPE

f32 = np.float32


def normalize_or_keep(v):
    """per row of v (N, 3) float32: unchanged where dot(v, v) == 0, else v * (1 / sqrt(dot(v, v)))"""
    v = np.asarray(v, dtype=f32)
    d = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    zero = d == f32(0.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = f32(1.0) / np.sqrt(np.where(zero, f32(1.0), d))
    return np.where(zero[:, None], v, v * inv[:, None]).astype(f32)


def blend(joints, weights, joint_matrices):
    """m (N, 12): ((w0 A0 + w1 A1) + w2 A2) + w3 A3 per entry, A_k = joint_matrices[joints[:, k]]"""
    J = np.asarray(joint_matrices, dtype=f32).reshape(-1, 12)
    w = np.asarray(weights, dtype=f32)
    A = [J[np.asarray(joints)[:, k].astype(np.int64)] for k in range(4)]
    return ((w[:, 0:1] * A[0] + w[:, 1:2] * A[1]) + w[:, 2:3] * A[2]) + w[:, 3:4] * A[3]


def _rows3(m, v):
    return np.stack([(m[:, 4 * r] * v[:, 0] + m[:, 4 * r + 1] * v[:, 1]) + m[:, 4 * r + 2] * v[:, 2] for r in range(3)], axis=1)


def pose(bind, joints=None, weights=None, joint_matrices=None, position_deltas=None, normal_deltas=None, morph_weights=None):
    """the posed vertices (VERTEX_DTYPE) of bind pose `bind`: morph targets (position_deltas (T, N, 3), normal_deltas the same or None,
    morph_weights (T,)) if given, then the skin (joints (N, 4), weights (N, 4), joint_matrices (J, 12)) if given"""
    bind = np.ascontiguousarray(bind, dtype=VERTEX_DTYPE)
    out = bind.copy()  # pos.w, normal.w, uv, _pad, color, tangent.w: the bind record's bits
    p, n, t = bind["pos"][:, :3].copy(), bind["normal"][:, :3].copy(), bind["tangent"][:, :3].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        if position_deltas is not None:
            mw = np.asarray(morph_weights, dtype=f32).reshape(-1)
            dp = np.asarray(position_deltas, dtype=f32)
            dn = None if normal_deltas is None else np.asarray(normal_deltas, dtype=f32)
            assert dp.shape == (len(mw), len(bind), 3)
            for k in range(len(mw)):  # ascending; a weight of exactly zero is skipped
                if mw[k] == f32(0.0):
                    continue
                p = p + mw[k] * dp[k]
                if dn is not None:
                    n = n + mw[k] * dn[k]
        if joints is not None:
            m = blend(joints, weights, joint_matrices)
            p = _rows3(m, p) + m[:, 3::4]
            n = _rows3(m, n)
            t = normalize_or_keep(_rows3(m, t))
        n = normalize_or_keep(n)
    out["pos"][:, :3], out["normal"][:, :3], out["tangent"][:, :3] = p, n, t
    return out
