"""CPU: tests/motion_reference.py, the float64 restatement of the motion texel, on hand-made triangles: for an affine map applied to all
vertices it returns A_prev A_cur^-1 position, because barycentric interpolation commutes with affine maps."""
import numpy as np
import pytest

import motion_reference as mr

TRI = np.array([[0.25, -1.0, 2.0], [3.0, 0.5, 1.5], [-1.0, 2.0, -0.75]])
BARY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.2, 0.3, 0.5], [1 / 3, 1 / 3, 1 / 3], [0.9, 0.05, 0.05]])


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def map3x4(scale, angles, t):
    return np.concatenate([rot(*angles) * np.asarray(scale)[None, :], np.asarray(t, np.float64)[:, None]], axis=1)


A_PREV = map3x4((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
A_CUR = map3x4((1.3, 0.7, 1.1), (0.2, -0.4, 0.9), (0.5, -2.0, 3.0))
A_OTHER = map3x4((0.6, 1.9, 1.0), (-1.1, 0.3, 0.2), (-4.0, 1.0, 0.25))
IDENTITY = map3x4((1, 1, 1), (0, 0, 0), (0, 0, 0))


def known(a_prev, a_cur, pos):
    return mr.affine(a_prev, mr.affine(mr.inverse3x4(a_cur), pos))


@pytest.mark.parametrize("a_prev,a_cur", [(A_PREV, A_CUR), (A_CUR, A_OTHER), (A_OTHER, A_OTHER)])
def test_rigid_is_prev_times_inverse_current(a_prev, a_cur):
    pos = (mr.affine(a_cur, TRI)[None] * BARY[:, :, None]).sum(axis=1)
    xyz, w = mr.motion_texel(mr.RIGID, pos, np.broadcast_to(TRI, (len(BARY), 3, 3)), BARY, a_prev)
    assert w == 1.0
    assert np.abs(xyz - known(a_prev, a_cur, pos)).max() <= 64 * np.finfo(np.float64).eps * np.abs(pos).max()


@pytest.mark.parametrize("a_prev,a_cur", [(A_PREV, A_CUR), (A_CUR, A_OTHER)])
def test_deformed_under_an_affine_map_of_all_vertices_is_the_same_answer(a_prev, a_cur):
    prev_v, cur_v = mr.affine(a_prev, TRI), mr.affine(a_cur, TRI)  # the vertices themselves move; the instance transform is the identity
    pos = (cur_v[None] * BARY[:, :, None]).sum(axis=1)
    xyz, w = mr.motion_texel(mr.DEFORMED, pos, np.broadcast_to(prev_v, (len(BARY), 3, 3)), BARY, IDENTITY)
    assert w == 1.0
    assert np.abs(xyz - known(a_prev, a_cur, pos)).max() <= 64 * np.finfo(np.float64).eps * np.abs(pos).max()
    # a deformation and a transform change in the same interval: the previous transform carries the previous vertices
    xyz2, _ = mr.motion_texel(mr.DEFORMED, pos, np.broadcast_to(prev_v, (len(BARY), 3, 3)), BARY, A_OTHER)
    assert np.abs(xyz2 - mr.affine(A_OTHER, xyz)).max() <= 64 * np.finfo(np.float64).eps * np.abs(xyz2).max()


def test_static_and_none_return_the_position():
    pos = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.0]])
    xyz, w = mr.motion_texel(mr.STATIC, pos, None, None, None)
    assert np.array_equal(xyz, pos) and w == 1.0
    xyz, w = mr.motion_texel(mr.NONE, pos, None, None, None)
    assert np.array_equal(xyz, pos) and w == 0.0


def test_corners_return_the_corners_and_locate_finds_the_triangle():
    xyz, _ = mr.motion_texel(mr.DEFORMED, TRI, np.broadcast_to(TRI, (3, 3, 3)), np.eye(3), A_CUR)
    assert np.abs(xyz - mr.affine(A_CUR, TRI)).max() <= 16 * np.finfo(np.float64).eps * np.abs(xyz).max()
    tris = np.stack([TRI, TRI + np.array([10.0, 0.0, 0.0]), TRI[::-1] + np.array([0.0, 0.0, 5.0])])
    pts = np.concatenate([(tris[k][None] * BARY[3:, :, None]).sum(axis=1) for k in range(3)])
    tri, b, dist = mr.locate(pts, tris)
    assert list(tri) == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert np.abs(b - np.tile(BARY[3:], (3, 1))).max() <= 1e-12 and dist.max() <= 1e-12
