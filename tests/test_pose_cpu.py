"""CPU: tests/pose_reference.py - the float32 restatement of DESIGN.md section 2 "Posed meshes" that the GPU tests hold k_pose to - against a
float64 evaluation of the same formulas, and its stated rules: targets of weight zero are skipped, a zero vector is not normalised, the
fields a pose does not compute are the bind record's bits.

The bound, per position component: |f32 - f64| <= 1.01 (T + 10) 2^-24 S, S the sum of the absolute values of every term of the fully
expanded expression  sum_k w_k A_k[r][c] (b_c + sum_t mw_t dp_t,c) + sum_k w_k A_k[r][3].  No term passes through more than T + 10
roundings: T morph sums and its product; the product w_k A_k and three sums of the blend; the product with p and three sums of the
row - 1 + T + 4 + 4 = T + 9, and one to spare; each rounding is at most 2^-24 relative, the 1.01 covers the second-order terms."""
import numpy as np
import pytest

import pose_reference as ref
from rust_renderer_amd.types import VERTEX_DTYPE

N, NJ = 500, 9


def inputs(seed, T, skin):
    rng = np.random.default_rng(seed)
    bind = np.zeros(N, dtype=VERTEX_DTYPE)
    for field in VERTEX_DTYPE.names:
        bind[field] = rng.uniform(-3.0, 3.0, bind[field].shape).astype(np.float32)
    kw = {}
    if T:
        kw.update(position_deltas=rng.uniform(-1, 1, (T, N, 3)).astype(np.float32), normal_deltas=rng.uniform(-1, 1, (T, N, 3)).astype(np.float32),
                  morph_weights=rng.uniform(-1.5, 1.5, T).astype(np.float32))
    if skin:
        w = rng.uniform(0, 1, (N, 4)).astype(np.float32)
        w[rng.uniform(size=(N, 4)) < 0.25] = 0.0
        w[:, 0] += np.float32(0.05)
        mats = (np.tile(np.eye(3, 4), (NJ, 1, 1)) + rng.uniform(-1, 1, (NJ, 3, 4))).astype(np.float32)
        mats[1, :, :3] = np.diag([-1, 1, 1])
        mats[2, :, :3] = np.eye(3) * 1e-3
        kw.update(joints=rng.integers(0, NJ, (N, 4)).astype(np.uint16), weights=w, joint_matrices=mats.reshape(NJ, 12))
    return bind, kw


def position_f64(bind, joints=None, weights=None, joint_matrices=None, position_deltas=None, normal_deltas=None, morph_weights=None):
    """(positions, S) in float64 from the float32 inputs"""
    p = bind["pos"][:, :3].astype(np.float64)
    s = np.abs(p)
    if position_deltas is not None:
        terms = morph_weights.astype(np.float64)[:, None, None] * position_deltas.astype(np.float64)
        p, s = p + terms.sum(axis=0), s + np.abs(terms).sum(axis=0)
    if joints is None:
        return p, s
    A = joint_matrices.astype(np.float64).reshape(-1, 3, 4)[joints.astype(np.int64)]  # (N, 4, 3, 4)
    wA = weights.astype(np.float64)[:, :, None, None] * A
    m, am = wA.sum(axis=1), np.abs(wA).sum(axis=1)
    return np.einsum("nrc,nc->nr", m[:, :, :3], p) + m[:, :, 3], np.einsum("nrc,nc->nr", am[:, :, :3], s) + am[:, :, 3]


@pytest.mark.parametrize("skin", [False, True], ids=["morph", "skin"])
@pytest.mark.parametrize("T", [0, 1, 5])
def test_positions_are_within_the_rounding_bound_of_float64(T, skin):
    worst = 0.0
    for seed in range(4):
        bind, kw = inputs(10 * T + seed, T, skin)
        got = ref.pose(bind, **kw)["pos"][:, :3].astype(np.float64)
        want, S = position_f64(bind, **kw)
        bound = 1.01 * (T + 10) * 2.0 ** -24 * S
        worst = max(worst, float((np.abs(got - want) / bound).max()))
        assert (np.abs(got - want) <= bound).all()
    print(f"T {T}, skin {skin}: worst |f32 - f64| / bound = {worst:.3f}")
    assert worst > 0.0 or (T == 0 and not skin), "the float32 path rounds somewhere"


@pytest.mark.parametrize("skin", [False, True], ids=["morph", "skin"])
def test_normals_and_tangents_are_unit_and_close_to_float64(skin):
    bind, kw = inputs(77, 5, skin)
    out = ref.pose(bind, **kw)
    n = bind["normal"][:, :3].astype(np.float64) + (kw["morph_weights"].astype(np.float64)[:, None, None] * kw["normal_deltas"].astype(np.float64)).sum(axis=0)
    t = bind["tangent"][:, :3].astype(np.float64)
    if skin:
        A = kw["joint_matrices"].astype(np.float64).reshape(-1, 3, 4)[kw["joints"].astype(np.int64)]
        m = (kw["weights"].astype(np.float64)[:, :, None, None] * A).sum(axis=1)[:, :, :3]
        n, t = np.einsum("nrc,nc->nr", m, n), np.einsum("nrc,nc->nr", m, t)
        t = t / np.linalg.norm(t, axis=1, keepdims=True)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    # directions, not a rounding analysis: cancellation in a blended row can cost several digits
    assert np.abs(out["normal"][:, :3] - n).max() < 1e-3 and np.abs(out["tangent"][:, :3] - t).max() < 1e-3
    assert np.abs(np.linalg.norm(out["normal"][:, :3].astype(np.float64), axis=1) - 1).max() < 1e-6
    if not skin:
        assert out["tangent"].tobytes() == bind["tangent"].tobytes(), "without a skin the tangent stays verbatim"


def test_a_target_of_weight_zero_is_skipped_not_added():
    bind, kw = inputs(3, 5, True)
    kw["morph_weights"][[1, 3]] = 0.0
    bind["pos"][::2, 0] = np.float32(-0.0)  # -0 + 0 * d would be +0: only a skipped target leaves the sign
    bind["normal"][::2, 1] = np.float32(-0.0)
    keep = [0, 2, 4]
    less = dict(kw, position_deltas=kw["position_deltas"][keep], normal_deltas=kw["normal_deltas"][keep], morph_weights=kw["morph_weights"][keep])
    assert ref.pose(bind, **kw).tobytes() == ref.pose(bind, **less).tobytes()
    morph_only = {k: v for k, v in kw.items() if k in ("position_deltas", "normal_deltas")}
    out = ref.pose(bind, morph_weights=np.zeros(5, np.float32), **morph_only)
    assert out["pos"].tobytes() == bind["pos"].tobytes() and np.signbit(out["pos"][::2, 0]).all(), "every target skipped: the bind position's bits"
    # and the skip is by value: -0.0 == 0.0 is skipped too
    out = ref.pose(bind, morph_weights=np.float32([-0.0] * 5), **morph_only)
    assert out["pos"].tobytes() == bind["pos"].tobytes()


def test_normalize_or_keep_on_a_zero_vector_and_a_singular_blend():
    v = np.float32([[0, 0, 0], [-0.0, 0, 0], [3, 0, 4], [1e-30, 0, 0]])
    out = ref.normalize_or_keep(v)
    assert out[:2].tobytes() == v[:2].tobytes() and np.array_equal(out[2], np.float32([0.6, 0, 0.8]))
    assert out[3].tobytes() == v[3].tobytes(), "its square, 1e-60, is zero in float32: kept, as on the device"
    # two joints that mirror each other in x, weighted a half each: the blend's first row is zero, a normal along x is annihilated
    bind = np.zeros(2, dtype=VERTEX_DTYPE)
    bind["pos"][:, :3] = [[1, 2, 3], [4, 5, 6]]
    bind["normal"][:, :3] = [[1, 0, 0], [0, 1, 0]]
    bind["tangent"][:, :3] = [[2, 0, 0], [0, 0, 0]]  # the second as the loader writes it for an asset without tangents
    mats = np.float32([np.eye(3, 4), np.diag([-1.0, 1.0, 1.0]) @ np.eye(3, 4)]).reshape(2, 12)
    out = ref.pose(bind, np.uint16([[0, 1, 0, 0]] * 2), np.float32([[0.5, 0.5, 0, 0]] * 2), mats)
    assert not np.isnan(out["normal"]).any() and not np.isnan(out["tangent"]).any()
    assert np.array_equal(out["normal"][:, :3], np.float32([[0, 0, 0], [0, 1, 0]])) and np.array_equal(out["tangent"][:, :3], np.zeros((2, 3), np.float32))
    assert np.array_equal(out["pos"][:, :3], np.float32([[0, 2, 3], [0, 5, 6]]))


@pytest.mark.parametrize("skin", [False, True], ids=["morph", "skin"])
def test_the_other_fields_are_the_bind_records_bits(skin):
    bind, kw = inputs(21, 5, skin)
    rng = np.random.default_rng(1)
    for field, columns in (("pos", [3]), ("normal", [3]), ("uv", [0, 1]), ("_pad", [0, 1]), ("color", [0, 1, 2, 3]), ("tangent", [3])):
        for c in columns:  # any bits: NaN payloads, infinities, denormals among them
            bind[field][:, c] = rng.integers(0, 2**32, N, dtype=np.uint32).view(np.float32)
    out = ref.pose(bind, **kw)
    for field, columns in (("pos", [3]), ("normal", [3]), ("uv", [0, 1]), ("_pad", [0, 1]), ("color", [0, 1, 2, 3]), ("tangent", [3])):
        assert np.array_equal(out[field][:, columns].view(np.uint32), bind[field][:, columns].view(np.uint32)), field
