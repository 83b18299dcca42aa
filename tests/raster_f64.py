"""An independent float64 rasteriser: the truth the four rasterised passes (forward, rasterised G-buffer, marching-cubes pass, cascaded
shadow maps) and their numpy restatements are held to. Plain numpy float64, no code shared with forward_reference, shadow_map_reference,
gbuffer_raster_reference or marching_cubes_pass_reference: no clip, no snap, no fill rule, no records - every triangle is evaluated at
every point with homogeneous edge functions. Not a conftest: test modules import it.

The decision rule (five_points): the truth is evaluated at the pixel centre and at the centre +- (DELTA, DELTA) on both diagonals, with
DELTA = 1/64 pixel - four times the 1/256-pixel grid the rasteriser snaps vertices to (a snapped vertex moves by at most 1/512 pixel per
axis). A pixel is *decided* when the five winners are equal (one draw index, or none at all five), the runner-up is farther than the
winner by more than MARGIN = 1e-5 at every point, and the winner's depth lies in [MARGIN, 1 - MARGIN] at every point. A pixel is *surely
covered* when all five points have a winner, whichever it is. Only decided pixels are held to the winner; surely covered ones must not be
empty and must show one of the five winners, which is what catches a crack along a shared, clipped or fan edge without naming a fill
rule. One amendment: a vertex that many triangles share and that sits on a pixel centre (a fan's apex) belongs, after the snap, to every
one of them, so there a triangle that reaches into the pixel's +-DELTA square at the winners' depth is accepted too (reaches).

Depth, barycentrics and world positions are held at decided covered pixels to the envelope of the truth over the five points, widened by
its own width and an absolute term measured on the case list (raster_f64_cases.py)."""
import numpy as np

DELTA = 1.0 / 64.0
MARGIN = 1e-5
ULP = 2.0 ** -24  # one float32 unit in the last place of values in [0.5, 1)
POINTS = ((0.0, 0.0), (DELTA, DELTA), (-DELTA, -DELTA), (DELTA, -DELTA), (-DELTA, DELTA))
NONE = 0xFFFFFFFF


# ---- matrices and triangles -----------------------------------------------------------------------------------------------------
def _mat(column_major16):
    return np.array(list(column_major16), np.float64).reshape(4, 4).T


def world_matrix(world3x4):
    m = np.eye(4)
    m[:3] = np.asarray(world3x4, np.float64).reshape(3, 4)
    return m


def clip_matrices(projection_view, meshes):
    """(P V) W per mesh in float64, column-major (16,), from the float32 column-major P V (16,) and each mesh's 3x4"""
    pv = _mat(projection_view)
    return [(pv @ world_matrix(m["world"])).T.reshape(16) for m in meshes]


def view_matrices(view, meshes):
    """clip_matrices for a view's projection and view matrices"""
    return clip_matrices((_mat(view.projection[:]) @ _mat(view.view[:])).T.reshape(16), meshes)


def world_triangles(meshes):
    """(T, 3, 3) float64 world-space vertices of every triangle in draw order"""
    out = []
    for m in meshes:
        p = np.concatenate([m["vertices"]["pos"][:, :3].astype(np.float64), np.ones((len(m["vertices"]), 1))], axis=1)
        out.append((p @ world_matrix(m["world"]).T)[:, :3][m["indices"].reshape(-1, 3).astype(np.int64)])
    return np.concatenate(out) if out else np.zeros((0, 3, 3))


def _clip_triangles(matrices, meshes):
    """clip vertices (T, 3, 4) of every triangle in draw order"""
    out = []
    for M, m in zip(matrices, meshes):
        p = np.concatenate([m["vertices"]["pos"][:, :3].astype(np.float64), np.ones((len(m["vertices"]), 1))], axis=1)
        out.append((p @ _mat(M).T)[m["indices"].reshape(-1, 3).astype(np.int64)])
    return np.concatenate(out) if out else np.zeros((0, 3, 4))


# ---- the truth ------------------------------------------------------------------------------------------------------------------
def truth(matrices, meshes, W, H, offset=(0.0, 0.0), seed=None, chunk=256):
    """every triangle at every pixel's point (px + 0.5 + ox, py + 0.5 + oy), NDC y up (viewport (0, H, W, -H)): with clip vertices
    c_k = (x, y, z, w), lambda = A^-1 (x_ndc, y_ndc, 1) for A = [[x0 x1 x2], [y0 y1 y2], [w0 w1 w2]], s = sum(lambda), b = lambda / s; the
    triangle covers the point when all b >= 0, s > 0 and d = sum(b z) / sum(b w) lies in [0, 1]. A triangle whose |det A|, scaled by the
    norms of A's rows, is below 1e-13 is skipped, as is one with a non-finite vertex.

    -> dict(winner (H, W) int64 draw index of the least d or -1, d (H, W) its d (inf for none), runner (H, W) the second least d (inf
    for none), b (H, W, 3) the winner's perspective-correct barycentrics). seed (H, W): a depth buffer the triangles are tested against,
    a triangle winning only where its d <= the seed's; where the seed wins the winner is -1, d the seed and runner the least triangle d."""
    tri = _clip_triangles(matrices, meshes)
    xs = (np.arange(W) + 0.5 + offset[0]) / W * 2.0 - 1.0
    ys = 1.0 - (np.arange(H) + 0.5 + offset[1]) / H * 2.0
    X, Y = np.meshgrid(xs, ys)
    p = np.stack([X.reshape(-1), Y.reshape(-1), np.ones(W * H)], axis=0)  # (3, N)
    N = W * H
    best, second = np.full(N, np.inf), np.full(N, np.inf)
    winner = np.full(N, -1, np.int64)
    bw = np.zeros((N, 3))
    with np.errstate(all="ignore"):
        rx, ry, rw, rz = tri[..., 0], tri[..., 1], tri[..., 3], tri[..., 2]  # (T, 3): the rows of A, and z
        c0, c1, c2 = np.cross(ry, rw), np.cross(rw, rx), np.cross(rx, ry)    # the columns of adj(A)
        det = (rx * c0).sum(-1)
        scale = np.linalg.norm(rx, axis=-1) * np.linalg.norm(ry, axis=-1) * np.linalg.norm(rw, axis=-1)
        ok = np.isfinite(tri).all(axis=(1, 2)) & (np.abs(det) >= 1e-13 * scale) & (scale > 0)
    use = np.nonzero(ok)[0]
    for at in range(0, len(use), chunk):
        t = use[at:at + chunk]
        inv = np.stack([c0[t], c1[t], c2[t]], axis=-1) / det[t][:, None, None]  # (t, 3, 3): A^-1
        with np.errstate(all="ignore"):
            lam = inv @ p                                   # (t, 3, N)
            s = lam.sum(1)                                  # (t, N)
            b = lam / s[:, None, :]
            zz, ww = (b * rz[t][:, :, None]).sum(1), (b * rw[t][:, :, None]).sum(1)
            d = zz / ww
            cover = (b >= 0).all(1) & (s > 0) & (d >= 0) & (d <= 1)
        d = np.where(cover, d, np.inf)
        i1 = d.argmin(0)
        cols = np.arange(N)
        d1 = d[i1, cols]
        b1 = b[i1, :, cols]                                 # (N, 3)
        d[i1, cols] = np.inf
        d2 = d.min(0)
        nearer = d1 < best
        second = np.where(nearer, np.minimum(best, d2), np.minimum(second, d1))
        winner = np.where(nearer, t[i1], winner)
        bw = np.where(nearer[:, None], b1, bw)
        best = np.where(nearer, d1, best)
    if seed is not None:
        sd = np.asarray(seed, np.float64).reshape(-1)
        hidden = sd < best
        second = np.where(hidden, best, np.minimum(second, sd))
        winner = np.where(hidden, -1, winner)
        bw = np.where(hidden[:, None], 0.0, bw)
        best = np.where(hidden, sd, best)
    return dict(winner=winner.reshape(H, W), d=best.reshape(H, W), runner=second.reshape(H, W), b=bw.reshape(H, W, 3))


class Five:
    """the truth at the five points of the decision rule: winners, d, runner (5, H, W), b (5, H, W, 3), and per pixel decided, covered
    (surely covered), winner (the common winner where decided, else the centre's), the envelopes d_lo, d_hi, b_lo, b_hi over the five"""

    def __init__(self, samples, matrices, meshes):
        self.matrices, self.meshes = matrices, meshes
        self.winners = np.stack([s["winner"] for s in samples])
        self.d = np.stack([s["d"] for s in samples])
        self.runner = np.stack([s["runner"] for s in samples])
        self.b = np.stack([s["b"] for s in samples])
        same = (self.winners == self.winners[0]).all(0)
        drawn = self.winners >= 0
        with np.errstate(invalid="ignore"):
            apart = np.where(np.isfinite(self.d), self.runner - self.d > MARGIN, True).all(0)
        inside = np.where(drawn, (self.d >= MARGIN) & (self.d <= 1.0 - MARGIN), True).all(0)
        self.decided = same & apart & inside
        self.covered = drawn.all(0)
        self.winner = self.winners[0]
        self.drawn = self.decided & (self.winner >= 0)  # decided and covered: where depth, b and positions are held
        self.d_lo, self.d_hi = self.d.min(0), self.d.max(0)
        self.b_lo, self.b_hi = self.b.min(0), self.b.max(0)

    def counts(self):
        n = self.decided.size
        return dict(pixels=n, decided=int(self.decided.sum()), undecided=int(n - self.decided.sum()), decided_covered=int(self.drawn.sum()),
                    surely_covered=int(self.covered.sum()))


def five_points(matrices, meshes, W, H, seed=None):
    """the decision rule (see the module's docstring): truth at the centre and the centre +- (DELTA, DELTA) on both diagonals"""
    return Five([truth(matrices, meshes, W, H, o, seed) for o in POINTS], matrices, meshes)


# ---- the checks, shared by the restatements' and the device's tests --------------------------------------------------------------
def reaches(five, pixel, draw, n=16):
    """whether triangle `draw` covers some point of the square of half-side DELTA around flat pixel index `pixel`, on a (2 n + 1)^2
    grid, at a depth no farther than MARGIN behind the farthest of the pixel's five winners"""
    W, H = five.winner.shape[1], five.winner.shape[0]
    tri = _clip_triangles(five.matrices, five.meshes)
    c = tri[int(draw)]                                       # (3, 4)
    o = np.arange(-n, n + 1) * (DELTA / n)
    ox, oy = np.meshgrid(o, o)
    x = (pixel % W + 0.5 + ox.reshape(-1)) / W * 2.0 - 1.0
    y = 1.0 - (pixel // W + 0.5 + oy.reshape(-1)) / H * 2.0
    A = np.stack([c[:, 0], c[:, 1], c[:, 3]])
    with np.errstate(all="ignore"):
        lam = np.linalg.solve(A, np.stack([x, y, np.ones_like(x)]))
        s = lam.sum(0)
        b = lam / s
        d = (b * c[:, 2, None]).sum(0) / (b * c[:, 3, None]).sum(0)
        far = five.d.reshape(5, -1)[:, pixel].max() + MARGIN
        return bool(((b >= 0).all(0) & (s > 0) & (d >= 0) & (d <= min(far, 1.0))).any())


def check_visibility(five, vis, excused=0):
    """decided pixels show the truth's winner (NONE for -1); surely covered pixels are never NONE and show one of the five winners. The
    one exception is counted: exactly `excused` surely covered pixels show another triangle, and each of those reaches into the pixel's
    +-DELTA square at the winners' depth (a fan's apex on a pixel centre belongs to every triangle of the fan)"""
    vis = np.asarray(vis).astype(np.int64)
    want = np.where(five.winner < 0, NONE, five.winner)
    wrong = five.decided & (vis != want)
    assert not wrong.any(), f"{int(wrong.sum())} decided pixels show another triangle than the float64 rasteriser, first at (y, x) " \
                            f"{tuple(np.argwhere(wrong)[0])}: {vis[wrong][0]} for {want[wrong][0]}"
    holes = five.covered & (vis == NONE)
    assert not holes.any(), f"{int(holes.sum())} surely covered pixels are empty (a crack), first at (y, x) {tuple(np.argwhere(holes)[0])}"
    stray = np.nonzero((five.covered & ~(vis[None] == five.winners).any(0)).reshape(-1))[0]
    assert len(stray) == excused, f"{len(stray)} surely covered pixels show none of the five winners, {excused} expected: flat indices {stray[:8]}"
    absent = [int(p) for p in stray if not reaches(five, int(p), vis.reshape(-1)[p])]
    assert not absent, f"{len(absent)} surely covered pixels show a triangle that is not there, first flat index {absent[0]}"


def excess(value, lo, hi):
    """how far value lies outside [lo, hi], in float32 ulps of 1.0 (0 inside)"""
    v = np.asarray(value, np.float64)
    return np.maximum(np.maximum(lo - v, v - hi), 0.0) / ULP


def widened(lo, hi, ulps):
    """the envelope widened on each side by its own width plus `ulps` float32 ulps of 1.0"""
    w = hi - lo
    return lo - w - ulps * ULP, hi + w + ulps * ULP


def check_depth(five, depth, ulps):
    """decided covered pixels: depth within the envelope of d over the five points, widened by its own width plus `ulps` ulps of 1.0 ->
    the largest excess over the un-widened envelope in ulps of 1.0 (a measurement, 0.0 without such pixels)"""
    m = five.drawn
    if not m.any():
        return 0.0
    z = np.asarray(depth, np.float64)[m]
    lo, hi = widened(five.d_lo[m], five.d_hi[m], ulps)
    bad = (z < lo) | (z > hi)
    assert not bad.any(), f"{int(bad.sum())} decided pixels' depth outside the float64 envelope, worst by {excess(z, lo, hi).max():.1f} ulp of 1.0"
    return float(excess(z, five.d_lo[m], five.d_hi[m]).max())


def check_barycentrics(five, pixels, b, ulps):
    """b (N, 3) at the flat pixel indices `pixels`: within the widened envelope of the truth's b at the decided covered ones -> the
    largest excess over the un-widened envelope in ulps of 1.0"""
    m = five.drawn.reshape(-1)[pixels]
    if not m.any():
        return 0.0
    got = np.asarray(b, np.float64)[m]
    blo, bhi = five.b_lo.reshape(-1, 3)[pixels[m]], five.b_hi.reshape(-1, 3)[pixels[m]]
    lo, hi = widened(blo, bhi, ulps)
    bad = (got < lo) | (got > hi)
    assert not bad.any(), f"{int(bad.any(-1).sum())} decided pixels' barycentrics outside the float64 envelope, worst by {excess(got, lo, hi).max():.1f} ulp"
    return float(excess(got, blo, bhi).max())


# float32 evaluation of W v and of (b0 p0 + b1 p1) + b2 p2: three products and sums for each world vertex, three products and two sums
# for the interpolation, each rounding within half an ulp of a term no larger than the largest vertex coordinate - 8 half-ulps, doubled
POSITION_ROUNDING_ULPS = 8


def check_positions(five, meshes, pixels, position, b_ulps):
    """world positions (N, 3) at the flat pixel indices `pixels`, at the decided covered ones, against sum(b world(v)) in float64: inside
    the interval v0 + [b1] (v1 - v0) + [b2] (v2 - v0) over the widened b envelope (the triangle's world vertices carry the envelope), plus
    the float32 rounding of the evaluation and of b's sum, (POSITION_ROUNDING_ULPS + 3 b_ulps) ulps of the largest |coordinate|"""
    m = five.drawn.reshape(-1)[pixels]
    if not m.any():
        return
    pix = pixels[m]
    got = np.asarray(position, np.float64)[m]
    v = world_triangles(meshes)[five.winner.reshape(-1)[pix]]  # (n, 3, 3)
    blo, bhi = widened(five.b_lo.reshape(-1, 3)[pix], five.b_hi.reshape(-1, 3)[pix], b_ulps)
    lo, hi = v[:, 0].copy(), v[:, 0].copy()
    for k in (1, 2):
        e = v[:, k] - v[:, 0]
        a, c = blo[:, k, None] * e, bhi[:, k, None] * e
        lo, hi = lo + np.minimum(a, c), hi + np.maximum(a, c)
    tol = (POSITION_ROUNDING_ULPS + 3 * b_ulps) * ULP * np.abs(v).max(axis=(1, 2))[:, None]
    bad = (got < lo - tol) | (got > hi + tol)
    assert not bad.any(), f"{int(bad.any(-1).sum())} decided pixels' world position outside the float64 interval, worst by " \
                          f"{np.maximum(lo - tol - got, got - hi - tol).max():.3g}"


def check_caps(five, exempt=False):
    """conditions on a case, not measurements: at least 300 decided covered pixels (tiny frames exempt) and at most 15 % undecided"""
    c = five.counts()
    assert exempt or c["decided_covered"] >= 300, c
    assert c["undecided"] <= 0.15 * c["pixels"], c
    return c
