"""Float64 brute-force ray/geometry reference (numpy only): what a ray hits, stated from the operation itself.

No octree, no BVH, no watertight shear, no float32, nothing imported from oracle/ or the product: every ray is tested
against every world-space triangle with Moeller-Trumbore in float64, and against every analytic shape (sphere, disk,
TriangleSimple) in the shape's object space through the float64 inverse of rigid @ PERM_YZ applied to the same float32
ray (direction not normalised, so t stays the world t).  tests/test_geometry_reference.py holds the oracle
(oracle/rtcore.hpp) to it on the CPU, tests/test_gpu_geometry.py the kernels themselves.

What float64 can arbitrate and what it cannot.  A float32 answer may differ from the float64 one only where the
geometry is within float32 rounding of a decision boundary, so a ray is *undecided* (from float64 quantities alone) if
  * a triangle's plane is crossed within the edge band of one of its edges: |min(u, v, 1-u-v)| < EDGE_BAND, or
    < EDGE_ULPS * 2^-24 * (distance travelled + |the triangle's coordinates|) / (smallest altitude x |cos incidence|):
    the renderer and the oracle round the world vertices and p - o to float32, and a grazing ray turns such a rounding
    into a long way along the plane (a CFG0 shadow ray through a crease at |cos| = 0.01 misses in float32 what float64
    hits 2e-5 inside an edge);
  * a shape's silhouette margin is within SIL_BAND * (|o - centre| + size), object units;
  * two distinct hits lie within W(t1) = t1 * 2^-16 + max|coordinate| * 2^-20 of each other (the traversal's own
    window, here only a tie band);
  * a plane is crossed inside (or within the edge band of) its triangle / shape at |t| < SELF_HIT, the self-hit zone
    of offset surface rays;
  * for occlusion: a candidate lies within W(tmax) of tmax.
A decided ray must match in hit or miss and in primitive; its t, barycentrics and hit point must lie within the
bounds below.  An undecided ray must still return one of the float64 near-tie *candidates* (every possible hit no
farther than the nearest certain hit plus W), or a miss if no hit is certain; it is never left unchecked.

Bounds on t, barycentrics and hit points: twice the largest error of the oracle against this reference over the
rays of tests/test_geometry_reference.py, measured on the CPU (never from GPU output); the factor 2 covers another
seed or ray count.  MEASURED holds the measured values, bounds() the asserted ones.
"""
from dataclasses import dataclass, field

import numpy as np

EDGE_BAND = 1e-5            # barycentric units
EDGE_ULPS = 8.0             # float32 roundings of (distance + coordinates) that may reach an edge function
SELF_HIT = 1e-3             # |t| below which a crossing may be rejected as a self hit
SIL_BAND = 2.0 ** -18       # silhouette band, x (|o - centre| + size)
SHAPE_UNIT = 2.0 ** -24     # unit of shape t / hit-point errors, x (|o - centre| + size)
MIN_COS = 0.1               # shape t and hit point are asserted only for |cos incidence| above this

# Largest error of the oracle against this reference over the decided rays of each case of
# tests/test_geometry_reference.py (CPU).  tri_t_w: |dt| of triangle hits in units of W(t); tri_bary: absolute
# barycentric error; shape_t / shape_p: |dt| and |p_hit - (O + D t64)| of shape hits at |cos incidence| > MIN_COS in
# units of SHAPE_UNIT x (|o - centre| + size).  Triangle errors grow with 1 / |cos incidence| (a float32 vertex
# rounding moves a grazing crossing far), hence the larger figures of the CFG0 blob seen edge-on from its camera.
MEASURED = {
    "cornell": dict(tri_t_w=0.410, tri_bary=9.80e-7),
    "blob8": dict(tri_t_w=0.0515, tri_bary=1.52e-5),
    "cfg0": dict(tri_t_w=2.90, tri_bary=8.01e-5),
    "shapes": dict(tri_t_w=0.0280, tri_bary=1.47e-5, shape_t=dict(sphere=42.8, disk=22.0, triangle=4.20),
                   shape_p=dict(sphere=29.6, disk=18.7, triangle=4.84)),
}
FACTOR = 2.0                # bound = FACTOR x measured: room for another seed or ray count


def bounds(case):
    """The asserted bounds of a case: FACTOR x MEASURED."""
    return {k: ({s: FACTOR * x for s, x in v.items()} if isinstance(v, dict) else FACTOR * v)
            for k, v in MEASURED[case].items()}


PERM_YZ = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.float64)


def window(t, wcoord):
    """W(t) = |t| 2^-16 + max|coordinate| 2^-20."""
    return np.abs(t) * 2.0 ** -16 + wcoord * 2.0 ** -20


def world_triangles(model):
    """(nt, 3, 3) float64 world-space corners: object_to_render applied to the float32 positions."""
    o2r = np.asarray(model.object_to_render(), np.float64)
    p = np.c_[np.asarray(model.positions, np.float64), np.ones(len(model.positions))] @ o2r.T
    return p[:, :3][np.asarray(model.indices, np.int64)]


def backface_mask(model):
    """Float64 back-face flags of a culled model: the mean vertex normal through the normal matrix against the look
    direction.  Returns (flag, |dot|); a flag is decisive where |dot| > 1e-5."""
    n2r = np.linalg.inv(np.asarray(model.object_to_render(), np.float64)).T[:3, :3]
    nv = np.asarray(model.normals, np.float64)[np.asarray(model.indices, np.int64)].mean(1)
    nv /= np.linalg.norm(nv, axis=1, keepdims=True)
    nw = nv @ n2r.T
    nw /= np.linalg.norm(nw, axis=1, keepdims=True)
    look = np.asarray(model.cull_look, np.float64)
    dot = nw @ (look / np.linalg.norm(look))
    return dot > 0, np.abs(dot)


# ------------------------------------------------------------------------------------------ candidates


@dataclass
class Candidates:
    """Sparse (ray, primitive) crossings that could be a hit.  strict: a hit in float64; certain: a hit beyond every
    band; t_lo: the smallest t a float32 evaluation could plausibly report for it."""
    ray: np.ndarray
    prim: np.ndarray
    t: np.ndarray
    t_lo: np.ndarray
    strict: np.ndarray
    certain: np.ndarray

    @staticmethod
    def concat(parts):
        return Candidates(*[np.concatenate([getattr(p, f) for p in parts]) for f in
                            ("ray", "prim", "t", "t_lo", "strict", "certain")])


def _first_two(n, ray, t):
    """Per ray: index (into the list) of the smallest t, that t, and the second smallest t (inf where absent)."""
    i1 = np.full(n, -1, np.int64)
    t1 = np.full(n, np.inf)
    t2 = np.full(n, np.inf)
    if len(ray):
        order = np.lexsort((t, ray))
        r = ray[order]
        first = np.r_[True, r[1:] != r[:-1]]
        second = np.r_[False, first[:-1]] & ~first
        i1[r[first]] = order[first]
        t1[r[first]] = t[order[first]]
        t2[r[second]] = t[order[second]]
    return i1, t1, t2


# ------------------------------------------------------------------------------------------- triangles


@dataclass
class TriangleHits:
    prim: np.ndarray          # nearest hit's triangle, -1: none
    t: np.ndarray             # its t (inf: none)
    bary: np.ndarray          # (n, 3) b0, b1, b2: the weights of corners 0, 1, 2
    t2: np.ndarray            # second-nearest distinct hit's t (inf: none)
    edge_margin: np.ndarray   # smallest |min(u, v, 1-u-v)| over the planes crossed at t > 0
    edge_in_band: np.ndarray  # some such margin lies inside that triangle's edge band
    t_plane: np.ndarray       # smallest |t| of a plane crossed inside (or in the edge band of) its triangle
    cand: Candidates


def brute_triangles(tris, ro, rd, skip=None, chunk=1024):
    """Every ray against every triangle, float64 Moeller-Trumbore.  skip: per-triangle mask of triangles left out."""
    tris = np.asarray(tris, np.float64)
    ro = np.asarray(ro, np.float64)
    rd = np.asarray(rd, np.float64)
    n, nt = len(ro), len(tris)
    p0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    nrm = np.cross(e1, e2)
    area2 = np.linalg.norm(nrm, axis=1)
    longest = np.sqrt(np.maximum.reduce([(e1 ** 2).sum(1), (e2 ** 2).sum(1), ((e2 - e1) ** 2).sum(1)]))
    valid = area2 > 0
    if skip is not None:
        valid = valid & ~np.asarray(skip, bool)
    alt = np.where(valid, area2 / np.where(longest > 0, longest, 1.0), 1.0)
    cmax = np.abs(tris).max((1, 2))
    out = TriangleHits(np.full(n, -1, np.int64), np.full(n, np.inf), np.full((n, 3), np.nan), np.full(n, np.inf),
                       np.full(n, np.inf), np.zeros(n, bool), np.full(n, np.inf), None)
    parts = []
    for a in range(0, n, chunk):
        o, d = ro[a:a + chunk], rd[a:a + chunk]
        m = len(o)
        s = o[:, None, :] - p0[None]
        det = -(d @ nrm.T)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            t = np.einsum("rtk,tk->rt", s, nrm) * inv
            mm = np.cross(s, d[:, None, :])
            u = np.einsum("rtk,tk->rt", mm, e2) * inv
            v = -np.einsum("rtk,tk->rt", mm, e1) * inv
            w = 1.0 - u - v
        minb = np.minimum(np.minimum(u, v), w)
        ok = valid[None] & (det != 0) & np.isfinite(t) & np.isfinite(minb)
        # edge band: the crossing point is known to EDGE_ULPS float32 roundings of (distance travelled + the
        # triangle's coordinates); seen along the ray the triangle's smallest altitude is altitude x |cos incidence|
        dl = np.linalg.norm(d, axis=1)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            cosi = np.abs(det) / (dl * area2[None])
            band = np.maximum(EDGE_BAND, EDGE_ULPS * 2.0 ** -24 * (np.abs(t) * dl + cmax[None]) / (alt[None] * cosi))
        band = np.where(ok, band, np.inf)
        strict = ok & (minb >= 0) & (t > 0)
        possible = ok & (minb > -band) & (t > -SELF_HIT)
        certain = ok & (minb >= band) & (t >= SELF_HIT)
        front = ok & (t > 0)
        am = np.where(front, np.abs(minb), np.inf)
        out.edge_margin[a:a + m] = am.min(1)
        out.edge_in_band[a:a + m] = (front & (np.abs(minb) < band)).any(1)
        out.t_plane[a:a + m] = np.where(ok & (minb > -band), np.abs(t), np.inf).min(1)
        ts = np.where(strict, t, np.inf)
        i1 = ts.argmin(1)
        rows = np.arange(m)
        t1 = ts[rows, i1]
        hit = np.isfinite(t1)
        out.prim[a:a + m] = np.where(hit, i1, -1)
        out.t[a:a + m] = t1
        out.bary[a:a + m] = np.where(hit[:, None], np.stack([w[rows, i1], u[rows, i1], v[rows, i1]], 1), np.nan)
        ts[rows, i1] = np.inf
        out.t2[a:a + m] = ts.min(1)
        rr, tt = np.nonzero(possible)
        parts.append(Candidates(rr + a, tt.astype(np.int64), t[rr, tt], t[rr, tt], strict[rr, tt], certain[rr, tt]))
    out.cand = Candidates.concat(parts) if parts else Candidates(*[np.zeros(0, k) for k in
                                                                   (np.int64, np.int64, float, float, bool, bool)])
    return out


# ---------------------------------------------------------------------------------------------- shapes


@dataclass
class ShapeSpec:
    kind: str                  # "sphere", "disk", "triangle"
    o2r: np.ndarray            # object to render, float64 (rigid @ PERM_YZ)
    radius: float = 1.0
    zmin: float = -1.0
    zmax: float = 1.0
    height: float = 0.0
    inner: float = 0.0
    outer: float = 1.0
    p: np.ndarray = None       # (3, 3) TriangleSimple corners, object space
    far_root: bool = False     # corruption switch of the tests: take the sphere's far root

    @property
    def size(self):
        if self.kind == "sphere":
            return self.radius
        if self.kind == "disk":
            return self.outer
        return float(max(np.linalg.norm(self.p[i] - self.p[(i + 1) % 3]) for i in range(3)))

    @property
    def centre(self):
        if self.kind == "sphere":
            return np.zeros(3)
        if self.kind == "disk":
            return np.array([0.0, 0.0, self.height])
        return self.p.mean(0)


def shape_specs(shapes):
    """ShapeSpec of each Sphere / Disk / TriangleSimple descriptor (by its attributes; parameters as the float32 the
    renderer receives)."""
    f32 = lambda x: float(np.float32(x))
    out = []
    for s in shapes:
        o2r = np.asarray(s.rigid, np.float64) @ PERM_YZ
        kind = type(s).__name__
        if kind == "Sphere":
            out.append(ShapeSpec("sphere", o2r, radius=f32(s.radius), zmin=-f32(s.radius), zmax=f32(s.radius)))
        elif kind == "Disk":
            out.append(ShapeSpec("disk", o2r, height=f32(s.height), inner=f32(s.inner_radius), outer=f32(s.outer_radius)))
        elif kind == "TriangleSimple":
            out.append(ShapeSpec("triangle", o2r, p=np.asarray(s.p, np.float32).astype(np.float64)))
        else:
            raise TypeError(kind)
    return out


@dataclass
class ShapeHits:
    hit: np.ndarray       # float64 hit
    t: np.ndarray         # its t; for a near miss the t of the closest approach / plane crossing
    t_lo: np.ndarray      # smallest t float32 could plausibly report (= t outside the silhouette band)
    p: np.ndarray         # (n, 3) object-space hit point
    margin: np.ndarray    # silhouette margin, object units, negative outside
    cos: np.ndarray       # |cos| of the incidence angle (object space)
    scale: np.ndarray     # |o - centre| + size, object units
    possible: np.ndarray
    certain: np.ndarray
    in_band: np.ndarray   # |margin| inside the silhouette band
    near0: np.ndarray     # a root / crossing within SELF_HIT of the origin


def brute_shape(spec, ro, rd):
    r2o = np.linalg.inv(spec.o2r)
    o = np.asarray(ro, np.float64) @ r2o[:3, :3].T + r2o[:3, 3]
    d = np.asarray(rd, np.float64) @ r2o[:3, :3].T
    n = len(o)
    dl = np.linalg.norm(d, axis=1)
    scale = np.linalg.norm(o - spec.centre, axis=1) + spec.size
    band = SIL_BAND * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        if spec.kind == "sphere":
            r = spec.radius
            tc = -(o * d).sum(1) / dl ** 2
            q = o + d * tc[:, None]
            dist = np.linalg.norm(q, axis=1)
            margin = r - dist
            h = np.sqrt(np.maximum(r * r - dist * dist, 0.0)) / dl
            t0, t1 = tc - h, tc + h
            inside = margin >= 0
            use1 = (t0 <= 0) | spec.far_root
            t = np.where(use1, t1, t0)
            p = o + d * t[:, None]
            clipped = (p[:, 2] < spec.zmin) | (p[:, 2] > spec.zmax)   # (zmin = -r, zmax = r: rounding only)
            hit = inside & (t > 0) & ~clipped
            t = np.where(inside, t, tc)
            hb = np.sqrt(np.maximum(r * r - np.maximum(dist - band, 0.0) ** 2, 0.0)) / dl
            near0 = (margin > -band) & ((np.abs(t0) < SELF_HIT) | (np.abs(t1) < SELF_HIT))
            t_lo = np.where(near0 & (t0 > -SELF_HIT), np.minimum(t0, t), t)
            t_lo = np.where(np.abs(margin) < band, np.minimum(t_lo, tc - hb), t_lo)
            cos = np.abs((p * d).sum(1)) / (np.linalg.norm(p, axis=1) * dl)
        elif spec.kind == "disk":
            t = (spec.height - o[:, 2]) / d[:, 2]
            p = o + d * t[:, None]
            rr = np.hypot(p[:, 0], p[:, 1])
            margin = spec.outer - rr if spec.inner <= 0 else np.minimum(spec.outer - rr, rr - spec.inner)
            margin = np.where(np.isfinite(t), margin, -np.inf)
            hit = (margin >= 0) & (t > 0)
            near0 = (margin > -band) & (np.abs(t) < SELF_HIT)
            t_lo = t
            cos = np.abs(d[:, 2]) / dl
        else:
            p1, e1, e2 = spec.p[0], spec.p[1] - spec.p[0], spec.p[2] - spec.p[0]
            nrm = np.cross(e1, e2)
            s = o - p1
            det = -(d @ nrm)
            t = (s @ nrm) / det
            mm = np.cross(s, d)
            u, v = (mm @ e2) / det, -(mm @ e1) / det
            minb = np.minimum(np.minimum(u, v), 1 - u - v)
            margin = np.where(np.isfinite(minb), minb * spec.size, -np.inf)
            hit = (margin >= 0) & (t >= 0)
            p = o + d * t[:, None]
            near0 = (margin > -band) & (np.abs(t) < SELF_HIT)
            t_lo = t
            cos = np.abs(d @ nrm) / (np.linalg.norm(nrm) * dl)
    fin = np.isfinite(t)
    possible = fin & (margin > -band) & (t > -SELF_HIT)
    certain = fin & hit & (margin >= band) & (t >= SELF_HIT) & ~near0
    return ShapeHits(hit & fin, np.where(fin, t, np.inf), np.where(fin, t_lo, np.inf), p, margin, cos, scale, possible,
                     certain, np.abs(margin) < band, near0)


# ----------------------------------------------------------------------------------------------- scene


@dataclass
class ClosestRef:
    n_tris: int
    wcoord: float
    prim: np.ndarray          # nearest float64 hit: triangle id, n_tris + k for shape k, -1 none
    t: np.ndarray
    t2: np.ndarray            # second-nearest distinct hit
    bary: np.ndarray          # triangle hits
    p_obj: np.ndarray         # shape hits: object-space point
    cos: np.ndarray           # shape hits
    scale: np.ndarray         # shape hits: |o - centre| + size
    decided: np.ndarray
    miss_ok: np.ndarray       # no certain hit: a miss is among the acceptable answers
    tri: TriangleHits
    shapes: list
    cand: Candidates
    kinds: list = field(default_factory=list)

    def acceptable(self, prim):
        """Per ray: is `prim` one of the near-tie candidates (or an acceptable miss)?"""
        prim = np.asarray(prim, np.int64)
        n, c = len(self.prim), self.cand
        _, tc, _ = _first_two(n, c.ray[c.certain], c.t[c.certain])
        lim = np.where(np.isfinite(tc), tc + window(tc, self.wcoord), np.inf)
        keep = c.t_lo <= lim[c.ray]
        stride = self.n_tris + len(self.shapes) + 1
        keys = c.ray[keep] * stride + c.prim[keep]
        mine = np.arange(n) * stride + prim
        return np.where(prim < 0, self.miss_ok, np.isin(mine, keys))


class SceneRef:
    """World triangles + analytic shapes; closest hit and occlusion by brute force in float64."""

    def __init__(self, tris, shapes=()):
        self.tris = np.asarray(tris, np.float64)
        self.shapes = list(shapes)
        self.wcoord = float(np.abs(self.tris).max())

    def closest(self, ro, rd, skip=None):
        ro = np.asarray(ro, np.float32).astype(np.float64)
        rd = np.asarray(rd, np.float32).astype(np.float64)
        n, nt = len(ro), len(self.tris)
        th = brute_triangles(self.tris, ro, rd, skip)
        sh = [brute_shape(s, ro, rd) for s in self.shapes]
        parts = [th.cand]
        for k, h in enumerate(sh):
            i = np.flatnonzero(h.possible)
            parts.append(Candidates(i, np.full(len(i), nt + k, np.int64), h.t[i], h.t_lo[i], h.hit[i], h.certain[i]))
        cand = Candidates.concat(parts)
        s = cand.strict
        i1, t1, t2 = _first_two(n, cand.ray[s], cand.t[s])
        sp = np.r_[cand.prim[s], -1]                       # (-1: so that a scene without any hit still indexes)
        prim = np.where(i1 >= 0, sp[np.maximum(i1, 0)], -1)
        bary = np.where((prim == th.prim)[:, None], th.bary, np.nan)
        p_obj = np.full((n, 3), np.nan)
        cos = np.full(n, np.nan)
        scale = np.full(n, np.nan)
        for k, h in enumerate(sh):
            m = prim == nt + k
            p_obj[m], cos[m], scale[m] = h.p[m], h.cos[m], h.scale[m]
        undecided = th.edge_in_band | (th.t_plane < SELF_HIT)
        for h in sh:
            undecided |= h.in_band | h.near0
        with np.errstate(invalid="ignore"):
            undecided |= np.isfinite(t2) & (t2 - t1 <= window(t1, self.wcoord))
        miss_ok = np.ones(n, bool)
        miss_ok[cand.ray[cand.certain]] = False
        return ClosestRef(nt, self.wcoord, prim, t1, t2, bary, p_obj, cos, scale, ~undecided, miss_ok, th, sh, cand,
                          [s.kind for s in self.shapes])

    def occluded(self, ref, tmax):
        """1 blocked, 0 clear, -1 undecided for the fixed tmax; `ref`: closest() of the same rays without a skip
        mask (shadow rays see every triangle)."""
        tmax = np.asarray(tmax, np.float32).astype(np.float64)
        c, n = ref.cand, len(tmax)
        w = window(tmax, self.wcoord)
        blocked = np.zeros(n, bool)
        b = c.certain & (c.t < (tmax - w)[c.ray])
        blocked[c.ray[b]] = True
        maybe = np.zeros(n, bool)
        m = c.t_lo < (tmax + w)[c.ray]
        maybe[c.ray[m]] = True
        return np.where(blocked, 1, np.where(maybe, -1, 0))


# ------------------------------------------------------------------------------------------ comparator


@dataclass
class Report:
    failures: list
    n: int
    undecided: int
    tri_t_w: float = 0.0          # largest |dt| / W(t) over decided triangle hits
    tri_bary: float = 0.0         # largest absolute barycentric error
    shape_t: dict = field(default_factory=dict)   # kind -> largest |dt| in shape units (|cos| > MIN_COS)
    shape_p: dict = field(default_factory=dict)   # kind -> largest hit-point error in shape units

    @property
    def ok(self):
        return not self.failures

    @property
    def undecided_share(self):
        return self.undecided / max(self.n, 1)


def compare_closest(ref, prim, bt, cap=None, bounds=None):
    """A traced result (prim, bt = (b0, b1, b2, t) or (object-space point, t)) against the float64 reference.
    bounds: bounds(case), or None to compare hits and primitives only (the errors are still reported)."""
    prim = np.asarray(prim, np.int64)
    bt = np.asarray(bt, np.float64)
    n, nt = len(prim), ref.n_tris
    fails = []
    dec = ref.decided
    rep = Report(fails, n, int((~dec).sum()))
    wrong = np.flatnonzero(dec & (prim != ref.prim))
    if len(wrong):
        i = wrong[0]
        fails.append(f"{len(wrong)} decided rays differ in hit/primitive; first ray {i}: got {prim[i]}, float64 "
                     f"{ref.prim[i]} at t {ref.t[i]:.9g} (t2 {ref.t2[i]:.9g}, edge margin {ref.tri.edge_margin[i]:.3g})")
    bad = np.flatnonzero(~dec & ~ref.acceptable(prim))
    if len(bad):
        i = bad[0]
        fails.append(f"{len(bad)} undecided rays return no float64 candidate; first ray {i}: got {prim[i]}, float64 "
                     f"{ref.prim[i]} at t {ref.t[i]:.9g}")
    if cap is not None and rep.undecided > cap * n:
        fails.append(f"undecided share {rep.undecided_share:.4f} above the cap {cap}")
    same = dec & (prim == ref.prim) & (prim >= 0)
    tri = same & (prim < nt)
    if tri.any():
        dt = np.abs(bt[tri, 3] - ref.t[tri]) / window(ref.t[tri], ref.wcoord)
        db = np.abs(bt[tri, :3] - ref.bary[tri]).max(1)
        rep.tri_t_w, rep.tri_bary = float(dt.max()), float(db.max())
        if bounds and rep.tri_t_w > bounds["tri_t_w"]:
            fails.append(f"triangle t off by {rep.tri_t_w:.3g} W(t) (bound {bounds['tri_t_w']})")
        if bounds and rep.tri_bary > bounds["tri_bary"]:
            fails.append(f"barycentrics off by {rep.tri_bary:.3g} (bound {bounds['tri_bary']})")
    for k, kind in enumerate(ref.kinds):
        m = same & (prim == nt + k) & (ref.cos > MIN_COS)
        if not m.any():
            continue
        unit = SHAPE_UNIT * ref.scale[m]
        dt = float((np.abs(bt[m, 3] - ref.t[m]) / unit).max())
        dp = float((np.linalg.norm(bt[m, :3] - ref.p_obj[m], axis=1) / unit).max())
        rep.shape_t[kind] = max(rep.shape_t.get(kind, 0.0), dt)
        rep.shape_p[kind] = max(rep.shape_p.get(kind, 0.0), dp)
        if bounds and dt > bounds["shape_t"][kind]:
            fails.append(f"{kind} {k}: t off by {dt:.3g} units (bound {bounds['shape_t'][kind]})")
        if bounds and dp > bounds["shape_p"][kind]:
            fails.append(f"{kind} {k}: hit point off by {dp:.3g} units (bound {bounds['shape_p'][kind]})")
    return rep


def compare_occluded(expected, occ):
    """expected: SceneRef.occluded (1 / 0 / -1); occ: the traced 0 / 1 answers.  Returns a list of failures."""
    occ = np.asarray(occ).astype(bool)
    fails = []
    for want, name in ((1, "blocked"), (0, "clear")):
        m = expected == want
        if not m.any():
            fails.append(f"no {name} answer among the queries")
        bad = np.flatnonzero(m & (occ != bool(want)))
        if len(bad):
            fails.append(f"{len(bad)} {name} queries answered otherwise; first {bad[0]}")
    return fails


def compare_backface(model, flags):
    """The float64 back-face mask against traced flags where it is decisive.  Returns (failures, mask, decisive)."""
    mask, mag = backface_mask(model)
    decisive = mag > 1e-5
    bad = np.flatnonzero(decisive & (mask != np.asarray(flags).astype(bool)))
    return ([f"{len(bad)} decisive back-face flags differ; first triangle {bad[0]}"] if len(bad) else []), mask, decisive
