"""An exact rational reference for the bottom-quad overlap and the IoUs of kitti_utils.get_iou3d (csrc/quad_clip.h), independent of
tests/train_input_twin.py.

    exact_overlap(ca, cb) -> (overlap, area_a, area_b)   fractions.Fraction, corners 0:4 in (x, z)
    exact_iou(ca, cb)     -> (iou3d, iou_bev)            fractions.Fraction
    quad_gap(ca, cb)      -> float                       distance between two bottoms whose overlap is 0 (a double; for liveness
                                                         conditions only, never for an expected value)
    self_test()                                          symmetry and closed-form rectangle overlaps, exact equality

Every fp32 coordinate is a dyadic rational, so every quantity below is exact.  The overlap is NOT a Sutherland-Hodgman clip: it
is the area of the convex hull of {vertices of A inside or on B} + {vertices of B inside or on A} + {points where an edge of A
crosses an edge of B}, deduplicated exactly, ordered around their centroid by exact cross products, shoelace.  For two convex
regions that point set is the vertex set of the intersection (plus, harmlessly, points on its edges).

Validity as quad_clip.h documents it: a quad whose four turns do not share one strict sign (exact test) has area 0, and a pair
with such a quad has IoU 0.  Orientation by the exact signed area.  The heights are what numpy does in fp32
(train_input_twin._heights, h = fp32(min - max)): that is the reference's arithmetic, not geometry; the fp32 results enter the
exact formula as exact rationals.
"""
from fractions import Fraction
from functools import cmp_to_key

import numpy as np

import train_input_twin as tw

ZERO = Fraction(0)


def _pts(c):
    return [(Fraction(float(c[k, 0])), Fraction(float(c[k, 2]))) for k in range(4)]


def _turn(a, b, p):
    """> 0 when p is to the left of a -> b"""
    return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])


def _signed_area(p):
    n = len(p)
    return sum(p[i][0] * p[(i + 1) % n][1] - p[(i + 1) % n][0] * p[i][1] for i in range(n)) / 2


_QUADS = {}


def _quad(c):
    """counter-clockwise vertices and the area; area 0 when the quad is not strictly convex (memoised on the fp32 bits: the
    sampler tests ask about the same few hundred boxes many times)"""
    key = np.ascontiguousarray(c[:4, [0, 2]], np.float32).tobytes()
    if key not in _QUADS:
        if len(_QUADS) > 100000:
            _QUADS.clear()
        _QUADS[key] = _make_quad(c)
    return _QUADS[key]


def _make_quad(c):
    p = _pts(c)
    turns = [_turn(p[k], p[(k + 1) % 4], p[(k + 2) % 4]) for k in range(4)]
    if not (all(t > 0 for t in turns) or all(t < 0 for t in turns)):
        return p, ZERO
    s = _signed_area(p)
    return (p if s > 0 else p[::-1]), abs(s)


def _inside_or_on(p, poly):
    return all(_turn(poly[k], poly[(k + 1) % 4], p) >= 0 for k in range(4))


def _crossing(p1, p2, q1, q2):
    """the point where segments p1p2 and q1q2 meet, for non-parallel segments; None otherwise (parallel segments add no vertex
    that the inside-or-on tests do not already give)"""
    rx, rz = p2[0] - p1[0], p2[1] - p1[1]
    sx, sz = q2[0] - q1[0], q2[1] - q1[1]
    den = rx * sz - rz * sx
    if den == 0:
        return None
    wx, wz = q1[0] - p1[0], q1[1] - p1[1]
    t = (wx * sz - wz * sx) / den
    u = (wx * rz - wz * rx) / den
    if 0 <= t <= 1 and 0 <= u <= 1:
        return (p1[0] + t * rx, p1[1] + t * rz)
    return None


def _hull_area(points):
    """area of a point set in convex position (points on the hull's edges allowed)"""
    pts = list(set(points))
    if len(pts) < 3:
        return ZERO
    cx = sum(p[0] for p in pts) / len(pts)
    cz = sum(p[1] for p in pts) / len(pts)

    def half(d):
        return 0 if (d[1] > 0 or (d[1] == 0 and d[0] >= 0)) else 1

    def cmp(p, q):
        dp, dq = (p[0] - cx, p[1] - cz), (q[0] - cx, q[1] - cz)
        hp, hq = half(dp), half(dq)
        if hp != hq:
            return hp - hq
        cr = dp[0] * dq[1] - dp[1] * dq[0]
        return -1 if cr > 0 else (1 if cr < 0 else 0)

    pts.sort(key=cmp_to_key(cmp))
    return abs(_signed_area(pts))


def _bounds_apart(ca, cb):
    """the axis-aligned bounds of the two vertex sets are strictly apart: the regions are disjoint (comparisons of fp32 values
    are exact)"""
    for d in (0, 2):
        if ca[:4, d].max() < cb[:4, d].min() or cb[:4, d].max() < ca[:4, d].min():
            return True
    return False


def exact_overlap(ca, cb):
    pa, area_a = _quad(ca)
    pb, area_b = _quad(cb)
    if area_a == 0 or area_b == 0 or _bounds_apart(ca, cb):
        return ZERO, area_a, area_b
    pts = [p for p in pa if _inside_or_on(p, pb)] + [p for p in pb if _inside_or_on(p, pa)]
    for i in range(4):
        for j in range(4):
            x = _crossing(pa[i], pa[(i + 1) % 4], pb[j], pb[(j + 1) % 4])
            if x is not None:
                pts.append(x)
    return _hull_area(pts), area_a, area_b


def exact_iou(ca, cb):
    ca, cb = np.asarray(ca, np.float32), np.asarray(cb, np.float32)
    lo_a, hi_a = tw._heights(ca)
    lo_b, hi_b = tw._heights(cb)
    h = np.float32(min(hi_a, hi_b) - max(lo_a, lo_b))
    if not h > 0:
        return ZERO, ZERO
    o, area_a, area_b = exact_overlap(ca, cb)
    if area_a == 0 or area_b == 0:
        return ZERO, ZERO
    h = Fraction(float(h))
    dh_a, dh_b = Fraction(float(np.float32(hi_a - lo_a))), Fraction(float(np.float32(hi_b - lo_b)))
    return o * h / (area_a * dh_a + area_b * dh_b - o * h), o / (area_a + area_b - o)


def quad_gap(ca, cb):
    """distance between the two bottoms' boundaries, in double (meaningful for pairs that do not overlap)"""
    a = [np.array([float(c[k, 0]), float(c[k, 2])]) for c in (ca,) for k in range(4)]
    b = [np.array([float(c[k, 0]), float(c[k, 2])]) for c in (cb,) for k in range(4)]

    def seg(p, s0, s1):
        d = s1 - s0
        dd = float(d @ d)
        t = 0.0 if dd == 0.0 else min(1.0, max(0.0, float((p - s0) @ d) / dd))
        return float(np.hypot(*(p - (s0 + t * d))))

    best = np.inf
    for P, Q in ((a, b), (b, a)):
        for p in P:
            for k in range(4):
                best = min(best, seg(p, Q[k], Q[(k + 1) % 4]))
    return best


def near_miss(ca, cb, tol):
    """two bottoms that do not overlap but come closer than tol"""
    for d in (0, 2):
        if ca[:4, d].max() + tol < cb[:4, d].min() or cb[:4, d].max() + tol < ca[:4, d].min():
            return False
    return quad_gap(ca, cb) < tol


def self_test(seed=0, n=60):
    """exact_overlap is symmetric and equals the closed-form overlap on axis-aligned rectangles, exactly"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        cx, cz, qx, qz = rng.uniform(-5, 5, 4)
        hx, hz, gx, gz = rng.uniform(0.2, 3, 4)
        if k % 3 == 0:                    # multiples of 1/8: the rectangles share an edge (every sixth: only a corner) exactly
            cx, cz, hx, hz, gx, gz = (np.ceil(v * 8) / 8 for v in (cx, cz, hx, hz, gx, gz))
            qx = cx + hx + gx
            qz = cz + hz + gz if k % 6 == 0 else cz + 0.125
        a = tw.rect_corners(cx, cz, hx, hz)
        b = tw.rect_corners(qx, qz, gx, gz)
        if k % 2:
            b = b[[1, 2, 3, 0, 5, 6, 7, 4]]
        if k % 5 == 0:
            b = b[[3, 2, 1, 0, 7, 6, 5, 4]]     # clockwise
        ax, az = [Fraction(float(v)) for v in a[:4, 0]], [Fraction(float(v)) for v in a[:4, 2]]
        bx, bz = [Fraction(float(v)) for v in b[:4, 0]], [Fraction(float(v)) for v in b[:4, 2]]
        ox = max(ZERO, min(max(ax), max(bx)) - max(min(ax), min(bx)))
        oz = max(ZERO, min(max(az), max(bz)) - max(min(az), min(bz)))
        want = (ox * oz, (max(ax) - min(ax)) * (max(az) - min(az)), (max(bx) - min(bx)) * (max(bz) - min(bz)))
        got, rev = exact_overlap(a, b), exact_overlap(b, a)
        assert got == want, (k, got, want)
        assert rev == (got[0], got[2], got[1]), k
    for k in range(n):                    # rotated pairs: symmetry, and overlap of a quad with itself
        bx = np.zeros((2, 7), np.float32)
        bx[:, 0] = rng.uniform(-2, 2, 2); bx[:, 2] = rng.uniform(-2, 2, 2); bx[:, 3] = 1.5
        bx[:, 4] = rng.uniform(0.5, 2, 2); bx[:, 5] = rng.uniform(1, 5, 2); bx[:, 6] = rng.uniform(-np.pi, np.pi, 2)
        c = tw.corners3d(bx)
        o, aa, ab = exact_overlap(c[0], c[1])
        assert exact_overlap(c[1], c[0]) == (o, ab, aa) and 0 <= o <= min(aa, ab)
        assert exact_overlap(c[0], c[0]) == (aa, aa, aa)
        assert exact_iou(c[0], c[0]) == (1, 1)
    sq = tw.rect_corners(0, 0, 1, 1)
    assert exact_overlap(sq, tw.rect_corners(0, 0, 1, 0))[0] == 0                 # zero width
    assert exact_overlap(sq, sq[[0, 2, 1, 3, 4, 6, 5, 7]]) == (0, 4, 0)           # bow-tie
    return True


if __name__ == "__main__":
    self_test()
    print("exact_quad self-test OK")
