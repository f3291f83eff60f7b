"""Box families on which the reference's polygon clip is NOT the true overlap, and the numpy restatement of the overlap bound that lets
the rotated NMS skip the clip (csrc/iou3d_geom.h: far_apart, cannot_exceed).

When an edge of one box is collinear with an edge of the other (same heading shifted along it, side by side, end to end, perpendicular
boxes touching, axis-aligned grids, duplicates), the reference's seg_intersection passes its sign tests on rounding noise and adds
spurious points: the clip's overlap can be several times the geometric one.  The kernels must reproduce that clip (keep lists identical
to the reference), so the bound must send such pairs to the clip instead of deciding them.

Every family is deterministic (seeded numpy), 64 boxes on a shared heading by default, with perturbations away from exact alignment
measured from the edge lines (offsets in metres, heading deltas in radians)."""
import numpy as np

f = np.float32

KINDS = ("along", "row", "end_to_end", "side_by_side", "perpendicular", "grid", "duplicates")
JITTERS = (0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2)          # offset from the nearest pair of edge lines (m)
HEADING_DELTAS = (0.0, 1e-6, 1e-4, 1e-2)                      # heading of a box minus the family's (rad)
FAR = (70.0, 35.0)                                            # the "far from the origin" shift: coordinates of a distant car

# cannot_exceed's collinearity guard (iou3d_geom.h); None in place of the pair = the round-6 bound without it
GUARD = (1e-3, 1e-3)


def _cpu():
    import oracle
    return oracle.cpu()


def _rbox(b, cpu):
    x1, y1, x2, y2, ang = [np.ascontiguousarray(b[:, i], f) for i in range(5)]
    hx, hy = (x2 - x1) * f(0.5), (y2 - y1) * f(0.5)
    return dict(hx=hx, hy=hy, cx=(x1 + x2) / f(2), cy=(y1 + y2) / f(2), c=cpu.ref_trig("cosf", ang), s=cpu.ref_trig("sinf", ang),
                rad=np.sqrt(hx * hx + hy * hy))


def _pao(h, d, e):          # padded_axis_overlap
    return np.maximum(np.minimum(h, d + e) - np.maximum(-h, d - e) + f(2e-3), f(0))


def _near(d, h, g, eps):   # |d| within eps of a distance at which an edge of the one box lies on an edge line of the other
    ad = np.abs(d)
    return (np.abs(ad - (h + g)) < eps) | (np.abs(ad - np.abs(h - g)) < eps)


def overlap_bound(A, B, guard=GUARD, cpu=None):
    """cannot_exceed's quantities for all pairs (rows A, columns B), operation for operation in float32:
    -> (u, Sa, Sb, ok): u >= the overlap, ok = the bound may decide the pair (positive extents, the collinearity guard passes).
    cannot_exceed(a, b, thresh) == ok & (thresh > 0.01) & (u < 0.9 * thresh * (Sa + Sb - u))."""
    cpu = cpu or _cpu()
    a = {k: v[:, None] for k, v in _rbox(A, cpu).items()}
    b = {k: v[None, :] for k, v in _rbox(B, cpu).items()}
    cd = np.abs(a["c"] * b["c"] + a["s"] * b["s"])
    sd = np.abs(b["s"] * a["c"] - b["c"] * a["s"])
    dx, dy = b["cx"] - a["cx"], b["cy"] - a["cy"]
    ax, ay = dx * a["c"] - dy * a["s"], dx * a["s"] + dy * a["c"]
    ok = (a["hx"] > 0) & (a["hy"] > 0) & (b["hx"] > 0) & (b["hy"] > 0)
    if guard is not None:
        ea, ed = f(guard[0]), f(guard[1])
        par = (sd < ea) & (_near(ax, a["hx"], b["hx"], ed) | _near(ay, a["hy"], b["hy"], ed))
        per = (cd < ea) & (_near(ax, a["hx"], b["hy"], ed) | _near(ay, a["hy"], b["hx"], ed))
        ok = ok & ~par & ~per
    u1 = _pao(a["hx"], ax, b["hx"] * cd + b["hy"] * sd) * _pao(a["hy"], ay, b["hx"] * sd + b["hy"] * cd)
    u2 = _pao(b["hx"], dy * b["s"] - dx * b["c"], a["hx"] * cd + a["hy"] * sd) * _pao(b["hy"], -dx * b["s"] - dy * b["c"], a["hx"] * sd + a["hy"] * cd)
    sa, sb = f(4) * a["hx"] * a["hy"], f(4) * b["hx"] * b["hy"]
    return np.minimum(np.minimum(u1, u2), np.minimum(sa, sb)), sa, sb, ok


def cannot_exceed(u, sa, sb, ok, thresh):
    return ok & (thresh > 0.01) & (u < f(0.9) * f(thresh) * (sa + sb - u))


def far_apart(A, B, cpu=None):
    cpu = cpu or _cpu()
    a = {k: v[:, None] for k, v in _rbox(A, cpu).items()}
    b = {k: v[None, :] for k, v in _rbox(B, cpu).items()}
    dx, dy = a["cx"] - b["cx"], a["cy"] - b["cy"]
    s = (a["rad"] + b["rad"]) * f(1.0001) + f(1e-3)
    return dx * dx + dy * dy > s * s


def greedy_nms_with_skip(iou, skip, thresh):
    """the greedy sweep over sorted boxes where a pair in `skip` never suppresses (what a prefiltered kernel computes)"""
    n = iou.shape[0]
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        dead[i + 1:] |= (iou[i, i + 1:] > thresh) & ~skip[i, i + 1:]
    return np.array(keep, np.int64)


def _place(c0, ang, a, b):
    """centres at (a, b) in the frame of a box with heading ang: its local x axis is (cos, -sin), its y axis (sin, cos) (iou3d_geom.h)"""
    c, s = np.cos(ang), np.sin(ang)
    return np.stack([c0[0] + a * c + b * s, c0[1] - a * s + b * c], 1)


def family_params(kind, seed, jitter=0.0, dtheta=0.0, shift=(0.0, 0.0), n=64):
    """-> centres (n,2), lengths (n), widths (n), headings (n) in float64"""
    rng = np.random.default_rng(seed)
    L, W = rng.choice([3.9, 4.2, 4.6]), rng.choice([1.5, 1.6, 1.8])
    ang0 = rng.uniform(-np.pi, np.pi)
    if kind == "grid":
        ang0 = rng.choice([0.0, np.pi / 2, -np.pi / 2, np.pi])
    sign = lambda m=n: rng.choice([-1.0, 1.0], m)                              # noqa: E731
    ang = ang0 + dtheta * rng.choice([-1.0, 0.0, 1.0], n)
    Ls, Ws = np.full(n, L), np.full(n, W)
    if kind == "along":                  # same heading, shifted along it; lateral offsets 0, +-W, +-W/2
        a = rng.uniform(-2 * L, 2 * L, n)
        b = rng.choice([0.0, W, -W, W / 2, -W / 2], n) + jitter * sign()
    elif kind == "row":                  # a parked row: same heading, neighbours 0.85-1.0 L apart along it, laterally on one line
        a = np.cumsum(rng.uniform(0.85, 1.0, n)) * L
        a = a - a.mean()
        b = jitter * sign()
    elif kind == "end_to_end":           # along-axis offsets of whole lengths (a parked row), some with a lateral shift
        a = np.round(rng.uniform(-4, 4, n)) * L + jitter * sign()
        b = rng.uniform(-W, W, n) * rng.choice([0, 0, 1], n)
    elif kind == "side_by_side":         # lateral offsets of whole widths
        a = rng.uniform(-L, L, n) * rng.choice([0, 1, 1], n)
        b = np.round(rng.uniform(-4, 4, n)) * W + jitter * sign()
    elif kind == "perpendicular":        # half the boxes at heading + pi/2, an edge on an edge line of the family's box
        h = n // 2
        ang[h:] += np.pi / 2
        Ls[h:], Ws[h:] = rng.choice([3.9, 4.2]), rng.choice([1.5, 1.7])
        a, b = rng.uniform(-L / 2, L / 2, n), rng.uniform(-W / 2, W / 2, n)
        e = rng.integers(0, 2, n - h)
        ex = sign(n - h) * (L / 2 + Ws[h:] / 2 * sign(n - h)) + jitter * sign(n - h)      # the turned box's x half extent is W'/2
        ey = sign(n - h) * (W / 2 + Ls[h:] / 2 * sign(n - h)) + jitter * sign(n - h)      # and its y half extent L'/2
        a[h:] = np.where(e == 0, ex, a[h:])
        b[h:] = np.where(e == 1, ey, b[h:])
    elif kind == "grid":                 # axis-aligned lattice at ry in {0, +-pi/2, pi}, pitch one (or half a) box
        a = rng.integers(-4, 5, n) * L * rng.choice([1.0, 0.5]) + jitter * sign()
        b = rng.integers(-4, 5, n) * W * rng.choice([1.0, 0.5]) + jitter * sign()
    elif kind == "duplicates":           # four copies of each box, some pushed along by the jitter
        k = n // 4
        a, b = np.repeat(rng.uniform(-3, 3, k), 4), np.repeat(rng.uniform(-3, 3, k), 4)
        ang = np.repeat(rng.uniform(-np.pi, np.pi, k), 4) + dtheta * rng.choice([-1.0, 0.0, 1.0], n)
        a = a + jitter * rng.choice([-1.0, 0.0, 1.0], n)
    else:
        raise ValueError(kind)
    ctr = _place(np.array([10.0, 20.0]) + np.asarray(shift, np.float64), ang0, a, b)
    return ctr, Ls, Ws, ang


def family_bev(kind, seed, jitter=0.0, dtheta=0.0, shift=(0.0, 0.0), n=64):
    """(n,5) float32 [x1, y1, x2, y2, ry]"""
    ctr, L, W, ang = family_params(kind, seed, jitter, dtheta, shift, n)
    return np.stack([ctr[:, 0] - L / 2, ctr[:, 1] - W / 2, ctr[:, 0] + L / 2, ctr[:, 1] + W / 2, ang], 1).astype(f)


def family_boxes3d(kind, seed, jitter=0.0, dtheta=0.0, shift=(0.0, 0.0), n=64):
    """(n,7) float32 [x, y, z, h, w, l, ry] whose BEV (kitti_utils.boxes3d_to_bev: x -+ l/2, z -+ w/2) is the family"""
    ctr, L, W, ang = family_params(kind, seed, jitter, dtheta, shift, n)
    return np.stack([ctr[:, 0], np.ones(n), ctr[:, 1], np.full(n, 1.5), W, L, ang], 1).astype(f)


# 64-box sets on which the bound WITHOUT the guard changes the greedy keep list at threshold 0.1 (RCNN.NMS_THRESH): a pair it skips
# has a clip IoU above 0.1 (tests/test_overlap_bound.py holds that on the host).  (kind, seed, shift, "bev" | "3d": the family as BEV
# boxes, or as 3-D boxes whose BEV the kernels compute)
FLIP_SETS = (("row", 2, (0.0, 0.0), "bev"), ("row", 223, FAR, "bev"), ("row", 2, (0.0, 0.0), "3d"), ("row", 1163, FAR, "3d"))

# the seed pair: two boxes of one heading, the second shifted along it by 0.92 of a length; the clip gives IoU 0.1145 (overlap 1.25 m^2),
# the geometric overlap is 0.47 m^2 (float32 bits of [x1, y1, x2, y2, ry])
SEED_PAIR = np.array([[int(h, 16) for h in r.split()] for r in ("41577e2a 419c73e2 418bfafa 41a891c0 4033852a",
                                                                 "411f5d04 4192a1f7 415fd4cd 419ebfd6 4033852a")], np.uint32).view(f)
# a pair of 3-D boxes of the same kind (boxes 24, 25 of the "row" family, seed 2): their BEV clip IoU is 0.1446, the bound says < 0.05
SEED_PAIR_3D_OF = ("row", 2, (24, 25))


def flip_set(kind, seed, shift, form):
    return family_bev(kind, seed, shift=shift) if form == "bev" else family_boxes3d(kind, seed, shift=shift)
