"""Seeded adversarial box pairs for the corner IoU (csrc/quad_clip.h) and the GT-augmentation sampler's collision test
(csrc/train_input.hip), shared by the CPU and GPU tests.  Expected values come from tests/exact_quad.py only.

    families(seed=0, n=24) -> {name: Family(a, b, ca, cb)}   a, b (n,7) fp32 boxes [x y z h w l ry]; ca, cb (n,8,3) corners
                                                              (train_input_twin.corners3d); pair i is (a[i], b[i])
    exact(seed=0, n=24)    -> {name: [(iou3d, iou_bev) Fraction per pair]}, cached
    check_liveness(...)                                       the conditions that keep the tests from passing vacuously
    parking_scene(...)                                        an axis-aligned lattice for the sampler (see there)

Geometry: a box's length axis in (x, z) is (cos ry, -sin ry), its width axis (sin ry, cos ry).  Every family but the parking rows
comes twice: "near" (|x| < 3, z in 4..10) and "far", KITTI's far corner (|x| about 38, z about 68), where one fp32 ulp of a
coordinate is 4-8 um and the sliver of a pair that touches up to rounding has an IoU around 1e-7: above the sampler's 1e-8.
Widths and lengths are multiples of 2^-10 m and >= 1 m (except thin / zero-width), so w - 0.5 and l - 0.5 are exact and the
sampler's + 0.5 enlargement gives the family's box back bit for bit (sampler_boxes).
"""
from collections import namedtuple
from fractions import Fraction
from functools import lru_cache

import numpy as np

import exact_quad as xq
import train_input_twin as tw

Family = namedtuple("Family", "a b ca cb")
F32 = np.float32
TOUCHING = ("touch_length", "touch_width", "corner_contact", "same_heading", "near_contact")      # collinear edges: the shortcut's hard cases


def _q(v):
    """round to a multiple of 2^-10"""
    return (np.round(np.asarray(v) * 1024) / 1024).astype(F32)


def _base(n, rng, far):
    b = np.zeros((n, 7), F32)
    if far:
        b[:, 0] = rng.uniform(36.5, 38.5, n) * rng.choice([-1.0, 1.0], n)
        b[:, 2] = rng.uniform(66.0, 69.0, n)
    else:
        b[:, 0] = rng.uniform(-3, 3, n)
        b[:, 2] = rng.uniform(4, 10, n)
    b[:, 1] = rng.uniform(1.4, 1.9, n)
    b[:, 3] = rng.uniform(1.3, 2.0, n)
    b[:, 4] = _q(rng.uniform(1.0, 2.5, n))
    b[:, 5] = _q(rng.uniform(2.0, 5.0, n))
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def _shift(b, along, across):
    """move each box by `along` metres on its length axis and `across` on its width axis, in fp32 like a data pipeline would"""
    out = b.copy()
    cs, sn = np.cos(b[:, 6]), np.sin(b[:, 6])
    along, across = np.asarray(along, F32), np.asarray(across, F32)
    out[:, 0] = b[:, 0] + (along * cs + across * sn)
    out[:, 2] = b[:, 2] + (across * cs - along * sn)
    return out


def _make(a, b, ca=None, cb=None):
    a, b = a.astype(F32), b.astype(F32)
    return Family(a, b, tw.corners3d(a) if ca is None else ca, tw.corners3d(b) if cb is None else cb)


def _place(n, rng, far):
    a = _base(n, rng, far)
    sign = rng.choice([-1.0, 1.0], n).astype(F32)
    fam = {}
    b = _base(n, rng, far)
    b[:, [0, 2]] = a[:, [0, 2]] + rng.uniform(-1.5, 1.5, (n, 2)).astype(F32)
    fam["random"] = _make(a, b)
    fam["same_heading"] = _make(a, _shift(a, sign * rng.uniform(0.2, 1.5, n).astype(F32) * a[:, 5], 0))
    fam["touch_length"] = _make(a, _shift(a, sign * a[:, 5], 0))
    fam["touch_width"] = _make(a, _shift(a, 0, sign * a[:, 4]))
    fam["identical"] = _make(a, a.copy())
    b = a.copy()
    b[:, 4:6] = _q(a[:, 4:6] * 0.5)
    b[:, 1] -= F32(0.2)
    fam["nested"] = _make(a, b)
    for name, turn in (("turn_90", F32(np.pi / 2)), ("turn_180", F32(np.pi))):
        b = a.copy()
        b[:, 6] = a[:, 6] + turn
        fam[name] = _make(a, b)
    fam["corner_contact"] = _make(a, _shift(a, sign * a[:, 5], rng.choice([-1.0, 1.0], n).astype(F32) * a[:, 4]))
    d = (10.0 ** rng.uniform(-3, -1, n) * rng.choice([-1.0, 1.0], n)).astype(F32)      # 1 mm .. 10 cm of overlap (+) or of gap (-)
    lengthwise = np.arange(n) % 2 == 0
    fam["near_contact"] = _make(a, _shift(a, np.where(lengthwise, sign * (a[:, 5] - d), 0), np.where(lengthwise, 0, sign * (a[:, 4] - d))))
    t = a.copy()
    t[:, 4] = F32(0.05)
    b = _shift(t, rng.uniform(0, 1, n).astype(F32) * t[:, 5], rng.uniform(-1, 1, n).astype(F32) * F32(0.05))
    b[: n // 2, 6] += rng.uniform(-0.02, 0.02, n // 2).astype(F32)
    fam["thin"] = _make(t, b)
    flat = a.copy()
    flat[:, 4] = 0                                               # rotated zero-width boxes ...
    cb = tw.corners3d(flat)
    cb[n // 2:] = tw.corners3d(a)[n // 2:][:, [0, 2, 1, 3, 4, 6, 5, 7]]       # ... and bow-tie corner orders
    fam["degenerate"] = _make(a, flat, cb=cb)
    return fam


def _parking(n, rng):
    """ry = 0 exactly, w = 2.0, l = 4.0 (1.5 and 3.5 after sampler_boxes) on a lattice of pitch 4.0 in x and 2.0 in z: neighbours
    share an edge or a corner exactly; every other pair has the neighbour moved inward by 2^-10 m"""
    a = np.zeros((n, 7), F32)
    a[:, 0] = 4.0 * rng.integers(-8, 9, n)
    a[:, 2] = 2.0 * rng.integers(3, 30, n)
    a[:, 1], a[:, 3], a[:, 4], a[:, 5] = 1.65, 1.5, 2.0, 4.0
    b = a.copy()
    step = np.array([(4.0, 0.0), (-4.0, 0.0), (0.0, 2.0), (0.0, -2.0), (4.0, 2.0), (-4.0, -2.0)], F32)[np.arange(n) % 6]
    inward = np.where(np.arange(n) % 2 == 1, F32(2.0 ** -10), F32(0))[:, None] * np.sign(step)
    b[:, [0, 2]] = a[:, [0, 2]] + (step - inward)
    return _make(a, b)


def families(seed=0, n=24):
    rng = np.random.default_rng(seed)
    out = {}
    for far in (False, True):
        for k, v in _place(n, rng, far).items():
            out[("far_" if far else "near_") + k] = v
    out["parking_rows"] = _parking(n, rng)
    return out


def sampler_boxes(boxes):
    """the boxes whose + 0.5 enlargement (w and l) is `boxes`, exactly"""
    b = np.asarray(boxes, F32).copy()
    b[:, 4:6] -= F32(0.5)
    assert np.array_equal(b[:, 4:6] + F32(0.5), np.asarray(boxes, F32)[:, 4:6]) and (b[:, 4:6] > 0).all()
    return b


@lru_cache(maxsize=None)
def exact(seed=0, n=24):
    return {k: [xq.exact_iou(f.ca[i], f.cb[i]) for i in range(len(f.ca))] for k, f in families(seed, n).items()}


@lru_cache(maxsize=None)
def check_liveness(seed=0, n=24):
    """every family has >= 10 pairs; over all pairs >= 25 % have exact IoU > 0, >= 15 % have exact IoU == 0 with the bottoms closer
    than 1 mm, and >= 20 pairs have exact IoU in (0, 1e-6).  Returns the three counts and the total."""
    fams, ex = families(seed, n), exact(seed, n)
    total = pos = close = sliver = 0
    for k, f in fams.items():
        assert len(f.a) >= 10 and len(f.a) == len(f.b) == len(f.ca) == len(f.cb), k
        for i, (v, _) in enumerate(ex[k]):
            total += 1
            pos += v > 0
            sliver += 0 < v < Fraction(1, 10 ** 6)
            close += v == 0 and xq.quad_gap(f.ca[i], f.cb[i]) < 1e-3
    assert pos >= 0.25 * total, (pos, total)
    assert close >= 0.15 * total, (close, total)
    assert sliver >= 20, sliver
    return pos, close, sliver, total


def parking_scene(seed, n_scene, n_db, cols=13, rows=30):
    """A car park for the sampler, ry = 0 everywhere so that no cosine is involved: slots on a lattice of pitch 4.0 (x) by 2.0 (z),
    boxes w = 1.5, l = 3.5 (2.0 by 4.0 once enlarged), so boxes in neighbouring slots touch exactly.  n_scene distinct slots hold
    the scene's boxes; the database holds n_db candidates, each on a slot (occupied or free) and every second one moved by 2^-10 m
    towards one of its four neighbours.  A candidate on a free slot whose neighbours it only touches must be accepted; one moved
    into an occupied neighbour, or on an occupied slot, must be rejected.  -> (scene (n_scene,7), db (n_db,7)) fp32"""
    rng = np.random.default_rng(seed)
    slots = np.array([(4.0 * (i - cols // 2), 2.0 * (j + 3)) for i in range(cols) for j in range(rows)], F32)

    def boxes(xz):
        b = np.zeros((len(xz), 7), F32)
        b[:, [0, 2]] = xz
        b[:, 1], b[:, 3], b[:, 4], b[:, 5] = 1.65, 1.5, 1.5, 3.5
        return b

    scene = boxes(slots[rng.permutation(len(slots))[:n_scene]])
    xz = slots[rng.integers(0, len(slots), n_db)].copy()
    nudge = np.array([(1, 0), (-1, 0), (0, 1), (0, -1)], F32)[rng.integers(0, 4, n_db)] * F32(2.0 ** -10)
    xz[1::2] += nudge[1::2]
    return scene, boxes(xz)


def rows_scene(seed, frames=4, n_db=300, rows=9, per_row=4, length=24.0, theta=None):
    """Crowded same-heading rows reaching KITTI's far corner, for the sampler.  All boxes are 1.6 x 3.9 (2.1 x 4.4 enlarged) with
    one heading theta (every second database box turned by fp32(pi): the same row, facing the other way).  Rows are 2.3 m apart;
    the even rows hold per_row scene boxes each at random places along the row, the odd rows are free.  Database candidates sit
    on any row, up to 8 cm off its centre line, anywhere along it: those on a scene row nearly always collide, those on a free row
    fit until the row fills up.  The region is a length x (rows * 2.3) rectangle centred at (26, 56) turned by theta, so it reaches
    x = 38, z = 68.  -> (scenes [frames x (G,7)], db (n_db,7), theta)"""
    rng = np.random.default_rng(seed)
    theta = F32(rng.uniform(0.3, 1.2) if theta is None else theta)
    pitch = 2.3

    def boxes(along, row, jitter, turned):
        b = np.zeros((len(along), 7), F32)
        b[:, 0], b[:, 2] = 26.0, 56.0
        b[:, 1], b[:, 3], b[:, 4], b[:, 5], b[:, 6] = 1.65, 1.5, 1.6, 3.9, theta
        b = _shift(b, np.asarray(along, F32) - F32(length / 2), (np.asarray(row, F32) - F32((rows - 1) / 2)) * F32(pitch) + jitter)
        b[:, 6] = np.where(turned, theta + F32(np.pi), theta)
        return b

    scenes = []
    for _ in range(frames):
        along, row = [], []
        for r in range(0, rows, 2):
            free = length - per_row * 4.4 - (per_row - 1) * 0.2              # slack to hand out as random extra gaps
            cuts = np.sort(rng.uniform(0, free, per_row))
            along += [2.2 + k * 4.6 + cuts[k] for k in range(per_row)]
            row += [r] * per_row
        scenes.append(boxes(along, row, 0, np.zeros(len(along), bool)))
    db = boxes(rng.uniform(2.2, length - 2.2, n_db), rng.integers(0, rows, n_db), rng.uniform(-0.08, 0.08, n_db).astype(F32),
               np.arange(n_db) % 2 == 1)
    return scenes, db, theta


def capacity_scene(seed, at, n_scene=192):
    """n_scene parked boxes (parking_scene's lattice, ry = 0) around one free slot whose +x neighbour is the scene box at list
    index `at`; every other neighbour of the free slot that is occupied only touches it.  -> (scene (n_scene,7), free (7,): the box
    that fits the free slot exactly, nudged (7,): the same moved 2^-10 m into the neighbour, free_slots (m,7): boxes for the other
    free slots of the lattice)"""
    rng = np.random.default_rng(seed)
    cols, rows = 13, 30
    slots = [(4.0 * (i - cols // 2), 2.0 * (j + 3)) for i in range(cols) for j in range(rows)]
    hole = slots[5 * rows + 12]
    neighbour = slots[6 * rows + 12]
    rest = [s for s in slots if s not in (hole, neighbour)]
    order = rng.permutation(len(rest))
    chosen = [rest[k] for k in order[:n_scene - 1]]
    chosen.insert(at, neighbour)

    def boxes(xz):
        b = np.zeros((len(xz), 7), F32)
        b[:, [0, 2]] = np.asarray(xz, F32).reshape(-1, 2)
        b[:, 1], b[:, 3], b[:, 4], b[:, 5] = 1.65, 1.5, 1.5, 3.5
        return b

    free = boxes([hole])[0]
    nudged = free.copy()
    nudged[0] += F32(2.0 ** -10)
    return boxes(chosen), free, nudged, boxes([rest[k] for k in order[n_scene - 1:]])
