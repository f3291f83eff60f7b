"""Seeded inputs for the KITTI evaluator kernels at the backend interface (`backend.statistics`, `backend.overlaps`): crowded
frames (more than 64 detections, so the matching kernel's bitmaps leave word 0), contended matches with exact ties, every
ignore-code combination, DontCare edges, empty and ragged shapes, AOS sums, degenerate box pairs.  Shared by the fixture
generator (tests/golden/make_kitti_stats_golden.py), the CPU test and the GPU test; inputs are regenerated from the seeds here
and the fixture records their CRC.

A frame is a dict: ov (nd, ng) overlaps, rows = detections; gt (ng, 5) [bbox, alpha]; dt (nd, 6) [bbox, alpha, score];
ign_gt (ng), ign_det (nd); dc (ndc, 4).  `pack` concatenates frames into the first ten arguments of `backend.statistics`.
A case is a dict: name, frames, args, thresholds, settings = [(metric, min_overlap, compute_aos)].
"""
import functools
import zlib

import numpy as np

OVS = np.array([0.0, 0.3, 0.5, 0.55, 0.7, 0.71, 0.9])          # min_overlap is 0.5 or 0.7: exact ties and equality are common
SCORES = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9])
# 0, grid values (a score equals the threshold), just above a grid value, above every score
THRESHOLDS = np.array([0.0, SCORES[2], SCORES[4], 0.5000001, SCORES[7], 0.95])
KS_MAX_DET = 1024
SETTINGS = [(0, 0.5, True), (0, 0.7, True), (1, 0.5, False), (2, 0.7, False)]


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.uint32(c)


def det_bbox(j):
    """detection j's 2-D box: a 10 x 10 square on a 40-pixel lattice, so no two detections' boxes touch"""
    x, y = 40.0 * (j % 32), 40.0 * (j // 32)
    return np.array([x, y, x + 10.0, y + 10.0])


def dc_over(j, q):
    """a DontCare box that covers the fraction q of detection j's box (q * 10 pixels of its width, its whole height)"""
    b = det_bbox(j)
    return np.array([b[0] + 10.0 * (1.0 - q), b[1], b[0] + 20.0, b[3]])


def dc_span(j0, j1):
    """a DontCare box that contains the boxes of detections j0..j1 of one lattice row"""
    a, b = det_bbox(j0), det_bbox(j1)
    return np.array([a[0] - 1.0, a[1] - 1.0, b[2] + 1.0, b[3] + 1.0])


def frame(ov, scores, ign_gt=None, ign_det=None, dc=(), gt_alpha=None, dt_alpha=None):
    ov = np.asarray(ov, np.float64)
    nd, ng = ov.shape
    gt = np.zeros((ng, 5))
    gt[:, 4] = 0.0 if gt_alpha is None else gt_alpha
    dt = np.zeros((nd, 6))
    if nd:
        dt[:, :4] = np.stack([det_bbox(j) for j in range(nd)])
    dt[:, 4] = 0.0 if dt_alpha is None else dt_alpha
    dt[:, 5] = scores
    return dict(ov=ov, gt=gt, dt=dt, ign_gt=np.zeros(ng, np.int32) if ign_gt is None else np.asarray(ign_gt, np.int32),
                ign_det=np.zeros(nd, np.int32) if ign_det is None else np.asarray(ign_det, np.int32),
                dc=np.asarray(dc, np.float64).reshape(-1, 4))


def off(counts):
    o = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=o[1:])
    return o


def pack(frames):
    """-> (overlaps, ov_off, gt_datas, gt_off, dt_datas, dt_off, ign_gt, ign_det, dc, dc_off)"""
    cat = lambda k, w: np.concatenate([f[k].reshape(-1, w) if w else f[k].reshape(-1) for f in frames])      # noqa: E731
    return (cat("ov", 0), off([f["ov"].size for f in frames]), cat("gt", 5), off([len(f["gt"]) for f in frames]),
            cat("dt", 6), off([len(f["dt"]) for f in frames]), cat("ign_gt", 0), cat("ign_det", 0), cat("dc", 4),
            off([len(f["dc"]) for f in frames]))


def case(name, frames, thresholds=THRESHOLDS, settings=SETTINGS):
    return dict(name=name, frames=frames, args=pack(frames), thresholds=np.asarray(thresholds, np.float64), settings=settings)


def case_crc(c):
    return crc(*c["args"], c["thresholds"], np.array([s[:2] for s in c["settings"]], np.float64))


def permuted(frames, order):
    return [frames[i] for i in order]


def random_frame(r, nd, ng, density=None):
    """random fill: overlaps from OVS (a share `density` of a ground truth's column is non-zero), scores from the grid,
    ignore codes mostly 0, a few DontCare boxes over random detections"""
    dens = r.choice([min(1.0, 3.0 / max(nd, 1)), 0.05, 0.5], ng) if density is None else np.full(ng, density)
    ov = np.where(r.random((nd, ng)) < dens[None, :], r.choice(OVS[1:], (nd, ng)), 0.0)
    dc = [dc_over(int(j), float(q)) for j, q in zip(r.integers(0, max(nd, 1), min(nd, 6)), r.choice([1.0, 0.5, 0.7, 0.71, 0.3], min(nd, 6)))]
    return frame(ov, r.choice(SCORES, nd), r.choice([0, 0, 0, 1, -1], ng), r.choice([0, 0, 0, 0, 1, -1], nd), dc,
                 r.uniform(-np.pi, np.pi, ng), r.uniform(-np.pi, np.pi, nd))


# ----------------------------------------------------------------------------------------------------------------
# families
# ----------------------------------------------------------------------------------------------------------------
def words_family():
    """frames of 63 .. 1024 detections; at the detection indices 63, 64, 127, 128, 1023 (and the last one) a planted detection
    wins, is ignored by the threshold, is too small (ign_det 1), or belongs to another class (ign_det -1); the four frames of
    1024 detections rotate those roles, so that index 1023 plays each of them"""
    r = np.random.default_rng(101)
    frames = []
    for nd, ng, shift in ((63, 6, 0), (64, 8, 0), (65, 12, 0), (128, 16, 0), (129, 24, 0), (1023, 40, 0),
                          (1024, 40, 0), (1024, 40, 1), (1024, 40, 2), (1024, 40, 3)):
        f = random_frame(r, nd, ng)
        planted = sorted({p for p in (63, 64, 127, 128, 1023, nd - 1) if p < nd})
        used = set(planted)
        ov, sc, ign_gt, ign_det = f["ov"], f["dt"][:, 5], f["ign_gt"], f["ign_det"]
        for n, p in enumerate(planted):
            g = 2 * n                            # two ground-truth columns per planted index
            # the fallback detection: the same bit in another word of the bitmaps where the frame has one
            lo = next(q for q in list(range(p % 64, nd, 64)) + list(range(nd)) if q not in used)
            used.add(lo)
            ov[p, :], ov[lo, :] = 0.0, 0.0
            ov[:, g], ov[:, g + 1] = 0.0, 0.0
            ign_gt[g], ign_gt[g + 1] = 0, 0
            ign_det[lo], sc[lo] = 0, SCORES[8]
            kind = (n + nd + shift) % 4
            # column g: p is the better candidate, lo the fallback (none when p simply wins);
            # column g + 1: only p again -- a miss when column g took p, a match when it took lo
            ov[p, g], ov[lo, g], ov[p, g + 1] = 0.9, 0.7 if kind else 0.0, 0.71
            ign_det[p], sc[p] = ((0, SCORES[8]), (0, SCORES[3]), (1, SCORES[8]), (-1, SCORES[8]))[kind]
        top = 32 * ((nd - 1) // 32)              # DontCare over the last lattice row: the DontCare loop sets the highest bits
        f["dc"] = np.concatenate([f["dc"], dc_span(top, nd - 1)[None], dc_over(nd - 1, 0.5)[None]])
        frames.append(f)
    return [case("words", frames, settings=[(0, 0.5, True), (0, 0.7, True), (1, 0.7, False)])]


def contention_family():
    """up to 6 detections on one ground truth, up to 4 ground truths sharing one detection, dense overlaps from OVS so that
    equal overlaps and equal scores are frequent; every frame also with both index orders reversed"""
    r = np.random.default_rng(102)
    frames = [frame([[0.7], [0.7]], [0.5, 0.5]), frame([[0.9], [0.9], [0.9]], [0.3, 0.5, 0.5]),
              frame([[0.7, 0.7, 0.7, 0.7]], [0.5]), frame([[0.9, 0.71], [0.9, 0.9]], [0.5, 0.5])]
    for n in range(40):
        nd, ng = int(r.integers(1, 7)), int(r.integers(1, 5))
        f = random_frame(r, nd, ng, density=0.8)
        if n % 2:
            f["ign_gt"][:], f["ign_det"][:] = 0, 0
        frames.append(f)
    for f in list(frames):
        g = frame(f["ov"][::-1, ::-1], f["dt"][::-1, 5], f["ign_gt"][::-1], f["ign_det"][::-1], f["dc"], f["gt"][::-1, 4], f["dt"][::-1, 4])
        g["dt"][:, :4] = f["dt"][::-1, :4]       # the boxes travel with their detections, so the DontCare boxes still fit
        frames.append(g)
    return [case("contention", frames)]


def ignore_family():
    """all nine (ign_gt, ign_det) combinations on a contended ground truth, followed by a counted ground truth that sees what
    was left over; frames whose ground truths are all -1 or all 1"""
    r = np.random.default_rng(103)
    frames = []
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            for ov0, ov1 in ((0.9, 0.7), (0.7, 0.9), (0.7, 0.7)):
                for codes in ((b, 0), (0, b), (b, b)):
                    frames.append(frame([[ov0, 0.71], [ov1, 0.55], [0.55, 0.0]], [0.5, 0.7, 0.9], [a, 0], codes + (0,)))
    for code in (-1, 1):
        for nd in (0, 3, 70):
            f = random_frame(r, nd, 4, density=0.6)
            f["ign_gt"][:] = code
            frames.append(f)
    # `|| assigned_ignored` in the counted branch decides only where a counted detection's overlap does not exceed max_overlap
    # == 0 and still passes min_overlap, that is for min_overlap < 0: outside the protocol, but defined alike by the reference,
    # the oracle and the kernel, and the only input on which dropping that term shows
    zero = [frame([[0.0], [0.0]], [0.5, 0.7], ign_det=[1, 0]), frame([[0.0], [0.0]], [0.5, 0.7], ign_det=[0, 1]),
            frame([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]], [0.5, 0.7, 0.9], ign_det=[1, 0, 1])]
    return [case("ignore_codes", frames), case("ignored_then_counted_at_zero_overlap", zero, settings=[(0, -0.5, True), (1, -0.5, False)])]


def dontcare_family():
    """detections inside no, one or two DontCare regions; coverage exactly min_overlap; an assigned detection, a too-small one
    and a low-scoring one inside a region; the same frames at metrics 0, 1 and 2"""
    frames = []
    ov = np.zeros((8, 2))
    ov[0, 0] = 0.9                               # detection 0 matches ground truth 0, the rest are false positives
    scores = [0.9, 0.9, 0.9, 0.9, 0.9, 0.2, 0.9, 0.9]
    ign_det = [0, 0, 0, 0, 0, 0, 1, -1]
    dcs = [dc_over(0, 1.0),                      # over the assigned detection
           dc_over(2, 1.0), dc_span(2, 2),       # detection 2 lies in two regions
           dc_over(3, 0.5), dc_over(4, 0.7),     # exactly min_overlap at 0.5 / at 0.7
           dc_over(5, 1.0), dc_over(6, 1.0), dc_over(7, 1.0)]
    frames.append(frame(ov, scores, [0, 0], ign_det, dcs))
    frames.append(frame(ov, scores, [0, 0], ign_det, dcs[::-1]))
    frames.append(frame(ov, scores, [0, 0], ign_det, [dc_span(0, 7)]))
    frames.append(frame(ov, scores, [0, 0], ign_det, [dc_over(1, 0.71), dc_over(1, 0.55), dc_over(3, 0.3), dc_over(3, 0.3)]))
    frames.append(frame(ov, scores, [0, 0], ign_det, []))
    frames.append(frame(np.zeros((3, 0)), [0.5, 0.5, 0.5], dc=[dc_span(0, 1)]))
    return [case("dontcare", frames, settings=[(0, 0.5, True), (0, 0.7, True), (1, 0.5, False), (1, 0.5, True), (2, 0.5, False)])]


def shapes_family():
    """nd == 0, ng == 0, both; F == 1 with T == 1 and T == 41; F * T no multiple of 64; neighbouring frames of 0, 1024, 1 and 65
    detections, so that the lanes of one wave do different amounts of work"""
    r = np.random.default_rng(105)
    ragged = [random_frame(r, nd, ng) for nd, ng in ((0, 3), (1024, 5), (1, 2), (65, 7), (0, 0), (4, 0), (5, 3))]
    one = [random_frame(r, 9, 4, density=0.5)]
    t41 = np.concatenate([[0.0], np.sort(r.choice(np.concatenate([SCORES, SCORES + 1e-7, SCORES - 0.05, SCORES + 0.03, SCORES - 0.02]), 39, replace=False)), [0.95]])
    sets = [(0, 0.5, True), (2, 0.7, False)]
    return [case("shapes_ragged", ragged, settings=sets), case("shapes_f1_t1", one, [SCORES[4]], sets),
            case("shapes_f1_t41", one, t41, sets), case("shapes_all_empty", [random_frame(r, 0, 0), random_frame(r, 0, 0)], settings=sets)]


def aos_family():
    """up to 40 true positives in a frame, alpha differences beyond +-pi, frames that end with similarity == -1"""
    r = np.random.default_rng(106)
    frames = []
    for ntp, extra in ((40, 8), (17, 0), (1, 3)):
        nd = ntp + extra
        ov = np.zeros((nd, ntp))
        ov[r.permutation(nd)[:ntp], np.arange(ntp)] = r.choice([0.71, 0.9], ntp)
        frames.append(frame(ov, r.choice(SCORES, nd), gt_alpha=r.uniform(-2 * np.pi, 2 * np.pi, ntp), dt_alpha=r.uniform(-2 * np.pi, 2 * np.pi, nd)))
    frames.append(frame([[0.9, 0.9]], [0.9], gt_alpha=[3.0, -3.0], dt_alpha=[-3.0]))           # difference 6 > pi
    frames.append(frame(np.zeros((2, 2)), [0.5, 0.5], [-1, -1], [-1, -1]))                    # nothing counts: -1
    frames.append(frame([[0.9]], [0.5], [1], [0]))                                            # consumed by an ignored gt: -1
    frames.append(frame([[0.9]], [0.5], [0], [1]))                                            # too small: -1
    frames.append(frame(np.zeros((0, 0)), []))                                                # empty: -1
    frames.append(frame(np.zeros((2, 1)), [0.5, 0.5]))                                        # only false positives: 0
    return [case("aos", frames, settings=[(0, 0.5, True), (0, 0.7, True), (1, 0.5, True)])]


@functools.lru_cache(maxsize=None)
def families():
    """name -> case, all families (built once per process; callers do not modify the arrays)"""
    out = {}
    for fam in (words_family, contention_family, ignore_family, dontcare_family, shapes_family, aos_family):
        for c in fam():
            out[c["name"]] = c
    return out


def over_limit_frames():
    """one frame of KS_MAX_DET + 1 detections between two ordinary ones: the call must be refused, not computed"""
    r = np.random.default_rng(107)
    return [random_frame(r, 5, 3), random_frame(r, KS_MAX_DET + 1, 2), random_frame(r, 3, 2)]


# ----------------------------------------------------------------------------------------------------------------
# hand cases: (name, frame, metric, min_overlap, threshold, compute_fp, expected)
# expected = (tp, fp, fn[, similarity]) for compute_fp (run with compute_aos), else the matched scores in ground-truth order
# (NaN = no true positive)
# ----------------------------------------------------------------------------------------------------------------
def hand_cases():
    nan = float("nan")
    two = [[0.6], [0.9]]
    box = np.array([0.0, 0.0, 10.0, 10.0])
    inside_two = frame(np.zeros((1, 1)), [0.9], dc=[[-1, -1, 20, 20], [0, 0, 10, 10]])
    half = frame(np.zeros((1, 1)), [0.9], dc=[[5, 0, 20, 10]])
    assert np.array_equal(inside_two["dt"][0, :4], box)
    return [
        ("pass 1: the larger score wins", frame(two, [0.9, 0.5]), 0, 0.5, 0.0, False, [0.9]),
        ("pass 2: the larger overlap wins", frame(two, [0.9, 0.5]), 0, 0.5, 0.0, True, (1, 1, 0)),
        ("pass 2: ... the one whose alpha is pi: similarity 0, not 1", frame(two, [0.9, 0.5], dt_alpha=[0.0, np.pi]), 0, 0.5, 0.0, True,
         (1, 1, 0, 0.0)),
        ("too small first, counted second", frame([[0.9], [0.6]], [0.5, 0.5], ign_det=[1, 0]), 0, 0.5, 0.0, True, (1, 0, 0)),
        ("counted first, too small second", frame([[0.6], [0.9]], [0.5, 0.5], ign_det=[0, 1]), 0, 0.5, 0.0, True, (1, 0, 0)),
        ("a single too-small detection", frame([[0.9]], [0.5], ign_det=[1]), 0, 0.5, 0.0, True, (0, 0, 0)),
        ("a single too-small detection, pass 1", frame([[0.9]], [0.5], ign_det=[1]), 0, 0.5, 0.0, False, [nan]),
        ("an ignored gt consumes a detection", frame([[0.9], [0.0]], [0.5, 0.5], ign_gt=[1]), 0, 0.5, 0.0, True, (0, 1, 0)),
        ("overlap == min_overlap", frame([[0.5]], [0.5]), 0, 0.5, 0.0, True, (0, 1, 1)),
        ("score == threshold", frame([[0.9]], [0.5]), 0, 0.5, 0.5, True, (1, 0, 0)),
        ("score just under the threshold", frame([[0.9]], [0.5]), 0, 0.5, 0.5000001, True, (0, 0, 1)),
        ("in two DontCare regions, metric 0", inside_two, 0, 0.5, 0.0, True, (0, 0, 1)),
        ("in two DontCare regions, metric 1", inside_two, 1, 0.5, 0.0, True, (0, 1, 1)),
        ("DontCare coverage == min_overlap", half, 0, 0.5, 0.0, True, (0, 1, 1)),
    ]


# ----------------------------------------------------------------------------------------------------------------
# overlap cases: frames of (dt7, gt7, dt_bbox, gt_bbox); 7-boxes are [x, y, z, l, h, w, ry], the rotated rectangle is (x, z, l, w, ry)
# ----------------------------------------------------------------------------------------------------------------
_HP = float(np.float32(np.pi / 2))
PROBES = np.array([                              # cx, cy, dx, dy, angle
    [0, 0, 4, 2, 0],                             # base (against itself: identical boxes)
    [0.5, -0.25, 3, 1.5, 0.75],                  # generic
    [0, 0, 2, 4, _HP],                           # the base rectangle written the other way
    [4, 0, 4, 2, 0],                             # shares a full edge with the base
    [4, 1, 4, 2, 0],                             # shares part of an edge
    [4, 2, 4, 2, 0],                             # touches the base at a corner
    [0, 0, 2, 1, 0],                             # contained, axis-aligned
    [0.25, 0.125, 1, 0.5, 0.25],                 # contained, rotated
    [0, 0, 2, 2, 0],                             # square ...
    [0, 0, 2, 2, _HP / 2],                       # ... and the same square at 45 degrees: eight crossings
    [0, 0, 4, 2, 1e-4],                          # the base turned by 1e-4
    [1, 0.5, 4, 2, -_HP],
    [-1, 0.25, 3, 1.5, float(np.float32(np.pi))],
], np.float64)


def _box7(rect, y=1.5, h=1.5):
    rect = np.asarray(rect, np.float64).reshape(-1, 5)
    n = len(rect)
    return np.stack([rect[:, 0], np.full(n, y), rect[:, 1], rect[:, 2], np.full(n, h), rect[:, 3], rect[:, 4]], 1)


def _bbox(r, n):
    x, y, w, h = r.uniform(0, 1000, n), r.uniform(100, 250, n), r.uniform(20, 200, n), r.uniform(20, 120, n)
    return np.stack([x, y, x + w, y + h], 1)


def _rand7(r, m):
    return np.concatenate([r.uniform(-4, 4, (m, 1)), r.uniform(1, 2, (m, 1)), r.uniform(-4, 4, (m, 1)), r.uniform(1, 4, (m, 1)),
                           r.uniform(1, 2, (m, 1)), r.uniform(1, 4, (m, 1)), r.uniform(-3.2, 3.2, (m, 1))], 1)


def overlap_frames():
    r = np.random.default_rng(108)
    P, n = PROBES, len(PROBES)
    far = P.copy()
    far[:, 0] += 68.5
    far[:, 1] += 70.25
    frames = [(_box7(P), _box7(P), _bbox(r, n), _bbox(r, n)),                     # nd * ng = 169: the stride loop
              (_box7(P), _box7(P[:1]), _bbox(r, n), _bbox(r, 1)),                 # ng == 1
              (_box7(P[:1]), _box7(P[3:9]), _bbox(r, 1), _bbox(r, 6)),            # nd == 1
              (_box7(far[[0, 1, 3, 5, 7, 9, 11]]), _box7(far[[0, 4, 6, 8, 12]]), _bbox(r, 7), _bbox(r, 5)),    # around 70 m
              (_box7(P[:0]), _box7(P[:3]), _bbox(r, 0), _bbox(r, 3)),             # no detections
              (_box7(P[:3]), _box7(P[:0]), _bbox(r, 3), _bbox(r, 0))]             # no ground truth
    # metric 2: gt spans y in [1, 2]; detections stacked under it with height overlap 0, < 0, > 0; full; BEV-disjoint (rinc == 0)
    gt = _box7(P[[0, 1]], y=2.0, h=1.0)
    dt = np.concatenate([_box7(P[[0]], y=1.0, h=1.0), _box7(P[[0]], y=0.5, h=1.0), _box7(P[[1]], y=1.5, h=1.0),
                         _box7(P[[7]], y=2.0, h=1.0), _box7(P[[0]] + [10, 0, 0, 0, 0], y=2.0, h=1.0),
                         _box7(P[[0]], y=3.0, h=1.0), _box7(P[[0]], y=3.5, h=1.0)])
    frames.append((dt, gt, _bbox(r, len(dt)), _bbox(r, 2)))
    # metric 0: iw == 0, ih == 0, disjoint, nested both ways, identical, partial
    gb = np.array([[0, 0, 10, 10], [100, 100, 130, 120.5]], np.float64)
    db = np.array([[10, 0, 20, 10], [0, 10, 10, 20], [10, 10, 20, 20], [50, 50, 60, 60], [2, 2, 8, 8], [-5, -5, 15, 15],
                   [0, 0, 10, 10], [5, 2.5, 12, 30], [90, 110, 100, 130], [110, 120.5, 120, 140], [99, 99, 131, 121]], np.float64)
    frames.append((_box7(r.uniform(-1, 1, (len(db), 5)) + [0, 0, 3, 2, 0]), _box7(r.uniform(-1, 1, (2, 5)) + [0, 0, 3, 2, 0]), db, gb))
    # random frames of ordinary boxes, one of them 9 x 8 (more than one pass of the stride loop with a ragged tail)
    for nd, ng in ((9, 8), (3, 2)):
        frames.append((_rand7(r, nd), _rand7(r, ng), _bbox(r, nd), _bbox(r, ng)))
    return frames


def overlap_args(frames, metric):
    """-> (metric, dt, dt_off, gt, gt_off, ov_off), the arguments of backend.overlaps"""
    k = 2 if metric == 0 else 0
    w = 4 if metric == 0 else 7
    dt = np.concatenate([f[k].reshape(-1, w) for f in frames])
    gt = np.concatenate([f[k + 1].reshape(-1, w) for f in frames])
    nd, ng = np.array([len(f[k]) for f in frames]), np.array([len(f[k + 1]) for f in frames])
    return metric, dt, off(nd), gt, off(ng), off(nd * ng)


def overlap_crc(frames):
    return crc(*[a for f in frames for a in f])


# ----------------------------------------------------------------------------------------------------------------
# a small crowded annotation set for eval_class
# ----------------------------------------------------------------------------------------------------------------
def crowded_annos():
    """12 frames from util.kitti_annos (each the objects of two of its frames); in four of them the detections are cloned with jitter until a frame holds more than
    64 of them (several on one ground truth); some clones are under 25 px high, on top of ground truths; Person_sitting
    ground truths sit under Pedestrian detections (Van under Car comes with kitti_annos); DontCare boxes (sizes kept positive,
    placed far away in 3-D) lie under false positives"""
    from util import kitti_annos
    raw = kitti_annos(24, seed=21)               # two frames' objects per frame: about eight ground truths each
    gt = [{k: np.concatenate([np.asarray(raw[2 * f][k]), np.asarray(raw[2 * f + 1][k])]) for k in raw[0]} for f in range(12)]
    dt = kitti_annos(12, seed=22, with_score=True, gt=gt)
    r = np.random.default_rng(23)
    for f in range(12):
        d, g = dt[f], gt[f]
        d["name"] = np.where(d["name"] == "Person_sitting", "Pedestrian", d["name"])
        n = len(d["name"])
        if n == 0:
            continue
        if f % 3 == 0:                           # crowd: clones of the frame's detections
            src = r.integers(0, n, 66 + 6 * (f // 3))
            clone = {k: np.asarray(v)[src].copy() for k, v in d.items()}
            m = len(src)
            clone["bbox"] = clone["bbox"] + r.normal(0, 2.0, (m, 4))
            clone["location"] = clone["location"] + r.normal(0, 0.1, (m, 3))
            clone["rotation_y"] = clone["rotation_y"] + r.normal(0, 0.05, m)
            clone["alpha"] = clone["alpha"] + r.normal(0, 0.2, m)
            clone["score"] = np.round(r.uniform(0.05, 1.0, m), 1)            # a coarse grid: equal scores are common
            small = r.random(m) < 0.15                                        # under 25 px high, same centre
            cy = (clone["bbox"][:, 1] + clone["bbox"][:, 3]) / 2
            clone["bbox"][small, 1], clone["bbox"][small, 3] = cy[small] - 10.0, cy[small] + 10.0
            dt[f] = d = {k: np.concatenate([np.asarray(d[k]), clone[k]]) for k in d}
        nfp = min(3, len(d["name"]))             # DontCare regions under the last detections (the false positives)
        dc_box = d["bbox"][-nfp:] + np.array([-3.0, -3.0, 3.0, 3.0])
        extra = dict(name=np.array(["DontCare"] * nfp), truncated=np.full(nfp, -1.0), occluded=np.full(nfp, -1), alpha=np.full(nfp, -10.0),
                     bbox=dc_box, dimensions=np.full((nfp, 3), 1.0), location=np.full((nfp, 3), -1000.0), rotation_y=np.full(nfp, -10.0),
                     score=np.zeros(nfp))
        gt[f] = {k: np.concatenate([np.asarray(g[k]), np.asarray(extra[k], dtype=np.asarray(g[k]).dtype if k != "name" else None)])
                 for k in g}
    return gt, dt


# ----------------------------------------------------------------------------------------------------------------
# checks shared by the CPU and the GPU test
# ----------------------------------------------------------------------------------------------------------------
def golden():
    import os
    from util import GOLDEN
    return np.load(os.path.join(GOLDEN, "kitti_stats_ref.npz"))


def run_setting(backend, c, k):
    """both passes of one (metric, min_overlap) setting, as eval_class calls them -> res (F, T, 4), p1res (F, 4), matched (G)"""
    metric, mo, aos = c["settings"][k]
    F, T = len(c["frames"]), len(c["thresholds"])
    p1res, matched = backend.statistics(*c["args"], metric, mo, np.zeros(1), False, False)
    res, _ = backend.statistics(*c["args"], metric, mo, c["thresholds"], True, aos)
    return np.asarray(res).reshape(F, T, 4), np.asarray(p1res).reshape(F, 4), np.asarray(matched)


def frame_names(c):
    return ["%s[%d] nd=%d ng=%d" % (c["name"], i, len(f["dt"]), len(f["gt"])) for i, f in enumerate(c["frames"])]


def check_case(backend, g, c):
    """one case on `backend` against the fixture: counts and matched scores exact, similarity to 1e-9.
    -> the largest similarity difference seen"""
    assert case_crc(c) == g[c["name"] + "_crc"], "seeded inputs of %s drifted from the fixture's" % c["name"]
    gt_off, worst = c["args"][3], 0.0
    for k, (metric, mo, aos) in enumerate(c["settings"]):
        res, p1res, matched = run_setting(backend, c, k)
        pre = "%s_s%d_" % (c["name"], k)
        want = g[pre + "res"]
        for f, name in enumerate(frame_names(c)):
            where = "%s metric %d min_overlap %s" % (name, metric, mo)
            assert np.array_equal(res[f, :, :3], want[f, :, :3]), (where, res[f, :, :3].tolist(), want[f, :, :3].tolist())
            np.testing.assert_allclose(res[f, :, 3], want[f, :, 3], rtol=0, atol=1e-9, equal_nan=True, err_msg=where)
            assert np.array_equal(p1res[f], g[pre + "p1res"][f]), (where, "pass 1", p1res[f], g[pre + "p1res"][f])
        worst = max(worst, float(np.abs(res[..., 3] - want[..., 3]).max(initial=0.0)))
        cnt = g[pre + "p1cnt"]
        thr_off = off(cnt)
        for f, name in enumerate(frame_names(c)):
            m = matched[gt_off[f]:gt_off[f + 1]]
            assert np.array_equal(m[~np.isnan(m)], g[pre + "p1thr"][thr_off[f]:thr_off[f + 1]]), (name, "matched", metric, mo)
    return worst


def check_hand_cases(backend):
    for name, fr, metric, mo, thr, compute_fp, want in hand_cases():
        res, matched = backend.statistics(*pack([fr]), metric, mo, np.array([thr]), compute_fp, compute_fp)
        if compute_fp:
            assert tuple(np.asarray(res).reshape(4)[:3]) == tuple(want[:3]), (name, np.asarray(res).reshape(4))
            assert len(want) == 3 or abs(np.asarray(res).reshape(4)[3] - want[3]) <= 1e-9, (name, res)
        else:
            assert np.array_equal(np.asarray(matched), np.array(want, np.float64), equal_nan=True), (name, matched)


def check_overlaps(backend, g, other=None):
    """backend.overlaps on the overlap frames against the fixture (1e-6 for 2-D boxes, 2e-6 rotated; pairs without a
    reference value: 0 <= IoU <= 1 + 1e-6) and, when `other` is given, bit for bit against that backend"""
    frames = overlap_frames()
    assert overlap_crc(frames) == g["ov_crc"], "seeded overlap inputs drifted from the fixture's"
    flag = g["ov_flag"]
    for metric, atol in ((0, 1e-6), (1, 2e-6), (2, 2e-6)):
        got = np.asarray(backend.overlaps(*overlap_args(frames, metric)))
        want = g["ov_m%d" % metric]
        assert got.shape == want.shape
        keep = np.ones(len(got), bool) if metric == 0 else ~flag
        np.testing.assert_allclose(got[keep], want[keep], rtol=0, atol=atol, err_msg="metric %d" % metric)
        if metric:
            assert ((got[flag] >= 0) & (got[flag] <= 1 + 1e-6)).all(), (metric, got[flag])
        if other is not None:
            assert np.array_equal(got, other.overlaps(*overlap_args(frames, metric))), metric


def check_eval_class(backend, g):
    from kitti_cases import MIN_OVERLAPS, annos_crc
    from pointrcnn_amd import kitti_eval
    gt, dt = crowded_annos()
    assert annos_crc(gt) == g["ec_crc"][0] and annos_crc(dt) == g["ec_crc"][1], "seeded annotations drifted from the fixture's"
    assert sum(len(a["name"]) > 64 for a in dt) >= 3
    for metric in (0, 1, 2):
        r = kitti_eval.eval_class(gt, dt, [0, 1, 2], [0, 1, 2], metric, MIN_OVERLAPS, compute_aos=(metric == 0), backend=backend)
        for k in ("recall", "precision", "orientation"):
            np.testing.assert_allclose(r[k], g["ec_m%d_%s" % (metric, k)], rtol=0, atol=1e-9, equal_nan=True, err_msg="%d %s" % (metric, k))
