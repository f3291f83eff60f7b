"""Synthetic frames for the RCNN offline sampler tests: labels are cars on the ground, RoIs are copies of them moved along the
label's own length axis by a fraction f of its length -- the IoU of such a pair is about (1 - f) / (1 + f) -- or put far away.

    near    f in [0, 0.1)      IoU >= 0.8: over the foreground threshold
    hard    f in [0.45, 0.8)   IoU in (0.1, 0.4): hard background, [CLS_BG_THRESH_LO, CLS_BG_THRESH)
    graze   f in [0.93, 0.97)  IoU in (0.01, 0.04): easy background with a positive IoU
    far     8 .. 20 m away     IoU 0

What every case is for, and the counts the twin must report for it, is in CASES; tests/test_rcnn_offline_cpu.py holds the twin to
those counts, so a case cannot silently stop being the case it is named after."""
import numpy as np

F32 = np.float32


def labels(rng, g):
    gt = np.empty((g, 7), F32)
    gt[:, 0] = (np.arange(g) % 6) * 9.0 - 22.0 + rng.uniform(-1, 1, g)
    gt[:, 1] = 1.6 + rng.uniform(-0.1, 0.1, g)
    gt[:, 2] = 8.0 + (np.arange(g) // 6) * 12.0 + rng.uniform(-1, 1, g)
    gt[:, 3] = rng.uniform(1.4, 1.7, g)
    gt[:, 4] = rng.uniform(1.5, 1.8, g)
    gt[:, 5] = rng.uniform(3.5, 4.3, g)
    gt[:, 6] = rng.uniform(-np.pi, np.pi, g)
    return gt


def moved(rng, box, kind):
    b = box.astype(np.float64)
    if kind == "far":
        b[0] += rng.uniform(8, 20) * rng.choice([-1, 1])
        b[2] += 40.0 + rng.uniform(0, 20)
        return b.astype(F32)
    lo, hi = {"near": (0.0, 0.1), "hard": (0.45, 0.8), "graze": (0.93, 0.97)}[kind]
    s = rng.uniform(lo, hi) * b[5] * rng.choice([-1, 1])
    b[0] += np.cos(b[6]) * s
    b[2] -= np.sin(b[6]) * s
    if kind == "near":
        b[3:6] *= rng.uniform(0.98, 1.02, 3)
        b[6] += rng.uniform(-0.03, 0.03)
    return b.astype(F32)


def frame(seed, m, g, kinds):
    """m RoIs over g labels: RoI i copies label i % g with kind kinds[(i // g) % len(kinds)] (every label meets every kind first)"""
    rng = np.random.default_rng(seed)
    gt = labels(rng, g)
    roi = np.stack([moved(rng, gt[i % g], kinds[(i // g) % len(kinds)]) for i in range(m)])
    return roi, gt


def shared_best():
    """one RoI over the threshold for two labels and the best RoI of both: three places in the foreground list"""
    rng = np.random.default_rng(77)
    gt = labels(rng, 2)
    gt[1] = gt[0]
    gt[1, 0] += F32(0.2)
    best = gt[0].copy()
    best[0] += F32(0.1)
    roi = np.stack([moved(rng, gt[0], "far"), best, moved(rng, gt[0], "hard"), moved(rng, gt[1], "far"), moved(rng, gt[1], "graze")])
    return roi, gt


def twins():
    """two identical RoIs, both the best of label 0: the first one stands for the label"""
    roi, gt = frame(78, 12, 3, ("hard", "far"))
    for i in (3, 6, 9):
        roi[i] = roi[0]
    return roi, gt


# name -> (builder, R, expected): expected holds status and any of nfg, nhard, neasy, fs the case is about (None: any positive number)
CASES = {
    "all three lists": (lambda: frame(1, 96, 5, ("near", "hard", "far", "graze")), 16, dict(status=0, fs=8)),
    "M 300 G 17": (lambda: frame(2, 300, 17, ("near", "hard", "far", "graze")), 16, dict(status=0, fs=8)),
    "assignment entries only": (lambda: frame(3, 40, 5, ("hard", "far")), 16, dict(status=0, nfg=5, fs=5)),
    "no foreground": (lambda: frame(4, 40, 5, ("far",)), 16, dict(status=0, nfg=0, nhard=0, neasy=40, fs=0)),
    "hard background only": (lambda: frame(5, 40, 5, ("hard",)), 16, dict(status=0, nfg=5, nhard=40, neasy=0, fs=5)),
    "easy background only": (lambda: frame(6, 40, 5, ("graze", "far")), 16, dict(status=0, nfg=5, nhard=0, neasy=40, fs=5)),
    "foreground only": (lambda: frame(7, 20, 5, ("near",)), 16, dict(status=1, nhard=0, neasy=0, fs=0)),
    "M 2 G 1": (lambda: frame(8, 2, 1, ("near", "far")), 16, dict(status=0, nfg=2, neasy=1, fs=2)),
    "shared best": (shared_best, 16, dict(status=0, nfg=3, fs=3)),
    "identical RoIs": (twins, 16, dict(status=0, nfg=3, fs=3)),
    "odd quota": (lambda: frame(9, 33, 4, ("near", "hard", "far")), 7, dict(status=0, fs=4)),
}


def box_line(b, score=None, cls="Car"):
    line = "%s 0.00 0 0.00 100.00 150.00 300.00 250.00 %.4f %.4f %.4f %.4f %.4f %.4f %.4f" % (cls, b[3], b[4], b[5], b[0], b[1], b[2], b[6])
    return line if score is None else line + " %.4f" % score


def label_text(gt):
    """a frame's label_2 lines: its labels between objects that filtrate_objects drops -- DontCare, another class, a Car outside
    PC_AREA_SCOPE"""
    return (["DontCare -1 -1 -10 500.00 160.00 520.00 180.00 -1 -1 -1 -1000 -1000 -1000 -10"] + [box_line(b) for b in gt] +
            ["Pedestrian 0.00 0 0.10 100.00 150.00 300.00 250.00 1.70 0.60 0.80 3.00 1.60 12.00 0.30",
             box_line([55.0, 1.6, 20.0, 1.5, 1.6, 3.9, 0.2])])


def roi_text(roi):
    return [box_line(b, 1.0 - 0.001 * i) for i, b in enumerate(roi)]


N_POINTS, N_CHANNELS, S_POINTS = 2048, 8, 64


def frame_points(k, gt, n=None, c=None):
    """the RPN dumps of fixture frame k: nine points in ten scattered about the labels (a label's enlarged box holds more than
    S_POINTS), the rest spread over the whole scene (an RoI far from every label holds a few or none); features are small integers"""
    rng = np.random.default_rng(1000 + k)
    n, c = n or N_POINTS, c or N_CHANNELS
    ctr = gt[rng.integers(0, len(gt), n)][:, :3]
    xyz = ctr + rng.normal(0, 1, (n, 3)) * [1.8, 0.6, 1.8] - [0, 0.8, 0]
    far = rng.random(n) < 0.1
    xyz[far] = rng.uniform([-45, 0, 0], [45, 2, 110], (int(far.sum()), 3))
    idx = np.arange(n)
    return dict(rpn_xyz=xyz.astype(F32), rpn_features=((idx[:, None] * 7 + np.arange(c) * 13) % 251).astype(F32),
                rpn_intensity=((idx * 5) % 64 / 64.0).astype(F32), seg_mask=(rng.random(n) > 0.5).astype(F32),
                rawscore=rng.normal(0, 2, n).astype(F32))


def frame_config(k):
    """(AUG_DATA, USE_INTENSITY) of fixture frame k: both on and off, in every combination"""
    return k % 3 != 1, k % 2 == 1


SEED = 20260112
METHOD = {"all three lists": "multiple", "M 300 G 17": "single", "shared best": "single", "odd quota": "single"}      # others: 'multiple'
_twin = {}


def twin_result(name, frame_id):
    """rcnn_offline_twin.sample_frame of one case under the tests' seed, computed once per process"""
    import rcnn_offline_twin as ot
    key = (name, frame_id)
    if key not in _twin:
        roi, gt = CASES[name][0]()
        _twin[key] = ot.sample_frame(roi, gt, SEED, frame_id, dict(ROI_PER_IMAGE=CASES[name][1], REG_AUG_METHOD=METHOD.get(name, "multiple")))
    return _twin[key]


def batch(names, pad_m=0, pad_g=0):
    """-> roi (B, M, 7), num_roi (B), gt (B, G, 7), num_gt (B) padded with rows of NaN (the kernel must not read past the counts)"""
    frames = [CASES[n][0]() for n in names]
    M = max(len(r) for r, _ in frames) + pad_m
    G = max(len(g) for _, g in frames) + pad_g
    roi = np.full((len(frames), M, 7), np.nan, F32)
    gt = np.full((len(frames), G, 7), np.nan, F32)
    for b, (r, g) in enumerate(frames):
        roi[b, :len(r)] = r
        gt[b, :len(g)] = g
    return roi, np.array([len(r) for r, _ in frames], np.int32), gt, np.array([len(g) for _, g in frames], np.int32)
