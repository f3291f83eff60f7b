"""numpy twins of the RoI pooling's selection (prcnn_roipool3d_index) and of its gradient (prcnn_roipool3d_grad), and the
constructed scene both test files use.  The selection twin is built on the oracle's point-in-box flags (the membership test the
suite already pins); the gradient twins are the closed form  gfeat[b, p, c] = sum_{(m, s): idx[b, m, s] == p} gpooled[b, m, s, col0 + c]
in float64, and in float32 added one addend after the other in ascending (m, s) -- the order the device contract fixes."""
import numpy as np

SCENE_COUNTS = (0, 1, 5, 15, 16, 17, 40)       # points in the seven RoIs of a frame; an eighth RoI repeats the 17-point one
SCENE_S = 16


def index_twin(cpu, xyz, boxes_enlarged, S):
    """xyz (B,N,3), boxes (B,M,7) already enlarged -> idx (B,M,S) i32 (first <= S in-box points, ascending, wrap-copied; -1 in an
    empty RoI), distinct (B,M) i32"""
    xyz, boxes = np.asarray(xyz, np.float32), np.asarray(boxes_enlarged, np.float32)
    B, M = boxes.shape[:2]
    idx = np.full((B, M, S), -1, np.int32)
    distinct = np.zeros((B, M), np.int32)
    for b in range(B):
        flags = cpu.pts_in_boxes3d(xyz[b], boxes[b])                       # (M, N)
        for m in range(M):
            hit = np.nonzero(flags[m])[0][:S]
            distinct[b, m] = len(hit)
            if len(hit):
                idx[b, m] = hit[np.arange(S) % len(hit)]
    return idx, distinct


def gather_twin(xyz, feat, idx):
    """[xyz | feat] rows at idx; zero rows where idx < 0 -> (B,M,S,3+C)"""
    rows = np.concatenate([np.asarray(xyz, np.float32), np.asarray(feat, np.float32)], 2)
    B = rows.shape[0]
    out = np.stack([rows[b][np.maximum(idx[b], 0)] for b in range(B)])
    out[idx < 0] = 0
    return out


def grad_twin(gpooled, idx, N, C, col0=0):
    """float64 closed form -> gfeat (B,N,C) f64, n (B,N) references per point, mag (B,N,C) sum of |addends| (the error bound's scale)"""
    g = np.asarray(gpooled)[..., col0:col0 + C].astype(np.float64)
    B = idx.shape[0]
    out, mag, n = np.zeros((B, N, C)), np.zeros((B, N, C)), np.zeros((B, N), np.int64)
    for b in range(B):
        live = idx[b] >= 0
        np.add.at(out[b], idx[b][live], g[b][live])
        np.add.at(mag[b], idx[b][live], np.abs(g[b][live]))
        np.add.at(n[b], idx[b][live], 1)
    return out, n, mag


def grad_twin_f32_sequential(gpooled, idx, N, C, col0=0):
    """float32, one addition per addend, from zero, in ascending (m, s) per point -> gfeat (B,N,C) f32"""
    g = np.ascontiguousarray(np.asarray(gpooled)[..., col0:col0 + C], dtype=np.float32)
    B, M, S = idx.shape
    out = np.zeros((B, N, C), np.float32)
    for b in range(B):
        ob = out[b]
        for m in range(M):
            if idx[b, m, 0] < 0:
                continue
            for s in range(S):
                p = idx[b, m, s]
                ob[p] = ob[p] + g[b, m, s]
    return out


def constructed_scene(N=1000, seed=0):
    """B = 2 frames of N points, placed explicitly: seven RoIs per frame holding SCENE_COUNTS points, the 15- and the 40-point RoI
    overlapping on four shared points, an eighth RoI identical to the 17-point one, and the remaining points far from every RoI.
    The in-box points are spread over the whole index range by a seeded permutation (the selection is in index order).
    -> xyz (2,N,3) f32, boxes (2,8,7) f32 [x, y(bottom), z, h, w, l, ry] taken as already enlarged"""
    rng = np.random.default_rng(seed)
    xyz = np.zeros((2, N, 3), np.float32)
    boxes = np.zeros((2, 8, 7), np.float32)
    for b in range(2):
        pts = []
        zc = 20.0 + 5.0 * b
        for k, cnt in enumerate(SCENE_COUNTS):
            cx = -30.0 + 10.0 * k
            ry = 0.0 if cnt in (15, 40) else 0.35 * k + 0.2 * b           # the overlapping pair stays axis-aligned (x extents below)
            boxes[b, k] = (cx, 1.0, zc, 2.0, 2.0, 2.0, ry)
            if cnt in (15, 40):
                continue
            # within 0.5 m of the centre: inside the 2 m cube under any rotation
            off = rng.uniform(-0.35, 0.35, (cnt, 3))
            pts.append(np.array([cx, 0.0, zc]) + off)
        # the overlapping pair: the 15-point RoI covers x in [-1, 1] around a, the 40-point one is shifted by 1.2 m
        ka, kb = SCENE_COUNTS.index(15), SCENE_COUNTS.index(40)
        ax = boxes[b, ka, 0]
        boxes[b, kb, 0] = ax + 1.2
        boxes[b, kb, 2] = boxes[b, ka, 2] = zc
        yz = lambda n: np.stack([rng.uniform(-0.4, 0.4, n), zc + rng.uniform(-0.4, 0.4, n)], 1)      # noqa: E731
        for xs in (ax + np.linspace(-0.9, -0.1, 11), ax + np.array([0.4, 0.5, 0.6, 0.7]), ax + np.linspace(1.3, 2.0, 36)):
            q = yz(len(xs))
            pts.append(np.stack([xs, q[:, 0], q[:, 1]], 1))
        boxes[b, 7] = boxes[b, SCENE_COUNTS.index(17)]
        pts = np.concatenate(pts)
        rest = N - len(pts)
        far = np.stack([rng.uniform(-35, 35, rest), rng.uniform(-0.5, 0.5, rest), rng.uniform(50, 70, rest)], 1)
        allp = np.concatenate([pts, far])
        xyz[b] = allp[rng.permutation(N)]
    return xyz, boxes


def scene_categories(cpu, xyz, boxes):
    """per frame: points per RoI, points shared by the overlapping pair, whether RoIs 5 and 7 hold the same points, points on no RoI"""
    out = []
    for b in range(xyz.shape[0]):
        flags = cpu.pts_in_boxes3d(xyz[b], boxes[b]) > 0
        ka, kb = SCENE_COUNTS.index(15), SCENE_COUNTS.index(40)
        out.append({"counts": flags.sum(1).tolist(), "shared": int((flags[ka] & flags[kb]).sum()),
                    "identical": bool(np.array_equal(boxes[b, 5], boxes[b, 7]) and np.array_equal(flags[5], flags[7])),
                    "free": int((~flags.any(0)).sum())})
    return out
