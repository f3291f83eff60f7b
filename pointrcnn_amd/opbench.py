"""Per-operator roofline report on one MI355X:  python -m pointrcnn_amd.opbench [--quick]

For every operator on the hot path, at the shapes of tools/cfgs/default.yaml (per-GPU batch 32, 16 384 pts) and the
BASELINE config-5 dense case (65 536 pts, 512 RoIs, batch 8), prints one JSON line with the average launch duration
(HIP events on the launch stream, 20 iterations after 3 warm-ups) and
    gather-class ops (gather / group / three_interpolate / roipool3d): two byte counts --
        compulsory  = what HBM must move at least once: every input tensor ONCE + the output (a gather re-reads its source from
                      L2 / MALL, which the 256 MB Infinity Cache serves);  this is the roofline number: GB/s and its fraction of
                      the 8 TB/s HBM3E peak and of the 6.3 TB/s a streaming copy achieves on this part;
        algorithmic = SURVEY 8(d)'s count (index + one read per gathered element + write): the rate the consumer SEES.  It may
                      exceed what HBM can deliver -- then the re-reads were cache hits, and the line says so
                      (`served_from_cache`) instead of reporting a fraction above 1 (the round-2 file listed 0.92 of 8 TB/s for
                      grouping_operation: 7.4 TB/s of algorithmic bytes, 1.3 TB/s of HBM traffic);
      PMC bytes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, gfx950 correction) are merged into the committed
      file by profiles/join_op_traffic.py when those passes were run;
    search ops (fps / ball_query / three_nn / nms): distance (pair) evaluations per second;
    fused MLP: algorithmic FLOP/s vs 157.3 TFLOP/s dense fp32 MFMA.
Algorithmic work per unit follows SURVEY.md 8(d).
"""
import argparse
import json
import os

import numpy as np
import torch

from . import ops, rpn

HBM_PEAK_GBS = 8000.0
HBM_COPY_GBS = 6300.0          # measured float4 copy ceiling (MI355X_MICROARCH.md)
MFMA_F32_PEAK_TF = 157.3


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def emit(name, shape, sec, **kw):
    d = {"op": name, "shape": shape, "avg_launch_us": round(sec * 1e6, 1)}
    if "bytes" in kw:
        comp = kw.get("compulsory", kw["bytes"])
        gbs, agbs = comp / sec / 1e9, kw["bytes"] / sec / 1e9
        d.update(bound="hbm", compulsory_MB=round(comp / 1e6, 1), achieved_GBps=round(gbs, 1),
                 frac_of_8TBps=round(gbs / HBM_PEAK_GBS, 3), frac_of_6p3TBps_copy_ceiling=round(gbs / HBM_COPY_GBS, 3),
                 algorithmic_MB=round(kw["bytes"] / 1e6, 1), algorithmic_GBps=round(agbs, 1),
                 served_from_cache=bool(agbs > HBM_COPY_GBS))
    if "kernels" in kw:            # [name substring, grid size in threads (0 = any)]: what profiles/join_op_traffic.py sums PMC bytes over
        d["kernels"] = [[k, int(g)] for k, g in kw["kernels"]]
    if "pairs" in kw:
        d.update(bound="valu", pair_evals=kw["pairs"], achieved_Gpairs_per_s=round(kw["pairs"] / sec / 1e9, 1))
    if "flops" in kw:
        tf = kw["flops"] / sec / 1e12
        d.update(bound="mfma", achieved_TFLOPs=round(tf, 2), frac_of_peak=round(tf / MFMA_F32_PEAK_TF, 3))
    d.update(kw.get("parts", {}))             # a composed row's own breakdown
    print(json.dumps(d), flush=True)


def train_scene_rows(dev, B=16, n_raw=115000, npoints=16384, D=2000):
    """The RPN training batch (kitti_input.TrainScenePreparer, default.yaml settings) and, next to it, the separate passes that do
    comparable work: scene_prepare, gt_aug_sample, gt_aug_edit, rpn_labels.  Every row is the mean of 5 timings of 20 launches,
    with their spread.  The gt_aug_edit row is a cost row only: the sampler's accepted boxes against a random cloud of the edited
    cloud's size and 4000 random pasted points, not the scene's own points."""
    import numpy as np
    from . import kitti_input
    r = np.random.default_rng(7)
    dbb = (r.random((D, 7)) * [60., .8, 60., .3, .3, 1., 6.28] + [-30., 1.2, 5., 1.4, 1.5, 3.4, -3.14]).astype(np.float32)
    npd = r.integers(5, 400, D)
    gdb = kitti_input.GTDatabase.from_arrays(dbb, np.zeros(D, np.float32), [r.random((int(n), 3)).astype(np.float32) + dbb[i, :3] for i, n in enumerate(npd)],
                                             [r.random(int(n)).astype(np.float32) for n in npd], device=dev)
    calib = kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT)
    scans = [kitti_input.synthetic_scan(n_raw + 97 * b, seed=900 + b) for b in range(B)]
    labels = [(r.random((12, 7)) * [60., .8, 60., .3, .3, 1., 6.28] + [-30., 1.2, 5., 1.4, 1.5, 3.4, -3.14]).astype(np.float32) for _ in range(B)]
    planes = [[0.0, -1.0, 0.0, 1.65]] * B
    prep = kitti_input.TrainScenePreparer(npoints=npoints, gt_database=gdb, device=dev)
    packed = prep.pack(scans, [calib] * B, [(375, 1242)] * B, labels, [np.zeros(12, np.float32)] * B, labels, planes)
    t = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in packed.items()}
    inf = kitti_input.ScenePreparer(npoints=npoints, device=dev)

    def row(name, shape, fn):
        ts = [timeit(fn) for _ in range(5)]
        d = {"op": name, "shape": shape, "avg_launch_us": round(sum(ts) / 5 * 1e6, 1), "min_us": round(min(ts) * 1e6, 1),
             "max_us": round(max(ts) * 1e6, 1)}
        print(json.dumps(d), flush=True)
        return sum(ts) / 5
    shape = "B%d ~%dk raw npoints %d D%d" % (B, n_raw // 1000, npoints, D)
    out = prep(packed, 5)
    total = row("train_scene_prepare", shape + " (H2D excluded: sampler + train scene + labels)", lambda: _train_scene_device(prep, t, packed["max_points"], 5))
    parts = row("scene_prepare", shape, lambda: ops.scene_prepare(t["raw"], t["offsets"], packed["max_points"], t["calib"], t["img_hw"], inf.scope, npoints, 5))
    parts += row("gt_aug_sample", "B%d G12 D%d" % (B, D), lambda: gdb.sample(t["all_gt_boxes3d"], t["num_all_gt"], t["planes"], seed=5))
    nv = int(out["nvalid"].max())
    xyz, inten = torch.randn(B, nv, 3, device=dev) * 20.0, torch.rand(B, nv, device=dev)
    npts, nint = torch.randn(B, 4000, 3, device=dev), torch.rand(B, 4000, device=dev)
    acc = gdb.sample(t["all_gt_boxes3d"], t["num_all_gt"], t["planes"], seed=5)["boxes3d"]
    parts += row("gt_aug_edit", "B%d N%d K%d P4000 (random cloud)" % (B, nv, acc.shape[1]), lambda: ops.gt_aug_edit(xyz, inten, acc, npts, nint))
    parts += row("rpn_labels", "B%d N%d G%d" % (B, npoints, out["gt_boxes3d"].shape[1]), lambda: ops.rpn_labels(out["pts_rect"], out["gt_boxes3d"], out["num_gt"]))
    print(json.dumps({"op": "train_scene_prepare vs separate passes", "train_scene_prepare_us": round(total * 1e6, 1),
                      "sum_of_separate_passes_us": round(parts * 1e6, 1)}), flush=True)


def _train_scene_device(prep, t, max_points, seed):
    acc = prep.db.sample(t["all_gt_boxes3d"], t["num_all_gt"], t["planes"], prep.extra_num, prep.rand_num, prep.apply_prob,
                         [prep.scope[0:2], prep.scope[2:4], prep.scope[4:6]], prep.try_times, prep.max_accept, seed)
    out = ops.train_scene_prepare(t["raw"], t["offsets"], max_points, t["calib"], t["img_hw"], prep.scope, prep.npoints, seed,
                                  t["gt_boxes3d"], t["gt_alpha"], t["num_gt"], acc, prep.db, prep.methods, prep.prob, prep.rot_range)
    return ops.rpn_labels(out["pts_rect"], out["gt_boxes3d"], out["num_gt"])


def scene_large_rows(dev, B=8, n_raw=400000, npoints=65536, D=2000):
    """Both input builders at BASELINE config 5 (65 536 points per frame, bs8) on 400 000-point synthetic scans with fov_frac 0.2:
    the large form (select, HBM sort, rows) and, alternately in the same process on the same scans, the one-workgroup form at
    16 384 points -- the cost of the HBM sort against the LDS sort.  Every row: median of five windows of 20 launches, min and max."""
    from . import kitti_input
    r = np.random.default_rng(7)
    box = lambda n: (r.random((n, 7)) * [60., .8, 60., .3, .3, 1., 6.28] + [-30., 1.2, 5., 1.4, 1.5, 3.4, -3.14]).astype(np.float32)   # noqa: E731
    dbb, npd = box(D), r.integers(5, 400, D)
    gdb = kitti_input.GTDatabase.from_arrays(dbb, np.zeros(D, np.float32), [r.random((int(n), 3)).astype(np.float32) + dbb[i, :3] for i, n in enumerate(npd)],
                                             [r.random(int(n)).astype(np.float32) for n in npd], device=dev)
    calib = kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT)
    scans = [kitti_input.synthetic_scan(n_raw + 97 * b, seed=900 + b, fov_frac=0.2) for b in range(B)]
    labels = [box(12) for _ in range(B)]
    preps = {n: kitti_input.TrainScenePreparer(npoints=n, gt_database=gdb, device=dev, large_clouds=n > ops.SCENE_SMALL_MAX) for n in (npoints, 16384)}
    packed = preps[npoints].pack(scans, [calib] * B, [(375, 1242)] * B, labels, [np.zeros(12, np.float32)] * B, labels, [[0.0, -1.0, 0.0, 1.65]] * B)
    t = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in packed.items()}
    scope = preps[npoints].scope
    acc = gdb.sample(t["all_gt_boxes3d"], t["num_all_gt"], t["planes"], seed=5)
    st = ops.scene_prepare(t["raw"], t["offsets"], packed["max_points"], t["calib"], t["img_hw"], scope, npoints, 5)
    calls = {}
    for n in (npoints, 16384):
        calls["scene_prepare", n] = lambda n=n: ops.scene_prepare(t["raw"], t["offsets"], packed["max_points"], t["calib"], t["img_hw"], scope, n, 5)
        calls["train_scene_prepare", n] = lambda n=n: ops.train_scene_prepare(
            t["raw"], t["offsets"], packed["max_points"], t["calib"], t["img_hw"], scope, n, 5, t["gt_boxes3d"], t["gt_alpha"], t["num_gt"], acc, gdb,
            large=n > ops.SCENE_SMALL_MAX)
    times = {k: [] for k in calls}
    for _ in range(5):                                           # the forms alternate, window by window
        for k, fn in calls.items():
            times[k].append(timeit(fn))
    for (name, n), ts in times.items():
        print(json.dumps({"op": name, "shape": "B%d ~%dk raw (fov_frac 0.2, %d..%d valid) npoints %d%s" % (
            B, n_raw // 1000, int(st[3].min()), int(st[3].max()), n, " K%d D%d (builder only: no sampler, no labels)" % (acc["db_id"].shape[1], D)
            if name.startswith("train") else ""), "form": "large (select, HBM sort, rows)" if n > ops.SCENE_SMALL_MAX else "one workgroup per frame",
            "median_us": round(float(np.median(ts)) * 1e6, 1), "min_us": round(min(ts) * 1e6, 1), "max_us": round(max(ts) * 1e6, 1)}), flush=True)


def gt_database_row(dev, B=8, n_raw=120000, nbox=8):
    """The GT-database builder (kitti_input.GTDatabase.from_kitti's device pass) at one KITTI-sized batch: count, scan, the host read
    of the total, fill.  Next to its time the traffic floor: the raw scans read twice (once per pass) plus the outputs written."""
    import numpy as np
    from . import kitti_input
    r = np.random.default_rng(17)
    calib = kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT)
    scans = [kitti_input.synthetic_scan(n_raw, seed=300 + b) for b in range(B)]
    boxes = np.zeros((B, nbox, 7), np.float32)
    for b, sc in enumerate(scans):                                   # car-sized boxes on scan points in front of the camera
        rect = kitti_input.lidar_to_rect_host(sc, calib.lidar_to_rect_matrix())
        c = rect[r.choice(np.nonzero((rect[:, 2] > 5) & (rect[:, 2] < 40) & (np.abs(rect[:, 0]) < 20))[0], nbox)]
        boxes[b] = np.concatenate([c[:, :1], c[:, 1:2] + 0.8, c[:, 2:3], np.tile([[1.6, 1.7, 4.0]], (nbox, 1)), r.uniform(-3.14, 3.14, (nbox, 1))], 1)
    pk = kitti_input.pack_scans(scans, [calib] * B, [(375, 1242)] * B, pin=False)
    raw, off, cal = pk["raw"].to(dev), pk["offsets"].to(dev), pk["calib"].to(dev)
    bx, nb = torch.from_numpy(boxes).to(dev), torch.full((B,), nbox, dtype=torch.int32, device=dev)
    P = ops.gt_database_build(raw, off, pk["max_points"], cal, bx, nb)[2].shape[0]
    emit("gt_database_build", "B%d x %d raw points x %d boxes (%d points kept; includes the host read of the total)" % (B, n_raw, nbox, P),
         timeit(lambda: ops.gt_database_build(raw, off, pk["max_points"], cal, bx, nb)),
         bytes=2 * raw.numel() * 4 + P * 20 + B * nbox * 4, kernels=[("gtdb_kernel", 0), ("gtdb_scan_kernel", 0)])


def aug_scene_row(dev, B=8, n_raw=120000, G=12, D=2000):
    """The offline GT-augmented scenes (kitti_input.AugSceneGenerator's device pass) at one KITTI-sized batch: the sampling loop, then
    count, scan, the host read of the total, fill, paste.  Traffic floor of the builder: the raw scans read twice plus the rows written."""
    import numpy as np
    from . import kitti_input
    r = np.random.default_rng(27)
    calib = kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT)
    box = lambda n: (r.random((n, 7)) * [60., .8, 60., .3, .3, 1., 6.28] + [-30., 1.2, 5., 1.4, 1.5, 3.4, -3.14]).astype(np.float32)   # noqa: E731
    dbb, npd = box(D), r.integers(5, 400, D)
    gdb = kitti_input.GTDatabase.from_arrays(dbb, np.zeros(D, np.float32), [r.random((int(n), 3)).astype(np.float32) + dbb[i, :3] for i, n in enumerate(npd)],
                                             [r.random(int(n)).astype(np.float32) for n in npd], hard_ratio=0.0, device=dev)
    pk = kitti_input.pack_scans([kitti_input.synthetic_scan(n_raw, seed=400 + b) for b in range(B)], [calib] * B, [(375, 1242)] * B, pin=False)
    raw, off, cal, hw = (pk[k].to(dev) for k in ("raw", "offsets", "calib", "img_hw"))
    gt = torch.from_numpy(np.stack([box(G) for _ in range(B)])).to(dev)
    planes = torch.tensor([[0.0, -1.0, 0.0, 1.65]] * B, dtype=torch.float64, device=dev)
    ids = torch.arange(10000, 10000 + B, dtype=torch.int32, device=dev)
    scope = kitti_input.aug_scene_scope("Car")
    sample = lambda: ops.aug_scene_sample(gt, None, planes, ids, gdb.boxes, gdb.npts, scope, 5)      # noqa: E731
    acc = sample()
    emit("aug_scene_sample", "B%d G%d D%d (%d objects accepted)" % (B, G, D, int(acc["count"].sum())), timeit(sample), kernels=[("augs_sample_kernel", 0)])
    build = lambda: ops.aug_scene_build(raw, off, pk["max_points"], cal, hw, scope, acc, gdb.points, gdb.intensity, gdb.offsets)      # noqa: E731
    rows = build()[2].shape[0]
    emit("aug_scene_build", "B%d x %d raw points (%d rows out; includes the host read of the total)" % (B, n_raw, rows), timeit(build),
         bytes=2 * raw.numel() * 4 + rows * 20, kernels=[("augs_tile_kernel", 0), ("augs_scan_kernel", 0), ("augs_paste_kernel", 0)])


def rpn_loss_rows(dev, B=16, N=16384, rounds=5):
    """`rpn_loss fwd+bwd`: train_functions.get_rpn_loss + backward at the training step's shape (bs16 x 16 384 points, C = 76, about
    3 % foreground and 10 % ignored), composed torch against the fused device passes, alternated in one process; per route the median
    and the minimum over `rounds` windows of 20 calls.  Traffic floor of the fused route: labels + foreground rows read in forward and
    again in backward + both gradients written once."""
    from . import train_functions as tf
    g = torch.Generator().manual_seed(7)
    u = torch.rand(B, N, generator=g)
    lab = torch.where(u < 0.03, 1, torch.where(u < 0.13, -1, 0)).to(dev)
    reg_lab = (torch.rand(B, N, 7, generator=g) * torch.tensor([6., 2., 6., 1., 1., 2., 6.28]) + torch.tensor([-3., -1., -3., 1., 1., 3., -3.14])).to(dev)
    cls = torch.randn(B, N, 1, generator=g).to(dev).requires_grad_(True)
    reg = torch.randn(B, N, 76, generator=g).to(dev).requires_grad_(True)

    def step(fused):
        cls.grad = reg.grad = None
        tf.get_rpn_loss(cls, reg, lab, reg_lab, fused=fused).backward()
    times = {False: [], True: []}
    for _ in range(rounds):
        for fused in (False, True):
            times[fused].append(timeit(lambda: step(fused)))
    n_fg, npts = int((lab > 0).sum()), B * N
    floor = 2 * (npts * (8 + 28 + 4) + n_fg * 76 * 4) + npts * 77 * 4
    for fused in (False, True):
        t = sorted(times[fused])
        d = {"op": "rpn_loss fwd+bwd (%s)" % ("fused" if fused else "composed"), "shape": "B%d N%d C76, %d foreground rows" % (B, N, n_fg),
             "median_us": round(t[len(t) // 2] * 1e6, 1), "min_us": round(t[0] * 1e6, 1), "max_us": round(t[-1] * 1e6, 1)}
        if fused:
            d.update(traffic_floor_MB=round(floor / 1e6, 1), floor_GBps_at_median=round(floor / t[len(t) // 2] / 1e9, 1))
        print(json.dumps(d), flush=True)


def rpn_loss_kind_rows(dev, B=16, N=16384, rounds=5):
    """`rpn_loss (dice|bce|focal) fwd+bwd`: the inputs of rpn_loss_rows under each RPN.LOSS_CLS, composed torch against the second level
    of the fused route (get_rpn_loss(fused=2)), alternated in one process; per route the median, minimum and maximum over `rounds`
    windows of 20 calls.  bench.py's training step always runs the default focal configuration: these rows are the only timing of
    the other two kinds."""
    from . import train_functions as tf
    g = torch.Generator().manual_seed(7)
    u = torch.rand(B, N, generator=g)
    lab = torch.where(u < 0.03, 1, torch.where(u < 0.13, -1, 0)).to(dev)
    reg_lab = (torch.rand(B, N, 7, generator=g) * torch.tensor([6., 2., 6., 1., 1., 2., 6.28]) + torch.tensor([-3., -1., -3., 1., 1., 3., -3.14])).to(dev)
    cls = torch.randn(B, N, 1, generator=g).to(dev).requires_grad_(True)
    reg = torch.randn(B, N, 76, generator=g).to(dev).requires_grad_(True)
    n_fg = int((lab > 0).sum())
    for kind, loss_cls in (("dice", "DiceLoss"), ("bce", "BinaryCrossEntropy"), ("focal", "SigmoidFocalLoss")):
        cfg = type("Cfg", (tf.RPNLossConfig,), {"LOSS_CLS": loss_cls})

        def step(fused):
            cls.grad = reg.grad = None
            tf.get_rpn_loss(cls, reg, lab, reg_lab, cfg, fused=fused).backward()
        times = {False: [], 2: []}
        for _ in range(rounds):
            for fused in (False, 2):
                times[fused].append(timeit(lambda: step(fused)))
        for fused in (False, 2):
            t = sorted(times[fused])
            print(json.dumps({"op": "rpn_loss (%s) fwd+bwd (%s)" % (kind, "fused level 2" if fused else "composed"),
                              "shape": "B%d N%d C76, %d foreground rows" % (B, N, n_fg), "median_us": round(t[len(t) // 2] * 1e6, 1),
                              "min_us": round(t[0] * 1e6, 1), "max_us": round(t[-1] * 1e6, 1)}), flush=True)


def train_split_rows(dev, B=16, rounds=5):
    """`train stack fwd+bwd`: one SharedMLPTrain forward + backward at four RPN training shapes -- an SA2-like padding-free stack
    (4096 -> 1024 centres, radius 2.5, nsample 32, [96 + 3, 64, 96, 128]), an SA4-like padding-free first layer (256 -> 64 centres,
    nsample 32, [512 + 3, 256]), an FP-like plain stack (B x 16 384 rows, [256, 128, 128]) and an FP-like stack with its interpolated
    first layer (4096 known -> 16 384 points, [128 + 128, 128, 128]) -- with train_mlp.TRAIN_SPLIT 0 (fp32 MFMA throughout) against 6
    (split-bf16 forward / dgrad on the plain-row layers) against train_mlp.TRAIN_SPLIT_ALL 6 (the gathered first layers and the
    ragged widths as well, one split-image launch per call), each also with train_mlp.TRAIN_SPLIT_WGRAD 6 (the wide layers' wgrad
    on train_wgrad_s_kernel), alternated in one process; per setting the median, minimum and maximum over `rounds` windows of 20
    calls.  `split_launches`: the weight split launches per forward + backward the setting adds; `split_wgrads`: the layers whose
    wgrad runs the split kernel."""
    from . import train_mlp
    g = torch.Generator().manual_seed(5)
    xyz = rpn.synthetic_clouds(B, 16384, device=dev)
    xyz1 = ops.gather_rows(xyz, ops.furthest_point_sample(xyz, 4096))
    nx2 = ops.gather_rows(xyz1, ops.furthest_point_sample(xyz1, 1024))
    idx = ops.ball_query(2.5, 32, xyz1, nx2)          # (radius 1.0 finds the centre alone among these uniform FPS samples)
    gr = train_mlp.GroupRows(idx, nx2, 4096)
    xyz3 = ops.gather_rows(nx2, ops.furthest_point_sample(nx2, 256))
    nx4 = ops.gather_rows(xyz3, ops.furthest_point_sample(xyz3, 64))
    gr4 = train_mlp.GroupRows(ops.ball_query(20.0, 32, xyz3, nx4), nx4, 256)
    _, idx3, w3 = ops.three_nn(xyz, xyz1, want_weight=True)
    stacks = (("SA2-like padding-free", train_mlp.Source("group", xyz=xyz1.reshape(1, -1, 3), rows=gr), 32,
               torch.randn(B, 4096, 96, generator=g).to(dev), None, [99, 64, 96, 128], B * 1024, gr),
              ("SA4-like padding-free first layer", train_mlp.Source("group", xyz=xyz3.reshape(1, -1, 3), rows=gr4), 32,
               torch.randn(B, 256, 512, generator=g).to(dev), None, [515, 256], B * 64, gr4),
              ("FP-like plain", train_mlp.Source("plain"), 0, torch.randn(B * 16384, 256, generator=g).to(dev), None, [256, 128, 128], B * 16384, None),
              ("FP-like interpolated", train_mlp.Source("interp", idx3=idx3, w3=w3), 0, torch.randn(B, 4096, 128, generator=g).to(dev),
               torch.randn(B, 16384, 128, generator=g).to(dev), [256, 128, 128], B * 16384, None))
    for name, src, ns, x0, x1, chans, groups, rows_of in stacks:
        x0.requires_grad_(True)
        bns = [torch.nn.BatchNorm1d(n).to(dev).train() for n in chans[1:]]
        params = []
        for k, n, bn in zip(chans[:-1], chans[1:], bns):
            params += [(torch.randn(n, k, generator=g) / k ** 0.5).to(dev).requires_grad_(True), bn.weight, bn.bias]
        gout = torch.randn(groups, chans[-1], generator=g).to(dev)

        def step():
            x0.grad = None
            train_mlp.SharedMLPTrain.apply(src, bns, ns, x0, x1, *params).backward(gout)
        settings = ((0, 0, 0, "fp32 MFMA"), (6, 0, 0, "split-bf16 x 6"), (6, 6, 0, "split-bf16 x 6 + split wgrad"),
                    (0, 0, 6, "split-bf16 x 6 all"), (0, 6, 6, "split-bf16 x 6 all + split wgrad"))
        times = {st[:3]: [] for st in settings}
        keep = train_mlp.TRAIN_SPLIT, train_mlp.TRAIN_SPLIT_WGRAD, train_mlp.TRAIN_SPLIT_ALL
        try:
            for _ in range(rounds):
                for terms, wterms, aterms, _ in settings:
                    train_mlp.TRAIN_SPLIT, train_mlp.TRAIN_SPLIT_WGRAD, train_mlp.TRAIN_SPLIT_ALL = terms, wterms, aterms
                    times[(terms, wterms, aterms)].append(timeit(step))
        finally:
            train_mlp.TRAIN_SPLIT, train_mlp.TRAIN_SPLIT_WGRAD, train_mlp.TRAIN_SPLIT_ALL = keep
        rows = int(rows_of.rows_dev.item()) if rows_of is not None else groups
        fwd_split = sum(1 for l, k in enumerate(chans[:-1]) if k % 32 == 0 and (l > 0 or src.mode == "plain"))
        bwd_split = sum(1 for n in chans[1:] if n % 32 == 0)
        wide = sum(1 for k, n in zip(chans[:-1], chans[1:]) if k > 64 and n > 64)
        for terms, wterms, aterms, label in settings:
            t = sorted(times[(terms, wterms, aterms)])
            print(json.dumps({"op": "train stack fwd+bwd (%s)" % label,
                              "shape": "%s: B%d, %d rows, %s" % (name, B, rows, chans), "median_us": round(t[len(t) // 2] * 1e6, 1),
                              "min_us": round(t[0] * 1e6, 1), "max_us": round(t[-1] * 1e6, 1),
                              "split_launches": 2 if aterms else (fwd_split + bwd_split) if terms else 0,
                              "split_wgrads": wide if wterms else 0}), flush=True)


def train_wgrad_rows(dev, rounds=5):
    """`train stack bwd`: the BACKWARD library call alone of stacks whose GEMM work is wide weight gradients, with the wgrad on
    train_wgrad_lds_kernel (prcnn_train_stack_bwd) against train_wgrad_s_kernel (prcnn_train_stack_bwd_wsplit, every dgrad on fp32),
    alternated in one process; per setting the median, minimum and maximum over `rounds` windows of 20 calls.  The first layer
    takes no input gradient, so besides the wgrads a call holds the BatchNorm backward reductions, the partial-tile reductions and
    the dgrads between the layers -- the same launches under both settings.  Shapes: 262 144 plain rows [128, 128, 128] (two
    262 144 x 128 x 128 wgrads, the second with the prologue), the 515 -> 256 padding-free first layer, a 128 -> 196 layer."""
    import ctypes
    from . import _cabi, train_mlp
    from .ops import _p, _stream
    g = torch.Generator().manual_seed(9)
    B = 16
    xyz = rpn.synthetic_clouds(B, 16384, device=dev)
    xyz1 = ops.gather_rows(xyz, ops.furthest_point_sample(xyz, 1024))
    nx2 = ops.gather_rows(xyz1, ops.furthest_point_sample(xyz1, 256))
    gr = train_mlp.GroupRows(ops.ball_query(4.0, 32, xyz1, nx2), nx2, 1024)
    stacks = (("plain", train_mlp.Source("plain"), 0, torch.randn(262144, 128, generator=g).to(dev), [128, 128, 128], 262144),
              ("padding-free first layer", train_mlp.Source("group", xyz=xyz1.reshape(1, -1, 3), rows=gr), 32,
               torch.randn(B, 1024, 512, generator=g).to(dev), [515, 256], B * 256),
              ("plain", train_mlp.Source("plain"), 0, torch.randn(262144, 128, generator=g).to(dev), [128, 196], 262144))
    L = _cabi.lib()
    for name, src, ns, x0, chans, groups in stacks:
        bns = [torch.nn.BatchNorm1d(n).to(dev).train() for n in chans[1:]]
        params = []
        for k, n, bn in zip(chans[:-1], chans[1:], bns):
            params += [(torch.randn(n, k, generator=g) / k ** 0.5).to(dev).requires_grad_(True), bn.weight, bn.bias]
        gout = torch.randn(groups, chans[-1], generator=g).to(dev)
        ctx = train_mlp.SharedMLPTrain.apply(src, bns, ns, x0, None, *params).grad_fn      # (x0 takes no gradient: no dgrad for layer 0)
        st = ctx.st
        work, nbytes = st.work(ctx.K0, True, dev)
        nulls = (ctypes.c_void_p * st.nl)()
        head = (ctypes.byref(ctx.S), st.layers, st.nl, ctx.ns, _p(ctx.a_dump), ctx.ld_dump, _p(gout), gout.stride(0), _p(ctx.arg), None, 0)
        tail = (train_mlp._aligned_ptr(work), nbytes, _stream())
        calls = {0: lambda: _cabi.check(L.prcnn_train_stack_bwd(*head, *tail), "prcnn_train_stack_bwd"),
                 6: lambda: _cabi.check(L.prcnn_train_stack_bwd_wsplit(*head, nulls, *tail), "prcnn_train_stack_bwd_wsplit")}
        times = {0: [], 6: []}
        for _ in range(rounds):
            for terms in (0, 6):
                times[terms].append(timeit(calls[terms]))
        rows = int(gr.rows_dev.item()) if ns else groups
        flops = sum(2.0 * rows * k * n for k, n in zip(chans[:-1], chans[1:]) if k > 64 and n > 64)
        for terms in (0, 6):
            t = sorted(times[terms])
            print(json.dumps({"op": "train stack bwd (%s)" % ("wgrad split-bf16 x 6" if terms else "wgrad fp32 LDS kernel"),
                              "shape": "%s: %d rows, %s" % (name, rows, chans), "median_us": round(t[len(t) // 2] * 1e6, 1),
                              "min_us": round(t[0] * 1e6, 1), "max_us": round(t[-1] * 1e6, 1), "wide_wgrad_GFLOP": round(flops / 1e9, 2)}), flush=True)


def head_tail_rows(dev, R=262144, K=128, rounds=5):
    """`head_tail fwd+bwd`: the tail of an RPN training head -- Dropout(0.5) and the output layer (N = 76 and N = 1) on R rows, forward
    and backward with all three gradients -- as the composed pieces (F.dropout on torch's generator + pytorch_utils._LinearRows) against
    the device tail (pytorch_utils._HeadTail: csrc/head_tail.hip), alternated in one process; per route the median, minimum and maximum
    over `rounds` windows of 20 calls.  Traffic floors, each tensor once: composed = what the ops read and write one by one, device =
    x, out / x, g, gx.  peak_MB: torch.cuda.max_memory_allocated over one forward + backward above what was allocated before it."""
    import torch.nn.functional as F
    import pointnet2_lib.pointnet2.pytorch_utils as pt_utils
    g = torch.Generator().manual_seed(13)
    x = torch.randn(R, K, generator=g).to(dev).requires_grad_(True)
    for N in (76, 1):
        w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev).requires_grad_(True)
        b = torch.zeros(N, device=dev, requires_grad=True)
        gout = torch.randn(R, N, generator=g).to(dev)
        call = [0]

        def composed():
            torch.autograd.grad(pt_utils._LinearRows.apply(F.dropout(x, 0.5, True, False), w, b), (x, w, b), gout)

        def device():
            call[0] += 1
            torch.autograd.grad(pt_utils._HeadTail.apply(x, w, b, (0, 70, call[0], 0.5)), (x, w, b), gout)
        routes = (("composed", composed), ("device", device))
        peak = {}
        for name, fn in routes:
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[name] = (torch.cuda.max_memory_allocated() - base) / 1e6
        times = {name: [] for name, _ in routes}
        for _ in range(rounds):
            for name, fn in routes:
                times[name].append(timeit(fn))
        xb, ob = 4 * R * K, 4 * R * N
        floor = {"composed": (xb + xb + xb // 4 + xb + ob) + (ob + xb + ob + xb + ob + xb + xb // 4 + xb), "device": (xb + ob) + (xb + ob + xb)}
        for name, _ in routes:
            t = sorted(times[name])
            print(json.dumps({"op": "head_tail fwd+bwd (%s)" % name, "shape": "R%d K%d N%d p0.5" % (R, K, N),
                              "median_us": round(t[len(t) // 2] * 1e6, 1), "min_us": round(t[0] * 1e6, 1), "max_us": round(t[-1] * 1e6, 1),
                              "traffic_floor_MB": round(floor[name] / 1e6, 1), "floor_GBps_at_median": round(floor[name] / t[len(t) // 2] / 1e9, 1),
                              "peak_MB": round(peak[name], 1)}), flush=True)


def head_tail_step_memory(dev, B=16, N=16384, steps=3):
    """`rpn train step memory`: torch.cuda.max_memory_allocated over RPNTrainer steps at the training shape (bs16 x 16 384 points,
    12 synthetic boxes per frame) with the heads on the composed path and on the device tail (pytorch_utils.HEAD_TAIL), one model each,
    in one process; the peak is reset after a first step of each setting"""
    import pointnet2_lib.pointnet2.pytorch_utils as pt_utils
    from . import train_functions as tf
    g = torch.Generator().manual_seed(99)
    pts = rpn.synthetic_clouds(B, N, device=dev)
    pick = torch.randint(0, N, (B, 12), generator=g).to(dev)
    ctr = torch.gather(pts, 1, pick[..., None].expand(-1, -1, 3))
    hwl = torch.tensor([1.56, 1.6, 3.9], device=dev) * 2.0
    ry = (torch.rand((B, 12, 1), generator=g) * 6.283 - 3.1416).to(dev)
    gt = torch.cat([ctr[..., 0:1], ctr[..., 1:2] + hwl[0] / 2, ctr[..., 2:3], hwl.expand(B, 12, 3), ry], 2).contiguous()
    cls, reg = ops.rpn_labels(pts, gt)
    batch = {"pts_input": pts, "rpn_cls_label": cls.long(), "rpn_reg_label": reg}
    was = pt_utils.HEAD_TAIL
    try:
        for on in (False, True):
            pt_utils.HEAD_TAIL = on
            torch.manual_seed(1234)
            model = tf.init_rpn_head_weights(rpn.randomize_bn_stats(rpn.RPN(), seed=7)).to(dev)
            trainer = tf.RPNTrainer(model)
            trainer.step(batch)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(steps):
                trainer.step(batch)
            torch.cuda.synchronize()
            print(json.dumps({"op": "rpn train step memory (%s)" % ("device tail" if on else "composed heads"), "shape": "B%d N%d" % (B, N),
                              "max_memory_allocated_MB": round(torch.cuda.max_memory_allocated() / 1e6, 1)}), flush=True)
            del trainer, model
            torch.cuda.empty_cache()
    finally:
        pt_utils.HEAD_TAIL = was


def optimizer_rows(dev, rounds=5):
    """`optimizer step`: one optim.OneCycleAdam.step() -- gradient-norm clip, decoupled decay, Adam, schedule -- over the parameter
    lists of rpn.RPN() and of the RCNN net, the composed torch route against the two launches of csrc/optim.hip, alternated in one
    process; per route the median, minimum and maximum over `rounds` windows of 20 calls.  The gradients are fixed tensors (the
    pointer table is uploaded once).  Traffic floor of the fused route: the gradient read twice, parameter and both moments read
    and written once: 32 bytes per element."""
    from . import point_rcnn
    from .optim import OneCycleAdam
    g = torch.Generator().manual_seed(3)
    for name, net in (("rpn.RPN()", rpn.RPN()), ("rcnn_net", point_rcnn.PointRCNN(mode="TRAIN").rcnn_net)):
        shapes = [p.shape for p in net.parameters() if p.requires_grad]
        opts = {}
        for fused in (False, True):
            ps = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.1).to(dev)) for s in shapes]
            for p in ps:
                p.grad = (torch.randn(p.shape, generator=g) * 0.01).to(dev)
            opts[fused] = OneCycleAdam(ps, 10000, fused=fused)
        times = {False: [], True: []}
        for _ in range(rounds):
            for fused in (False, True):
                times[fused].append(timeit(opts[fused].step))
        n = sum(int(torch.Size(s).numel()) for s in shapes)
        for fused in (False, True):
            t = sorted(times[fused])
            d = {"op": "optimizer step (%s)" % ("fused" if fused else "composed"), "shape": "%s: %d tensors, %d elements" % (name, len(shapes), n),
                 "median_us": round(t[len(t) // 2] * 1e6, 1), "min_us": round(t[0] * 1e6, 1), "max_us": round(t[-1] * 1e6, 1)}
            if fused:
                d.update(traffic_floor_MB=round(32 * n / 1e6, 2), floor_GBps_at_median=round(32 * n / t[len(t) // 2] / 1e9, 1),
                         table_uploads=opts[True].table_uploads)
            print(json.dumps(d), flush=True)


def optimizer_mode_rows(dev, rounds=5):
    """`optimizer step adam` / `optimizer step sgd`: one optim.ClipAdam / ClipSGD step on the device route over rpn.RPN()'s parameter
    list (TRAIN.LR, WEIGHT_DECAY, MOMENTUM, GRAD_NORM_CLIP of default.yaml) against clip_grad_norm_ + torch.optim.Adam / SGD
    (foreach=True) on the same shapes, alternated in one process; per route the median, minimum and maximum over `rounds` windows of
    20 calls.  The gradients are fixed tensors; clip_grad_norm_ rescales the torch route's in memory, which after the first call
    leaves their norm at the clip and changes no timing.
    Traffic floor of the device route: the gradient read twice, the parameter and its state read and written once: 32 bytes per
    element for adam, 24 for sgd."""
    from .optim import ClipAdam, ClipSGD
    g = torch.Generator().manual_seed(3)
    shapes = [p.shape for p in rpn.RPN().parameters() if p.requires_grad]
    n = sum(int(torch.Size(s).numel()) for s in shapes)

    def tensors():
        ps = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.1).to(dev)) for s in shapes]
        for p in ps:
            p.grad = (torch.randn(p.shape, generator=g) * 0.01).to(dev)
        return ps
    for mode, floor_bytes in (("adam", 32), ("sgd", 24)):
        ps, qs = tensors(), tensors()
        if mode == "adam":
            ours, stock = ClipAdam(ps, lr=0.002, weight_decay=0.001, grad_norm_clip=1.0, fused=True), \
                torch.optim.Adam(qs, lr=0.002, weight_decay=0.001, foreach=True)
        else:
            ours, stock = ClipSGD(ps, lr=0.002, momentum=0.9, weight_decay=0.001, grad_norm_clip=1.0, fused=True), \
                torch.optim.SGD(qs, lr=0.002, momentum=0.9, weight_decay=0.001, foreach=True)

        def torch_step():
            torch.nn.utils.clip_grad_norm_(qs, 1.0, foreach=True)
            stock.step()
        routes = {"torch foreach": torch_step, "device": ours.step}
        times = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                times[k].append(timeit(fn))
        for k in routes:
            t = sorted(times[k])
            d = {"op": "optimizer step %s (%s)" % (mode, k), "shape": "rpn.RPN(): %d tensors, %d elements" % (len(shapes), n),
                 "median_us": round(t[len(t) // 2] * 1e6, 1), "min_us": round(t[0] * 1e6, 1), "max_us": round(t[-1] * 1e6, 1)}
            if k == "device":
                d.update(traffic_floor_MB=round(floor_bytes * n / 1e6, 2), floor_GBps_at_median=round(floor_bytes * n / t[len(t) // 2] / 1e9, 1),
                         table_uploads=ours.table_uploads)
            print(json.dumps(d), flush=True)


def rcnn_offline_rows(dev, B=4, M=300, G=12, R=64, N=16384, C=128, S=512):
    """`rcnn_offline_batch`: kitti_input.RCNNOfflinePreparer's device side (`--train_mode rcnn_offline`, ROI_SAMPLE_JIT False) at the
    workload's shape -- RoI sampling (IoU matrix + lists + picks + noise loop), pooling of the sampled RoIs (prcnn_roipool3d, mask +
    depth + C feature channels) and the finish pass (per-RoI rotate / scale / flip, canonical transform, labels) -- the whole call and
    the three parts.  Scene: every label has 8 RoIs near it (foreground), 8 shifted by half its length (hard background), the rest
    scattered (easy background).  Also the sampler alone at its RoI cap (M = 4096), where one lane builds the candidate lists."""
    import numpy as np
    from . import kitti_input, rcnn
    rng = np.random.default_rng(12)

    def scene(M):
        gt = (rng.random((B, G, 7)) * [60., .3, 50., .3, .3, .8, 6.28] + [-30., 1.4, 8., 1.4, 1.5, 3.5, -3.14]).astype(np.float32)
        roi = (rng.random((B, M, 7)) * [70., .4, 60., .3, .3, 1., 6.28] + [-35., 1.3, 4., 1.4, 1.5, 3.4, -3.14]).astype(np.float32)
        for j in range(G):
            near = gt[:, j:j + 1] + rng.normal(0, 1, (B, 8, 7)) * [.1, .03, .1, .03, .03, .06, .03]
            hard = gt[:, j:j + 1] + rng.normal(0, 1, (B, 8, 7)) * [.1, .03, .1, .03, .03, .06, .03]
            hard[..., 0] += np.cos(gt[:, j:j + 1, 6]) * 0.5 * gt[:, j:j + 1, 5]
            hard[..., 2] -= np.sin(gt[:, j:j + 1, 6]) * 0.5 * gt[:, j:j + 1, 5]
            roi[:, 16 * j:16 * j + 8], roi[:, 16 * j + 8:16 * j + 16] = near, hard
        return roi, gt
    roi, gt = scene(M)
    ctr = gt[np.arange(B)[:, None], rng.integers(0, G, (B, N))][..., :3]
    xyz = (ctr + rng.normal(0, 1, (B, N, 3)) * [1.8, .6, 1.8] - [0, .8, 0]).astype(np.float32)
    frames = [{"sample_id": b, "rpn_xyz": xyz[b], "rpn_features": rng.normal(0, 1, (N, C)).astype(np.float32),
               "rpn_intensity": rng.random(N).astype(np.float32), "seg_mask": (rng.random(N) > 0.5).astype(np.float32),
               "roi_boxes3d": roi[b], "roi_scores": np.zeros(M, np.float32), "gt_boxes3d": gt[b]} for b in range(B)]
    cfg = type("Cfg", (rcnn.RCNNConfig,), dict(ROI_SAMPLE_JIT=False, ROI_PER_IMAGE=R, NUM_POINTS=S))
    prep = kitti_input.RCNNOfflinePreparer(cfg, dev)
    d = prep._upload(prep.pack(frames, pin=False))
    out = prep(d, seed=3)
    assert not out["status"].any() and (out["cls_label"] == 1).any() and (out["cls_label"] == 0).any()
    thr = (cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH, cfg.CLS_BG_THRESH)
    sample = lambda: ops.rcnn_offline_sample(d["roi_boxes3d"], d["num_roi"], d["gt_boxes3d"], d["num_gt"], R, seed=3, frame_ids=d["frame_ids"])   # noqa: E731
    s = sample()
    _, feat = prep._point_features(d)
    pooled, empty = rcnn.roipool3d_gpu(d["rpn_xyz"], feat, s["rois"], cfg.POOL_EXTRA_WIDTH, S)
    t_all = timeit(lambda: prep(d, seed=3))
    t_s = timeit(sample)
    t_p = timeit(lambda: rcnn.roipool3d_gpu(d["rpn_xyz"], feat, s["rois"], cfg.POOL_EXTRA_WIDTH, S))
    t_f = timeit(lambda: ops.rcnn_offline_finish(pooled, s, empty, thr, prep.aug_methods, prep.flip_prob, cfg.AUG_ROT_RANGE, 3, d["frame_ids"]))
    emit("rcnn_offline_batch", "bs%d M%d G%d R%d N%d S%d C%d (upload excluded; includes the (B,N,%d) feature concat)" % (B, M, G, R, N, S, C, 2 + C),
         t_all, bytes=B * R * S * (5 + C) * 4, parts={"sample_us": round(t_s * 1e6, 1), "pool_us": round(t_p * 1e6, 1), "finish_us": round(t_f * 1e6, 1)})
    big, bgt = scene(4096)
    T = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)          # noqa: E731
    br, bg, bn, bm = T(big), T(bgt), T(np.full(B, 4096), np.int32), T(np.full(B, G), np.int32)
    emit("rcnn_offline_sample", "bs%d M4096 G%d R%d (the RoI cap)" % (B, G, R), timeit(lambda: ops.rcnn_offline_sample(br, bn, bg, bm, R, seed=3)),
         pairs=B * 4096 * G)


def rcnn_loss_rows(dev, R=256, rounds=5):
    """`rcnn_loss fwd+bwd`: train_functions.get_rcnn_loss + backward at the RCNN training step's shape (bs4 x 64 RoIs, C = 46, default
    BinaryCrossEntropy; about a third of the rows regressed, 15 % ignored), composed torch against the fused device passes, alternated
    in one process; per route the median and the minimum over `rounds` windows of 20 calls.  256 rows are launch latency, not traffic:
    no floor is printed."""
    from . import train_functions as tf
    from .rcnn import RCNNConfig
    g = torch.Generator().manual_seed(9)
    u = torch.rand(R, generator=g)
    mean = torch.tensor(tf.RPNLossConfig.MEAN_SIZE)
    roi, gt = torch.zeros(R, 7), torch.zeros(R, 7)
    roi[:, 3:6] = (torch.rand(R, 3, generator=g) * 0.4 + 0.8) * mean
    gt[:, 0:3] = (torch.rand(R, 3, generator=g) * 2.8 - 1.4) * torch.tensor([1.0, 0.3, 1.0])
    gt[:, 3:6] = (torch.rand(R, 3, generator=g) * 0.4 + 0.8) * mean
    gt[:, 6] = torch.rand(R, generator=g) * 2.0 - 1.0
    ret = {"rcnn_cls": (torch.randn(R, 1, generator=g) * 2).to(dev).requires_grad_(True),
           "rcnn_reg": torch.randn(R, 46, generator=g).to(dev).requires_grad_(True),
           "cls_label": torch.where(u < 0.3, 1, torch.where(u < 0.45, -1, 0)).to(dev),
           "reg_valid_mask": (torch.rand(R, generator=g) < 0.35).long().to(dev), "roi_boxes3d": roi.to(dev), "gt_of_rois": gt.to(dev)}

    def step(fused):
        ret["rcnn_cls"].grad = ret["rcnn_reg"].grad = None
        tf.get_rcnn_loss(ret, RCNNConfig, fused=fused).backward()
    times = {False: [], True: []}
    for _ in range(rounds):
        for fused in (False, True):
            times[fused].append(timeit(lambda: step(fused)))
    for fused in (False, True):
        t = sorted(times[fused])
        print(json.dumps({"op": "rcnn_loss fwd+bwd (%s)" % ("fused" if fused else "composed"),
                          "shape": "R%d C46, %d regressed rows" % (R, int(ret["reg_valid_mask"].sum())),
                          "median_us": round(t[len(t) // 2] * 1e6, 1), "min_us": round(t[0] * 1e6, 1), "max_us": round(t[-1] * 1e6, 1)}), flush=True)


def _joint_batch(dev, B=4, N=16384, G=10):
    """the RCNN training tests' scene (uniform clouds, G car-sized ground-truth boxes on drawn points) with synthetic RPN labels"""
    from . import train_functions as tf
    pts = rpn.synthetic_clouds(B, N, seed0=300).to(dev)
    g = torch.Generator().manual_seed(5)
    pick = torch.randint(0, N, (B, G), generator=g).to(dev)
    ctr = torch.gather(pts, 1, pick[..., None].expand(-1, -1, 3))
    hwl = torch.tensor([1.56, 1.6, 3.9], device=dev)
    ry = (torch.rand((B, G, 1), generator=g) * 6.283 - 3.1416).to(dev)
    gt = torch.cat([ctr[..., 0:1], ctr[..., 1:2] + hwl[0] / 2, ctr[..., 2:3], hwl.expand(B, G, 3), ry], 2).contiguous()
    cls, reg = tf.synthetic_rpn_labels(pts, gt, ops.pts_in_boxes3d)
    return {"pts_input": pts, "gt_boxes3d": gt, "rpn_cls_label": cls, "rpn_reg_label": reg}


def roipool_grad_rows(dev, B=4, N=16384, M=64, S=512, C=128, rounds=5):
    """`roipool3d grad`: the pooling's gradient with respect to the per-point features at the RCNN step's shape, on RoIs a
    ProposalTargetLayer samples from the training tests' scene (its own pooling call's idx / distinct).  The device route
    (ops.roipool3d_grad: list build + gather, no atomics) against the composed torch route on the same idx (index_add_ into zeros:
    float atomics), alternated in one process; per route the median, minimum and maximum over `rounds` windows of 20 calls.  gpooled is
    the step's layout: (B*M, S, 133) rows, the C feature columns behind 5 others.  Floor: every gpooled feature column read once, every
    gfeat element written once."""
    from .proposal_target_layer import ProposalTargetLayer
    from .rcnn import RCNNConfig
    batch = _joint_batch(dev, B, N)
    g = torch.Generator().manual_seed(3)
    layer = ProposalTargetLayer(RCNNConfig, seed=21, pool_grad=True)
    rois = (batch["gt_boxes3d"].repeat(1, 30, 1) + (torch.randn((B, 300, 7), generator=g) * 0.25).to(dev)).contiguous()      # jittered proposals
    feat = torch.randn((B, N, C), generator=g).to(dev)
    with torch.no_grad():
        out = layer({"roi_boxes3d": rois, "gt_boxes3d": batch["gt_boxes3d"], "rpn_xyz": batch["pts_input"], "rpn_features": feat,
                     "seg_mask": torch.zeros((B, N), device=dev), "pts_depth": torch.norm(batch["pts_input"], p=2, dim=2)})
    idx, distinct = out["pool_idx"], out["pool_distinct"]
    assert tuple(idx.shape) == (B, M, S)
    gp = torch.randn((B * M, S, 5 + C), generator=g).to(dev)
    flat = (idx.long() + (torch.arange(B, device=dev) * N).view(B, 1, 1)).reshape(-1)
    live = (idx >= 0).reshape(-1)
    flat_live, rows_live = flat[live].contiguous(), live.nonzero().squeeze(1)

    def device():
        return ops.roipool3d_grad(gp, idx, distinct, N, C, col0=5)

    def composed():
        return torch.zeros((B * N, C), device=dev).index_add_(0, flat_live, gp.view(-1, 5 + C)[rows_live, 5:]).view(B, N, C)
    a, b = device(), composed()
    err = (a - b).abs().max().item()
    times = {"device": [], "composed": []}
    for _ in range(rounds):
        for name, fn in (("device", device), ("composed", composed)):
            times[name].append(timeit(fn))
    floor = 4 * (int(live.sum()) * C + B * N * C)
    refs = torch.bincount(flat_live, minlength=B * N)
    for name in ("device", "composed"):
        t = sorted(times[name])
        print(json.dumps({"op": "roipool3d grad (%s)" % name,
                          "shape": "B%d N%d M%d S%d C%d, %d empty RoIs, distinct median %d, refs per point max %d"
                                   % (B, N, M, S, C, int((distinct == 0).sum()), int(distinct.float().median()), int(refs.max())),
                          "median_us": round(t[len(t) // 2] * 1e6, 1), "min_us": round(t[0] * 1e6, 1), "max_us": round(t[-1] * 1e6, 1),
                          "traffic_floor_MB": round(floor / 1e6, 1), "floor_GBps_at_median": round(floor / t[len(t) // 2] / 1e9, 1),
                          "max_abs_diff_between_routes": err}), flush=True)


def joint_step_rows(dev, B=4, rounds=5, iters=5):
    """`joint step`: train_functions.JointTrainer.step at bs4 on the training tests' scene, pool_grad off against on (two trainers on
    copies of one model), alternated in one process; per setting the median, minimum and maximum over `rounds` windows of `iters`
    steps.  bench.py has no workload for this step: these rows are its only timing."""
    import copy
    from . import point_rcnn, train_functions as tf
    torch.manual_seed(11)
    model = point_rcnn.PointRCNN(mode="TRAIN", rpn_fixed=False).to(dev)
    batch = _joint_batch(dev, B)
    trainers = {flag: tf.JointTrainer(copy.deepcopy(model), pool_grad=flag) for flag in (False, True)}
    times = {False: [], True: []}
    for flag in (False, True):
        for _ in range(3):
            trainers[flag].step(batch, next_batch=batch)
    for _ in range(rounds):
        for flag in (False, True):
            times[flag].append(timeit(lambda: trainers[flag].step(batch, next_batch=batch), iters, 1))
    for flag in (False, True):
        t = sorted(times[flag])
        print(json.dumps({"op": "joint step (pool_grad %s)" % ("on" if flag else "off"), "shape": "bs%d N16384, 64 RoIs per frame" % B,
                          "median_ms": round(t[len(t) // 2] * 1e3, 3), "min_ms": round(t[0] * 1e3, 3), "max_ms": round(t[-1] * 1e3, 3)}), flush=True)


def eval_stats_rows(dev, B=32, shapes=((100, 12), (512, 24)), N=16384, rounds=5):
    """`eval_stats`: the per-batch statistics of eval_one_epoch_joint (tools/eval_rcnn.py:539-573) at bs32 -- recall of the ground truth
    by the RoIs and the refined boxes at five thresholds, the segmentation IoU, the detection count.  Composed route: the reference's
    loop as it runs on this library, per frame ops.boxes_iou3d x 2, max, compares and `.item()` reads.  Device route: EvalStats.update
    (two launches, no host read; the window ends on one synchronisation).  Alternated in one process; per route the median, minimum and
    maximum over `rounds` windows of 20 calls."""
    from .eval_stats import THRESH_LIST, EvalStats
    gq = torch.Generator().manual_seed(21)
    span, base = torch.tensor([60., .8, 60., .3, .3, 1., 6.28]), torch.tensor([-30., 1.2, 5., 1.4, 1.5, 3.4, -3.14])
    seg = (torch.rand(B, N, generator=gq) < 0.2).float().to(dev)
    label = (torch.rand(B, N, generator=gq) < 0.2).long().to(dev)
    for M, G in shapes:
        gt = torch.rand(B, G, 7, generator=gq) * span + base
        gt[:, G - G // 4:] = 0                                    # a quarter of the rows is padding
        near = gt[:, torch.randint(0, G - G // 4, (M,), generator=gq)] + torch.randn(B, M, 7, generator=gq) * 0.2
        far = torch.rand(B, M, 7, generator=gq) * span + base
        rois = torch.where(torch.rand(B, M, 1, generator=gq) < 0.5, near, far).to(dev).contiguous()
        pred = (rois + torch.randn(B, M, 7, generator=gq).to(dev) * 0.05).contiguous()
        gt = gt.to(dev)
        num = torch.randint(0, 20, (B,), generator=gq, dtype=torch.int32).to(dev)
        stats = EvalStats("joint", dev)

        def composed():
            total = [0] * 5, [0] * 5
            total_gt = final_total = 0
            total_rpn_iou = 0.0
            for k in range(B):
                cur = gt[k]
                n = cur.shape[0] - 1
                while n >= 0 and cur[n].sum().item() == 0:
                    n -= 1
                if n >= 0:
                    cur = cur[:n + 1].contiguous()
                    for which, boxes in enumerate((pred[k], rois[k])):
                        gt_max_iou, _ = ops.boxes_iou3d(boxes, cur).max(dim=0)
                        for idx, thresh in enumerate(THRESH_LIST):
                            total[which][idx] += (gt_max_iou > thresh).sum().item()
                    total_gt += cur.shape[0]
                fg_mask = label > 0
                correct = ((seg == label) & fg_mask).sum().float()
                union = fg_mask.sum().float() + (seg > 0).sum().float() - correct
                total_rpn_iou += (correct / torch.clamp(union, min=1.0)).item()
                final_total += int(num[k].item())
            return total, total_gt, total_rpn_iou, final_total

        def device():
            stats.update(rois, gt, pred_boxes3d=pred, det_num=num, seg_result=seg, rpn_cls_label=label)
        times = {"composed": [], "device": []}
        for _ in range(rounds):
            times["composed"].append(timeit(composed))
            times["device"].append(timeit(device))
        for route in ("composed", "device"):
            t = sorted(times[route])
            print(json.dumps({"op": "eval_stats (%s)" % route, "shape": "B%d M%d G%d N%d joint" % (B, M, G, N),
                              "median_us": round(t[len(t) // 2] * 1e6, 1), "min_us": round(t[0] * 1e6, 1), "max_us": round(t[-1] * 1e6, 1),
                              "launches_per_update": 2 if route == "device" else None}), flush=True)


class _P2:
    """KITTI training frame 000000's camera matrix: what a calibration object carries for the result writers"""
    P2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]], np.float32)


def _kitti_like_detections(B, M, g):
    """boxes in front of the camera as a detector emits them (a few very close or off to the side: clipped, some dropped by the
    0.8-of-the-image test), scores, a shuffled keep list and per-frame counts"""
    span = torch.tensor([50., 1.4, 68., .76, .81, 1.94, 6.28])
    base = torch.tensor([-25., .8, 2., 1.22, 1.30, 3.11, -3.14])
    boxes = torch.rand(B, M, 7, generator=g) * span + base
    boxes[:, :4, 2] = torch.rand(B, 4, generator=g) * 1.8 + 1.2
    scores = torch.randn(B, M, generator=g) * 3
    keep = torch.stack([torch.randperm(M, generator=g) for _ in range(B)]).to(torch.int32)
    num = torch.randint(M // 2, M + 1, (B,), generator=g, dtype=torch.int32)
    return boxes, scores, keep, num


def _tmpfs_dir():
    import tempfile
    return tempfile.mkdtemp(prefix="prcnn_opbench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)


def result_writer_rows(dev, B=32, Ms=(100, 512), rounds=5, iters=5):
    """`result_writer`: one batch of detections -> one KITTI result file per frame, at bs32 x 100 and bs32 x 512 boxes, files on a
    memory-backed path.  Host route: kitti_output.write_detections (four device-to-host copies, then numpy and a Python `%` per line).
    Device route: DeviceResultWriter.format + write (one launch, the text's copy, bytes into files).  Both are timed on the host
    clock from a drained device, back to back (the device route's wait for its own kernel and copy is inside its time), alternated in
    one process; the kernel alone is timed with HIP events.  The device route must be the faster one in every round."""
    import shutil
    import time
    from . import kitti_output
    g = torch.Generator().manual_seed(33)
    for M in Ms:
        boxes, scores, keep, num = (t.to(dev).contiguous() for t in _kitti_like_detections(B, M, g))
        calibs, shapes, ids = [_P2] * B, [(375, 1242, 3)] * B, list(range(B))
        writer = kitti_output.DeviceResultWriter(dev)
        dirs = {"host": _tmpfs_dir(), "device": _tmpfs_dir()}

        def host():
            kitti_output.write_detections(boxes, scores, keep, num, ids, calibs, shapes, dirs["host"])

        def device():
            writer.write(writer.format(boxes, scores, keep, num, calibs, shapes), ids, dirs["device"])

        def window(fn):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            return (time.perf_counter() - t0) / iters
        times = {"host": [], "device": []}
        try:
            for _ in range(rounds):
                times["host"].append(window(host))
                times["device"].append(window(device))
            lines = sum(open("%s/%06d.txt" % (dirs["device"], i)).read().count("\n") for i in ids)
        finally:
            for d in dirs.values():
                shutil.rmtree(d, ignore_errors=True)
        P2 = torch.from_numpy(_P2.P2).double().reshape(1, 12).repeat(B, 1).to(dev)
        hw = torch.tensor([[375, 1242]] * B, dtype=torch.int32, device=dev)
        out = ops.kitti_result_text(boxes, scores, P2, hw, keep=keep, num=num)
        kernel = timeit(lambda: ops.kitti_result_text(boxes, scores, P2, hw, keep=keep, num=num, out=out))
        faster = all(d < h for d, h in zip(times["device"], times["host"]))
        for route in ("host", "device"):
            t = sorted(times[route])
            print(json.dumps({"op": "result_writer (%s)" % route, "shape": "B%d M%d, %d lines" % (B, M, lines),
                              "median_ms_per_batch": round(t[len(t) // 2] * 1e3, 3), "min_ms": round(t[0] * 1e3, 3), "max_ms": round(t[-1] * 1e3, 3),
                              "rounds_ms": [round(x * 1e3, 3) for x in times[route]],
                              "kernel_us": round(kernel * 1e6, 1) if route == "device" else None,
                              "device_faster_in_every_round": faster}), flush=True)
        if not faster:
            raise AssertionError("result_writer: the device route was not faster than the host route in every round at M=%d: %s" % (M, times))


def eval_loop_rows(dev, B=16, nbatches=3, rounds=5):
    """`eval_loop`: eval_one_epoch_joint over synthetic scenes (randomly initialised detector) in frames per second, with the host
    result writer (writer=None) and with the device writer, alternated in one process.  No bar attached."""
    import shutil
    import time
    from . import eval_stats, kitti_output
    from .point_rcnn import PointRCNN
    torch.manual_seed(0)
    model = rpn.randomize_bn_stats(PointRCNN(mode="TEST")).to(dev).eval()
    pts = rpn.synthetic_clouds(B * nbatches, 16384, device=dev)
    batches = [{"sample_id": list(range(k * B, (k + 1) * B)), "pts_input": pts[k * B:(k + 1) * B]} for k in range(nbatches)]
    writer = kitti_output.DeviceResultWriter(dev)
    times = {"host": [], "device": []}
    out = _tmpfs_dir()
    try:
        for r in range(rounds + 1):                               # round 0 warms both routes up
            for route, w in (("host", None), ("device", writer)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eval_stats.eval_one_epoch_joint(model, batches, "%s/%s" % (out, route), lambda i: _P2, lambda i: (375, 1242, 3), writer=w)
                torch.cuda.synchronize()
                if r:
                    times[route].append(time.perf_counter() - t0)
        files = ["%s/device/final_result/data/%06d.txt" % (out, i) for i in range(B * nbatches)]
        lines = sum(open(f).read().count("\n") for f in files if os.path.exists(f))
    finally:
        shutil.rmtree(out, ignore_errors=True)
    for route in ("host", "device"):
        fps = sorted(B * nbatches / t for t in times[route])
        print(json.dumps({"op": "eval_loop joint (%s writer)" % route, "shape": "%d batches of %d frames, 16384 points, %d detections" % (nbatches, B, lines),
                          "median_frames_per_s": round(fps[len(fps) // 2], 1), "min": round(fps[0], 1), "max": round(fps[-1], 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", default=None, help="run one row family only: scene_large | train_scene | eval_stats | optimizer | rpn_loss_kinds | train_split (= train_stack) | train_wgrad | head_tail | result_writer | eval_loop")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.only == "scene_large":
        scene_large_rows(dev)
        return
    if args.only == "train_scene":
        train_scene_rows(dev)
        return
    if args.only == "result_writer":
        result_writer_rows(dev)
        return
    if args.only == "eval_loop":
        eval_loop_rows(dev)
        return
    if args.only == "eval_stats":
        eval_stats_rows(dev)
        return
    if args.only == "roipool_grad":
        roipool_grad_rows(dev)
        return
    if args.only == "joint_step":
        joint_step_rows(dev)
        return
    if args.only == "optimizer":
        optimizer_rows(dev)
        optimizer_mode_rows(dev)
        return
    if args.only == "rpn_loss_kinds":
        rpn_loss_kind_rows(dev)
        return
    if args.only in ("train_split", "train_stack"):
        train_split_rows(dev)
        return
    if args.only == "train_wgrad":
        train_wgrad_rows(dev)
        return
    if args.only == "head_tail":
        head_tail_rows(dev)
        head_tail_step_memory(dev)
        return
    B = 8 if args.quick else 32
    N = 16384
    xyz = rpn.synthetic_clouds(B, N, device=dev)
    g = torch.Generator(device="cpu").manual_seed(0)

    # ---- what plain streams reach on THIS box (1 GiB buffers): the ceilings the gather ops are read against, next to the 8 TB/s headline.
    # A pure write stream (roipool3d's 1 GB of pooled rows written once) and a read + write copy are different ceilings.
    buf_a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    buf_b = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    t_fill = timeit(lambda: buf_a.fill_(1.0), 10, 2)
    t_copy = timeit(lambda: buf_b.copy_(buf_a), 10, 2)
    print(json.dumps({"op": "stream ceilings", "shape": "1 GiB fp32", "write_only_GBps": round(buf_a.numel() * 4 / t_fill / 1e9, 1),
                      "copy_read_plus_write_GBps": round(2 * buf_a.numel() * 4 / t_copy / 1e9, 1),
                      "note": "torch fill_ / copy_ on this box; an op that writes W bytes and reads R cannot finish before W / write_only (R << W) or "
                              "(R + W) / copy (R ~ W)"}), flush=True)
    del buf_a, buf_b
    torch.cuda.empty_cache()

    # ---- search ops
    emit("fps", "B%d %d->4096" % (B, N), timeit(lambda: ops.furthest_point_sample(xyz, 4096), 5, 1), pairs=B * N * 4096)
    new_xyz = ops.gather_rows(xyz, ops.furthest_point_sample(xyz, 4096))
    emit("ball_query2", "B%d N%d M4096 r(.1,.5) ns(16,32)" % (B, N),
         timeit(lambda: ops.ball_query2(0.1, 16, 0.5, 32, xyz, new_xyz)), pairs=B * N * 4096)
    emit("three_nn", "B%d n%d m4096" % (B, N), timeit(lambda: ops.three_nn(xyz, new_xyz)), pairs=B * N * 4096)
    # the short levels (scans of neighbor.hip; several lanes share a query): SA3 / SA4 ball query, FP2 / FP3 three_nn, and the RCNN
    # stage's first query on 512-point RoI clouds
    lv = [new_xyz]
    for npoint in (1024, 256, 64):
        lv.append(ops.gather_rows(lv[-1], ops.furthest_point_sample(lv[-1], npoint)))
    emit("ball_query2 SA3", "B%d N1024 M256 r(1,2) ns(16,32)" % B, timeit(lambda: ops.ball_query2(1.0, 16, 2.0, 32, lv[1], lv[2])), pairs=B * 1024 * 256)
    emit("ball_query2 SA4", "B%d N256 M64 r(2,4) ns(16,32)" % B, timeit(lambda: ops.ball_query2(2.0, 16, 4.0, 32, lv[2], lv[3])), pairs=B * 256 * 64)
    emit("three_nn FP2", "B%d n1024 m256" % B, timeit(lambda: ops.three_nn(lv[1], lv[2], want_weight=True)), pairs=B * 1024 * 256)
    emit("three_nn FP3", "B%d n256 m64" % B, timeit(lambda: ops.three_nn(lv[2], lv[3], want_weight=True)), pairs=B * 256 * 64)
    R = 16 * B
    roi_pts = (torch.rand(R, 512, 3, generator=g) * torch.tensor([2.0, 2.0, 4.5])).to(dev)
    roi_ctr = ops.gather_rows(roi_pts, ops.furthest_point_sample(roi_pts, 128))
    emit("ball_query RCNN SA1", "B%d N512 M128 r.2 ns64" % R, timeit(lambda: ops.ball_query(0.2, 64, roi_pts, roi_ctr)), pairs=R * 512 * 128)
    del lv, roi_pts, roi_ctr

    # ---- gather-class ops in the op-surface (B,C,N) layout
    feat = torch.randn(B, 96, 4096, device=dev)
    xyz1 = new_xyz
    nx2 = ops.gather_rows(xyz1, ops.furthest_point_sample(xyz1, 1024))
    idx = ops.ball_query(1.0, 32, xyz1, nx2)
    emit("grouping_operation", "B%d C96 N4096 M1024 ns32" % B, timeit(lambda: ops.group(feat, idx)),
         bytes=B * (1024 * 32 * 4 + 2 * 96 * 1024 * 32 * 4), compulsory=B * (1024 * 32 * 4 + 96 * 4096 * 4 + 96 * 1024 * 32 * 4),
         kernels=[("gather_pm_kernel", 0)])
    fidx = ops.furthest_point_sample(xyz1, 1024)
    emit("gather_operation", "B%d C96 N4096 M1024" % B, timeit(lambda: ops.gather(feat, fidx)),
         bytes=B * (1024 * 4 + 2 * 96 * 1024 * 4), compulsory=B * (1024 * 4 + 2 * 96 * 1024 * 4), kernels=[("gather_kernel", B * 1024)])
    d2, i3, w3 = ops.three_nn(xyz, xyz1, want_weight=True)
    kf = torch.randn(B, 256, 4096, device=dev)
    emit("three_interpolate", "B%d C256 m4096 n%d" % (B, N), timeit(lambda: ops.three_interpolate(kf, i3, w3)),
         bytes=B * (N * 24 + 3 * 256 * N * 4 + 256 * N * 4), compulsory=B * (N * 24 + 256 * 4096 * 4 + 256 * N * 4),
         kernels=[("three_interp", 0)])

    # ---- roipool3d: config 3 (M=100, C=130, S=512) and config 5 dense (65536 pts, 512 RoIs, batch 8)
    def rois_for(x, M, seed):
        gg = torch.Generator().manual_seed(seed)
        pick = torch.randint(0, x.shape[1], (x.shape[0], M), generator=gg).to(dev)
        ctr = torch.gather(x, 1, pick.unsqueeze(-1).expand(-1, -1, 3))
        sz = torch.tensor([1.6 + 2, 1.7 + 2, 4.0 + 2], device=dev).expand(x.shape[0], M, 3)
        ry = (torch.rand(x.shape[0], M, 1, generator=gg).to(dev) - 0.5) * 6.28
        return torch.cat([ctr[..., 0:1], ctr[..., 1:2] + 1.8, ctr[..., 2:3], sz, ry], 2).contiguous()

    pf = torch.randn(B, N, 130, device=dev)
    rois = rois_for(xyz, 100, 1)
    emit("roipool3d", "B%d N%d M100 C130 S512 (config 3)" % (B, N), timeit(lambda: ops.roipool3d(xyz, rois, pf, 512)),
         bytes=B * 2 * 100 * 512 * 133 * 4, compulsory=B * (100 * 512 * 133 * 4 + N * 133 * 4),
         kernels=[("roipool3d_kernel", B * 100 * 256)] + [("rp_bins_%s_kernel" % k, 0) for k in ("extent", "count", "scan", "fill")])
    if not args.quick:
        Bd, Nd, Md = 8, 65536, 512
        xd = rpn.synthetic_clouds(Bd, Nd, seed0=500, device=dev)
        pfd = torch.randn(Bd, Nd, 130, device=dev)
        rd = rois_for(xd, Md, 2)
        emit("roipool3d", "B%d N%d M%d C130 S512 (config 5 dense)" % (Bd, Nd, Md),
             timeit(lambda: ops.roipool3d(xd, rd, pfd, 512), 5, 1), bytes=Bd * 2 * Md * 512 * 133 * 4,
             compulsory=Bd * (Md * 512 * 133 * 4 + Nd * 133 * 4),
             kernels=[("roipool3d_kernel", Bd * Md * 256)] + [("rp_bins_%s_kernel" % k, 0) for k in ("extent", "count", "scan", "fill")])
        del xd, pfd, rd

    # ---- GT-augmentation scene edit (kitti_rcnn_dataset.py:484-507): 15 accepted objects per scene, ~4000 pasted points
    ab = rois_for(xyz, 15, 3)
    npts, nint = torch.randn(B, 4000, 3, device=dev), torch.rand(B, 4000, device=dev)
    inten = torch.rand(B, N, device=dev)
    emit("gt_aug_edit", "B%d N%d K15 P4000" % (B, N), timeit(lambda: ops.gt_aug_edit(xyz, inten, ab, npts, nint)),
         bytes=B * (2 * N * 16 + 2 * 4000 * 16))

    # ---- GT-augmentation sampling (kitti_rcnn_dataset.py:414-497): corner IoU pairs, and the whole sampling loop at B = 16
    from . import kitti_input
    gq = torch.Generator().manual_seed(11)
    cb = torch.rand(256, 7, generator=gq) * torch.tensor([60., 1., 60., 1., 1., 3., 6.28]) + torch.tensor([-30., 1., 5., 1., 1., 2., -3.14])
    hw, hl, c, s_ = cb[:, 4:5] / 2, cb[:, 5:6] / 2, torch.cos(cb[:, 6:7]), torch.sin(cb[:, 6:7])
    lx = torch.cat([hl, hl, -hl, -hl] * 2, 1); lz = torch.cat([hw, -hw, -hw, hw] * 2, 1)
    ly = torch.cat([torch.zeros(256, 4), -cb[:, 3:4].expand(-1, 4)], 1)
    corners = torch.stack([cb[:, 0:1] + lx * c + lz * s_, cb[:, 1:2] + ly, cb[:, 2:3] - lx * s_ + lz * c], 2).to(dev).contiguous()
    emit("corner_iou3d", "256 x 256 pairs", timeit(lambda: ops.corner_iou3d(corners, corners)), pairs=256 * 256)
    Bs, D = 16, 2000
    dbb = (torch.rand(D, 7, generator=gq) * torch.tensor([60., .8, 60., .3, .3, 1., 6.28]) + torch.tensor([-30., 1.2, 5., 1.4, 1.5, 3.4, -3.14]))
    npd = torch.randint(5, 400, (D,), generator=gq)
    gdb = kitti_input.GTDatabase.from_arrays(dbb.numpy(), torch.zeros(D).numpy(), [torch.zeros(int(n), 3).numpy() for n in npd],
                                             [torch.zeros(int(n)).numpy() for n in npd], device=dev)
    sg = (torch.rand(Bs, 12, 7, generator=gq) * torch.tensor([60., .8, 60., .3, .3, 1., 6.28]) + torch.tensor([-30., 1.2, 5., 1.4, 1.5, 3.4, -3.14])).to(dev)
    ngt = torch.full((Bs,), 12, dtype=torch.int32, device=dev)
    planes = torch.tensor([[0.0, -1.0, 0.0, 1.65]] * Bs, dtype=torch.float64, device=dev)
    emit("gt_aug_sample", "B%d G12 D%d (default.yaml: 10-14 extra, 100 tries)" % (Bs, D),
         timeit(lambda: gdb.sample(sg, ngt, planes, seed=5)))

    # ---- the RCNN offline training batch: sample + pool + finish (csrc/rcnn_offline.hip, kitti_input.RCNNOfflinePreparer)
    rcnn_offline_rows(dev)

    # ---- the RPN training batch from raw scans (kitti_input.TrainScenePreparer) next to the separate passes
    train_scene_rows(dev, B=4 if args.quick else 16)
    # ---- both input builders at 65 536 points per frame (BASELINE config 5) next to the 16 384-point call on the same scans
    if not args.quick:
        scene_large_rows(dev)

    # ---- the GT-augmentation database from raw scans and labels (kitti_input.GTDatabase.from_kitti)
    gt_database_row(dev)

    # ---- the offline GT-augmented scenes, the train_aug split (kitti_input.AugSceneGenerator)
    aug_scene_row(dev)

    # ---- the RPN training loss and its gradient: composed torch against the one-pass kernels (csrc/rpn_loss.hip)
    rpn_loss_rows(dev)
    rpn_loss_kind_rows(dev)
    # ---- the RCNN training loss and its gradient: composed torch against the device passes (csrc/rcnn_loss.hip)
    rcnn_loss_rows(dev)
    # ---- a training stack forward + backward: fp32 MFMA against the opt-in split-bf16 forward / dgrad (csrc/mlp_train.h)
    train_split_rows(dev, B=4 if args.quick else 16)
    train_wgrad_rows(dev)
    # ---- the adam_onecycle parameter update: composed torch against the two launches of csrc/optim.hip
    optimizer_rows(dev)
    # ---- TRAIN.OPTIMIZER adam and sgd: clip_grad_norm_ + torch's foreach step against the same two launches
    optimizer_mode_rows(dev)
    # ---- the evaluation statistics of a batch: the reference's per-frame loop on this library against the device passes (csrc/eval_stats.hip)
    eval_stats_rows(dev)
    # ---- the result files of a batch: kitti_output.write_detections against the text formatted on the device (csrc/kitti_text.hip),
    # and the joint evaluation loop with either writer
    result_writer_rows(dev)
    eval_loop_rows(dev)

    # ---- NMS (default RPN path: normal, 6300 boxes, thr 0.8) and rotated
    c = torch.rand(6300, 2, generator=g) * torch.tensor([80.0, 70.0])
    s = torch.rand(6300, 2, generator=g) * torch.tensor([0.5, 1.5]) + torch.tensor([0.8, 1.7])
    bev = torch.cat([c - s, c + s, (torch.rand(6300, 1, generator=g) - 0.5) * 6.28], 1).to(dev)
    emit("nms_normal", "N6300 thr0.8", timeit(lambda: ops.nms_sorted(bev, 0.8, rotated=False)), pairs=6300 * 6299 // 2)
    emit("nms_rotated", "N6300 thr0.8", timeit(lambda: ops.nms_sorted(bev, 0.8, rotated=True), 5, 1), pairs=6300 * 6299 // 2)

    # ---- proposal stage, whole batch per call: decode 76 regression channels -> boxes, then
    # score sort + distance split + NMS + top-k.  Scene: 40 % of the points vote for one of 24 cars (tight clusters
    # of overlapping high-score boxes), the rest is clutter -- the regime where NMS has to reject most candidates.
    reg = torch.randn(B * N, 76, device=dev)
    anchor = (1.52563191462, 1.62856739989, 3.88311640418)
    emit("decode_bbox_target", "B%d N%d C76" % (B, N),
         timeit(lambda: ops.decode_bbox_target(xyz.view(-1, 3), reg, 3.0, 0.5, 12, anchor, y_to_bottom=True)),
         bytes=B * N * (76 + 3 + 7) * 4, kernels=[("decode_kernel", 0)])
    gg = torch.Generator().manual_seed(3)
    nfg = int(N * 0.4)
    obj = torch.rand(B, 24, 7, generator=gg) * torch.tensor([70., .4, 62., .3, .3, 1., 6.28]) + torch.tensor([-35., .8, 4., 1.4, 1.5, 3.4, -3.14])
    own = torch.randint(0, 24, (B, nfg), generator=gg)
    fgb = torch.gather(obj, 1, own.unsqueeze(-1).expand(-1, -1, 7)) + torch.randn(B, nfg, 7, generator=gg) * torch.tensor([.08, .03, .12, .03, .03, .06, .03])
    bgb = torch.rand(B, N - nfg, 7, generator=gg) * torch.tensor([80., 4., 70., 1., .8, 2., 6.28]) + torch.tensor([-40., -1., .2, 1., 1.2, 3., -3.14])
    boxes3d = torch.cat([fgb, bgb], 1).to(dev).contiguous()
    scores = torch.cat([torch.randn(B, nfg, generator=gg) + 2.5, torch.randn(B, N - nfg, generator=gg) - 3.0], 1).to(dev)
    for rot in (False, True):
        emit("proposal_layer(%s nms 0.8, 6300/2700 -> 70/30)" % ("rotated" if rot else "normal"), "B%d N%d" % (B, N),
             timeit(lambda: ops.proposal_layer(scores, boxes3d, (6300, 2700), (70, 30), 0.8, rotated=rot)), pairs=B * N)
    rb = boxes3d[:, :100].contiguous()
    rs = scores[:, :100].contiguous()
    emit("nms_batched(rotated 0.1)", "B%d M100" % B, timeit(lambda: ops.nms_batched(rb, rs, None, 0.1, True)), pairs=B * 100)

    # ---- fused MLP: the whole RPN graph's MLP FLOPs are reported by bench.py; here two representative stacks
    model = rpn.randomize_bn_stats(rpn.RPN()).to(dev).eval()
    sa2 = model.backbone_net.SA_modules[1]
    f1 = torch.randn(B, 96, 4096, device=dev)
    with torch.no_grad():
        sec = timeit(lambda: sa2(xyz1, f1))
    macs = 1024 * (16 * (99 * 64 + 64 * 64 + 64 * 128) + 32 * (99 * 64 + 64 * 96 + 96 * 128))
    emit("SA2 module (fps+ball_query+fused MLP chains)", "B%d 4096->1024" % B, sec, flops=2.0 * B * macs)


if __name__ == "__main__":
    main()
