"""GPU parity tests added in round 2 (VERDICT r01 "Next round" item 1 and friends):
  * the WHOLE default.yaml RPN graph with every default optimisation on (first-layer hoisting, padding-free grouping, grid
    neighbour search, pruned FPS) against the oracle graph: every index of every level bit-exact, outputs within 1e-5 scale;
  * the two-stage mirror against outputs of the REFERENCE'S OWN unchanged lib/net PointRCNN run on the drop-in surface
    (tests/golden/net_ref.npz, generated in the build container by ref_net.py);
  * one RPN training forward/backward through the HIP operator kernels against the reference's own training step
    (train_ref.npz);
  * BASELINE config 5 shapes (65 536 points, 512 RoIs);
  * upstream-order FPS, device RPN labels, two-thread / two-stream re-entrancy."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

from util import GOLDEN, enlarge, kitti_cloud, load_net_ref, mlp_tol, rand_boxes3d

sys.path.insert(0, GOLDEN)

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Recorder:
    """records the index outputs of the operator calls a model forward makes (fused inference path)"""

    def __init__(self):
        from pointrcnn_amd import ops
        self.ops, self.saved = ops, {}
        self.fps, self.ball, self.nn_idx, self.nn_w = [], [], [], []

    def __enter__(self):
        ops = self.ops
        for name in ("furthest_point_sample", "ball_query2", "three_nn"):
            self.saved[name] = getattr(ops, name)

        def fps(xyz, npoint, *a, **k):
            r = self.saved["furthest_point_sample"](xyz, npoint, *a, **k)
            self.fps.append(r)
            return r

        def bq2(*a, **k):
            r = self.saved["ball_query2"](*a, **k)
            self.ball.append(r)
            return r

        def nn(unknown, known, want_weight=False):
            r = self.saved["three_nn"](unknown, known, want_weight=want_weight)
            self.nn_idx.append(r[1])
            if want_weight:
                self.nn_w.append(r[2])
            return r
        ops.furthest_point_sample, ops.ball_query2, ops.three_nn = fps, bq2, nn
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.ops, name, fn)


def test_full_default_rpn_graph_vs_oracle_graph(dev, cpu):
    """bs2 x 16384 points, default.yaml RPN, all defaults on: indices of every level == oracle bit for bit, rpn_cls / rpn_reg /
    backbone features within 1e-5 * scale of the un-hoisted, un-deduplicated, double-accumulated oracle graph"""
    from oracle import rpn_cpu
    from pointrcnn_amd import rpn
    from pointnet2_lib.pointnet2 import pointnet2_modules as pm
    assert pm.HOIST_FIRST_LAYER and pm.GROUP_DEDUP
    torch.manual_seed(11)
    model = rpn.randomize_bn_stats(rpn.RPN(), seed=3).to(dev).eval()
    clouds = rpn.synthetic_clouds(2, 16384, seed0=500)
    with _Recorder() as rec, torch.no_grad():
        out = model({"pts_input": clouds.to(dev)})
    spec = rpn_cpu.extract_rpn_weights(model)
    for f in range(2):
        trace = {}
        want = rpn_cpu.rpn_forward_frame(cpu, clouds[f].numpy(), spec, trace=trace)
        for lvl in range(4):
            assert np.array_equal(rec.fps[lvl][f].cpu().numpy(), trace["fps"][lvl]), "fps level %d" % lvl
            for sc in range(2):
                assert np.array_equal(rec.ball[lvl][sc][f].cpu().numpy(), trace["ball"][lvl][sc]), "ball query level %d scale %d" % (lvl, sc)
            assert np.array_equal(rec.nn_idx[lvl][f].cpu().numpy(), trace["nn_idx"][lvl]), "three_nn FP step %d" % lvl
            assert np.array_equal(rec.nn_w[lvl][f].cpu().numpy(), trace["nn_w"][lvl]), "three_nn weights FP step %d" % lvl
        for k, got in (("rpn_cls", out["rpn_cls"][f]), ("rpn_reg", out["rpn_reg"][f]), ("backbone_features", out["backbone_features"][f].t())):
            assert np.abs(got.float().cpu().numpy() - want[k]).max() <= mlp_tol(want[k]), k


def _fill(model, seed):
    import cpu_ops
    return cpu_ops.fill_params_by_name(model, seed)


def test_two_stage_mirror_matches_reference_lib_net_golden(dev):
    """net_ref.npz = outputs of the reference's own unchanged PointRCNN(mode='TEST') (lib/net/point_rcnn.py:8-71 and everything
    it calls) executed on the drop-in op surface in the build container.  Same parameters (a pure function of the state-dict
    names, which must therefore be IDENTICAL to the reference's), same clouds -> same outputs from the HIP path."""
    from make_golden import NET_CASE, crc
    from pointrcnn_amd import rpn
    from pointrcnn_amd.point_rcnn import PointRCNN
    g = load_net_ref()
    c = NET_CASE
    model = PointRCNN(mode="TEST")
    sd = model.state_dict()
    assert sorted(sd) == g["keys"].tolist(), "mirror state-dict keys differ from the reference's"
    assert [str(tuple(sd[k].shape)) for k in sorted(sd)] == g["shapes"].tolist()
    _fill(model, c["wseed"])
    model = model.to(dev).eval()
    clouds = rpn.synthetic_clouds(c["B"], c["N"], seed0=c["seed0"])
    assert crc(clouds.numpy()) == g["crc_in"]
    with torch.no_grad():
        out = model({"pts_input": clouds.to(dev)})
    tol = lambda ref: 1e-5 * max(1.0, float(np.abs(ref).max()))      # noqa: E731
    cls = out["rpn_cls"][:, :, 0].cpu().numpy()
    assert np.abs(cls - g["rpn_cls"]).max() <= tol(g["rpn_cls"])
    reg = out["rpn_reg"].cpu().numpy()
    assert np.abs(reg[:, ::8] - g["rpn_reg_s8"]).max() <= tol(g["rpn_reg_s8"])
    assert np.allclose(np.abs(reg.astype(np.float64)).sum((1, 2)), g["rpn_reg_abs_sum"], rtol=1e-5)
    feat = out["backbone_features"].cpu().numpy()
    assert np.abs(feat[:, :, ::16] - g["feat_s16"]).max() <= tol(g["feat_s16"])
    assert np.array_equal(out["seg_result"].cpu().numpy(), g["seg_result"])
    # proposals: 100 RoIs per frame chosen by score sort + distance split + NMS on 16384 decoded boxes -- identical
    # selections; coordinates agree to the decode's float rounding of 1e-6-perturbed regression inputs
    rois, want = out["rois"].cpu().numpy(), g["rois"]
    assert rois.shape == want.shape
    assert np.abs(out["roi_scores_raw"].cpu().numpy() - g["roi_scores_raw"]).max() <= tol(g["roi_scores_raw"])
    assert np.abs(rois - want).max() <= 2e-4, np.abs(rois - want).max()
    assert np.abs(out["rcnn_cls"].cpu().numpy() - g["rcnn_cls"]).max() <= 5e-5 * max(1.0, float(np.abs(g["rcnn_cls"]).max()))
    assert np.abs(out["rcnn_reg"].cpu().numpy() - g["rcnn_reg"]).max() <= 5e-5 * max(1.0, float(np.abs(g["rcnn_reg"]).max()))


def test_rpn_training_step_matches_reference_golden(dev):
    """train_ref.npz 'step_*' = loss and parameter gradients of ONE training forward/backward of the reference's own
    PointRCNN(mode='TRAIN') + model_fn (lib/net/train_functions.py) on the drop-in surface (CPU, oracle-backed operators).
    Here: the mirror RPN in training mode on the GPU -- HIP forward AND backward kernels for FPS / ball query / grouping /
    3-NN interpolation, MIOpen for the convolutions -- same parameters, same batch, same labels."""
    from make_golden import TRAIN_CASE, crc, train_batch
    from pointrcnn_amd import rpn, train_functions as tf
    g = np.load(os.path.join(GOLDEN, "train_ref.npz"))
    c = TRAIN_CASE
    pts, gt, cls, reg = train_batch(c)
    assert crc(pts, gt, cls, reg) == g["step_crc"]
    model = rpn.RPN()
    _fill(_Wrap(model), c["wseed"])                 # the reference's keys carry the 'rpn.' prefix of PointRCNN
    model = model.to(dev)
    trainer = tf.RPNTrainer(model, ddp=False)
    trainer.model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()                                  # the golden step runs without dropout (RNG streams differ CPU/GPU)
    batch = {"pts_input": T(pts, dev), "rpn_cls_label": T(cls, dev), "rpn_reg_label": T(reg, dev)}
    loss = trainer.loss(batch)
    loss.backward()
    want = float(g["step_loss"])
    assert abs(float(loss.item()) - want) <= 1e-5 * max(1.0, abs(want)), (float(loss.item()), want)
    params = {"rpn." + n: p for n, p in model.named_parameters()}
    names = g["step_names"].tolist()
    assert sorted(n for n, p in params.items() if p.grad is not None) == sorted(names)
    # Tolerances: the step is ill-conditioned beyond the heads -- max-pooling routes a whole gradient to ONE of several
    # near-equal rows, so rounding-level forward differences re-route gradients.  The reference's own step on CPU differs from
    # ITSELF by up to 2.7e-3 of a tensor's largest entry (and 2.5e-5 in norm) between 1 and 8 BLAS threads
    # (measured in the build container); the GPU step is held to the same order: heads (no pooling behind them) 1e-4,
    # everything else 3e-2 in norm with a median below 1e-3, sampled entries within 0.1 of the tensor's sampled maximum.
    rel_norm, rel_samp = {}, {}
    for i, n in enumerate(names):
        gr = params[n].grad
        rel_norm[n] = abs(float(gr.double().norm()) - float(g["step_gnorm"][i])) / float(g["step_gnorm"][i])
        got = np.resize(gr.reshape(-1)[:8].cpu().numpy(), 8)
        ref = g["step_gsample"][i]
        rel_samp[n] = float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-12))
    heads = [n for n in names if "rpn_cls_layer" in n or "rpn_reg_layer" in n]
    assert len(heads) == 10
    assert max(rel_norm[n] for n in heads) <= 1e-4 and max(rel_samp[n] for n in heads) <= 1e-4, [(n, rel_norm[n], rel_samp[n]) for n in heads]
    assert max(rel_norm.values()) <= 3e-2, max(rel_norm.items(), key=lambda kv: kv[1])
    assert float(np.median(list(rel_norm.values()))) <= 1e-3
    assert max(rel_samp.values()) <= 0.1, max(rel_samp.items(), key=lambda kv: kv[1])


class _Wrap(torch.nn.Module):
    """gives the mirror RPN the key prefix it has inside the reference's PointRCNN ('rpn.')"""

    def __init__(self, rpn_module):
        super().__init__()
        self.rpn = rpn_module


# ---- BASELINE config 5: 65 536 points per frame, 512 RoIs ----------------------------------------------------------
def test_config5_roipool3d_65536_points_512_rois(dev, cpu):
    from pointrcnn_amd import ops
    N, M, S, C = 65536, 512, 512, 130
    xyz = kitti_cloud(1, N, seed=77)
    boxes = enlarge(rand_boxes3d(xyz[0], M, seed=78), 1.0)[None]
    boxes[0, -1, 0] += 500.0                                   # one empty RoI
    feat = np.random.default_rng(79).normal(size=(1, N, C)).astype(np.float32)
    pooled, empty = ops.roipool3d(T(xyz, dev), T(boxes, dev), T(feat, dev), S)
    wp, we = cpu.roipool3d(xyz, boxes, feat, S)
    assert np.array_equal(empty.cpu().numpy(), we) and we[0, -1] == 1
    assert np.array_equal(pooled.cpu().numpy(), wp)
    assert tuple(pooled.shape) == (1, M, S, 3 + C)             # 139.5 MB per frame


def test_config5_point_ops_at_65536_points(dev, cpu):
    """FPS (N > 16384 kernel), grid ball query (both MSG radii) and grid three_nn at config-5 size, bit-exact vs oracle"""
    from pointrcnn_amd import ops
    N, npoint = 65536, 4096
    xyz = kitti_cloud(1, N, seed=91)
    tx = T(xyz, dev)
    fidx = ops.furthest_point_sample(tx, npoint)
    want = cpu.fps(xyz, npoint)
    assert np.array_equal(fidx.cpu().numpy(), want)
    new_xyz = xyz[:, want[0]]
    ia, ib = ops.ball_query2(0.1, 16, 0.5, 32, tx, T(new_xyz, dev))
    assert np.array_equal(ia.cpu().numpy(), cpu.ball_query(0.1, 16, xyz, new_xyz))
    assert np.array_equal(ib.cpu().numpy(), cpu.ball_query(0.5, 32, xyz, new_xyz))
    d2, i3, w3 = ops.three_nn(tx, T(new_xyz, dev), want_weight=True)
    rd2, ri3 = cpu.three_nn(xyz, new_xyz)
    assert np.array_equal(i3.cpu().numpy(), ri3) and np.array_equal(d2.cpu().numpy(), rd2)
    assert np.array_equal(w3.cpu().numpy(), cpu.three_weights(rd2))


def test_fps_multi_workgroup_kernel_ties_and_ragged_sizes(dev, cpu):
    """N > 16384: a frame is split over ceil(N / 16384) workgroups that exchange candidates through L2 every sample; the tie
    rule (lowest point index) has to hold ACROSS the slices, for slice counts 2..4, ragged last slices and several frames"""
    from pointrcnn_amd import ops
    r = np.random.default_rng(5)
    lat = np.stack(np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(1, -1, 3).astype(np.float32)   # 32768 pts, ties everywhere
    rag = r.random((3, 40000, 3), dtype=np.float32) * np.array([80, 4, 70], np.float32)
    dup = np.concatenate([rag[:1, :20000], rag[:1, :20000]], 1)                   # the second slice-and-a-half repeats the first
    for pts, npoint in ((lat, 700), (rag, 1500), (dup, 900), (r.random((2, 16385, 3), dtype=np.float32), 300)):
        got = ops.furthest_point_sample(T(pts, dev), npoint).cpu().numpy()
        assert (got >= 0).all(), "a workgroup gave up waiting for its partners"
        assert np.array_equal(got, cpu.fps(pts, npoint))


def test_config5_rpn_graph_runs_at_65536_points(dev, cpu):
    """the whole RPN graph on one 65 536-point frame (fused path) vs the oracle graph"""
    from oracle import rpn_cpu
    from pointrcnn_amd import rpn
    torch.manual_seed(5)
    model = rpn.randomize_bn_stats(rpn.RPN(), seed=4).to(dev).eval()
    cloud = rpn.synthetic_clouds(1, 65536, seed0=900)
    with torch.no_grad():
        out = model({"pts_input": cloud.to(dev)})
    want = rpn_cpu.rpn_forward_frame(cpu, cloud[0].numpy(), rpn_cpu.extract_rpn_weights(model))
    for k in ("rpn_cls", "rpn_reg"):
        assert np.abs(out[k][0].cpu().numpy() - want[k]).max() <= mlp_tol(want[k]), k


# ---- upstream-order FPS, labels, re-entrancy -----------------------------------------------------------------------
def test_fps_upstream_order_mode(dev, cpu):
    from pointrcnn_amd import ops
    lat = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(8), indexing="ij"), -1).reshape(1, -1, 3).astype(np.float32)
    rnd = np.random.default_rng(0).random((3, 5000, 3), dtype=np.float32)
    dup = np.concatenate([rnd[:, :1500], rnd[:, :1500]], 1)
    small = np.random.default_rng(1).random((2, 50, 3), dtype=np.float32)          # T = 32 < 64 lanes
    for pts, npoint in ((lat, 512), (rnd, 1200), (dup, 1700), (small, 50), (np.repeat(lat, 2, 0)[:, :1000], 300)):
        got = ops.furthest_point_sample(T(pts, dev), npoint, order="upstream").cpu().numpy()
        assert np.array_equal(got, cpu.fps_upstream(pts, npoint))
    # and the canonical kernels still follow the canonical rule on the same tie-heavy inputs
    assert np.array_equal(ops.furthest_point_sample(T(lat, dev), 512).cpu().numpy(), cpu.fps(lat, 512))
    with pytest.raises(ValueError):
        ops.furthest_point_sample(T(lat, dev), 4, order="other")


def test_rpn_labels_kernel_equals_oracle_and_reference_golden(dev, cpu):
    from make_golden import label_scene
    from pointrcnn_amd import ops
    g = np.load(os.path.join(GOLDEN, "labels_ref.npz"))
    scenes = [label_scene(s) for s in (0, 1, 2)]
    pts, gt = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    cls, reg = ops.rpn_labels(T(pts, dev), T(gt, dev))
    wc, wr = cpu.rpn_labels(pts, gt)
    assert np.array_equal(cls.cpu().numpy(), wc) and np.array_equal(reg.cpu().numpy(), wr)
    for i, s in enumerate((0, 1, 2)):                        # == the reference's own generate_rpn_training_labels
        assert np.array_equal(cls[i].cpu().numpy(), g["cls%d" % s].astype(np.int32)) and np.array_equal(reg[i].cpu().numpy(), g["reg%d" % s])
    num = np.array([10, 4, 0], np.int32)
    c2, r2 = ops.rpn_labels(T(pts, dev), T(gt, dev), T(num, dev))
    w2, wr2 = cpu.rpn_labels(pts, gt, num_gt=num)
    assert np.array_equal(c2.cpu().numpy(), w2) and np.array_equal(r2.cpu().numpy(), wr2) and not c2[2].any()


def test_concurrent_threads_and_streams_are_reentrant(dev, cpu):
    """two host threads, each on its own HIP stream, drive the library at the same time (the reference's DataParallel
    convention is one thread per device; on this 1-GPU box: one thread per stream).  Every kernel family with a raised
    dynamic-LDS limit is exercised (pruned FPS + sort, grid build, proposal sort/NMS); results must equal the serial ones."""
    from pointrcnn_amd import ops
    rng = np.random.default_rng(3)
    clouds = [kitti_cloud(2, 16384, seed=10 + i) for i in range(2)]
    scores = [rng.normal(size=(2, 16384)).astype(np.float32) for _ in range(2)]
    boxes = [np.concatenate([c, np.tile([1.5, 1.6, 3.9], (2, 16384, 1)), rng.uniform(-3, 3, (2, 16384, 1))], 2).astype(np.float32) for c in clouds]

    def work(i, out):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                x = T(clouds[i], dev)
                res = []
                for _ in range(3):
                    f = ops.furthest_point_sample(x, 4096)
                    nx = ops.gather_rows(x, f)
                    ia, ib = ops.ball_query2(0.1, 16, 0.5, 32, x, nx)
                    rois, rs, cnt = ops.proposal_layer(T(scores[i], dev), T(boxes[i], dev), (6300, 2700), (70, 30), 0.8, rotated=False)
                    res = [f, ia, ib, rois, cnt]
                torch.cuda.current_stream().synchronize()
                out[i] = [r.cpu().numpy() for r in res]
        except Exception as e:  # noqa: BLE001
            out[i] = e
    serial = {}
    for i in range(2):
        work(i, serial)
    par = {}
    th = [threading.Thread(target=work, args=(i, par)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(2):
        assert not isinstance(par[i], Exception), par[i]
        for a, b in zip(par[i], serial[i]):
            assert np.array_equal(a, b)
        assert np.array_equal(serial[i][0], cpu.fps(clouds[i], 4096))


@pytest.mark.gpu
def test_short_plain_layers_rows32_kernel(dev, cpu):
    """mlp_rows32_kernel (plain layers on <= 4096 rows, 256 <= K <= 1024): equal to the oracle at the MLP tolerance and BIT-identical
    to the 128-row layer kernel (the same rows inside a longer launch), ragged row counts, column tails, wider output buffers"""
    from pointrcnn_amd import ops
    rng = np.random.default_rng(3)
    for rows, K, N in ((2048, 1024, 512), (1, 256, 128), (33, 264, 200), (4096, 512, 512), (31, 1024, 130)):
        x = rng.normal(size=(8192, K)).astype(np.float32)
        w = (rng.normal(size=(N, K)) * 0.05).astype(np.float32)
        b = rng.normal(size=(N,)).astype(np.float32)
        xt = torch.from_numpy(x).to(dev)
        lin = ops.PackedLinear(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev), relu=True)
        long_run = ops.mlp_rows(xt, lin)                                  # 8192 rows: the layer kernel
        out = torch.full((rows, N + 7), -7.0, device=dev)
        ops.mlp_rows(xt[:rows], lin, out=(out, 3))                        # <= 4096 rows: the 32-row kernel, into a wider buffer
        got = out.cpu().numpy()
        assert np.array_equal(got[:, 3:3 + N], long_run[:rows].cpu().numpy())
        assert (got[:, :3] == -7.0).all() and (got[:, 3 + N:] == -7.0).all()
        ref = cpu.linear_rows(x[:rows], w, b, relu=True)
        assert np.abs(got[:, 3:3 + N] - ref).max() <= mlp_tol(ref)
    # device-side row count
    cnt = torch.tensor([100], dtype=torch.int32, device=dev)
    out = torch.zeros((4096, N), device=dev)
    ops.mlp_rows(xt[:4096], lin, out=(out, 0), rows_dev=cnt)
    assert np.array_equal(out[:100].cpu().numpy(), long_run[:100].cpu().numpy()) and not out[100:].any()
