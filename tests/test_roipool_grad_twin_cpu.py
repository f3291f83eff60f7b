"""The numpy twins of the RoI pooling's selection and gradient (tests/roipool_grad_twin.py) against the CPU oracle and against a
dense statement of the closed form, on the constructed scene; and the Python surface of the joint step (no device needed)."""
import inspect

import numpy as np

import roipool_grad_twin as tw


def _scene(cpu):
    xyz, boxes = tw.constructed_scene()
    cats = tw.scene_categories(cpu, xyz, boxes)
    # a scene that lacks a category is a test error: assert the construction before anything is compared
    for c in cats:
        assert c["counts"] == list(tw.SCENE_COUNTS) + [17], c
        assert c["shared"] >= 3 and c["identical"] and c["free"] >= 1, c
    return xyz, boxes


def test_constructed_scene_holds_every_category(cpu):
    xyz, boxes = _scene(cpu)
    assert xyz.shape == (2, 1000, 3) and boxes.shape == (2, 8, 7)
    idx, distinct = tw.index_twin(cpu, xyz, boxes, tw.SCENE_S)
    assert distinct.tolist() == [[0, 1, 5, 15, 16, 16, 16, 16]] * 2            # min(points, S)
    assert (idx[:, 0] == -1).all() and (idx[:, 1:] >= 0).all()
    # the in-box points are not the first indices of the frame: truncation at S and the ascending order are exercised
    assert idx.max() > 900 and (np.diff(idx[0, 6]) > 0).all()


def test_index_twin_reproduces_the_oracle_pooling_bit_for_bit(cpu):
    xyz, boxes = _scene(cpu)
    rng = np.random.default_rng(1)
    for C in (3, 130):
        feat = rng.normal(size=(2, 1000, C)).astype(np.float32)
        want, empty = cpu.roipool3d(xyz, boxes, feat, tw.SCENE_S)
        idx, distinct = tw.index_twin(cpu, xyz, boxes, tw.SCENE_S)
        assert np.array_equal(tw.gather_twin(xyz, feat, idx).view(np.uint32), want.view(np.uint32))
        assert np.array_equal(distinct == 0, empty != 0)
        s = np.arange(tw.SCENE_S)
        for b in range(2):
            for m in range(8):
                if distinct[b, m]:
                    assert np.array_equal(idx[b, m], idx[b, m][s % distinct[b, m]])


def test_grad_twins_are_the_closed_form(cpu):
    xyz, boxes = _scene(cpu)
    N, S, C, col0 = 1000, tw.SCENE_S, 7, 5
    idx, _ = tw.index_twin(cpu, xyz, boxes, S)
    rng = np.random.default_rng(2)
    g = rng.normal(size=(2, 8, S, col0 + C + 2)).astype(np.float32)
    g[:, 0] = np.nan                                                         # the empty RoI's rows are never read
    f64, n, mag = tw.grad_twin(g, idx, N, C, col0)
    # dense statement: one-hot selection matrix times the gradient rows
    for b in range(2):
        onehot = (idx[b].reshape(-1, 1) == np.arange(N)[None, :]).astype(np.float64)        # (M S, N)
        rows = np.nan_to_num(g[b].reshape(-1, g.shape[-1])[:, col0:col0 + C].astype(np.float64))
        assert np.allclose(onehot.T @ rows, f64[b], rtol=0, atol=1e-12)
        assert np.array_equal(onehot.sum(0).astype(np.int64), n[b])
    assert np.isfinite(f64).all() and n.max() == S and (n == 0).any()         # the one-point RoI: S references to one point
    assert (n[0][idx[0, 5]] >= 2).all()                                      # the identical pair: every point referenced from both
    f32 = tw.grad_twin_f32_sequential(g, idx, N, C, col0)
    assert f32.dtype == np.float32 and np.isfinite(f32).all()
    assert (np.abs(f32.astype(np.float64) - f64) <= n[..., None] * 2.0 ** -24 * mag).all()
    # integer addends: every partial sum is exact, the two twins agree to the bit
    gi = rng.integers(-4, 5, size=g.shape).astype(np.float32)
    assert np.array_equal(tw.grad_twin_f32_sequential(gi, idx, N, C, col0), tw.grad_twin(gi, idx, N, C, col0)[0].astype(np.float32))


def test_joint_step_python_surface():
    """the opt-in arguments exist with defaults that leave today's routes alone"""
    from pointrcnn_amd import ops, point_rcnn, proposal_target_layer, rcnn, train_functions as tf
    assert inspect.signature(point_rcnn.PointRCNN.__init__).parameters["rpn_fixed"].default is True
    assert inspect.signature(rcnn.RCNNNet.__init__).parameters["pool_grad"].default is False
    assert inspect.signature(proposal_target_layer.ProposalTargetLayer.__init__).parameters["pool_grad"].default is False
    assert inspect.signature(ops.roipool3d).parameters["want_index"].default is False
    p = inspect.signature(tf.JointTrainer.__init__).parameters
    assert p["pool_grad"].default is False and p["fused_loss"].default is None and p["optimizer"].default is None
    assert "next_batch" in inspect.signature(tf.JointTrainer.step).parameters            # what train_loop.TrainLoop looks for
    assert hasattr(ops, "roipool3d_grad") and issubclass(proposal_target_layer.RoIPoolFeatures, __import__("torch").autograd.Function)
