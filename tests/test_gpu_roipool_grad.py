"""prcnn_roipool3d_index (the pooling that reports its selection) and prcnn_roipool3d_grad (the pooling's gradient with respect to
the per-point features, a gather without float atomics) against the numpy twins of tests/roipool_grad_twin.py.

The reference's roipool3d has no backward, so nothing there pins this gradient: the tests pin it to the closed form
    gfeat[b, p, c] = sum over (m, s) with idx[b, m, s] == p of gpooled[b, m, s, col0 + c]
-- bit for bit where every partial sum is exact (integer addends), bit for bit against the float32 twin that adds in the contract's
order (ascending (m, s)), and within n 2^-24 sum|addends| of the float64 twin (first-order bound of an n-term float32 sum)."""
import ctypes

import numpy as np
import pytest
import torch

import roipool_grad_twin as tw

pytestmark = pytest.mark.gpu

_CACHE = {}


def _scene(cpu, dev):
    """the constructed scene, its twin selection and the device's, computed once and left unchanged"""
    if "scene" not in _CACHE:
        from pointrcnn_amd import ops
        xyz, boxes = tw.constructed_scene()
        for c in tw.scene_categories(cpu, xyz, boxes):
            assert c["counts"] == list(tw.SCENE_COUNTS) + [17] and c["shared"] >= 3 and c["identical"] and c["free"] >= 1, c
        idx, distinct = tw.index_twin(cpu, xyz, boxes, tw.SCENE_S)
        _CACHE["scene"] = (xyz, boxes, idx, distinct, torch.from_numpy(xyz).to(dev), torch.from_numpy(boxes).to(dev),
                           torch.from_numpy(idx).to(dev), torch.from_numpy(distinct).to(dev))
        assert ops.ROIPOOL_BINS and boxes.shape[1] >= ops.ROIPOOL_BINS_MIN_BOXES          # the default route here is the binned form
    return _CACHE["scene"]


@pytest.mark.parametrize("C", [3, 130])
def test_selection_matches_twin_and_existing_export(cpu, dev, C):
    from pointrcnn_amd import ops
    xyz, boxes, idx, distinct, dxyz, dboxes, _, _ = _scene(cpu, dev)
    S = tw.SCENE_S
    feat = torch.randn((2, 1000, C), generator=torch.Generator().manual_seed(C)).to(dev)
    got = {}
    for form in ("bins", "linear"):
        ops.ROIPOOL_BINS = form == "bins"
        try:
            pooled0, empty0 = ops.roipool3d(dxyz, dboxes, feat, S)
            got[form] = ops.roipool3d(dxyz, dboxes, feat, S, want_index=True)
        finally:
            ops.ROIPOOL_BINS = True
        pooled, empty, didx, ddist = got[form]
        assert torch.equal(pooled, pooled0) and torch.equal(empty, empty0), form
        assert didx.dtype == torch.int32 and ddist.dtype == torch.int32
        assert np.array_equal(didx.cpu().numpy(), idx) and np.array_equal(ddist.cpu().numpy(), distinct), form
        assert torch.equal(ddist == 0, empty != 0)
        for b in range(2):
            live = didx[b] >= 0
            assert torch.equal(pooled[b][..., 3:][live], feat[b][didx[b][live].long()])
            assert torch.equal(pooled[b][..., :3][live], dxyz[b][didx[b][live].long()])
            assert (pooled[b][~live] == 0).all()
    for a, b in zip(got["bins"], got["linear"]):
        assert torch.equal(a, b)


def _check_grad(dev, idx, didx, ddist, N, C, col0, pad_g, pad_out, seed):
    """integer and standard-normal gpooled of row stride col0 + C + pad_g into NaN-filled rows of stride C + pad_out"""
    from pointrcnn_amd import ops
    B, M, S = idx.shape
    rng = np.random.default_rng(seed)
    W = col0 + C + pad_g
    empty_rois = idx[:, :, 0] < 0
    figures = {}
    for kind in ("integer", "normal"):
        g = rng.integers(-4, 5, size=(B, M, S, W)).astype(np.float32) if kind == "integer" else rng.normal(size=(B, M, S, W)).astype(np.float32)
        g[empty_rois] = np.nan                                     # rows of an empty RoI must never be read
        dg = torch.from_numpy(g).to(dev)
        out = torch.full((B, N, C + pad_out), float("nan"), device=dev)
        ret = ops.roipool3d_grad(dg, didx, ddist, N, C, col0=col0, out=out)
        assert ret is out
        got = out[..., :C]
        assert torch.isfinite(got).all(), "%s: NaN left or leaked" % kind
        assert torch.isnan(out[..., C:]).all(), "%s: columns beyond C written" % kind
        again = ops.roipool3d_grad(dg, didx, ddist, N, C, col0=col0)
        assert again.shape == (B, N, C) and torch.equal(again, got), "%s: two calls differ" % kind
        f64, n, mag = tw.grad_twin(np.nan_to_num(g), idx, N, C, col0)
        gn = got.cpu().numpy()
        assert (gn[n == 0] == 0).all() and not np.signbit(gn[n == 0]).any()                 # unreferenced points: an exact +0
        if kind == "integer":
            assert np.array_equal(gn, f64.astype(np.float32))
        else:
            err = np.abs(gn.astype(np.float64) - f64)
            bound = n[..., None] * 2.0 ** -24 * mag
            figures["worst err / bound"] = float((err / np.maximum(bound, 1e-300)).max())
            print("roipool3d_grad C=%d col0=%d ld_g=%d N=%d M=%d S=%d: max |dev - f64| %.3e, worst err/bound %.3f, max refs %d"
                  % (C, col0, W, N, M, S, err.max(), figures["worst err / bound"], n.max()))
            assert (err <= bound).all()
            assert np.array_equal(gn, tw.grad_twin_f32_sequential(np.nan_to_num(g), idx, N, C, col0))
    return figures


# (C, col0, extra columns of gpooled, extra columns of gfeat): ld_g > col0 + C and ld_out > C throughout; the last two are the
# layouts whose rows are 16-byte aligned (the float4 form of the gather), every other one takes the single-float form
@pytest.mark.parametrize("C,col0,pad_g,pad_out", [(1, 5, 2, 3), (3, 5, 1, 1), (128, 5, 3, 2), (130, 5, 1, 6), (256, 5, 2, 1),
                                                  (128, 4, 4, 4), (256, 0, 8, 4)])
def test_gradient_exact_float_and_layout(cpu, dev, C, col0, pad_g, pad_out):
    _, _, idx, distinct, _, _, didx, ddist = _scene(cpu, dev)
    _check_grad(dev, idx, didx, ddist, 1000, C, col0, pad_g, pad_out, seed=C + col0)


def test_gradient_at_the_rcnn_step_shape(cpu, dev):
    """N = 16 384, M = 64, S = 512, the RCNN step's column layout (col0 = 5 of 133 + padding): more than one point chunk of the
    list builder, RoIs from empty to far beyond S points, the selection taken from the device and checked against the twin"""
    from pointrcnn_amd import ops, rpn
    B, N, M, S = 2, 16384, 64, 512
    xyz = rpn.synthetic_clouds(B, N, seed0=40)
    g = torch.Generator().manual_seed(9)
    ctr = torch.gather(xyz, 1, torch.randint(0, N, (B, M), generator=g)[..., None].expand(-1, -1, 3))
    size = torch.tensor([2.0, 1.0, 3.0, 6.0, 12.0, 40.0])[torch.randint(0, 6, (B, M), generator=g)]            # a few to thousands of points
    boxes = torch.cat([ctr[..., 0:1], ctr[..., 1:2] + 2.0, ctr[..., 2:3], torch.full((B, M, 1), 4.0), size[..., None], size[..., None],
                       torch.rand((B, M, 1), generator=g) * 6.283 - 3.1416], 2).contiguous()
    boxes[:, 0, 0] = 500.0                                                                                   # an empty RoI per frame
    boxes[:, 5] = boxes[:, 4]                                                                                # two identical RoIs
    dxyz, dboxes = xyz.to(dev), boxes.to(dev)
    feat = torch.randn((B, N, 4), generator=g).to(dev)
    pooled, empty, didx, ddist = ops.roipool3d(dxyz, dboxes, feat, S, want_index=True)
    p0, e0 = ops.roipool3d(dxyz, dboxes, feat, S)
    assert torch.equal(pooled, p0) and torch.equal(empty, e0)
    idx, distinct = tw.index_twin(cpu, xyz.numpy(), boxes.numpy(), S)
    assert np.array_equal(didx.cpu().numpy(), idx) and np.array_equal(ddist.cpu().numpy(), distinct)
    assert distinct.min() == 0 and distinct.max() == S and ((distinct > 0) & (distinct < 64)).any()
    _check_grad(dev, idx, didx, ddist, N, 128, 5, 3, 0, seed=77)


def test_rejected_domains_launch_nothing(cpu, dev):
    from pointrcnn_amd import _cabi, ops
    _, _, idx, distinct, _, _, didx, ddist = _scene(cpu, dev)
    L = _cabi.lib()
    B, M, S = idx.shape
    N, C = 1000, 8
    g = torch.randn((B, M, S, 300), device=dev)
    out = torch.full((B, N, 300), 7.0, device=dev)
    work = torch.empty((L.prcnn_roipool3d_grad_work_bytes(B, N, M, S),), dtype=torch.uint8, device=dev)
    assert work.numel() == 4 * (B * (N + 1) + B * M * S)

    def call(ld_g=300, col0=0, N=N, M=M, S=S, C=C, ld_out=300, w=work):
        return L.prcnn_roipool3d_grad(g.data_ptr(), ld_g, col0, didx.data_ptr(), ddist.data_ptr(), B, N, M, S, C, out.data_ptr(), ld_out,
                                      None if w is None else w.data_ptr(), 0 if w is None else w.numel(), torch.cuda.current_stream().cuda_stream)

    unsupported, invalid = _cabi.EUNSUPPORTED, -1
    assert call(C=257) == unsupported and call(N=65537) == unsupported and call(S=513) == unsupported
    assert call(M=1 << 22, S=512) == unsupported                                             # M S = 2^31
    assert call(C=0) == invalid and call(ld_g=7) == invalid and call(col0=296) == invalid and call(ld_out=7) == invalid
    assert call(w=None) == invalid and call(col0=-1) == invalid
    assert L.prcnn_roipool3d_grad_work_bytes(B, 65537, M, S) == 0 and L.prcnn_roipool3d_grad_work_bytes(B, N, M, 513) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises(_cabi.PointOpsError):
        ops.roipool3d_grad(torch.zeros((B, M, S, 257), device=dev), didx, ddist, N)
    assert call() == 0                                                                        # the accepted call does write
    torch.cuda.synchronize()
    assert not (out[..., :C] == 7.0).any() and (out[..., C:] == 7.0).all()
    assert ctypes.sizeof(ctypes.c_size_t) == 8


def test_autograd_node(cpu, dev):
    from pointrcnn_amd import ops
    from pointrcnn_amd.proposal_target_layer import RoIPoolFeatures
    _, _, idx, distinct, dxyz, dboxes, _, _ = _scene(cpu, dev)
    S, N, C = tw.SCENE_S, 1000, 12
    gen = torch.Generator().manual_seed(4)
    feat = torch.randn((2, N, C), generator=gen).to(dev).requires_grad_(True)
    extra = torch.randn((2, N), generator=gen).to(dev).requires_grad_(True)
    xyz_g, boxes_g = dxyz.clone().requires_grad_(True), dboxes.clone().requires_grad_(True)
    with torch.no_grad():
        pooled, _, didx, ddist = ops.roipool3d(dxyz, dboxes, torch.cat([extra[..., None], feat], 2), S, want_index=True)
    cols = pooled[..., 4:]
    out = RoIPoolFeatures.apply(feat, cols, didx, ddist, xyz_g, boxes_g, extra)
    assert out.requires_grad and torch.equal(out, cols) and out.data_ptr() == cols.data_ptr()      # handed out, not pooled again
    w = torch.randn(out.shape, generator=gen).to(dev)
    w[didx[..., None].expand_as(w) < 0] = float("nan")
    grads = torch.autograd.grad((out * w)[didx >= 0].sum(), [feat, xyz_g, boxes_g, extra], allow_unused=True)
    assert grads[1] is None and grads[2] is None and grads[3] is None
    want = ops.roipool3d_grad(torch.nan_to_num(w), didx, ddist, N)
    assert torch.equal(grads[0], want)
    # through a torch.cat, as RCNNNet builds pts_input: the gradient reaches the node as a column slice of the wider rows
    out2 = RoIPoolFeatures.apply(feat, cols.reshape(-1, S, C), didx, ddist, xyz_g, boxes_g, extra)
    full = torch.cat((pooled[..., :4].reshape(-1, S, 4), out2), 2)
    wf = torch.randn(full.shape, generator=gen).to(dev)
    (g2,) = torch.autograd.grad((full * wf).sum(), [feat])
    assert torch.equal(g2, ops.roipool3d_grad(wf, didx, ddist, N, C, col0=4))
