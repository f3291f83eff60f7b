"""Neighbour search on the short levels and on partial chunks (csrc/neighbor.hip, csrc/grid.hip): scans that stop at the
frame's end, several lanes sharing one query, the grid staged in LDS, dense frames scanned inside the grid launch.  Every
result is compared with np.array_equal against the CPU oracle (float outputs with equal_nan: a query with fewer than three
finite neighbours has +inf distances and 0/0 weights on both sides)."""
import numpy as np
import pytest
import torch

from util import kitti_cloud

pytestmark = pytest.mark.gpu


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _three_nn(ops, unk, known, grid=None):
    B, n, _ = unk.shape
    m = known.shape[1]
    d2 = torch.empty((B, n, 3), device=unk.device)
    i3 = torch.empty((B, n, 3), dtype=torch.int32, device=unk.device)
    w3 = torch.empty((B, n, 3), device=unk.device)
    lib = ops._cabi.lib()
    if grid is None:
        ops._cabi.check(lib.prcnn_three_nn(unk.data_ptr(), known.data_ptr(), B, n, m, d2.data_ptr(), i3.data_ptr(), w3.data_ptr(), _stream()), "scan")
    else:
        ops._cabi.check(lib.prcnn_three_nn_grid(grid.buf.data_ptr(), unk.data_ptr(), B, n, m, d2.data_ptr(), i3.data_ptr(), w3.data_ptr(),
                                                _stream()), "grid")
    return d2.cpu().numpy(), i3.cpu().numpy(), w3.cpu().numpy()


def _known_sets(B, n, m, seed):
    """(name, unknown, known): random; duplicated points (ties go to the lower index); a query equal to a known point; all known
    points identical; NaN and +-inf rows in `known` together with a NaN query"""
    r = np.random.default_rng(seed)
    unk = kitti_cloud(B, n, seed=seed)
    known = kitti_cloud(B, m, seed=seed + 1)
    yield "random", unk, known
    dup = known.copy()
    dup[:, m // 2:] = dup[:, :m - m // 2]
    yield "duplicates", unk, dup
    eq = unk.copy()
    eq[:, 0] = known[:, m - 1]
    eq[:, n // 2] = dup[:, 0]
    yield "query_is_a_known_point", eq, dup
    yield "identical", unk, np.tile(known[:, :1], (1, m, 1))
    bad, ubad = known.copy(), unk.copy()
    bad[0, r.integers(0, m)] = np.nan
    bad[0, r.integers(0, m), 0] = np.inf
    bad[1, r.integers(0, m), 2] = -np.inf
    bad[1, 0] = np.nan
    ubad[0, n - 1] = np.nan
    ubad[1, 0, 1] = np.nan
    yield "nonfinite", ubad, bad


# m: 3 and 5 leave lanes without a candidate, 64 / 65 and 1 023 / 1 024 / 1 025 sit around the 8-candidate step and the 1 024-slot
# chunk; 130 is added to the issue's list because it is the only size here at which 16 lanes share a query (8, 32 and 64 come from
# the others)
@pytest.mark.parametrize("n", [1, 70, 256, 1030])
def test_three_nn_scan_on_short_and_partial_chunks(dev, cpu, n):
    from pointrcnn_amd import ops
    B = 2
    for m in (3, 5, 64, 65, 130, 256, 1023, 1024, 1025):
        for name, unk_np, known_np in _known_sets(B, n, m, seed=7 * m + n):
            d2, i3, w3 = _three_nn(ops, torch.from_numpy(unk_np).to(dev), torch.from_numpy(known_np).to(dev))
            od, oi = cpu.three_nn(unk_np, known_np)
            assert np.array_equal(i3, oi), (name, n, m)
            assert _same(d2, od), (name, n, m)
            assert _same(w3, cpu.three_weights(od)), (name, n, m)


def test_three_nn_one_lane_per_query_stops_at_the_frame_end(dev, cpu):
    """65 536 queries: the launch fills the chip, so every query keeps a lane of its own; the known sets end inside a chunk"""
    from pointrcnn_amd import ops
    B, n = 2, 32768
    for m in (5, 257, 1025):
        for name, unk_np, known_np in _known_sets(B, n, m, seed=m):
            if name in ("random", "nonfinite"):
                d2, i3, w3 = _three_nn(ops, torch.from_numpy(unk_np).to(dev), torch.from_numpy(known_np).to(dev))
                od, oi = cpu.three_nn(unk_np, known_np)
                assert np.array_equal(i3, oi) and _same(d2, od) and _same(w3, cpu.three_weights(od)), (name, m)


def _line_frames(N, M, order):
    """frame 0: the points k = 0 .. N-1 on the x axis, one unit apart, stored in `order`, so that distances are exact and the hit
    count of a radius is known; frame 1: N identical points.  Centroids of frame 0 cycle through: on a point, midway between two
    points, far away, NaN; the centroids of frame 1 sit on its point."""
    pts = np.zeros((2, N, 3), np.float32)
    pts[0, :, 0] = order.astype(np.float32)
    pts[1] = np.array([3.0, 1.0, 20.0], np.float32)
    q = np.zeros((2, M, 3), np.float32)
    j = (np.arange(M) * 37) % N
    q[0, :, 0] = j
    q[0, 1::4, 0] += 0.5
    q[0, 2::4, 0] = -1000.0
    q[0, 3::4] = np.nan
    q[1] = pts[1, 0]
    return pts, q


def _hit_counts(pts, q, radius):
    d = pts[0, None, :, 0].astype(np.float64) - q[0, :, None, 0].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (d * d < np.float32(radius) * np.float32(radius)).sum(1)


@pytest.mark.parametrize("N", [1, 7, 64, 255, 256, 257, 1024, 1025, 2047])
def test_ball_query_single_and_dual_on_short_frames(dev, cpu, N):
    """radii 0.25 (no hit between two points, one hit on a point), ns / 2 (exactly ns hits around a midpoint), 1e4 (every point);
    identity order puts a ball's hits in one run of consecutive indices, which crosses the segment boundaries of lanes that share
    a query; the shuffled order spreads them over the whole frame"""
    from pointrcnn_amd import ops
    lib = ops._cabi.lib()
    r = np.random.default_rng(N)
    seen = set()
    for order in (np.arange(N), r.permutation(N)):
        for M in (1, 63, 64, 65, 100):
            pts, q = _line_frames(N, M, order)
            x, qq = torch.from_numpy(pts).to(dev), torch.from_numpy(q).to(dev)
            want = {}

            def oracle(radius, ns):
                if (radius, ns) not in want:
                    want[radius, ns] = cpu.ball_query(radius, ns, pts, q)
                    for c in _hit_counts(pts, q, radius):
                        seen.add("none" if c == 0 else "one" if c == 1 else "exact" if c == ns else "more" if c > ns else "some")
                return want[radius, ns]

            for ns in (1, 16, 32, 64):
                for radius in (0.25, ns / 2.0, 1e4):
                    out = torch.empty((2, M, ns), dtype=torch.int32, device=dev)
                    ops._cabi.check(lib.prcnn_ball_query(x.data_ptr(), qq.data_ptr(), 2, N, M, radius, ns, out.data_ptr(), _stream()), "single")
                    got = out.cpu().numpy()
                    assert np.array_equal(got, oracle(radius, ns)), (N, M, ns, radius)
                    if N >= ns:                # identical points, a centroid on them: the first ns indices
                        assert np.array_equal(got[1], np.tile(np.arange(ns, dtype=np.int32), (M, 1)))
            for (ra, nsa), (rb, nsb) in (((0.25, 1), (1e4, 1)), ((8.0, 16), (16.0, 32)), ((1e4, 16), (0.25, 32)), ((16.0, 16), (8.0, 32))):
                oa = torch.empty((2, M, nsa), dtype=torch.int32, device=dev)
                ob = torch.empty((2, M, nsb), dtype=torch.int32, device=dev)
                ops._cabi.check(lib.prcnn_ball_query2(x.data_ptr(), qq.data_ptr(), 2, N, M, ra, nsa, oa.data_ptr(), rb, nsb, ob.data_ptr(),
                                                      _stream()), "dual")
                assert np.array_equal(oa.cpu().numpy(), oracle(ra, nsa)), (N, M, ra, nsa)
                assert np.array_equal(ob.cpu().numpy(), oracle(rb, nsb)), (N, M, rb, nsb)
    if N >= 256:                               # the cases the radii were chosen for did occur
        assert {"none", "one", "exact", "more"} <= seen, seen


def test_ball_query_one_lane_per_centroid_stops_at_the_frame_end(dev, cpu):
    """65 536 centroids (a launch that fills the chip) on frames that end inside a chunk"""
    from pointrcnn_amd import ops
    lib = ops._cabi.lib()
    M = 32768
    for N in (255, 1025):
        pts, q = _line_frames(N, M, np.random.default_rng(N).permutation(N))
        x, qq = torch.from_numpy(pts).to(dev), torch.from_numpy(q).to(dev)
        oa = torch.empty((2, M, 16), dtype=torch.int32, device=dev)
        ob = torch.empty((2, M, 32), dtype=torch.int32, device=dev)
        ops._cabi.check(lib.prcnn_ball_query2(x.data_ptr(), qq.data_ptr(), 2, N, M, 8.0, 16, oa.data_ptr(), 1e4, 32, ob.data_ptr(), _stream()), "dual")
        assert np.array_equal(oa.cpu().numpy(), cpu.ball_query(8.0, 16, pts, q)), N
        assert np.array_equal(ob.cpu().numpy(), cpu.ball_query(1e4, 32, pts, q)), N


@pytest.mark.parametrize("m", [1024, 1500, 4096, 4097])
def test_three_nn_grid_staged_and_in_place(dev, cpu, m):
    """64-cell grids of up to 4 096 points are searched from LDS, 128-cell grids and larger frames in place.  Frame 0 is a
    KITTI-like cloud, frame 1 a tight cluster; with a 500 m minimum cell every known point of both falls into one cell.  The
    queries overlap the known points' bounding box and reach outside it; two are not finite."""
    from pointrcnn_amd import ops
    n = 3000
    known_np = kitti_cloud(2, m, seed=m)
    known_np[1] = known_np[1] * 0.01 + np.array([2.0, 1.0, 30.0], np.float32)
    known_np[0, m // 2:] = known_np[0, :m - m // 2]                     # exact duplicates: index ties
    unk_np = (kitti_cloud(2, n, seed=11) * np.array([1.3, 1.0, 1.2], np.float32) - np.array([5, 0, 8], np.float32)).astype(np.float32)
    unk_np[0, 3] = np.nan
    unk_np[1, 9, 0] = np.inf
    known, unk = torch.from_numpy(known_np).to(dev), torch.from_numpy(unk_np).to(dev)
    od, oi = cpu.three_nn(unk_np, known_np)
    ow = cpu.three_weights(od)
    sd, si, sw = _three_nn(ops, unk, known)
    assert np.array_equal(si, oi) and _same(sd, od) and _same(sw, ow)
    for cells, min_cell in ((64, 0.0), (128, 0.0), (64, 500.0), (128, 500.0)):
        g = ops.Grid(known, min_cell, cells)
        d2, i3, w3 = _three_nn(ops, unk, known, grid=g)
        assert np.array_equal(i3, oi), (cells, min_cell)
        assert _same(d2, od) and _same(w3, ow), (cells, min_cell)
        assert np.array_equal(d2.view(np.int32), sd.view(np.int32)) and np.array_equal(w3.view(np.int32), sw.view(np.int32))


def test_ball_query_grid_scans_dense_frames_in_the_same_launch(dev, cpu):
    """a batch mixing sparse and dense frames (as test_gpu_grid's dense-frame test builds it): the grid launch, which scans the
    dense frames itself, against the scan export, the oracle and the grid kernel on every frame (xyz=None)"""
    from pointrcnn_amd import ops
    lib = ops._cabi.lib()
    r = np.random.default_rng(3)
    N, M = 16384, 1000                         # M is no multiple of the 64-centroid block
    sparse = kitti_cloud(1, N, seed=21)[0]
    cube = (r.random((N, 3), dtype=np.float32) * 1.6 + np.array([-0.8, 0.2, 20.0], np.float32)).astype(np.float32)
    medium = (r.random((N, 3), dtype=np.float32) * np.array([12, 3, 12], np.float32)).astype(np.float32)
    pts = np.stack([cube, sparse, medium, cube[::-1].copy()])
    q_np = np.ascontiguousarray(pts[:, ::N // M][:, :M])
    q_np[0, 5] = np.nan
    x, q = torch.from_numpy(pts).to(dev), torch.from_numpy(q_np).to(dev)
    ra, nsa, rb, nsb = 0.1, 16, 0.5, 32
    g = ops.Grid(x, rb, 128)
    fb = lib.prcnn_grid_bytes(1, N)
    cand = [float(g.buf[f * fb: f * fb + 32].view(torch.float32)[5].item()) for f in range(4)]
    assert cand[0] > N / 32 > cand[1] and cand[3] > N / 32, cand                 # both kinds of frame are in the batch
    ga, gb = ops.ball_query_grid(g, q, ra, nsa, rb, nsb, xyz=x)
    ha, hb = ops.ball_query_grid(g, q, ra, nsa, rb, nsb)
    sa, sb = torch.empty_like(ga), torch.empty_like(gb)
    ops._cabi.check(lib.prcnn_ball_query2(x.data_ptr(), q.data_ptr(), 4, N, M, ra, nsa, sa.data_ptr(), rb, nsb, sb.data_ptr(), _stream()), "scan")
    assert torch.equal(ga, sa) and torch.equal(gb, sb)
    assert torch.equal(ha, sa) and torch.equal(hb, sb)
    assert np.array_equal(ga.cpu().numpy(), cpu.ball_query(ra, nsa, pts, q_np))
    assert np.array_equal(gb.cpu().numpy(), cpu.ball_query(rb, nsb, pts, q_np))
    for xyz in (x, None):                      # one radius, and lists larger than the scan's chunk
        assert torch.equal(ops.ball_query_grid(g, q, rb, nsb, xyz=xyz), sb)
    big = ops.ball_query_grid(g, q, rb, 100, 0.3, 40, xyz=x)
    assert np.array_equal(big[0].cpu().numpy(), cpu.ball_query(rb, 100, pts, q_np))
    assert np.array_equal(big[1].cpu().numpy(), cpu.ball_query(0.3, 40, pts, q_np))


def test_rpn_forward_neighbour_outputs_are_the_same_in_a_graph_replay(dev):
    """one RPN forward of 2 frames x 16 384 points, eager and replayed from a captured graph: every ball-query and three_nn output
    of every level is equal (no allocation, no synchronisation and no host-side state in the new launches)"""
    from pointrcnn_amd import ops, rpn
    torch.manual_seed(11)
    model = rpn.randomize_bn_stats(rpn.RPN(), seed=3).to(dev).eval()
    clouds = rpn.synthetic_clouds(2, 16384, seed0=500).to(dev)
    saved = {name: getattr(ops, name) for name in ("ball_query2", "three_nn")}
    rec = []

    def bq2(*a, **k):
        out = saved["ball_query2"](*a, **k)
        rec.extend(out)
        return out

    def nn(unknown, known, want_weight=False):
        out = saved["three_nn"](unknown, known, want_weight=want_weight)
        rec.extend(out)
        return out
    ops.ball_query2, ops.three_nn = bq2, nn
    try:
        inp = clouds.clone()
        with torch.no_grad():
            model({"pts_input": inp})
        torch.cuda.synchronize()
        eager = [t.clone() for t in rec]
        del rec[:]
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph, stream=stream):
            model({"pts_input": inp})
    finally:
        ops.ball_query2, ops.three_nn = saved["ball_query2"], saved["three_nn"]
    assert len(rec) == len(eager) == 4 * 2 + 4 * 3
    for t in rec:
        t.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for k, (got, want) in enumerate(zip(rec, eager)):
        assert torch.equal(got, want), k
