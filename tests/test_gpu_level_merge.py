"""GPU: both radii of an MSG set-abstraction level through one split, one grouped-stack and one pool launch
(prcnn_group_compact_pair, prcnn_mlp_chain_group_multi, prcnn_level_pool; pointnet2_modules._forward_merged) against the
per-radius launches they replace.  The merged launches run the same kernel bodies on the same rows, and the grouped stacks are
fp32 under both MLP arithmetics, so every comparison is torch.equal; list order alone is arbitrary (atomic appends) and lists are
compared as sets.  The widths are the RPN's: the instantiations exist only for them."""
import numpy as np
import pytest
import torch

from util import unit_cloud

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
# level -> (C of the gathered source, hoisted?, layer widths of scale a / b after the hoisted layer, nsample a / b, dense lists?)
LEVELS = {
    "sa1": (0, False, (16, 16, 32), (32, 32, 64), True),
    "sa2": (64, True, (64, 128), (96, 128), True),
    "sa3": (128, True, (196, 256), (196, 256), False),
    "sa4": (256, True, (256, 512), (384, 512), False),
}
NS = (16, 32)


def _layers(k, widths, seed):
    from pointrcnn_amd import ops
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in widths:
        w = (torch.randn(n, k, generator=g) * (1.0 / np.sqrt(k))).cuda()
        out.append(ops.PackedLinear(w, (torch.randn(n, generator=g) * 0.1).cuda(), relu=True))
        k = n
    return out


# ------------------------------------------------------------------------------------------------ split
def _hand_idx(B, M, N, ns, cnts, seed):
    """(B, M, ns) ball-query shaped indices: group g has cnts[g % len] strictly ascending hits, then its first hit repeated"""
    rng = np.random.default_rng(seed)
    idx = np.zeros((B * M, ns), np.int32)
    for g in range(B * M):
        c = cnts[g % len(cnts)]
        hits = np.sort(rng.choice(N, c, replace=False))
        idx[g, :c] = hits
        idx[g, c:] = hits[0]
    return torch.from_numpy(idx.reshape(B, M, ns)).cuda()


def _as_sets(sp):
    rows, cd, cs = (int(v) for v in sp.counts.cpu())
    sl, so, sc = (t[:cs].cpu().numpy() for t in (sp.slist, sp.soff, sp.scnt))
    ridx, rnx = sp.ridx.view(-1).cpu().numpy(), sp.rnx.view(-1, 3).cpu().numpy()
    sparse = {(int(g), int(c), tuple(ridx[o:o + c].tolist()), tuple(rnx[o:o + c].ravel().tolist())) for g, o, c in zip(sl, so, sc)}
    order = np.argsort(so)
    assert cs == 0 or (so[order][0] == 0 and np.array_equal(so[order][1:], np.cumsum(sc[order])[:-1]) and sc.sum() == rows)   # a partition
    ln = sp.listn[:cd].cpu().numpy()
    idxn, nxn = sp.idxn.view(-1, sp.ns)[:cd].cpu().numpy(), sp.nxn.view(-1, 3)[:cd].cpu().numpy()
    dense = {(int(g), tuple(i.tolist()), tuple(x.tolist())) for g, i, x in zip(ln, idxn, nxn)}
    assert len(sparse) == cs and len(dense) == cd
    return (rows, cd, cs), sparse, dense


@pytest.mark.parametrize("case", ["mixed", "all_sparse", "all_dense"])
def test_compact_pair_equals_two_compacts(dev, case):
    from pointrcnn_amd import ops
    B, N, M = 2, 256, 70                                   # 140 groups: not a multiple of 64, one 1024-thread block per scale
    T = {"mixed": (4, 8), "all_sparse": (16, 32), "all_dense": (1, 3)}[case]
    idxs = []
    for ns, t in zip(NS, T):
        cnts = {"mixed": [1, t, t + 1, ns, 2, ns - 1], "all_sparse": [1, t, ns - 1, 5], "all_dense": [t + 1, ns, ns - 1]}[case]
        idxs.append(_hand_idx(B, M, N, ns, cnts, seed=ns))
    new_xyz = torch.from_numpy(unit_cloud(B, M, seed=5)).cuda()
    a, b = ops.GroupSplit.pair(idxs[0], T[0], idxs[1], T[1], new_xyz, N)
    assert a.counts.data_ptr() + 12 == b.counts.data_ptr() and a.counts.shape == b.counts.shape == (3,)
    for sp, idx, t in ((a, idxs[0], T[0]), (b, idxs[1], T[1])):
        want = ops.GroupSplit(idx, new_xyz, N, t)
        got_counts, got_sparse, got_dense = _as_sets(sp)
        want_counts, want_sparse, want_dense = _as_sets(want)
        assert got_counts == want_counts and got_sparse == want_sparse and got_dense == want_dense
        assert (sp.G, sp.ns, sp.max_rows) == (want.G, want.ns, want.max_rows)
        assert torch.equal(sp.rows, want.rows) and torch.equal(sp.count_dense, want.count_dense) and torch.equal(sp.count_sparse, want.count_sparse)
        if case == "all_sparse":
            assert got_counts[1] == 0 and got_counts[2] == B * M
        if case == "all_dense":
            assert got_counts[0] == 0 and got_counts[1] == B * M
        if case == "mixed":
            assert got_counts[1] > 0 and got_counts[2] > 0


# ------------------------------------------------------------------------------------------------ grouped stacks
class _Problems:
    """the grouped-stack problems of one level shape on hand-made lists: flat b, flat a (, dense b, dense a), heaviest first"""

    def __init__(self, level, cap_flat, cap_dense, seed=0):
        C, hoisted, wa, wb, dense = LEVELS[level]
        g = torch.Generator().manual_seed(100 + seed)
        self.nsrc = 600
        self.xyz = torch.rand(1, self.nsrc, 3, generator=g).cuda()
        self.src = torch.randn(1, self.nsrc, C, generator=g).cuda() if C else None
        self.act = ((torch.randn(C, 3, generator=g) * 0.3).cuda(), (torch.randn(C, generator=g) * 0.1).cuda()) if hoisted else None
        self.layers = {16: _layers(C if C else 3, wa, 1), 32: _layers(C if C else 3, wb, 2)}
        self.specs = [(32, 1, cap_flat), (16, 1, cap_flat)] + ([(32, 32, cap_dense), (16, 16, cap_dense)] if dense else [])
        self.lists = []
        for scale, ns, cap in self.specs:
            idx = torch.randint(0, self.nsrc, (1, cap, ns), generator=g, dtype=torch.int32).cuda()
            ctr = torch.rand(1, cap, 3, generator=g).cuda()
            self.lists.append((idx, ctr))

    def problems(self, counts):
        """-> (list of mlp_chain_group keyword dicts, their sentinel-filled output buffers, the count tensors)"""
        prs, outs, keep = [], [], []
        for (scale, ns, cap), (idx, ctr), n in zip(self.specs, self.lists, counts):
            assert n <= cap
            out = torch.full((cap, self.layers[scale][-1].nout), SENTINEL, device="cuda")
            cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
            prs.append(dict(xyz=self.xyz, new_xyz=ctr, idx=idx, feat_cl=self.src, layers=self.layers[scale], out=(out, 0),
                            pool_ns=ns if ns > 1 else 0, act=self.act, groups_dev=cnt))
            outs.append(out)
            keep.append(cnt)
        return prs, outs, keep


def _multi_equals_separate(P, counts):
    from pointrcnn_amd import ops
    prs, want, _k1 = P.problems(counts)
    for pr in prs:
        ops.mlp_chain_group(**pr)
    prs, got, _k2 = P.problems(counts)
    assert ops.mlp_chain_group_multi(prs) is True
    torch.cuda.synchronize()
    for q, (w, g_, n) in enumerate(zip(want, got, counts)):
        assert torch.equal(w, g_), (q, n)
        assert bool((g_[n:] == SENTINEL).all()) and (n == 0 or bool((g_[:n] != SENTINEL).any())), (q, n)


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_multi_launch_equals_the_separate_launches(dev, level):
    """row counts 1, 31, 33, 70 (a single ragged 32-row tile, one row past a tile, ragged 128-row tiles), dealt differently to the
    problems; one problem empty; all empty: nothing is written"""
    P = _Problems(level, cap_flat=200, cap_dense=80)
    n = len(P.specs)
    for counts in ((70, 33, 31, 1), (1, 31, 33, 70), (33, 70, 0, 31), (31, 0, 1, 33), (0, 0, 0, 0)):
        _multi_equals_separate(P, counts[:n])


@pytest.mark.parametrize("level", ["sa1", "sa3", "sa4"])
def test_multi_launch_strides_across_the_problem_boundary(dev, level):
    """more work units than the problems' workgroups: the persistent SA-level-0 bodies (768 / 512 workgroups of four 32-row tiles)
    and the stacks under the launch's cap of 2048 workgroups walk their lists in several strides, next to a problem that does not.
    (the straight-line chains of SA2 have one workgroup per tile of capacity: no stride loop)"""
    big = 110000 if level == "sa1" else 41000            # > 768 * 128 rows; > 1024 tiles of 32 rows per problem
    P = _Problems(level, cap_flat=big, cap_dense=80, seed=1)
    counts = (big - 7, 4099, 33, 0) if level == "sa1" else (big - 7, big)
    _multi_equals_separate(P, counts[:len(P.specs)])


def test_multi_export_refuses_what_it_has_no_kernel_for(dev):
    from pointrcnn_amd import ops
    P = _Problems("sa2", cap_flat=70, cap_dense=40)
    prs, outs, _keep = P.problems((70, 33, 5, 5))
    # both problems on the SAME instance <2, 4, 0>: each is supported, the combination is not instantiated
    assert ops.mlp_chain_group_multi([prs[1], prs[1]]) is False
    # a stack the chain kernels have no instance for (64 -> 64 -> 64)
    odd = dict(prs[1], layers=_layers(64, (64, 64), 3), out=(torch.full((70, 64), SENTINEL, device="cuda"), 0))
    assert not ops.chain_supported(1, odd["layers"], 0)
    assert ops.mlp_chain_group_multi([prs[0], odd]) is False
    # problems of two different kernel families
    Q = _Problems("sa3", cap_flat=70, cap_dense=40)
    qrs, qouts, _keep2 = Q.problems((70, 33))
    assert ops.mlp_chain_group_multi([qrs[0], prs[0]]) is False
    torch.cuda.synchronize()
    for o in outs + qouts + [odd["out"][0]]:
        assert bool((o == SENTINEL).all())                 # nothing was launched


# ------------------------------------------------------------------------------------------------ pool
def test_level_pool_equals_segmax_scatter_and_scatter_rows(dev):
    from pointrcnn_amd import ops
    B, N, M = 2, 256, 70
    T = (4, 8)
    idxs = [_hand_idx(B, M, N, ns, [1, t, t + 1, ns, 2, ns - 1], seed=ns) for ns, t in zip(NS, T)]
    new_xyz = torch.from_numpy(unit_cloud(B, M, seed=5)).cuda()
    sps = ops.GroupSplit.pair(idxs[0], T[0], idxs[1], T[1], new_xyz, N)
    g = torch.Generator().manual_seed(9)
    widths, cols, ld = (32, 64), (3, 3 + 32), 3 + 32 + 64 + 5         # the two column ranges, with untouched columns before and after
    t1 = [torch.randn(sp.max_rows, w, generator=g).cuda() for sp, w in zip(sps, widths)]
    tn = [torch.randn(sp.G, w, generator=g).cuda() for sp, w in zip(sps, widths)]
    want = torch.full((B * M, ld), SENTINEL, device="cuda")
    for sp, a, d, c in zip(sps, t1, tn, cols):
        ops.segmax_scatter(a, sp, want, c)
        ops.scatter_rows(d, sp.listn, sp.count_dense, want, c)
    got = torch.full((B * M, ld), SENTINEL, device="cuda")
    ops.level_pool([(t1[1], sps[1], cols[1], "flat"), (t1[0], sps[0], cols[0], "flat"), (tn[1], sps[1], cols[1], "dense"),
                    (tn[0], sps[0], cols[0], "dense")], got)
    assert torch.equal(got, want)
    inside = torch.zeros(ld, dtype=torch.bool, device="cuda")
    inside[3:3 + 32 + 64] = True
    assert bool((got[:, inside] != SENTINEL).all())        # every group is in exactly one list of its scale: every cell written
    assert bool((got[:, ~inside] == SENTINEL).all())       # and nothing outside the two column ranges
    # each problem alone writes its own list's cells only: together they are a partition of the two ranges
    written = torch.zeros((B * M, ld), dtype=torch.int32, device="cuda")
    for pr in [(t1[0], sps[0], cols[0], "flat"), (t1[1], sps[1], cols[1], "flat"), (tn[0], sps[0], cols[0], "dense"), (tn[1], sps[1], cols[1], "dense")]:
        one = torch.full((B * M, ld), SENTINEL, device="cuda")
        ops.level_pool([pr], one)
        written += (one != SENTINEL).int()
    assert bool((written[:, inside] == 1).all()) and bool((written[:, ~inside] == 0).all())


# ------------------------------------------------------------------------------------------------ module
MODULES = {
    "sa1": (0, [[0, 16, 16, 32], [0, 32, 32, 64]]),
    "sa2": (96, [[96, 64, 64, 128], [96, 64, 96, 128]]),
    "sa3": (256, [[256, 128, 196, 256], [256, 128, 196, 256]]),
    "sa4": (512, [[512, 256, 256, 512], [512, 256, 384, 512]]),
}


def _module(mlps, cin, seed, batches=1):
    from pointnet2_lib.pointnet2 import pointnet2_modules as pm
    from pointrcnn_amd.rpn import randomize_bn_stats
    torch.manual_seed(seed)
    B, N = 2, 512
    mod = pm.PointnetSAModuleMSG(npoint=128, radii=[0.25, 0.6], nsamples=list(NS), mlps=[list(m) for m in mlps], use_xyz=True, bn=True)
    randomize_bn_stats(mod).cuda().eval()
    data = []
    for k in range(batches):
        base = unit_cloud(B, N, seed=seed + 31 * k)
        base[:, : N // 2] *= 0.15                          # half the points in a dense clump, the rest spread out: both lists populated
        base[:, N // 2:] *= 12.0
        data.append((torch.from_numpy(base).cuda(), torch.randn(B, cin, N, device="cuda") if cin else None))
    return pm, mod, data


def _forward(pm, mod, xyz, feat, merge, calls=None):
    from pointrcnn_amd import ops
    keep, real = pm.LEVEL_MERGE, ops.mlp_chain_group_multi

    def spy(problems):
        rc = real(problems)
        calls.append(rc)
        return rc
    pm.LEVEL_MERGE = merge
    if calls is not None:
        ops.mlp_chain_group_multi = spy
    try:
        with torch.no_grad():
            return mod(xyz, feat)[1].clone()
    finally:
        pm.LEVEL_MERGE, ops.mlp_chain_group_multi = keep, real


@pytest.mark.parametrize("level", sorted(MODULES))
def test_module_forward_merged_equals_per_radius_launches(dev, level):
    cin, mlps = MODULES[level]
    pm, mod, [(xyz, feat)] = _module(mlps, cin, seed=3)
    calls = []
    got = _forward(pm, mod, xyz, feat, True, calls)
    want = _forward(pm, mod, xyz, feat, False, calls)
    assert calls == [True]                                  # the merged path ran, with one grouped-stack launch; the other path never asks
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())


def test_module_forward_merged_in_a_replayed_graph(dev):
    """captured once, replayed on a second batch copied into the static input: the six counters of the split are cleared by a
    kernel node of the graph, as every counter of a capturable path (a memset node is what faulted replays before)"""
    cin, mlps = MODULES["sa2"]
    pm, mod, data = _module(mlps, cin, seed=4, batches=2)
    want = [_forward(pm, mod, x, f, False) for x, f in data]
    sx, sf = data[0][0].clone(), data[0][1].clone()
    keep = pm.LEVEL_MERGE
    pm.LEVEL_MERGE = True
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            mod(sx, sf)                                     # warm-up outside the capture (weight images, caches)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            out = mod(sx, sf)[1]
        for k in (0, 1, 0):
            sx.copy_(data[k][0])
            sf.copy_(data[k][1])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want[k]), k
    finally:
        pm.LEVEL_MERGE = keep


@pytest.mark.parametrize("kind", ["second_scale_on_layer_kernels", "combination_not_instantiated"])
def test_module_falls_back_to_the_per_radius_launches(dev, kind):
    """a level whose second scale has no chain instance never reaches the merged path; one whose scales are each supported but
    whose combination the multi export has no kernel for gets PRCNN_EUNSUPPORTED from it and issues the launches one by one"""
    mlps = {"second_scale_on_layer_kernels": [[96, 64, 64, 128], [96, 64, 64, 64]],
            "combination_not_instantiated": [[96, 64, 64, 128], [96, 64, 64, 128]]}[kind]
    pm, mod, [(xyz, feat)] = _module(mlps, 96, seed=5)
    calls = []
    got = _forward(pm, mod, xyz, feat, True, calls)
    assert calls == ([] if kind == "second_scale_on_layer_kernels" else [False])
    assert torch.equal(got, _forward(pm, mod, xyz, feat, False))
