"""GPU: the grouped stacks of an MSG set-abstraction level storing by destination (PRCNN_POOL_DIRECT; prcnn_group_compact_pair_dst,
prcnn_mlp_chain_group_multi_dst, prcnn_level_pool_residual) against the sequence they replace: every result row through the flat
buffer and the full pool launch.  A row that is its group's only one is the same float stored elsewhere, a dense group's pooled row
likewise, and the groups left to the pool run the same fmaxf chain over the same rows in the same order: every comparison is of
BITS (NaN included).  The clouds are built so that the group sizes are known: clusters far apart, each within both radii of its
centre, so a centre's group holds exactly its cluster in both scales."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
NS = (16, 32)
RADII = (0.25, 0.6)
# level -> (input feature channels, MLP specs of the two scales, the kernel body its stacks end in, has dense lists)
LEVELS = {
    "xyz_only": (0, [[0, 16, 16, 32], [0, 32, 32, 64]], "sa_xyz_chain_body", True),
    "hoisted_chain": (32, [[32, 64, 64, 128], [32, 64, 96, 128]], "mlp_chain_fast_body", True),
    "hoisted_stack": (32, [[32, 128, 196, 256], [32, 128, 196, 256]], "mlp_stack2_body", False),
}
MIXED = [1, 2, 1, 3, 1, 5, 1, 9, 1, 2, 1, 17]       # group sizes: solo, 2..T rows, above T of both scales (T = 4 / 8 where lists are dense)
PAIRS = [2, 3, 2, 4]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cloud(sizes, N, seed):
    """sizes: per frame the M group sizes.  -> xyz (B, N, 3), new_xyz (B, M, 3), per frame the point index of every centre"""
    rng = np.random.default_rng(seed)
    B, M = len(sizes), len(sizes[0])
    lattice = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 3.0
    xyz, ctr, where = np.empty((B, N, 3), np.float32), np.empty((B, M, 3), np.float32), []
    for b in range(B):
        assert sum(sizes[b]) <= N and M <= len(lattice)
        centres = lattice[rng.permutation(len(lattice))[:M]]
        pts = [centres]
        for k, s in enumerate(sizes[b]):
            pts.append(centres[k] + rng.uniform(-0.1, 0.1, (s - 1, 3)).astype(np.float32))       # within 0.18 of the centre: inside both radii
        pts = np.concatenate(pts)
        filler = lattice[:N - len(pts)] + np.float32(100.0)                                       # lone points nobody's ball reaches
        assert len(filler) == N - len(pts)
        pts = np.concatenate([pts, filler])
        perm = rng.permutation(N)
        xyz[b, perm] = pts
        ctr[b] = centres
        where.append(perm[:M])
    return torch.from_numpy(xyz).cuda(), torch.from_numpy(ctr).cuda(), where


def _module(level, seed=3):
    from pointnet2_lib.pointnet2 import pointnet2_modules as pm
    from pointrcnn_amd.rpn import randomize_bn_stats
    cin, mlps, _body, _dense = LEVELS[level]
    torch.manual_seed(seed)
    # (npoint only selects the ball-query groupers: every test passes its own centres as new_xyz)
    mod = pm.PointnetSAModuleMSG(npoint=128, radii=list(RADII), nsamples=list(NS), mlps=[list(m) for m in mlps], use_xyz=True, bn=True)
    return pm, randomize_bn_stats(mod).cuda().eval()


def _run(pm, mod, xyz, feat, new_xyz, direct):
    """-> output (B, C, M), [(return value of the multi launch, did its problems carry destinations)], the level's two GroupSplits"""
    from pointrcnn_amd import ops
    calls = []
    real_multi, real_merged = ops.mlp_chain_group_multi, mod._forward_merged

    def multi(problems):
        rc = real_multi(problems)
        calls.append((rc, [pr.get("dst") is not None for pr in problems]))
        return rc

    def merged(xyz_, new_xyz_, idxs, hoist, feat_cl, out_cl, c_outs):
        out_cl.fill_(SENTINEL)                              # every cell the level does not write stays visible
        return real_merged(xyz_, new_xyz_, idxs, hoist, feat_cl, out_cl, c_outs)

    keep = pm.POOL_DIRECT
    pm.POOL_DIRECT, ops.mlp_chain_group_multi, mod._forward_merged, ops._split_log = direct, multi, merged, []
    try:
        with torch.no_grad():
            out = mod(xyz, feat, new_xyz)[1].clone()
        torch.cuda.synchronize()
        return out, calls, list(ops._split_log)
    finally:
        pm.POOL_DIRECT, ops.mlp_chain_group_multi, ops._split_log = keep, real_multi, None
        del mod._forward_merged


def _lists(sp):
    """-> counts (flat rows, dense groups, sparse groups), solo / multi-row / dense group ids, the sparse groups' (id, first row, rows)"""
    rows, cd, cs = (int(v) for v in sp.counts.cpu())
    sl, so, sc = (t[:cs].cpu().numpy() for t in (sp.slist, sp.soff, sp.scnt))
    return (rows, cd, cs), sl[sc == 1], sl[sc > 1], sp.listn[:cd].cpu().numpy(), (sl, so, sc)


def _check_level(level, sizes, N=512, seed=0, feat_edit=None):
    """on against off on one cloud; -> the two GroupSplits of the on run, as _lists gives them"""
    cin, _mlps, _body, has_dense = LEVELS[level]
    pm, mod = _module(level)
    xyz, new_xyz, where = _cloud(sizes, N, seed)
    B, M = new_xyz.shape[:2]
    feat = torch.randn(B, cin, N, generator=torch.Generator().manual_seed(seed + 1)).cuda() if cin else None
    if feat_edit is not None:
        feat_edit(feat, where)
    on, calls_on, splits = _run(pm, mod, xyz, feat, new_xyz, True)
    off, calls_off, _ = _run(pm, mod, xyz, feat, new_xyz, False)
    nprob = 4 if has_dense else 2
    assert calls_on == [(True, [True] * nprob)], calls_on     # ONE multi launch, every problem storing by destination: no fallback
    assert calls_off == [(True, [False] * nprob)], calls_off
    assert torch.equal(_bits(on), _bits(off))
    assert not bool((on == SENTINEL).any()) and not bool((off == SENTINEL).any())       # every group row written, in every column
    assert len(splits) == 2
    out = []
    for sp, ns in zip(splits, NS):
        counts, solo, multi, dense, (sl, so, sc) = got = _lists(sp)
        T = ns // 4 if has_dense else ns
        # what the split must have found, from the cloud's construction
        flat_sizes = [min(s, ns) for fr in sizes for s in fr]
        assert counts == (sum(s for s in flat_sizes if s <= T), sum(s > T for s in flat_sizes), sum(s <= T for s in flat_sizes)), counts
        # solo, multi-row and dense groups: a partition of 0 .. G-1 -- each group's row has exactly one writer
        assert np.array_equal(np.sort(np.concatenate([solo, multi, dense])), np.arange(B * M))
        rdst = sp.rdst.view(-1).cpu().numpy()
        for g, o, c in zip(sl, so, sc):
            assert (rdst[o] == g) if c == 1 else bool((rdst[o:o + c] == -1).all()), (g, o, c)
        out.append(got)
    return out


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_all_one_row_groups_nothing_left_to_pool(dev, level):
    for counts, solo, multi, dense, _ in _check_level(level, [[1] * 128] * 2):
        assert counts == (256, 0, 256) and len(solo) == 256 and len(multi) == 0 and len(dense) == 0


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_solo_multi_row_and_dense_groups_in_one_launch(dev, level):
    sizes = [[MIXED[(k + 5 * b) % len(MIXED)] for k in range(128)] for b in range(2)]
    for counts, solo, multi, dense, _ in _check_level(level, sizes, seed=1):
        assert len(solo) > 0 and len(multi) > 0
        if LEVELS[level][3]:
            assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0 and len(dense) > 0
        else:
            assert len(dense) == 0                           # the stack scales send every group through the flat list


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_every_group_has_two_or_more_rows_nothing_stored_directly(dev, level):
    sizes = [[PAIRS[k % len(PAIRS)] for k in range(128)]] * 2
    for counts, solo, multi, dense, _ in _check_level(level, sizes, seed=2):
        assert len(solo) == 0 and len(multi) == 256 and len(dense) == 0


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_ragged_tiles_and_a_frame_with_fewer_hits(dev, level):
    """B = 3, M = 125: neither the groups nor the flat rows are a multiple of 32, the middle frame holds one-row groups only, and
    some multi-row group straddles a 32-row tile of the flat list"""
    sizes = [[MIXED[k % len(MIXED)] for k in range(125)], [1] * 125, [MIXED[(k + 7) % len(MIXED)] for k in range(125)]]
    for counts, solo, multi, dense, (sl, so, sc) in _check_level(level, sizes, seed=3):
        assert counts[0] % 32 != 0 and (3 * 125) % 32 != 0
        assert bool(((so // 32) != ((so + sc - 1) // 32)).any())


@pytest.mark.parametrize("level", ["hoisted_chain", "hoisted_stack"])
def test_nonfinite_feature_rows_keep_their_bits(dev, level):
    """frame 0: a row of +-inf, frame 1: a row of NaN, each at the centre of a one-row group, of a multi-row group and of a group above
    T (dense where the level has dense lists).  (the xyz-only level has no feature rows)"""
    sizes = [[MIXED[k % len(MIXED)] for k in range(128)]] * 2
    hit = []

    def edit(feat, where):
        for k in (0, 1, 11):                                # sizes 1, 2 and 17
            assert MIXED[k] == (1, 2, 17)[(0, 1, 11).index(k)]
            feat[0, 0::2, where[0][k]] = float("inf")
            feat[0, 1::2, where[0][k]] = float("-inf")
            feat[1, :, where[1][k]] = float("nan")
            hit.append(k)
    _check_level(level, sizes, seed=4, feat_edit=edit)
    assert hit == [0, 1, 11]


def test_non_finite_rows_reach_the_output(dev):
    """the same cloud once more, for the claim the test above rests on: the edited rows do change the groups they belong to"""
    pm, mod = _module("hoisted_chain")
    sizes = [[MIXED[k % len(MIXED)] for k in range(128)]] * 2
    xyz, new_xyz, where = _cloud(sizes, 512, 4)
    feat = torch.randn(2, 32, 512, generator=torch.Generator().manual_seed(5)).cuda()
    plain, _calls, _splits = _run(pm, mod, xyz, feat, new_xyz, True)
    feat[1, 0::2, where[1][0]] = float("inf")               # (a NaN activation is squashed by the ReLU's fmaxf(v, 0): infinities show)
    out, _calls, _splits = _run(pm, mod, xyz, feat, new_xyz, True)
    assert not torch.equal(_bits(out[1, :, 0]), _bits(plain[1, :, 0]))          # the one-row group of the edited point


# ------------------------------------------------------------------------------------------------ whole network
@pytest.mark.parametrize("clouds", ["uniform", "saturated"])
def test_rpn_outputs_keep_their_bits(dev, clouds):
    from pointnet2_lib.pointnet2 import pointnet2_modules as pm
    from pointrcnn_amd import rpn
    cfg = type("Cfg", (rpn.RPNConfig,), {"SA_NPOINTS": [512, 128, 32, 8], "NUM_POINTS": 2048})
    torch.manual_seed(3)
    model = rpn.randomize_bn_stats(rpn.RPN(cfg=cfg), seed=2).to(dev).eval()
    pts = {"uniform": rpn.synthetic_clouds, "saturated": rpn.saturated_clouds}[clouds](2, 2048, seed0=300).to(dev)
    keep = pm.POOL_DIRECT
    try:
        outs = []
        for direct in (True, False):
            pm.POOL_DIRECT = direct
            with torch.no_grad():
                outs.append({k: v.clone() for k, v in model({"pts_input": pts}).items()})
    finally:
        pm.POOL_DIRECT = keep
    for k in ("backbone_features", "rpn_cls", "rpn_reg"):
        assert torch.equal(_bits(outs[0][k]), _bits(outs[1][k])), k
