"""The case table of the training SharedMLP (pointrcnn_amd/csrc/mlp_train.h through pointrcnn_amd/train_mlp.py), shared by
tests/test_train_stack_variants_cpu.py (the table reaches every kernel variant) and tests/test_gpu_train_stack_f64.py (every case
against float64), with the seeded CPU inputs of a case and the float64 restatement of one SharedMLPTrain invocation in closed form.

A case is one SharedMLPTrain.apply: source (plain rows, nsample-padded groups, padding-free groups = "flat", 3-NN interpolation),
the shape that fixes the row count, the channel list [K0, N1, ...], BatchNorm or Conv(+bias) -> ReLU, pooled or not, whether the
inputs take a gradient, and native switches.  The shapes are the smallest that reach each variant: derived from the dispatch in
prcnn_train_stack_fwd / _bwd and wgrad_plan, confirmed by tests/train_launch_record.cpp.  A variant added to the dispatch later
must get a case here, or the CPU coverage test fails.

The closed form (`reference`) works on the nsample-PADDED rows for both grouped forms: ball_query pads a group with copies of its
first hit, the reference network pushes every copy through every layer, and the padding-free rows of the device (distinct rows +
multiplicities, the rule at bwd_dy4) must give the same numbers row for row; `Rows` maps the device's rows to the padded ones.
Where float64 cannot tell (a pre-activation within 1e-5 of zero, two rows of a group within 1e-5 of the maximum) the reference
takes the decision it is handed (the device's), and `check_decisions` holds the device to float64 everywhere else."""
import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
EPS, MOMENTUM = 1e-5, 0.1
BAND = 1e-5                        # relative width of the bands inside which a decision is taken from the device
MAX_BAND_SHARE = 1e-3              # of the mask entries + arg slots of a case


class Case:
    def __init__(self, name, source, chans, bn=True, bias=True, pool=False, need_x=True, switches=None, cloud="mixed", **shape):
        assert source in ("plain", "group", "flat", "interp")
        self.name, self.source, self.chans, self.bn, self.bias, self.need_x = name, source, list(chans), bn, bias, need_x
        self.pool = pool or source == "flat"                      # padding-free rows are always pooled
        self.switches, self.cloud, self.shape = dict(switches or {}), cloud, shape

    def __repr__(self):
        return self.name

    @property
    def rows(self):
        """the host-side row count (flat: the padded count B * M * ns, what the launcher sizes its grids by)"""
        s = self.shape
        return s["R"] if self.source == "plain" else s["B"] * s["n"] if self.source == "interp" else s["B"] * s["M"] * s["ns"]

    @property
    def pool_ns(self):
        return self.shape["ns"] if self.pool else 0

    def recorder_args(self):
        """arguments of `train_launch_record --case`"""
        return ([self.source, str(self.rows), str(self.pool_ns), str(int(self.bn)), str(int(self.need_x)),
                 str(int("PRCNN_TRAIN_FWD_GENERIC" in self.switches)), str(int("PRCNN_WGRAD_DIRECT" in self.switches))]
                + [str(c) for c in self.chans])


def _wgrad_split_rows(K, N, want):
    """smallest row count > 1024 whose wgrad_plan (csrc/mlp_train.h) has >= 3 splits and rows % rows_per_split == want
    (-1: one row short of a multiple)"""
    WK, WN = (1 if K <= 64 else 2), (1 if N <= 64 else 2)
    WR = 4 // (WK * WN)
    tiles = -(-K // (32 * (1 if K <= 32 else 2) * WK)) * -(-N // (32 * (1 if N <= 32 else 2) * WN))
    for rows in range(1025, 200000):
        s = max(1, min(-(-1024 // tiles), (rows + 511) // 512, (48 << 20) // (N * K * 4 * WR)))
        unit = 32 if (WK == 2 and WN == 2) else 2 * WR
        per = -(-(-(-rows // s)) // unit) * unit
        splits = -(-rows // per)
        if splits >= 3 and rows % per == want % per:
            return rows, per, splits
    raise AssertionError("no such row count")


SPLIT_BELOW, SPLIT_ON, SPLIT_ABOVE = (_wgrad_split_rows(16, 16, w) for w in (-1, 0, 1))

G, D = {"PRCNN_TRAIN_FWD_GENERIC": "1"}, {"PRCNN_WGRAD_DIRECT": "1"}
CASES = [
    # ---- wide forward / dgrad (WNB == 2): NB >= 4 and ceil(rows / 128) * ceil(NB / 4) >= 192
    Case("plain_wide_6100", "plain", [128, 512, 128], R=6100),                    # wide + narrow forward and dgrad in one call
    Case("plain_narrow_6016", "plain", [128, 512, 128], R=6016),                  # 47 tiles: the last narrow row count at width 512
    Case("plain_wide_6017", "plain", [128, 512, 128], R=6017),                    # 48 tiles: the first wide one
    Case("plain_wide_switches", "plain", [128, 512], R=6017, switches={**G, **D}),  # generic wide forward, direct <2,2,2,2> wgrad
    Case("plain_wide_k515", "plain", [515, 512], R=6017),                         # K0 % 4 != 0: wide bounds-checked fetch, zero-padded copy
    Case("group_wide", "group", [16, 512, 64], pool=True, B=2, N=400, M=50, ns=64),             # wide grouped forward, wide pooled dgrad
    Case("flat_wide", "flat", [16, 512, 64], B=2, N=400, M=50, ns=64),                            # ... and its padding-free twin
    Case("interp_wide", "interp", [64, 512], B=2, n=3010, m=200, C1=16),
    # ---- LDS wgrad (K > 64 and N > 64), all eight forms
    Case("plain_lds", "plain", [128, 128, 128], R=333),                           # <0,false,false>, <0,false,true>
    Case("group_lds_pooled", "group", [16, 96, 128], pool=True, B=2, N=200, M=20, ns=16),       # <1,false,true>
    Case("flat_lds", "flat", [16, 96, 128, 160], B=2, N=200, M=20, ns=16),                        # <0,true,true>, <2,true,true>
    Case("flat_lds_first", "flat", [99, 68, 32], B=2, N=150, M=12, ns=16),                        # <0,true,false>; direct pool 2 + prologue
    Case("group_lds_one_layer", "group", [70, 132], pool=True, B=2, N=120, M=10, ns=16),        # <1,false,false>
    Case("flat_lds_one_layer", "flat", [70, 132], B=2, N=120, M=10, ns=16),                       # <2,true,false>
    # ---- direct wgrad tilings and its run-time forms, interpolation, layers without BatchNorm
    Case("interp_small", "interp", [37, 36, 28], B=2, n=333, m=70, C1=7),         # C2 = 30: a 4-group straddles known | skip
    Case("interp_noskip", "interp", [32, 16], B=1, n=129, m=40, C1=0, need_x=False),
    Case("group_one_layer", "group", [3, 16], pool=True, B=2, N=100, M=10, ns=8),               # no features; direct pool 1, no prologue
    Case("group_nobn_nobias", "group", [11, 32, 16], bn=False, bias=False, pool=True, B=2, N=100, M=12, ns=8),
    Case("group_unpooled", "group", [8, 16, 16], B=1, N=90, M=9, ns=8, need_x=False),
    Case("plain_nobn_k99", "plain", [99, 64, 32], bn=False, R=300),               # zero-padded copy; Conv + bias -> ReLU
    Case("plain_one_row_nobn", "plain", [8, 8, 4], bn=False, R=1),
    # ---- row edges (64-row statistics slab, 128-row tile) on the channel edges
    Case("rows_2", "plain", [3, 4, 4], R=2),
    Case("rows_63", "plain", [4, 28, 16], R=63),
    Case("rows_64", "plain", [5, 36, 16], R=64),
    Case("rows_65", "plain", [31, 16, 4], R=65),
    Case("rows_127", "plain", [33, 16], R=127),
    Case("rows_128", "plain", [65, 68, 16], R=128),
    Case("rows_129", "plain", [16, 16, 16], R=129, need_x=False),
    # ---- one row below, on and one above a multiple of wgrad_plan's rows_per_split (>= 3 splits)
    Case("split_below", "plain", [16, 16], R=SPLIT_BELOW[0]),
    Case("split_on", "plain", [16, 16], R=SPLIT_ON[0]),
    Case("split_above", "plain", [16, 16], R=SPLIT_ABOVE[0]),
    # ---- padding-free rows in two extreme clouds, and the uint8 slot limit
    Case("flat_sparse", "flat", [11, 16, 32], cloud="sparse", B=2, N=500, M=60, ns=16),         # live rows ~ groups << max_rows
    Case("flat_dense", "flat", [11, 16], cloud="dense", B=1, N=300, M=20, ns=16),               # live == max_rows; direct pool 2, no prologue
    Case("group_ns255", "group", [8, 16, 8], pool=True, cloud="hand255", B=1, N=300, M=4, ns=255),
    Case("flat_ns255", "flat", [8, 16, 8], cloud="hand255", B=1, N=300, M=4, ns=255),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the two cases run twice for bit-identical results: a wide plain stack, a padding-free pooled stack with LDS wgrad layers
REPEAT_CASES = ("plain_wide_6017", "flat_lds")


# ---- seeded inputs, on the CPU -------------------------------------------------------------------------------------------------
class Inputs:
    pass


def _group_idx(case, g):
    s = case.shape
    B, N, M, ns = s["B"], s["N"], s["M"], s["ns"]
    idx = torch.empty((B, M, ns), dtype=torch.int64)
    for b in range(B):
        for m in range(M):
            if case.cloud == "dense":
                k = ns
            elif case.cloud == "sparse":
                k = 1 if (b * M + m) % 29 else 3
            elif case.cloud == "hand255":
                k = (ns, 100, 1, ns)[m % 4]
            else:
                k = int(torch.randint(1, ns + 1, (1,), generator=g))
            hits = torch.randperm(N, generator=g)[:k]
            idx[b, m, :k] = hits
            idx[b, m, k:] = hits[0]                              # ball_query's padding: copies of the first hit
    return idx


def build_inputs(case):
    """every tensor of the invocation, float32 / int32 on the CPU, from a seed that depends on the case's name only"""
    g = torch.Generator().manual_seed(1000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)))
    I = Inputs()
    s, K0 = case.shape, case.chans[0]
    rn = lambda *shape: torch.randn(*shape, generator=g)
    I.x0 = I.x1 = I.xyz = I.new_xyz = I.idx = I.idx3 = I.w3 = None
    if case.source == "plain":
        I.x0 = rn(s["R"], K0) * 1.5 + 0.3
    elif case.source == "interp":
        C1 = s["C1"]
        I.x0 = rn(s["B"], s["m"], K0 - C1)
        I.x1 = rn(s["B"], s["n"], C1) if C1 else None
        I.idx3 = torch.randint(0, s["m"], (s["B"], s["n"], 3), generator=g).int()
        w = torch.rand(s["B"], s["n"], 3, generator=g) + 0.05
        I.w3 = w / w.sum(-1, keepdim=True)
    else:
        I.xyz = torch.rand(s["B"], s["N"], 3, generator=g)
        I.new_xyz = I.xyz[:, :s["M"]].contiguous()
        I.idx = _group_idx(case, g).int()
        I.x0 = rn(s["B"], s["N"], K0 - 3) if K0 > 3 else None
    I.W, I.gamma, I.beta, I.rm0, I.rv0 = [], [], [], [], []
    for k, n in zip(case.chans[:-1], case.chans[1:]):
        I.W.append(rn(n, k) / np.sqrt(k))
        I.gamma.append(torch.rand(n, generator=g) + 0.5 if case.bn else None)
        I.beta.append(rn(n) * 0.2 if (case.bn or case.bias) else None)          # BatchNorm's beta, or the conv bias
        I.rm0.append(rn(n) * 0.1)
        I.rv0.append(torch.rand(n, generator=g) + 0.5)
    groups = case.rows // case.shape["ns"] if case.pool else case.rows
    I.gout = rn(groups, case.chans[-1])
    return I


class Rows:
    """the padded rows of a case and how the device's rows map to them"""

    def __init__(self, case, I):
        self.R = R = case.rows
        self.ns = case.shape["ns"] if case.pool else 1
        self.first_of = torch.arange(R)                            # padded row -> the padded row it is a copy of
        self.slot_map = None
        if case.source in ("group", "flat"):
            idx = I.idx.long()
            B, M, ns = idx.shape
            copy = idx == idx[:, :, :1]
            copy[:, :, 0] = False
            base = (torch.arange(B * M) * ns).view(B, M, 1).expand(B, M, ns)
            self.first_of = torch.where(copy, base, base + torch.arange(ns).view(1, 1, ns)).reshape(-1)
        if case.source == "flat":
            distinct = ~copy.reshape(B * M, ns)
            self.live = torch.nonzero(distinct.reshape(-1)).reshape(-1)          # device row -> padded row (group order, slots ascending)
            inv = torch.full((R,), -1, dtype=torch.int64)
            inv[self.live] = torch.arange(self.live.numel())
            self.dev_row = inv[self.first_of]                      # padded row -> device row
            order = torch.argsort((~distinct).to(torch.int8), dim=1, stable=True)      # distinct slots first, ascending
            self.slot_map = order                                  # (groups, ns): device slot -> padded slot
            self.cnt = distinct.sum(1)
        else:
            self.live = torch.arange(R)
            self.dev_row = torch.arange(R)


# ---- the closed form -----------------------------------------------------------------------------------------------------------
def first_rows(case, I, dt):
    """the rows entering the first layer, (R, K0), torch's column order"""
    s = case.shape
    if case.source == "plain":
        return I.x0.to(dt)
    if case.source == "interp":
        B, n, m = s["B"], s["n"], s["m"]
        bi = torch.arange(B)[:, None]
        known = I.x0.to(dt)
        a = sum(I.w3[:, :, t, None].to(dt) * known[bi, I.idx3[:, :, t].long()] for t in range(3))
        if I.x1 is not None:
            a = torch.cat([a, I.x1.to(dt)], dim=2)
        return a.reshape(B * n, -1)
    bi = torch.arange(s["B"])[:, None, None]
    idx = I.idx.long()
    a = (I.xyz[bi, idx] - I.new_xyz[:, :, None, :]).to(dt)        # the fp32 difference is the kernels' own input
    if I.x0 is not None:
        a = torch.cat([a, I.x0.to(dt)[bi, idx]], dim=3)
    return a.reshape(case.rows, -1)


class Ref:
    pass


def reference(case, I, rows, dt=F64, masks=None, arg=None):
    """One invocation in closed form, in `dt`.  masks (per layer, (R, N) bool on the padded rows) and arg ((groups, N) padded slots)
    are the decisions to take; None: this evaluation's own (pre-activation > 0, the first maximum)."""
    r = Ref()
    nl, R = len(case.chans) - 1, case.rows
    A = first_rows(case, I, dt)
    r.A, r.y, r.pre, r.band, r.mask, r.xhat, r.invstd, r.cst, r.run_mean, r.run_var = [], [], [], [], [], [], [], [], [], []
    for l in range(nl):
        W = I.W[l].to(dt)
        y = (A @ W.t())[rows.first_of]                             # copies of a row: exactly the row
        beta = I.beta[l].to(dt) if I.beta[l] is not None else torch.zeros(W.shape[0], dtype=dt)
        if case.bn:
            gamma = I.gamma[l].to(dt)
            mean = y.mean(0)
            var = ((y - mean) ** 2).mean(0)
            invstd = (var + EPS) ** -0.5
            xhat = (y - mean) * invstd
            gx = xhat * gamma
            r.run_mean.append((1 - MOMENTUM) * I.rm0[l].to(dt) + MOMENTUM * mean)
            r.run_var.append((1 - MOMENTUM) * I.rv0[l].to(dt) + MOMENTUM * (var * R / (R - 1) if R > 1 else var))
            scale = gamma * invstd
            r.cst.append((scale, beta - mean * scale, mean, invstd))
        else:
            xhat, invstd, gx = None, None, y
            r.cst.append((torch.ones_like(beta), beta, torch.zeros_like(beta), torch.ones_like(beta)))
        pre = gx + beta
        mask = (pre > 0) if masks is None else masks[l]
        r.A.append(A); r.y.append(y); r.pre.append(pre); r.mask.append(mask); r.xhat.append(xhat); r.invstd.append(invstd)
        r.band.append(pre.abs() <= BAND * (gx.abs() + beta.abs()))
        A = torch.where(mask, pre, torch.zeros_like(pre))
    N = case.chans[-1]
    if case.pool:
        ns = rows.ns
        act = A.view(R // ns, ns, N)
        gmax = act.max(1)[0]
        eq = act == gmax[:, None, :]
        r.first_max = ((eq.cumsum(1) == 1) & eq).to(torch.int8).argmax(1)          # exactly one True per (group, channel)
        r.arg = r.first_max if arg is None else arg
        r.act, r.gmax = act, gmax
        r.out = act.gather(1, r.arg[:, None, :])[:, 0]
        tol = BAND * gmax.clamp(min=1.0)
        r.arg_band = ((act >= (gmax - tol)[:, None, :]) & ~eq).any(1)              # a row float64 cannot tell from the maximum
        Gr = torch.zeros_like(act).scatter_(1, r.arg[:, None, :], I.gout.to(dt)[:, None, :]).reshape(R, N)
    else:
        r.out, r.arg = A, None
        Gr = I.gout.to(dt)
    r.dW, r.S_dW, r.dgamma, r.dbeta = [None] * nl, [None] * nl, [None] * nl, [None] * nl
    for l in reversed(range(nl)):
        dyhat = torch.where(r.mask[l], Gr, torch.zeros_like(Gr))
        if case.bn:
            xhat = r.xhat[l]
            r.dbeta[l] = dyhat.sum(0)
            r.dgamma[l] = (dyhat * xhat).sum(0)
            sc, c1, c2 = I.gamma[l].to(dt) * r.invstd[l], dyhat.mean(0), (dyhat * xhat).mean(0)
            dy = sc * (dyhat - c1 - xhat * c2)
            dy_terms = sc.abs() * (dyhat.abs() + c1.abs() + xhat.abs() * c2.abs())
        else:
            dy = dy_terms = dyhat
            r.dbeta[l] = dyhat.sum(0) if I.beta[l] is not None else None
        dy_terms = dy_terms.abs()
        r.dW[l] = dy.t() @ r.A[l]
        r.S_dW[l] = dy_terms.t() @ r.A[l].abs()
        W = I.W[l].to(dt)
        Gr, S_G = dy @ W, dy_terms @ W.abs()
    # the first layer's row gradient back through the source
    s = case.shape
    r.gx0 = r.gx1 = r.S_gx0 = r.S_gx1 = None
    if not case.need_x:
        return r
    if case.source == "plain":
        r.gx0, r.S_gx0 = Gr, S_G
    elif case.source == "interp":
        B, n, m, C2 = s["B"], s["n"], s["m"], case.chans[0] - s["C1"]
        flat3 = (torch.arange(B)[:, None, None] * m + I.idx3.long()).reshape(B * n, 3)
        r.gx0, r.S_gx0 = torch.zeros((B * m, C2), dtype=dt), torch.zeros((B * m, C2), dtype=dt)
        for t in range(3):
            w = I.w3.reshape(B * n, 3)[:, t, None].to(dt)
            r.gx0.index_add_(0, flat3[:, t], w * Gr[:, :C2])
            r.S_gx0.index_add_(0, flat3[:, t], w.abs() * S_G[:, :C2])
        r.gx0, r.S_gx0 = r.gx0.view(B, m, C2), r.S_gx0.view(B, m, C2)
        if s["C1"]:
            r.gx1, r.S_gx1 = Gr[:, C2:].reshape(B, n, -1), S_G[:, C2:].reshape(B, n, -1)
    elif case.chans[0] > 3:
        B, Np, C = s["B"], s["N"], case.chans[0] - 3
        pt = (torch.arange(B)[:, None, None] * Np + I.idx.long()).reshape(-1)
        r.gx0 = torch.zeros((B * Np, C), dtype=dt).index_add_(0, pt, Gr[:, 3:]).view(B, Np, C)
        r.S_gx0 = torch.zeros((B * Np, C), dtype=dt).index_add_(0, pt, S_G[:, 3:]).view(B, Np, C)
    return r


def band_share(case, ref):
    """(mask entries inside the band, arg slots inside the band, all entries) of one evaluation"""
    inside = sum(int(b.sum()) for b in ref.band)
    total = sum(b.numel() for b in ref.band)
    slots = 0
    if case.pool:
        slots = int(ref.arg_band.sum())
        total += ref.arg_band.numel()
    return inside, slots, total


def check_decisions(case, ref, dev_masks, dev_arg):
    """the device's decisions against the float64 evaluation `ref` that took them: outside the bands they must be float64's own"""
    for l, (mask, band) in enumerate(zip(dev_masks, ref.band)):
        wrong = (mask != (ref.pre[l] > 0)) & ~band
        assert not bool(wrong.any()), "%s: layer %d: %d ReLU decisions differ from float64 outside the band, first at %s" % (
            case.name, l, int(wrong.sum()), torch.nonzero(wrong)[0].tolist())
    if case.pool:
        at = ref.act.gather(1, dev_arg[:, None, :])[:, 0]
        tol = BAND * ref.gmax.clamp(min=1.0)
        far = at < ref.gmax - tol
        assert not bool(far.any()), "%s: %d arg-max slots name a row below the float64 maximum, first at %s" % (
            case.name, int(far.sum()), torch.nonzero(far)[0].tolist())
        not_first = (at == ref.gmax) & (dev_arg != ref.first_max)
        assert not bool(not_first.any()), "%s: %d arg-max slots are not the FIRST of float64's exact maxima, first at %s" % (
            case.name, int(not_first.sum()), torch.nonzero(not_first)[0].tolist())


def entry_ratio(got, ref, S):
    """worst |got - ref| / S over the entries with terms; entries without any term must be exact.  S is the float64 sum of the
    absolute values of the entry's terms with dy expanded into ITS terms, scale * (dyhat, mean(dyhat), xhat * mean(dyhat * xhat)):
    an entry of dW is sum_r dy[r, n] a[r, k] and dy itself is a difference.  With sum |dy| |a| instead, the two-row BatchNorm case
    (xhat = +-1, dy cancels to the size of eps) puts the plain float32 CPU evaluation at 1.9e-2 and the bar of every case at 0.15."""
    err = (got.to(F64) - ref.to(F64)).abs()
    none = S == 0
    assert float(err[none].max()) == 0.0 if bool(none.any()) else True, "an entry without terms is not exactly zero"
    return float((err[~none] / S[~none]).max()) if bool((~none).any()) else 0.0


def cpu_f32_ratios(case, I=None, rows=None, ref=None):
    """a plain float32 CPU evaluation of the closed form (float64's decisions) against float64, per quantity:
    worst |f32 - f64| / S for dW (over the layers) and for the input gradients"""
    I = I or build_inputs(case)
    rows = rows or Rows(case, I)
    ref = ref or reference(case, I, rows)
    r32 = reference(case, I, rows, F32, masks=ref.mask, arg=ref.arg)
    out = {"dW": max(entry_ratio(a, b, S) for a, b, S in zip(r32.dW, ref.dW, ref.S_dW)), "dx": 0.0}
    for a, b, S in ((r32.gx0, ref.gx0, ref.S_gx0), (r32.gx1, ref.gx1, ref.S_gx1)):
        if b is not None:
            out["dx"] = max(out["dx"], entry_ratio(a, b, S))
    return out


# worst over CASES of cpu_f32_ratios (dW: flat_ns255, dx: group_ns255); the device's bar on
# the per-entry ratios is 8 x these and never less than 2^-20 (tests/test_gpu_train_stack_f64.py); the CPU test re-measures them
CPU_F32_RATIO = {"dW": 4.11e-6, "dx": 1.66e-6}


def ratio_bar(what):
    return max(8.0 * CPU_F32_RATIO[what], 2.0 ** -20)
