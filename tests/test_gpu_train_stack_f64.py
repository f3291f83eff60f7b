"""Every kernel variant of the training SharedMLP (csrc/mlp_train.h) against float64, entry by entry.

tests/train_stack_cases.py holds the cases (the smallest shapes that reach each instantiation the host code can pick;
tests/test_train_stack_variants_cpu.py proves on the CPU that their union is everything a broad sweep reaches) and the float64
restatement of one SharedMLPTrain invocation in closed form.  A case runs SharedMLPTrain.apply, reads every layer's saved
pre-normalisation y, its constant rows (scale, shift, mean, invstd) and the pooling `arg` from the autograd context, runs backward
with a seeded gout, and compares everything.

Decisions.  Pooled training tests elsewhere allow 5e-3 in norm because a near-tie of the max, or a pre-activation next to zero, may
go one way in fp32 and the other in the reference.  Here the reference takes those two kinds of decisions from the device -- the
ReLU mask as the exact sign of y_dev * scale_dev + shift_dev, the arg-max as the device's arg -- and checks them wherever float64
can tell: a mask entry must be float64's unless |pre-activation| <= 1e-5 (|gamma xhat| + |beta|); the row named by arg must be
within 1e-5 max(1, group max) of the float64 maximum, and where it attains the maximum exactly (copies of a row in a padded
group, a column that is zero throughout) it must be the FIRST row that does.  The share of entries inside the bands is printed and
must stay <= 1e-3, so the bands cannot swallow a case (the seeded cases: at most 1.6e-5, flat_wide).

Bars, with decisions shared (no pooled exception):
  saved y of every layer        per entry 1e-5 sum |a| |w|       (the form tests/test_gpu_mlp.py uses)
  constant rows, output rows    1e-5 max(1, max |ref|)
  running mean / variance       1e-5 max(1, max |ref|);  num_batches_tracked exact
  every gradient                1e-4 max(1, max |ref|)           (dW, dgamma, dbeta / bias, feature / known / skip / row gradients)
  dW, input gradients           additionally per entry |got - ref| / S, S = the float64 sum of the absolute values of the
                                entry's terms (train_stack_cases.entry_ratio): at most 8 x the worst ratio of a plain float32
                                CPU evaluation of the same closed form over all cases, never less than 2^-20.  8 x: the kernels
                                add up to rows_per_split (512 .. several thousand) products in one fp32 accumulator where a CPU
                                BLAS sums in short blocks; 8 covers a 64-fold longer chain at sqrt(n) growth.
                                  float32 on the CPU:  dW 4.1e-06 (flat_ns255)   input gradient 1.7e-06 (group_ns255)
                                  bars:                dW 3.3e-05                 input gradient 1.3e-05
                                  device, worst seen:  dW 1.9e-06 (group_wide)   input gradient 1.6e-06 (group_ns255); saved y: 1.0e-06 sum |a| |w| (rows_65)
  untouched memory              gout is handed over as a slice of a wider buffer whose other columns are NaN (the one buffer of an
                                invocation the caller owns: SharedMLPTrain allocates the output and the row-gradient buffer itself);
                                nothing the caller reads (output, every gradient, statistics) may be NaN

Variants -> cases (train_launch_record --case; `pool` / `pro` are the direct wgrad kernel's run-time forms):
  train_fwd_kernel<PLAIN, 1, fast>      most cases            <PLAIN, 2, fast>       plain_wide_6100, plain_wide_6017
  train_fwd_kernel<PLAIN, 1, generic>   rows_2 .. rows_128, plain_nobn_k99           <PLAIN, 2, generic>  plain_wide_switches, plain_wide_k515
  train_fwd_kernel<GROUP, 1>            every small group_* / flat_* case            <GROUP, 2>   group_wide, flat_wide
  train_fwd_kernel<INTERP, 1>           interp_small, interp_noskip                  <INTERP, 2>  interp_wide
  train_dgrad_kernel<1, 0>              most cases            <2, 0>  plain_wide_6100, plain_wide_6017, plain_wide_k515
  train_dgrad_kernel<1, 1>              group_lds_pooled, group_lds_one_layer, group_nobn_nobias, group_ns255      <2, 1>  group_wide
  train_dgrad_kernel<1, 2>              flat_lds, flat_lds_first, flat_lds_one_layer, flat_sparse, flat_dense, flat_ns255   <2, 2>  flat_wide
  train_wgrad_kernel<1,1,1,1>           rows_*, split_*, group_one_layer, ...        <1,2,1,1>  rows_64
  train_wgrad_kernel<1,2,1,2>           group_wide, flat_wide, group_lds_pooled, flat_lds        <2,1,1,1>  interp_small, plain_nobn_k99, rows_64, rows_127
  train_wgrad_kernel<2,1,2,1>           flat_lds_first, rows_128                     <2,2,1,1>  interp_small
  train_wgrad_kernel<2,2,1,2>           interp_wide           <2,2,2,1>  group_wide, flat_wide, plain_nobn_k99    <2,2,2,2>  plain_wide_switches
  direct wgrad pool 0 / pro 0, 1        interp_wide, ... / rows_*, interp_small, ...
  direct wgrad pool 1 / pro 0, 1        group_one_layer / group_wide, group_nobn_nobias, group_ns255
  direct wgrad pool 2 / pro 0, 1        flat_dense / flat_wide, flat_lds_first, flat_sparse, flat_ns255
  train_wgrad_lds_kernel<0,false,false> plain_wide_*, plain_narrow_6016, plain_lds, rows_128     <0,false,true>  plain_wide_6100, plain_lds, ...
  train_wgrad_lds_kernel<0,true,false>  flat_lds_first        <0,true,true>  flat_lds
  train_wgrad_lds_kernel<1,false,false> group_lds_one_layer   <1,false,true> group_lds_pooled
  train_wgrad_lds_kernel<2,true,false>  flat_lds_one_layer    <2,true,true>  flat_lds
  the reductions, train_pack_kernel, train_pool_kernel: every case; nobn_cst_kernel: the three *_nobn_* cases"""
import pytest
import torch
import torch.nn as nn

import train_stack_cases as T
from train_stack_cases import F64

pytestmark = [pytest.mark.gpu, pytest.mark.own_arithmetic]


class _Run:
    pass


def _run(case, I, dev, read_saved=True):
    """one SharedMLPTrain invocation of the case on the device, forward + backward; everything it produced, on the CPU"""
    from pointrcnn_amd import _cabi, train_mlp
    nl = len(case.chans) - 1
    bns, params = [], []
    for l in range(nl):
        bn = None
        if case.bn:
            bn = nn.BatchNorm1d(case.chans[l + 1], eps=T.EPS, momentum=T.MOMENTUM).to(dev).train()
            with torch.no_grad():
                bn.running_mean.copy_(I.rm0[l])
                bn.running_var.copy_(I.rv0[l])
        bns.append(bn)
        params += [None if t is None else t.to(dev).requires_grad_(True) for t in (I.W[l], I.gamma[l], I.beta[l])]
    leaf = lambda t: None if t is None else t.to(dev).requires_grad_(case.need_x)
    x0, x1 = leaf(I.x0), leaf(I.x1)
    r = _Run()
    if case.source == "plain":
        src = train_mlp.Source("plain")
    elif case.source == "interp":
        src = train_mlp.Source("interp", idx3=I.idx3.to(dev), w3=I.w3.to(dev))
    else:
        xyz, new_xyz, idx = I.xyz.to(dev), I.new_xyz.to(dev), I.idx.to(dev)
        if case.source == "flat":
            gr = train_mlp.GroupRows(idx, new_xyz, xyz.shape[1])
            src = train_mlp.Source("group", xyz=xyz.view(1, -1, 3), rows=gr)
            r.live, r.ridx = int(gr.rows_dev.item()), gr.ridx.cpu()
        else:
            src = train_mlp.Source("group", xyz=xyz, new_xyz=new_xyz, idx=idx)
    N = case.chans[-1]
    gbuf = torch.full((I.gout.shape[0], N + 4), float("nan"), device=dev)          # the caller's gradient: a slice, NaN around it
    gbuf[:, :N] = I.gout.to(dev)
    with _cabi.switches(**case.switches):
        out = train_mlp.SharedMLPTrain.apply(src, bns, case.pool_ns, x0, x1, *params)
        if read_saved:
            ctx = out.grad_fn
            st = ctx.st
            r.y, r.cst, yo, co = [], [], 0, 0
            for n in st.nout:
                ld_c = (n + 127) // 128 * 128
                r.y.append(st.ybuf[yo: yo + st.rows * n].view(st.rows, n).cpu())
                r.cst.append(st.cbuf[co: co + 6 * ld_c].view(6, ld_c)[:4, :n].cpu())
                yo, co = yo + st.rows * n, co + 6 * ld_c
            r.arg = None if ctx.arg is None else ctx.arg.cpu().long()
        out.backward(gbuf[:, :N])
        torch.cuda.synchronize()
    r.out = out.detach().cpu()
    r.grads = [None if p is None else p.grad.cpu() for p in params]
    r.gx0 = x0.grad.cpu() if (case.need_x and x0 is not None) else None
    r.gx1 = x1.grad.cpu() if (case.need_x and x1 is not None) else None
    r.run_mean = [None if b is None else b.running_mean.cpu() for b in bns]
    r.run_var = [None if b is None else b.running_var.cpu() for b in bns]
    r.tracked = [None if b is None else int(b.num_batches_tracked) for b in bns]
    return r


def _close(got, want, rel, what):
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    err = float((got.to(F64) - want).abs().max()) if got.numel() else 0.0
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    assert err <= rel * scale, "%s: max abs err %.3e > %.1e * %.3e" % (what, err, rel, scale)


@pytest.mark.parametrize("case", T.CASES, ids=[c.name for c in T.CASES])
def test_case_equals_float64_closed_form(dev, case):
    I = T.build_inputs(case)
    rows = T.Rows(case, I)
    r = _run(case, I, dev)
    nl, name = len(case.chans) - 1, case.name
    live = rows.live
    if case.source == "flat":
        s = case.shape
        assert r.live == live.numel(), "live rows %d != %d" % (r.live, live.numel())
        pt = (torch.arange(s["B"])[:, None, None] * s["N"] + I.idx.long()).reshape(-1)
        assert torch.equal(r.ridx[:r.live].long(), pt[live]), "the device's distinct rows are not the groups' distinct hits in order"
    nlive = live.numel()
    # the decisions, from what the device saved
    masks = []
    for l in range(nl):
        y_pad = r.y[l][rows.dev_row].to(F64)
        masks.append(y_pad * r.cst[l][0].to(F64) + r.cst[l][1].to(F64) > 0)          # the fp32 product is exact in float64
    arg = None
    if case.pool:
        arg = r.arg
        if case.source == "flat":
            assert bool((arg < rows.cnt[:, None]).all()), "arg names a slot past its group's distinct rows"
            arg = rows.slot_map.gather(1, arg)
    ref = T.reference(case, I, rows, F64, masks, arg)
    T.check_decisions(case, ref, masks, arg)
    inside, slots, total = T.band_share(case, ref)
    print("\n%s: rows %d live %d; inside the bands: %d mask entries + %d arg slots of %d (%.1e)"
          % (name, case.rows, nlive, inside, slots, total, (inside + slots) / total))
    assert inside + slots <= T.MAX_BAND_SHARE * total
    # forward
    for l in range(nl):
        bar = 1e-5 * (ref.A[l].abs() @ I.W[l].to(F64).abs().t())[live]
        got = r.y[l][:nlive]
        assert bool(torch.isfinite(got).all()), "y of layer %d: not finite" % l
        over = (got.to(F64) - ref.y[l][live]).abs() - bar
        print("  layer %d: y worst (err - bar) %.3e, worst err / sum|a||w| %.2e" % (l, float(over.max()), float(
            ((got.to(F64) - ref.y[l][live]).abs() / bar.clamp(min=1e-300)).max()) * 1e-5))
        assert float(over.max()) <= 0.0, "%s: y of layer %d exceeds 1e-5 sum |a||w| by %.3e at %s" % (
            name, l, float(over.max()), torch.nonzero(over == over.max())[0].tolist())
        for k, what in enumerate(("scale", "shift", "mean", "invstd")):
            _close(r.cst[l][k], ref.cst[l][k], 1e-5, "%s: %s of layer %d" % (name, what, l))
        if case.bn:
            _close(r.run_mean[l], ref.run_mean[l], 1e-5, "%s: running_mean of layer %d" % (name, l))
            _close(r.run_var[l], ref.run_var[l], 1e-5, "%s: running_var of layer %d" % (name, l))
            assert r.tracked[l] == 1
    _close(r.out, ref.out, 1e-5, "%s: output rows" % name)
    # backward
    worst = {"dW": 0.0, "dx": 0.0}
    for l in range(nl):
        dW, dg, db = r.grads[3 * l: 3 * l + 3]
        _close(dW, ref.dW[l], 1e-4, "%s: dW of layer %d" % (name, l))
        worst["dW"] = max(worst["dW"], T.entry_ratio(dW, ref.dW[l], ref.S_dW[l]))
        if case.bn:
            _close(dg, ref.dgamma[l], 1e-4, "%s: dgamma of layer %d" % (name, l))
        if ref.dbeta[l] is not None:
            _close(db, ref.dbeta[l], 1e-4, "%s: dbeta / bias gradient of layer %d" % (name, l))
        else:
            assert db is None
    for got, want, S, what in ((r.gx0, ref.gx0, ref.S_gx0, "first input"), (r.gx1, ref.gx1, ref.S_gx1, "skip features")):
        assert (got is None) == (want is None), what
        if want is not None:
            _close(got, want, 1e-4, "%s: gradient of the %s" % (name, what))
            worst["dx"] = max(worst["dx"], T.entry_ratio(got, want, S))
    print("  per-entry ratios: dW %.2e (bar %.2e), input gradient %.2e (bar %.2e)" % (worst["dW"], T.ratio_bar("dW"), worst["dx"], T.ratio_bar("dx")))
    assert worst["dW"] <= T.ratio_bar("dW"), "%s: dW per-entry ratio %.3e > %.3e" % (name, worst["dW"], T.ratio_bar("dW"))
    assert worst["dx"] <= T.ratio_bar("dx"), "%s: input-gradient per-entry ratio %.3e > %.3e" % (name, worst["dx"], T.ratio_bar("dx"))


@pytest.mark.parametrize("name", T.REPEAT_CASES)
def test_two_runs_are_bit_identical(dev, name):
    """the fixed summation orders (statistics, wgrad partials, reductions): outputs and parameter gradients of two runs are equal
    bit for bit on a wide plain stack and on a padding-free pooled stack with LDS wgrad layers"""
    case = T.BY_NAME[name]
    I = T.build_inputs(case)
    a, b = _run(case, I, dev, read_saved=False), _run(case, I, dev, read_saved=False)
    assert torch.equal(a.out, b.out)
    for l, (ga, gb) in enumerate(zip(a.grads, b.grads)):
        assert (ga is None and gb is None) or torch.equal(ga, gb), "parameter gradient %d of layer %d" % (l % 3, l // 3)
    for ma, mb in zip(a.run_mean + a.run_var, b.run_mean + b.run_var):
        assert torch.equal(ma, mb)


def test_nsample_256_is_refused(dev):
    """the pooling slot is a uint8: nsample 255 is the limit (group_ns255, flat_ns255); 256 fails the library's argument check,
    which precedes every launch (the CPU coverage test sees none)"""
    from pointrcnn_amd import _cabi, train_mlp
    g = torch.Generator().manual_seed(256)
    xyz = torch.rand(1, 300, 3, generator=g).to(dev)
    idx = torch.stack([torch.randperm(300, generator=g)[:256] for _ in range(2)]).view(1, 2, 256).int().to(dev)
    W = torch.randn(4, 3, generator=g).to(dev).requires_grad_(True)
    bn = nn.BatchNorm1d(4).to(dev).train()
    src = train_mlp.Source("group", xyz=xyz, new_xyz=xyz[:, :2].contiguous(), idx=idx)
    with pytest.raises(_cabi.PointOpsError, match="bad pooling arguments"):
        train_mlp.SharedMLPTrain.apply(src, [bn], 256, None, None, W, bn.weight, bn.bias)
