"""Run the REFERENCE's own create_optimizer / create_scheduler (tools/train_rcnn.py:88-143), its CosineWarmupLR and its
checkpoint functions (tools/train_utils/train_utils.py) on the CPU and keep what they give.

Only used to GENERATE tests/golden/train_loop_ref.npz and train_loop_ckpt_ref.pt (needs the reference tree; build container only).
The reference's modules are imported, nothing of them is copied; tools/train_rcnn.py parses its arguments at import, so it is
imported under a patched sys.argv.  Recorded:
    order_<mode>_g0 / _g1   parameter names of the two groups of the adam_onecycle optimizer, <mode> = rpn | rcnn | rcnn_offline
    order_adam              parameter names of the single group under TRAIN.OPTIMIZER adam (the rcnn model)
    lr_epochs, lr_fresh     the rate LambdaLR leaves after step(epoch) for epochs 0 .. 220 under default.yaml, last_epoch -1
    lr_resumed_start, lr_resumed_epochs, lr_resumed   the same with last_epoch 121: the rate at creation, then after step(epoch)
    bnm_args, bnm           bnm_lmbd at 0, 100, .. 2000
    warmup                  the rate CosineWarmupLR(T_max 10, eta_min WARMUP_MIN) leaves after step(0 .. 10)
    ckpt_x                  the input of the small model of the checkpoint case (small_model below: Conv1d / BatchNorm1d / Conv1d);
                            loss = mean(model(x)^2), ten-step OneCycle, clip 1.0: four steps, the checkpoint (written by the
                            reference's save_checkpoint(checkpoint_state(...)), kept as train_loop_ckpt_ref.pt), two further steps
    ckpt_params             the model's parameters after those six steps, flat, in named_parameters order
    ckpt_group_sizes, ckpt_steps   the checkpoint's group sizes and the `step` of every state entry"""
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch

REFERENCE = os.environ.get("PRCNN_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
MODES = {"rpn": (True, False, False), "rcnn": (True, True, True), "rcnn_offline": (False, True, False)}   # RPN.ENABLED, RCNN.ENABLED, RPN.FIXED
CKPT_TOTAL_STEPS, CKPT_STEPS, CKPT_MORE = 10, 4, 2
# kept under the suffix .pt: a file named *.pth is a path configuration file to Python's site module wherever it lands on sys.path
CKPT = os.path.join(HERE, "train_loop_ckpt_ref.pt")


def available():
    return os.path.isfile(os.path.join(REFERENCE, "tools", "train_rcnn.py"))


def small_model():
    torch.manual_seed(11)
    return torch.nn.Sequential(torch.nn.Conv1d(3, 8, 1), torch.nn.BatchNorm1d(8), torch.nn.Conv1d(8, 2, 1))


def small_input():
    return torch.randn(4, 3, 16, generator=torch.Generator().manual_seed(12))


def _reference():
    for p in (ROOT, TESTS, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import cpu_ops
    import ref_net
    ns = ref_net.load()
    sys.path.insert(0, os.path.join(REFERENCE, "tools"))
    spec = importlib.util.spec_from_file_location("prcnn_compat_adapters", os.path.join(TESTS, "compat", "usercustomize.py"))
    spec.loader.exec_module(importlib.util.module_from_spec(spec))
    argv, sys.argv = sys.argv, ["train_rcnn.py", "--train_mode", "rpn", "--batch_size", "2", "--epochs", "3"]
    try:
        with cpu_ops.cuda_is_cpu():
            tr = importlib.import_module("train_rcnn")
    finally:
        sys.argv = argv
    return ns, tr, cpu_ops


def generate():
    ns, tr, cpu_ops = _reference()
    cfg = ns.cfg
    out = {}
    # (a) parameter orders
    for mode, (rpn, rcnn, fixed) in MODES.items():
        cfg.RPN.ENABLED, cfg.RCNN.ENABLED, cfg.RPN.FIXED = rpn, rcnn, fixed
        cfg.TRAIN.OPTIMIZER = "adam_onecycle"
        with cpu_ops.cuda_is_cpu():
            model = ns.PointRCNN(num_classes=2, use_xyz=True, mode="TRAIN")
        names = {id(p): n for n, p in model.named_parameters()}
        opt = tr.create_optimizer(model)
        for k, g in enumerate(opt.opt.param_groups):
            out["order_%s_g%d" % (mode, k)] = np.array([names[id(p)] for p in g["params"]])
        if mode == "rcnn":
            cfg.TRAIN.OPTIMIZER = "adam"
            adam = tr.create_optimizer(model)
            out["order_adam"] = np.array([names[id(p)] for p in adam.param_groups[0]["params"]])
    # (b) - (d) schedules, under default.yaml
    cfg.TRAIN.OPTIMIZER = "adam"
    tr.model = model = small_model()
    epochs = list(range(221))

    def rates(last_epoch, steps):
        opt = tr.create_optimizer(model)
        if last_epoch != -1:
            for g in opt.param_groups:                   # as a loaded optimizer_state carries it
                g["initial_lr"] = cfg.TRAIN.LR
        sched, bnm = tr.create_scheduler(opt, 30, last_epoch)
        start = opt.param_groups[0]["lr"]
        got = []
        for e in steps:
            sched.step(e)
            got.append(opt.param_groups[0]["lr"])
        return start, np.array(got, np.float64), bnm, opt
    _, out["lr_fresh"], bnm, opt = rates(-1, epochs)
    out["lr_epochs"] = np.array(epochs)
    out["lr_resumed_epochs"] = np.array(range(121, 221))
    start, out["lr_resumed"], _, _ = rates(121, range(121, 221))
    out["lr_resumed_start"] = np.float64(start)
    out["bnm_args"] = np.arange(0, 2001, 100)
    out["bnm"] = np.array([bnm.lmbd(int(x)) for x in out["bnm_args"]], np.float64)
    opt = tr.create_optimizer(model)
    warm = tr.train_utils.CosineWarmupLR(opt, T_max=10, eta_min=cfg.TRAIN.WARMUP_MIN)
    got = []
    for i in range(11):
        warm.step(i)
        got.append(opt.param_groups[0]["lr"])
    out["warmup"] = np.array(got, np.float64)
    # (e) the checkpoint
    cfg.TRAIN.OPTIMIZER = "adam_onecycle"
    cfg.RPN.ENABLED, cfg.RPN.FIXED = False, False
    tr.model = model = small_model()
    opt = tr.create_optimizer(model)
    sched, _ = tr.create_scheduler(opt, CKPT_TOTAL_STEPS, -1)
    x = small_input()

    def steps(first, n):
        for it in range(first, first + n):
            sched.step(it)
            model.train()
            opt.zero_grad()
            model(x).pow(2).mean().backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.TRAIN.GRAD_NORM_CLIP)
            opt.step()
    steps(0, CKPT_STEPS)
    state = tr.train_utils.checkpoint_state(model, opt, 1, CKPT_STEPS)
    for g in state["optimizer_state"]["param_groups"]:   # OneCycle leaves numpy scalars; plain floats load with weights_only=True
        g.update({k: (float(v) if isinstance(v, np.floating) else tuple(float(b) for b in v) if k == "betas" else v) for k, v in g.items()})
    tr.train_utils.save_checkpoint(state, filename=os.path.join(HERE, "train_loop_ckpt_ref"))      # the reference appends ".pth"
    os.replace(os.path.join(HERE, "train_loop_ckpt_ref.pth"), CKPT)
    sd = opt.state_dict()
    out["ckpt_group_sizes"] = np.array([len(g["params"]) for g in sd["param_groups"]])
    out["ckpt_steps"] = np.array([int(sd["state"][k]["step"]) for k in sorted(sd["state"])])
    steps(CKPT_STEPS, CKPT_MORE)
    out["ckpt_x"] = x.numpy()
    out["ckpt_params"] = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    np.savez_compressed(os.path.join(HERE, "train_loop_ref.npz"), **out)
    return out


if __name__ == "__main__":
    if not available():
        sys.exit("the reference tree is not at %s" % REFERENCE)
    res = generate()
    for k, v in res.items():
        print(k, getattr(v, "shape", None))
    print(os.path.getsize(os.path.join(HERE, "train_loop_ref.npz")), os.path.getsize(CKPT))
