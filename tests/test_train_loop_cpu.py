"""CPU: pointrcnn_amd/train_loop.py against what the reference's own create_optimizer / create_scheduler / CosineWarmupLR /
checkpoint functions gave (tests/golden/train_loop_ref.npz and train_loop_ckpt_ref.pt; generator tests/golden/ref_train_loop.py),
and the loop itself on a plain-torch Linear / BatchNorm1d model."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import optim_cases as oc
from pointrcnn_amd import optim
from pointrcnn_amd import train_functions as tf
from pointrcnn_amd import train_loop as tl
from util import GOLDEN

CKPT = os.path.join(GOLDEN, "train_loop_ckpt_ref.pt")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "train_loop_ref.npz")))


def small_model():
    """the model of the checkpoint case (tests/golden/ref_train_loop.py small_model)"""
    torch.manual_seed(11)
    return nn.Sequential(nn.Conv1d(3, 8, 1), nn.BatchNorm1d(8), nn.Conv1d(8, 2, 1))


# ---------------------------------------------------------------------------------------------- schedules
def test_config_is_the_train_section_of_default_yaml():
    c = tl.TrainConfig
    assert (c.LR, c.LR_CLIP, c.LR_DECAY, tuple(c.DECAY_STEP_LIST), c.LR_WARMUP, c.WARMUP_MIN, c.WARMUP_EPOCH) == \
        (0.002, 0.00001, 0.5, (100, 150, 180, 200), True, 0.0002, 1)
    assert (c.BN_MOMENTUM, c.BN_DECAY, c.BNM_CLIP, tuple(c.BN_DECAY_STEP_LIST)) == (0.1, 0.5, 0.01, (1000,))
    assert (c.OPTIMIZER, c.WEIGHT_DECAY, c.MOMENTUM, tuple(c.MOMS), c.DIV_FACTOR, c.PCT_START, c.GRAD_NORM_CLIP) == \
        ("adam_onecycle", 0.001, 0.9, (0.95, 0.85), 10.0, 0.4, 1.0)


class _Adam(tl.TrainConfig):
    OPTIMIZER = "adam"


@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_lambda_lr_equals_the_references_exactly(fx, name):
    class cfg(tl.TrainConfig):
        OPTIMIZER = name
    model = small_model()
    opt = tl.create_optimizer(cfg, model.parameters())
    assert type(opt) is (optim.ClipAdam if name == "adam" else optim.ClipSGD)
    sched, bnm = tl.create_scheduler(cfg, opt, model, -1)
    got = []
    for e in fx["lr_epochs"]:
        tl.step_scheduler_to(sched, int(e))
        got.append(opt.param_groups[0]["lr"])
    assert np.array_equal(np.array(got, np.float64), fx["lr_fresh"])
    assert fx["lr_fresh"][0] == 0.002 and fx["lr_fresh"][100] == 0.001 and fx["lr_fresh"][220] == 0.000125
    # resumed: last_epoch = start_epoch + 1 = 121 on a fresh optimizer (no initial_lr in its group yet)
    opt = tl.create_optimizer(cfg, model.parameters())
    sched, _ = tl.create_scheduler(cfg, opt, model, 121)
    assert opt.param_groups[0]["lr"] == float(fx["lr_resumed_start"])
    got = []
    for e in fx["lr_resumed_epochs"]:
        tl.step_scheduler_to(sched, int(e))
        got.append(opt.param_groups[0]["lr"])
    assert np.array_equal(np.array(got, np.float64), fx["lr_resumed"])


def test_bn_momentum_and_warmup_equal_the_references_exactly(fx):
    assert np.array_equal(np.array([tl.bn_momentum_at(int(x)) for x in fx["bnm_args"]], np.float64), fx["bnm"])
    assert fx["bnm"][9] == 0.1 and fx["bnm"][10] == 0.05
    model = small_model()
    opt = tl.create_optimizer(_Adam, model.parameters())
    warm = tl.CosineWarmupLR(opt, T_max=10, eta_min=tl.TrainConfig.WARMUP_MIN)
    got = []
    for i in range(11):
        tl.step_scheduler_to(warm, i)
        got.append(opt.param_groups[0]["lr"])
        assert warm.get_last_lr()[0] == got[-1]
    assert np.array_equal(np.array(got, np.float64), fx["warmup"])
    assert got[0] == 0.0002 and got[10] == 0.002
    # the scheduler object reaches every BatchNorm, at construction (last_epoch + 1) and at step
    sched = tl.BNMomentumScheduler(model, tl.bn_momentum_at, last_epoch=-1)
    assert model[1].momentum == 0.1
    sched.step(1000)
    assert model[1].momentum == 0.05 and sched.last_epoch == 1000
    with pytest.raises(RuntimeError):
        tl.BNMomentumScheduler(object(), tl.bn_momentum_at)


def test_adam_onecycle_has_no_lr_scheduler_and_create_optimizer_knows_three_names():
    model = small_model()
    opt = tl.create_optimizer(tl.TrainConfig, model.parameters(), total_steps=10)
    assert type(opt) is optim.OneCycleAdam and opt.param_groups[0]["total_steps"] == 10
    sched, bnm = tl.create_scheduler(tl.TrainConfig, opt, model)
    assert sched is None and isinstance(bnm, tl.BNMomentumScheduler)
    with pytest.raises(ValueError, match="total_steps"):
        tl.create_optimizer(tl.TrainConfig, model.parameters())

    class cfg(tl.TrainConfig):
        OPTIMIZER = "rmsprop"
    with pytest.raises(NotImplementedError):
        tl.create_optimizer(cfg, model.parameters())


# ---------------------------------------------------------------------------------------------- checkpoints
def _onecycle(model):
    return tl.create_optimizer(tl.TrainConfig, model.parameters(), total_steps=10)


def _steps(model, opt, x, n):
    for _ in range(n):
        model.train()
        opt.zero_grad()
        model(x).pow(2).mean().backward()
        opt.step()


def test_the_references_adam_onecycle_checkpoint_continues_here(fx):
    model = small_model()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)                                  # the checkpoint must bring the weights
    opt = _onecycle(model)
    it, epoch = tl.load_checkpoint(model, opt, CKPT)
    assert (it, epoch) == (4, 1) and opt.iteration == 4
    assert sum(1 for p in model.parameters() if opt.state.get(p)) == 6
    x = torch.from_numpy(fx["ckpt_x"])
    _steps(model, opt, x, 2)
    got = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    want = fx["ckpt_params"]
    lr_sum = sum(optim.one_cycle(t, 10)[0] for t in (4, 5))
    e_p = float(np.max(np.abs(got.astype(np.float64) - want) / (np.abs(want) + lr_sum)))
    yard = oc.fixture()["clip_yard"][0]
    print("two steps after the reference's checkpoint: E_p %.3e (bar %g x %.3e), %d of %d entries differ"
          % (e_p, oc.MARGIN, yard, int((got != want).sum()), got.size))
    assert e_p <= oc.MARGIN * yard
    assert opt.iteration == 6
    # ... and the way back: the reference's layout, rebuilt from the model
    ref = torch.load(CKPT, weights_only=True)
    model2 = small_model()
    opt2 = _onecycle(model2)
    tl.load_checkpoint(model2, opt2, CKPT)
    state = tl.checkpoint_state(model2, opt2, 1, 4, optimizer_layout="reference")
    assert sorted(state) == sorted(ref) == ["epoch", "it", "model_state", "optimizer_state"]
    sd, rd = state["optimizer_state"], ref["optimizer_state"]
    assert [len(g["params"]) for g in sd["param_groups"]] == [len(g["params"]) for g in rd["param_groups"]] == fx["ckpt_group_sizes"].tolist() == [4, 2]
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in rd["param_groups"]]
    assert sorted(sd["state"]) == sorted(rd["state"])
    assert [int(sd["state"][k]["step"]) for k in sorted(sd["state"])] == fx["ckpt_steps"].tolist() == [4] * 6
    for k in rd["state"]:
        assert torch.equal(sd["state"][k]["exp_avg"], rd["state"][k]["exp_avg"])
        assert torch.equal(sd["state"][k]["exp_avg_sq"], rd["state"][k]["exp_avg_sq"])
    for g, r in zip(sd["param_groups"], rd["param_groups"]):
        assert g["lr"] == r["lr"] and tuple(g["betas"]) == tuple(r["betas"]) and g["eps"] == r["eps"] and g["weight_decay"] == r["weight_decay"]
    assert all(torch.equal(state["model_state"][k], ref["model_state"][k]) for k in ref["model_state"])
    # a parameter in the groups without state (the reference's frozen RPN) stays without state
    del ref["optimizer_state"]["state"][0]
    model3 = small_model()
    opt3 = _onecycle(model3)
    tl._load_reference_onecycle(model3, opt3, ref["optimizer_state"], 4)
    assert not opt3.state.get(model3[0].weight) and opt3.state[model3[0].bias]["step"] == 4
    # the default layout is the optimizer's own, and group sizes that do not fit are refused
    assert len(tl.checkpoint_state(model2, opt2, 1, 4)["optimizer_state"]["param_groups"]) == 1
    with pytest.raises(ValueError, match="groups of"):
        tl._load_reference_onecycle(nn.Sequential(nn.Conv1d(3, 8, 1)), opt3, ref["optimizer_state"], 4)


def test_group_order_of_this_packages_models_is_the_references(fx):
    from pointrcnn_amd import point_rcnn, rcnn, rpn
    model = point_rcnn.PointRCNN(mode="TRAIN")
    for key, m, prefix in (("rpn", rpn.RPN(), "rpn."), ("rcnn", model, ""), ("rcnn_offline", rcnn.RCNNNet(), "rcnn_net.")):
        groups = tl.reference_param_groups(m)
        for k in (0, 1):
            assert [prefix + n for n in groups[k]] == fx["order_%s_g%d" % (key, k)].tolist(), (key, k)
    assert [len(fx["order_rpn_g%d" % k]) for k in (0, 1)] == [38, 68]
    assert [n for n, _ in model.named_parameters()] == fx["order_adam"].tolist()
    assert tl.reference_param_groups(nn.DataParallel(model)) == tl.reference_param_groups(model)


def test_load_part_ckpt_and_wrapped_models(tmp_path):
    model = small_model()
    tl.save_checkpoint(tl.checkpoint_state(nn.DataParallel(model), None, 3, 7), filename=str(tmp_path / "part"))
    ckpt = torch.load(str(tmp_path / "part.pth"), weights_only=True)
    assert ckpt["epoch"] == 3 and ckpt["it"] == 7 and ckpt["optimizer_state"] is None and "0.weight" in ckpt["model_state"]
    bigger = nn.Sequential(nn.Conv1d(3, 8, 1), nn.BatchNorm1d(8), nn.Conv1d(8, 2, 1), nn.Conv1d(2, 2, 1))
    kept = bigger[3].weight.detach().clone()
    tl.load_part_ckpt(bigger, str(tmp_path / "part.pth"))
    assert torch.equal(bigger[0].weight, model[0].weight) and torch.equal(bigger[3].weight, kept)
    with pytest.raises(RuntimeError):
        tl.load_part_ckpt(nn.Sequential(nn.Sequential(nn.Linear(2, 2))), str(tmp_path / "part.pth"))     # no key in common
    with pytest.raises(FileNotFoundError):
        tl.load_checkpoint(model, None, str(tmp_path / "missing.pth"))
    assert tl.load_checkpoint(model, None, str(tmp_path / "part.pth")) == (7, 3)


# ---------------------------------------------------------------------------------------------- the loop
class LoopCfg(tl.TrainConfig):
    OPTIMIZER = "adam"
    DECAY_STEP_LIST = (1, 2)
    BN_DECAY_STEP_LIST = (3,)


class PlainTrainer:
    """the trainers' interface (model, loss, step) on a plain torch model"""

    def __init__(self, model, optimizer, cfg=LoopCfg):
        self.model, self.optimizer, self.cfg = model, optimizer, cfg
        self.momenta, self.rates, self.nexts = [], [], []

    def loss(self, batch, tb_dict=None):
        loss = (self.model(batch["x"]) - batch["y"]).pow(2).mean()
        if tb_dict is not None:
            tb_dict.update(iou=0.25, mse=loss.item())
        return loss

    def step(self, batch, tb_dict=None, next_batch=None):
        self.model.train()
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.loss(batch, tb_dict)
        loss.backward()
        self.momenta.append([m.momentum for m in self.model.modules() if isinstance(m, nn.BatchNorm1d)])
        self.rates.append(self.optimizer.param_groups[0].get("lr"))
        self.nexts.append(next_batch)
        if not getattr(self.optimizer, "clips_in_step", False):
            nn.utils.clip_grad_norm_(self.model.parameters(), self.cfg.GRAD_NORM_CLIP)
        self.optimizer.step()
        return loss


class TbLog:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def of(self, tag):
        return [(v, s) for t, v, s in self.rows if t == tag]


def plain_model():
    torch.manual_seed(3)
    return nn.Sequential(nn.Linear(5, 6), nn.BatchNorm1d(6), nn.ReLU(), nn.Linear(6, 6), nn.BatchNorm1d(6), nn.Linear(6, 2))


def batches(n=2):
    gen = torch.Generator().manual_seed(4)
    return [{"x": torch.randn(8, 5, generator=gen), "y": torch.randn(8, 2, generator=gen)} for _ in range(n)]


def build(cfg, ckpt_dir, warmup=False, resume=None, log_interval=50, tb=None):
    model = plain_model()
    opt = tl.create_optimizer(cfg, model.parameters(), total_steps=6)
    it = start_epoch = 0
    last_epoch = -1
    if resume is not None:
        it, start_epoch = tl.load_checkpoint(model, opt, resume)
        last_epoch = start_epoch + 1
    sched, bnm = tl.create_scheduler(cfg, opt, model, last_epoch)
    warm = tl.CosineWarmupLR(opt, T_max=cfg.WARMUP_EPOCH * 2, eta_min=cfg.WARMUP_MIN) if warmup else None
    trainer = PlainTrainer(model, opt, cfg)
    loop = tl.TrainLoop(trainer, opt, sched, bnm, str(ckpt_dir), tb_log=tb, lr_warmup_scheduler=warm,
                        warmup_epoch=cfg.WARMUP_EPOCH if warmup else -1, log_interval=log_interval)
    return model, opt, trainer, loop, it, start_epoch


@pytest.mark.parametrize("warmup", [False, True])
def test_loop_follows_the_schedules(tmp_path, warmup):
    tb = TbLog()
    model, opt, trainer, loop, it, ep = build(LoopCfg, tmp_path, warmup=warmup, tb=tb)
    end = loop.train(it, ep, 3, batches(), test_batches=batches(1), ckpt_save_interval=2)
    assert end == 6
    c = LoopCfg
    want = [c.LR * tl.lr_decay_factor(e, c) for e in (0, 0, 1, 1, 2, 2)]
    if warmup:                                           # epoch 0 < WARMUP_EPOCH: the cosine from WARMUP_MIN, per iteration
        want[:2] = [c.WARMUP_MIN + (c.LR - c.WARMUP_MIN) * (1 - np.cos(np.pi * i / 2)) / 2 for i in (0, 1)]
    assert trainer.rates == want and want[2:] == [0.001, 0.001, 0.0005, 0.0005]
    assert [v for v, _ in tb.of("learning_rate")] == want and [s for _, s in tb.of("learning_rate")] == [1, 2, 3, 4, 5, 6]
    # bnm_scheduler.step(it) at the head of an epoch: BN_DECAY_STEP_LIST [3] is reached by the iteration count 4 of epoch 2
    assert trainer.momenta == [[0.1, 0.1]] * 4 + [[0.05, 0.05]] * 2
    assert tb.of("bn_momentum") == [(0.1, 0), (0.1, 2), (0.1, 4)]       # logged as lmbd(epoch), as the reference does
    assert sorted(os.listdir(tmp_path)) == ["checkpoint_epoch_2.pth"]
    tags = {t for t, _, _ in tb.rows}
    assert tags >= {"train_loss", "learning_rate", "bn_momentum", "val_loss", "val_iou", "val_mse"}
    assert len(tb.of("train_loss")) == 6 and len(tb.of("val_loss")) == 3 and all(np.isfinite(v) for v, _ in tb.of("train_loss"))
    assert [n is not None for n in trainer.nexts] == [True, False] * 3  # the next batch is handed to the step
    assert loop.host_reads == 3 and loop.last_loss == tb.of("train_loss")[-1][0]


def test_eval_epoch_averages_as_the_reference():
    model, opt, trainer, loop, _, _ = build(LoopCfg, ".")
    bs = batches(3)
    loss, ev, perf = loop.eval_epoch(bs)
    assert not model.training and perf == ev["iou"] == 0.25
    with torch.no_grad():
        want = [float(trainer.loss(b)) for b in bs]
    assert loss == pytest.approx(sum(want) / 3, rel=1e-6) and ev["mse"] == pytest.approx(sum(want) / 3, rel=1e-6)
    trainer.loss = lambda batch, tb=None: (tb.update(recalled_cnt=3, gt_cnt=4), torch.tensor(1.0))[1]
    loss, ev, perf = loop.eval_epoch(bs)
    assert perf == ev["recall"] == 0.75 and loss == 1.0


@pytest.mark.parametrize("name", ["adam", "sgd", "adam_onecycle"])
def test_a_resumed_run_ends_where_the_uninterrupted_run_ends(tmp_path, name):
    class cfg(LoopCfg):
        OPTIMIZER = name
    warmup = name != "adam_onecycle"
    a_dir, b_dir = tmp_path / "a", tmp_path / "b"
    os.makedirs(a_dir)
    os.makedirs(b_dir)
    model, opt, trainer, loop, it, ep = build(cfg, a_dir, warmup=warmup, log_interval=1)
    loop.train(it, ep, 3, batches(), ckpt_save_interval=1)
    assert sorted(os.listdir(a_dir)) == ["checkpoint_epoch_%d.pth" % k for k in (1, 2, 3)]
    model2, opt2, trainer2, loop2, it, ep = build(cfg, b_dir, warmup=warmup, resume=str(a_dir / "checkpoint_epoch_1.pth"))
    assert (it, ep) == (2, 1)
    loop2.train(it, ep, 3, batches(), ckpt_save_interval=1)
    assert trainer2.rates == trainer.rates[2:] and trainer2.momenta == trainer.momenta[2:]
    for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(a, b), k
    sa, sb = opt.state_dict(), opt2.state_dict()
    assert sorted(sa["state"]) == sorted(sb["state"])
    for k in sa["state"]:
        for key, v in sa["state"][k].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(sb["state"][k][key])), (k, key)
    assert loop.host_reads == 6 and loop2.host_reads == 2                  # log_interval 1: every iteration; 50: the end of an epoch


# ---------------------------------------------------------------------------------------------- trainers
def test_trainers_take_an_optimizer_and_do_not_clip_twice(monkeypatch):
    import cpu_ops
    import oracle
    import test_train_ddp_gloo as g
    oracle.cpu()
    calls = []
    real = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    pts, cls, reg = g._batch(1, seed=0)
    batch = {"pts_input": pts, "rpn_cls_label": cls, "rpn_reg_label": reg}

    def one_step(make):
        model = g._model(True)
        trainer = tf.RPNTrainer(model, optimizer=make(model))
        g._freeze_norm_and_dropout(trainer, True)
        del calls[:]
        with cpu_ops.oracle_ops():
            loss = trainer.step(batch)
        assert np.isfinite(float(loss.detach()))
        return trainer, len(calls)
    # an instance that clips in its step (the composed route on the CPU calls clip_grad_norm_ itself: once, not twice)
    trainer, n = one_step(lambda m: tl.create_optimizer(_Adam, m.parameters()))
    assert type(trainer.optimizer) is optim.ClipAdam and n == 1 and float(trainer.optimizer.last_grad_norm) > 0
    # a callable params -> Optimizer
    trainer, n = one_step(lambda m: (lambda params: optim.ClipSGD(params, lr=0.01, momentum=0.9, grad_norm_clip=1.0)))
    assert type(trainer.optimizer) is optim.ClipSGD and n == 1 and trainer.optimizer_name == "ClipSGD"
    trainer, n = one_step(lambda m: (lambda params: optim.OneCycleAdam(params, 10)))
    assert type(trainer.optimizer) is optim.OneCycleAdam and n == 0        # its composed route forms the norm itself
    # an instance that does not: the trainer clips, as it always did
    trainer, n = one_step(lambda m: torch.optim.Adam(m.parameters(), lr=0.001))
    assert type(trainer.optimizer) is torch.optim.Adam and n == 1
    # defaults and strings build what they built
    assert type(tf.RPNTrainer(g._model(True)).optimizer) is torch.optim.AdamW
    assert type(tf.RPNTrainer(g._model(True), optimizer="sgd").optimizer) is torch.optim.SGD
    assert type(tf.RPNTrainer(g._model(True), optimizer="adam_onecycle", total_steps=10).optimizer) is optim.OneCycleAdam


def test_rcnn_trainers_take_an_optimizer_too():
    from pointrcnn_amd import rcnn

    class cfg(rcnn.RCNNConfig):
        ROI_SAMPLE_JIT = False
    net = rcnn.RCNNNet(cfg=cfg)
    trainer = tf.RCNNOfflineTrainer(net, optimizer=lambda params: optim.ClipAdam(params, lr=0.002, grad_norm_clip=1.0))
    assert type(trainer.optimizer) is optim.ClipAdam and trainer.optimizer.param_groups[0]["params"] == trainer.params
    opt = optim.ClipSGD(net.parameters(), lr=0.01)
    assert tf.RCNNOfflineTrainer(net, optimizer=opt).optimizer is opt
    assert type(tf.RCNNOfflineTrainer(net).optimizer) is torch.optim.AdamW
