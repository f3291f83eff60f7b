"""The train loop of the reference's tools/train_rcnn.py: epochs, the step-decay learning rate, the cosine warm-up, the BatchNorm
momentum decay, checkpoints and resume (tools/train_utils/train_utils.py; create_optimizer / create_scheduler of
tools/train_rcnn.py:88-143), around this package's trainers (train_functions.RPNTrainer, RCNNTrainer, RCNNOfflineTrainer).

    TrainConfig                              the TRAIN section of tools/cfgs/default.yaml
    lr_decay_factor, bn_momentum_at          the two lambdas of create_scheduler
    BNMomentumScheduler, CosineWarmupLR      train_utils.py:24-57
    create_optimizer, create_scheduler       TRAIN.OPTIMIZER adam / sgd / adam_onecycle -> optim.ClipAdam / ClipSGD / OneCycleAdam
    checkpoint_state, save_checkpoint,       the reference's dictionary {epoch, it, model_state, optimizer_state}; an optimizer_state
    load_checkpoint, load_part_ckpt          in the reference's adam_onecycle layout is read into, and written from, OneCycleAdam
    reference_param_groups                   the two parameter groups of the reference's adam_onecycle, by parameter name
    TrainLoop                                Trainer.train and Trainer.eval_epoch

The loop reads nothing from the device per iteration: loss and gradient norm go into a small device ring that is copied out every
`log_interval` iterations and at the end of an epoch (TrainLoop.host_reads counts the copies)."""
import inspect
import logging
import math
import os
import warnings

import torch
import torch.nn as nn

from . import optim

_LOG = logging.getLogger(__name__)
BN_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)


class TrainConfig:
    """tools/cfgs/default.yaml:129-154"""
    LR = 0.002
    LR_CLIP = 0.00001
    LR_DECAY = 0.5
    DECAY_STEP_LIST = (100, 150, 180, 200)
    LR_WARMUP = True
    WARMUP_MIN = 0.0002
    WARMUP_EPOCH = 1
    BN_MOMENTUM = 0.1
    BN_DECAY = 0.5
    BNM_CLIP = 0.01
    BN_DECAY_STEP_LIST = (1000,)
    OPTIMIZER = "adam_onecycle"
    WEIGHT_DECAY = 0.001
    MOMENTUM = 0.9
    MOMS = (0.95, 0.85)
    DIV_FACTOR = 10.0
    PCT_START = 0.4
    GRAD_NORM_CLIP = 1.0


# ------------------------------------------------------------------------------------------------ schedules
def lr_decay_factor(epoch, cfg=TrainConfig):
    """lr_lbmd (train_rcnn.py:121-126): LR_DECAY for every step of DECAY_STEP_LIST reached, not below LR_CLIP / LR"""
    decay = 1
    for step in cfg.DECAY_STEP_LIST:
        if epoch >= step:
            decay = decay * cfg.LR_DECAY
    return max(decay, cfg.LR_CLIP / cfg.LR)


def bn_momentum_at(epoch, cfg=TrainConfig):
    """bnm_lmbd (train_rcnn.py:128-133).  Trainer.train hands it the ITERATION count (train_utils.py:183), and so does TrainLoop"""
    decay = 1
    for step in cfg.BN_DECAY_STEP_LIST:
        if epoch >= step:
            decay = decay * cfg.BN_DECAY
    return max(cfg.BN_MOMENTUM * decay, cfg.BNM_CLIP)


def set_bn_momentum(momentum):
    def fn(m):
        if isinstance(m, BN_TYPES):
            m.momentum = momentum
    return fn


class BNMomentumScheduler:
    """sets `momentum` of every BatchNorm of `model` to bn_lambda(epoch).  The hand-written training stacks read bn.momentum at
    every call, so the value reaches them with the next forward pass."""

    def __init__(self, model, bn_lambda, last_epoch=-1, setter=set_bn_momentum):
        if not isinstance(model, nn.Module):
            raise RuntimeError("BNMomentumScheduler: %s is not an nn.Module" % type(model).__name__)
        self.model, self.setter, self.lmbd = model, setter, bn_lambda
        self.step(last_epoch + 1)
        self.last_epoch = last_epoch

    def step(self, epoch=None):
        if epoch is None:
            epoch = self.last_epoch + 1
        self.last_epoch = epoch
        self.model.apply(self.setter(self.lmbd(epoch)))


class CosineWarmupLR(torch.optim.lr_scheduler.LRScheduler):
    """eta_min + (base_lr - eta_min) * (1 - cos(pi * step / T_max)) / 2: from eta_min up to the base rate in T_max steps"""

    def __init__(self, optimizer, T_max, eta_min=0, last_epoch=-1):
        self.T_max, self.eta_min = T_max, eta_min
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        return [self.eta_min + (base - self.eta_min) * (1 - math.cos(math.pi * self.last_epoch / self.T_max)) / 2 for base in self.base_lrs]


def step_scheduler_to(scheduler, epoch):
    """scheduler.step(epoch) of the reference, without the deprecated argument: both schedulers here are closed forms of last_epoch"""
    scheduler.last_epoch = epoch - 1
    with warnings.catch_warnings():                      # the reference steps its schedulers at the head of an epoch, before optimizer.step()
        warnings.filterwarnings("ignore", message="Detected call of `lr_scheduler.step\\(\\)` before")
        scheduler.step()


def create_optimizer(cfg, params, total_steps=None):
    """TRAIN.OPTIMIZER -> ClipAdam, ClipSGD or OneCycleAdam over `params`; each clips to GRAD_NORM_CLIP inside its step().
    total_steps (adam_onecycle): iterations per epoch times epochs."""
    params = list(params)
    if cfg.OPTIMIZER == "adam":
        return optim.ClipAdam(params, lr=cfg.LR, weight_decay=cfg.WEIGHT_DECAY, grad_norm_clip=cfg.GRAD_NORM_CLIP)
    if cfg.OPTIMIZER == "sgd":
        return optim.ClipSGD(params, lr=cfg.LR, weight_decay=cfg.WEIGHT_DECAY, momentum=cfg.MOMENTUM, grad_norm_clip=cfg.GRAD_NORM_CLIP)
    if cfg.OPTIMIZER == "adam_onecycle":
        if total_steps is None:
            raise ValueError("create_optimizer: adam_onecycle needs total_steps")
        return optim.OneCycleAdam(params, total_steps, lr_max=cfg.LR, moms=tuple(cfg.MOMS), div_factor=cfg.DIV_FACTOR,
                                  pct_start=cfg.PCT_START, weight_decay=cfg.WEIGHT_DECAY, grad_norm_clip=cfg.GRAD_NORM_CLIP)
    raise NotImplementedError("TRAIN.OPTIMIZER %r" % (cfg.OPTIMIZER,))


def create_scheduler(cfg, optimizer, model, last_epoch=-1):
    """-> (lr_scheduler, bnm_scheduler).  lr_scheduler is None for adam_onecycle, whose schedule lives in OneCycleAdam.step().
    On resume the caller passes last_epoch = start_epoch + 1 (train_rcnn.py:208)."""
    if isinstance(optimizer, optim.OneCycleAdam):
        lr_scheduler = None
    else:
        if last_epoch != -1:
            for g in optimizer.param_groups:             # a loaded optimizer_state carries it; a fresh optimizer does not
                g.setdefault("initial_lr", cfg.LR)
        lr_scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda epoch: lr_decay_factor(epoch, cfg), last_epoch=last_epoch)
    return lr_scheduler, BNMomentumScheduler(model, lambda epoch: bn_momentum_at(epoch, cfg), last_epoch=last_epoch)


# ------------------------------------------------------------------------------------------------ checkpoints
def _unwrap(model):
    if isinstance(model, (nn.DataParallel, nn.parallel.DistributedDataParallel)):
        return model.module
    return model


def reference_param_groups(model):
    """The two parameter groups of the reference's adam_onecycle optimizer (OptimWrapper.create over split_bn_bias,
    train_rcnn.py:96-108) as lists of parameter names of `model`: the parameters of every module without children that is not a
    BatchNorm, in depth-first order, then those of every BatchNorm.  Parameters held directly by a module that has children are
    in neither, as in the reference.  Frozen parameters are included: the reference builds the groups before it freezes the RPN."""
    groups, seen = ([], []), set()

    def walk(m, prefix):
        kids = list(m.named_children())
        for name, c in kids:
            walk(c, prefix + name + ".")
        if not kids:
            for name, p in m.named_parameters(recurse=False):
                if id(p) not in seen:
                    seen.add(id(p))
                    groups[1 if isinstance(m, BN_TYPES) else 0].append(prefix + name)
    walk(_unwrap(model), "")
    return list(groups)


def _reference_onecycle_state(model, optimizer, it):
    """OneCycleAdam's state in the layout torch.optim.Adam under the reference's OptimWrapper saves"""
    names = reference_param_groups(model)
    by_name = dict(_unwrap(model).named_parameters())
    g = optimizer.param_groups[0]
    lr, mom = optimizer.schedule(max(int(it) - 1, 0))          # what OneCycle.step(it - 1) left in the groups
    state, groups, at = {}, [], 0
    for group in names:
        groups.append({"lr": lr, "betas": (mom, g["betas2"]), "eps": g["eps"], "weight_decay": 0, "amsgrad": False,
                       "params": list(range(at, at + len(group)))})
        for name in group:
            st = optimizer.state.get(by_name[name])
            if st:
                state[at] = {"step": int(st["step"]), "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
            at += 1
    return {"state": state, "param_groups": groups}


def checkpoint_state(model=None, optimizer=None, epoch=None, it=None, optimizer_layout="own"):
    """optimizer_layout "reference": a OneCycleAdam's state is written in the reference's two-group layout, so that the reference's
    load_checkpoint reads it; "own": optimizer.state_dict() (which, for ClipAdam and ClipSGD, IS the reference's)"""
    if optimizer_layout not in ("own", "reference"):
        raise ValueError("checkpoint_state: optimizer_layout must be 'own' or 'reference'")
    optim_state = None
    if optimizer is not None:
        if optimizer_layout == "reference" and isinstance(optimizer, optim.OneCycleAdam):
            if model is None:
                raise ValueError("checkpoint_state: the reference layout is rebuilt from the model")
            optim_state = _reference_onecycle_state(model, optimizer, optimizer.iteration if it is None else it)
        else:
            optim_state = optimizer.state_dict()
    state = {"epoch": epoch, "it": it, "model_state": None if model is None else _unwrap(model).state_dict(), "optimizer_state": optim_state}
    pt_utils = _head_tail_utils()
    if pt_utils is not None and model is not None:      # PRCNN_HEAD_TAIL: the Dropout call counters, so that a resumed run replays the masks
        state["dropout_calls"] = pt_utils.dropout_state(_unwrap(model))
    return state


def _head_tail_utils():
    """pytorch_utils when the training heads' device tail is switched on (its masks are keyed by per-module call counters), else None"""
    import pointrcnn_amd
    pointrcnn_amd.install()
    import pointnet2_lib.pointnet2.pytorch_utils as pt_utils
    return pt_utils if pt_utils.HEAD_TAIL else None


def save_checkpoint(state, filename="checkpoint"):
    torch.save(state, "%s.pth" % filename)


def _load_reference_onecycle(model, optimizer, sd, it):
    names = reference_param_groups(model)
    sizes = [len(g["params"]) for g in sd["param_groups"]]
    if sizes != [len(n) for n in names]:
        raise ValueError("load_checkpoint: the optimizer_state has groups of %s parameters, the model's reference layout has %s"
                         % (sizes, [len(n) for n in names]))
    by_name = dict(_unwrap(model).named_parameters())
    own = {id(p): k for k, p in enumerate(optimizer.param_groups[0]["params"])}
    state = {}
    for idx, name in zip([i for g in sd["param_groups"] for i in g["params"]], names[0] + names[1]):
        st = sd["state"].get(idx)
        if not st:
            continue                                     # a frozen parameter: in the groups, never stepped
        if id(by_name[name]) not in own:
            raise ValueError("load_checkpoint: %s has optimizer state but is not among the optimizer's parameters" % name)
        state[own[id(by_name[name])]] = {"step": int(it), "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
    optimizer.load_state_dict({"state": state, "param_groups": optimizer.state_dict()["param_groups"]})


def load_checkpoint(model=None, optimizer=None, filename="checkpoint", logger=_LOG, weights_only=True):
    """-> (it, epoch).  An optimizer_state of two parameter groups offered to a OneCycleAdam is the reference's adam_onecycle
    layout: it is mapped onto the single group by parameter name, and the iteration count is set from `it`.
    weights_only: torch.load's; a checkpoint the reference wrote under adam_onecycle holds numpy scalars (lr, betas) and needs
    False -- unpickling runs code, so only for a file you trust."""
    if not os.path.isfile(filename):
        raise FileNotFoundError(filename)
    logger.info("==> Loading from checkpoint '%s'", filename)
    ckpt = torch.load(filename, map_location="cpu", weights_only=weights_only)
    epoch = ckpt["epoch"] if "epoch" in ckpt else -1
    it = ckpt.get("it", 0.0)
    if model is not None and ckpt["model_state"] is not None:
        _unwrap(model).load_state_dict(ckpt["model_state"])
    pt_utils = _head_tail_utils()
    if pt_utils is not None and model is not None and ckpt.get("dropout_calls") is not None:
        pt_utils.load_dropout_state(_unwrap(model), ckpt["dropout_calls"])
    sd = ckpt["optimizer_state"]
    if optimizer is not None and sd is not None:
        if isinstance(optimizer, optim.OneCycleAdam) and len(sd["param_groups"]) == 2:
            if model is None:
                raise ValueError("load_checkpoint: the reference's adam_onecycle state is mapped through the model's parameter names")
            _load_reference_onecycle(model, optimizer, sd, it)
        else:
            optimizer.load_state_dict(sd)
    logger.info("==> Done")
    return it, epoch


def load_part_ckpt(model, filename, logger=_LOG, total_keys=-1, weights_only=True):
    """the entries of the checkpoint's model_state that the model has (train_rcnn.py --rpn_ckpt)"""
    if not os.path.isfile(filename):
        raise FileNotFoundError(filename)
    logger.info("==> Loading part model from checkpoint '%s'", filename)
    model = _unwrap(model)
    state = model.state_dict()
    update = {k: v for k, v in torch.load(filename, map_location="cpu", weights_only=weights_only)["model_state"].items() if k in state}
    if not update:
        raise RuntimeError("load_part_ckpt: %s holds no entry of this model" % filename)
    state.update(update)
    model.load_state_dict(state)
    logger.info("==> Done (loaded %d/%d)", len(update), total_keys)


# ------------------------------------------------------------------------------------------------ the loop
class TrainLoop:
    """Trainer of tools/train_utils/train_utils.py around one of this package's trainers; a step is
    trainer.step(batch, next_batch=...), so the furthest-point-sampling prefetch keeps working.  The order of operations is the
    reference's: lr_scheduler.step(epoch) only from warmup_epoch on, the warm-up scheduler per iteration before that,
    bnm_scheduler.step(it) with the ITERATION count, checkpoint every ckpt_save_interval epochs, evaluation every eval_frequency.

    lr_scheduler None: the schedule is the optimizer's own (OneCycleAdam), and `learning_rate` is its `lr`.
    tb_log: anything with add_scalar(tag, value, step); it receives train_loss, learning_rate, bn_momentum, grad_norm, val_loss
    and val_*, the per-iteration ones when the ring is copied out.  model: what the checkpoints hold (default trainer.model)."""

    def __init__(self, trainer, optimizer, lr_scheduler, bnm_scheduler, ckpt_dir, tb_log=None, eval_frequency=1,
                 lr_warmup_scheduler=None, warmup_epoch=-1, log_interval=50, model=None, optimizer_layout="own"):
        self.trainer, self.optimizer, self.lr_scheduler, self.bnm_scheduler = trainer, optimizer, lr_scheduler, bnm_scheduler
        self.ckpt_dir, self.tb_log, self.eval_frequency = ckpt_dir, tb_log, eval_frequency
        self.lr_warmup_scheduler, self.warmup_epoch = lr_warmup_scheduler, warmup_epoch
        self.log_interval = max(int(log_interval), 1)
        self.model = trainer.model if model is None else model
        self.optimizer_layout = optimizer_layout
        self.host_reads = 0                            # copies of the ring to the host (each one waits for the device)
        self.last_loss = None                          # the loss of the last iteration copied out
        self._ring, self._pending = None, []
        self._prefetches = "next_batch" in inspect.signature(trainer.step).parameters

    # ---------------------------------------------------------------- the ring
    def _record(self, it, lr, loss, norm):
        if self._ring is None or self._ring.device != loss.device:
            self._ring = torch.zeros((self.log_interval, 2), dtype=torch.float32, device=loss.device)
        row = self._ring[len(self._pending)]
        row[0].copy_(loss.detach())
        if norm is not None:
            row[1].copy_(norm.detach())
        self._pending.append((it, lr, norm is not None))
        if len(self._pending) == self.log_interval:
            self._flush()

    def _flush(self):
        if not self._pending:
            return
        vals = self._ring[:len(self._pending)].cpu().tolist()      # the one host read
        self.host_reads += 1
        for (it, lr, has_norm), (loss, norm) in zip(self._pending, vals):
            if self.tb_log is not None:
                self.tb_log.add_scalar("train_loss", loss, it)
                self.tb_log.add_scalar("learning_rate", lr, it)
                if has_norm:
                    self.tb_log.add_scalar("grad_norm", norm, it)
        self.last_loss = vals[-1][0]
        self._pending = []

    # ---------------------------------------------------------------- evaluation
    def eval_epoch(self, batches):
        """-> (mean loss, mean of every tb_dict entry [+ recall], cur_performance), as Trainer.eval_epoch"""
        self.model.eval()
        eval_dict, total, count = {}, 0.0, 0
        with torch.no_grad():
            for batch in batches:
                tb = {}
                total += float(self.trainer.loss(batch, tb))
                count += 1
                for k, v in tb.items():
                    eval_dict[k] = eval_dict.get(k, 0) + v
        for k in eval_dict:
            eval_dict[k] = eval_dict[k] / max(count, 1)
        performance = 0
        if "recalled_cnt" in eval_dict:
            eval_dict["recall"] = eval_dict["recalled_cnt"] / max(eval_dict["gt_cnt"], 1)
            performance = eval_dict["recall"]
        elif "iou" in eval_dict:
            performance = eval_dict["iou"]
        return total / count, eval_dict, performance

    # ---------------------------------------------------------------- training
    def train(self, start_it, start_epoch, n_epochs, train_batches, test_batches=None, ckpt_save_interval=5):
        """train_batches / test_batches: anything that can be iterated once per epoch"""
        eval_frequency = self.eval_frequency if self.eval_frequency > 0 else 1
        it = start_it
        for epoch in range(start_epoch, n_epochs):
            if self.lr_scheduler is not None and self.warmup_epoch <= epoch:
                step_scheduler_to(self.lr_scheduler, epoch)
            if self.bnm_scheduler is not None:
                self.bnm_scheduler.step(it)
                if self.tb_log is not None:
                    self.tb_log.add_scalar("bn_momentum", self.bnm_scheduler.lmbd(epoch), it)
            batches = iter(train_batches)
            batch = next(batches, None)
            while batch is not None:
                next_batch = next(batches, None)
                if self.lr_scheduler is None:
                    cur_lr = float(self.optimizer.lr)
                elif self.lr_warmup_scheduler is not None and epoch < self.warmup_epoch:
                    step_scheduler_to(self.lr_warmup_scheduler, it)
                    cur_lr = self.lr_warmup_scheduler.get_last_lr()[0]
                else:
                    cur_lr = self.lr_scheduler.get_last_lr()[0]
                loss = self.trainer.step(batch, next_batch=next_batch) if self._prefetches else self.trainer.step(batch)
                it += 1
                self._record(it, cur_lr, loss, getattr(self.optimizer, "last_grad_norm", None))
                batch = next_batch
            self._flush()
            trained_epoch = epoch + 1
            if trained_epoch % ckpt_save_interval == 0:
                save_checkpoint(checkpoint_state(self.model, self.optimizer, trained_epoch, it, self.optimizer_layout),
                                filename=os.path.join(self.ckpt_dir, "checkpoint_epoch_%d" % trained_epoch))
            if epoch % eval_frequency == 0 and test_batches is not None:
                val_loss, eval_dict, _ = self.eval_epoch(test_batches)
                if self.tb_log is not None:
                    self.tb_log.add_scalar("val_loss", val_loss, it)
                    for k, v in eval_dict.items():
                        self.tb_log.add_scalar("val_" + k, v, it)
        return it
