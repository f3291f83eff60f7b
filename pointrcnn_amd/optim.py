"""adam_onecycle -- the optimizer the reference trains with (tools/cfgs/default.yaml TRAIN.OPTIMIZER; tools/train_rcnn.py:95-108 and
:135-138): Adam(betas=(mom, 0.99)) inside fastai's OptimWrapper(wd, true_wd=True, bn_wd=True) under OneCycle(total_steps, LR,
MOMS=[0.95, 0.85], DIV_FACTOR=10, PCT_START=0.4) stepped every iteration, with clip_grad_norm_ in front of every step
(tools/train_utils/train_utils.py:135, :188-190).

    one_cycle(step, ...)      the schedule's (lr, mom) of iteration `step` (learning_schedules_fastai.py:40-73)
    adam_scalars(...)         the seven float scalars of one update, formed in double the way torch.optim.Adam forms them
    OneCycleAdam              clip + decoupled decay + Adam + schedule in ONE step(); two routes, one arithmetic contract
                              (csrc/optim_math.h): composed torch ops on any device, or two launches of csrc/optim.hip over all
                              parameter tensors (ops.optim_grad_norm, ops.optim_step) for CUDA(HIP) parameters.

Per element and iteration t = 1, 2, ... with (lr, beta1) = one_cycle(t - 1):
    g = grad * coef,  coef = min(max_norm / (norm + 1e-6), 1)        norm: 2-norm over all gradients; always applied, as torch does
    p *= 1 - wd * lr                                                 every trainable parameter, with or without a gradient
    m += (1 - beta1) * (g - m);  v = v * beta2 + (1 - beta2) * g * g
    p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)   the first bias correction uses the CURRENT beta1

Where this differs from `clip_grad_norm_` + `torch.optim.Adam`:
  * `.grad` is NOT rescaled in memory (the clipped gradient exists in registers only): a trainer drops it next anyway.  Read the
    norm from `last_grad_norm`, not from the gradients.
  * `t` is one counter for the whole optimizer (state[p]["step"] of every parameter holds it), so a parameter whose gradient
    is missing in some iteration is decayed, keeps its moments, and is bias-corrected by the global t afterwards.
  * Non-finite gradients are not special-cased (a NaN norm gives NaN parameters, as in torch).
"""
import os

import numpy as np
import torch

# PRCNN_FUSED_OPTIM=0 forces the composed route (A/B); read here, next to train_functions' two loss switches
FUSED_OPTIM = os.environ.get("PRCNN_FUSED_OPTIM", "1") != "0"


def _annealing_cos(start, end, pct):
    return end + (start - end) / 2 * (np.cos(np.pi * pct) + 1)


def one_cycle(step, total_steps, lr_max=0.002, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4):
    """-> (lr, mom) as Python floats: what OneCycle.step(step) leaves in the optimizer.  Two cosine phases that meet at
    int(total_steps * pct_start): lr low -> max -> low / 1e4 (low = lr_max / div_factor), mom moms[0] -> moms[1] -> moms[0].
    Nothing is clamped: past total_steps the second phase's formula simply continues, as the reference's does."""
    a1 = int(pct_start * total_steps)
    low = lr_max / div_factor
    lr, mom = low, moms[0]
    # every phase that has begun is evaluated, the last one wins (LRSchedulerStep.step), so an empty phase divides by zero here too
    for start, end, lr_ends, mom_ends in ((0, a1, (low, lr_max), (moms[0], moms[1])),
                                          (a1, total_steps, (lr_max, low / 1e4), (moms[1], moms[0]))):
        if step >= start:
            pct = (step - start) / (end - start)
            lr, mom = _annealing_cos(lr_ends[0], lr_ends[1], pct), _annealing_cos(mom_ends[0], mom_ends[1], pct)
    return float(lr), float(mom)


def adam_scalars(lr, beta1, beta2, t, weight_decay, eps):
    """the scalars of csrc/optim_math.h (ops.OPTIM_SCALARS), in double; each is rounded to float32 once, where it is used"""
    bias1 = 1 - beta1 ** t
    bias2 = 1 - beta2 ** t
    return (1 - weight_decay * lr, 1 - beta1, beta2, 1 - beta2, bias2 ** 0.5, eps, -(lr / bias1))


class _Staging:
    """pinned host slots for the pointer table: a slot is rewritten only after the copy that last read it has finished"""

    def __init__(self, shape, slots=2):
        self.slots = [torch.empty(shape, dtype=torch.int64).pin_memory() for _ in range(slots)]
        self.events = [None] * slots
        self.next = 0

    def upload(self, rows, dst):
        i = self.next
        self.next = (i + 1) % len(self.slots)
        if self.events[i] is not None:
            self.events[i].synchronize()            # almost always complete already: the slot was used `slots` uploads ago
        self.slots[i].copy_(torch.tensor(rows, dtype=torch.int64).reshape(self.slots[i].shape))
        dst.copy_(self.slots[i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[i] = ev


class OneCycleAdam(torch.optim.Optimizer):
    """See the module docstring.  fused: None = the device route when every parameter is a CUDA(HIP) float32 tensor and
    PRCNN_FUSED_OPTIM is not 0, the composed route otherwise; True insists on the device route (an error if it cannot run);
    False is the composed route.  grad_norm_clip None: no clip (coef 1; last_grad_norm stays None).

    last_grad_norm: a 0-dim tensor on the parameters' device holding the gradient norm of the last step; reading it is the
    caller's synchronisation, step() itself reads nothing back.  table_uploads counts the pointer-table uploads of the device route."""

    def __init__(self, params, total_steps, lr_max=0.002, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4, weight_decay=0.001,
                 grad_norm_clip=1.0, betas2=0.99, eps=1e-8, fused=None):
        if int(total_steps) < 1 or int(pct_start * int(total_steps)) < 1 or int(pct_start * int(total_steps)) >= int(total_steps):
            raise ValueError("OneCycleAdam: total_steps %r with pct_start %r leaves one of the two phases empty" % (total_steps, pct_start))
        if grad_norm_clip is not None and not grad_norm_clip > 0:
            raise ValueError("OneCycleAdam: grad_norm_clip must be > 0 or None, got %r" % (grad_norm_clip,))
        defaults = dict(total_steps=int(total_steps), lr_max=lr_max, moms=tuple(moms), div_factor=div_factor, pct_start=pct_start,
                        weight_decay=weight_decay, grad_norm_clip=grad_norm_clip, betas2=betas2, eps=eps)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("OneCycleAdam: one parameter group (the reference sets the same hyper-parameters on all of its groups)")
        self.fused = fused
        self.last_grad_norm = None
        self.table_uploads = 0
        self._dev = None                               # the device route's tables, built at its first step

    # ------------------------------------------------------------------ schedule
    @property
    def iteration(self):
        """optimizer steps taken so far (travels in state_dict as every parameter's "step")"""
        for p in self.param_groups[0]["params"]:
            st = self.state.get(p)
            if st:
                return int(st["step"])
        return 0

    def schedule(self, step=None):
        """(lr, mom) of iteration `step` (default: the one the next step() will use)"""
        g = self.param_groups[0]
        return one_cycle(self.iteration if step is None else step, g["total_steps"], g["lr_max"], g["moms"], g["div_factor"], g["pct_start"])

    @property
    def lr(self):
        return self.schedule()[0]

    # ------------------------------------------------------------------ step
    @staticmethod
    def _device_ok(params):
        return all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and (p.grad is None or (
            p.grad.is_cuda and p.grad.dtype == torch.float32 and p.grad.is_contiguous() and not p.grad.is_sparse)) for p in params)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        params = [p for p in g["params"] if p.requires_grad]
        t = self.iteration + 1
        lr, beta1 = self.schedule(t - 1)
        rows = []                                        # the device route's pointer table, collected in the same pass
        for p in params:
            st = self.state[p]
            if not st:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["step"] = t
            rows.append((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                         p.numel()))
        scalars = adam_scalars(lr, beta1, g["betas2"], t, g["weight_decay"], g["eps"])
        want = self.fused if self.fused is not None else (FUSED_OPTIM and bool(params) and params[0].is_cuda)
        # the full eligibility check runs when an address changed; the same addresses are the tensors that passed it last time
        if want and not (self._dev is not None and rows == self._dev["rows"]) and not self._device_ok(params):
            if self.fused:
                raise RuntimeError("OneCycleAdam(fused=True): the device route needs contiguous float32 CUDA(HIP) parameters and gradients")
            want = False
        if want:
            self._step_device(params, rows, scalars, g["grad_norm_clip"])
        else:
            self._step_composed(params, scalars, g["grad_norm_clip"])
        return loss

    def _step_composed(self, params, scalars, max_norm):
        decay, omb1, beta2, omb2, bias2_sqrt, eps, neg_step = scalars
        with_grad = [p for p in params if p.grad is not None]
        coef = None
        self.last_grad_norm = None
        if max_norm is not None:
            if with_grad:
                norms = [torch.linalg.vector_norm(p.grad, 2.0) for p in with_grad]
                total = torch.linalg.vector_norm(torch.stack([n.to(norms[0].device) for n in norms]), 2.0)
            else:
                total = torch.zeros((), dtype=torch.float32, device=params[0].device if params else "cpu")
            coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
            self.last_grad_norm = total
        for p in params:
            p.mul_(decay)
            if p.grad is None:
                continue
            st = self.state[p]
            m, v = st["exp_avg"], st["exp_avg_sq"]
            grad = p.grad if coef is None else p.grad * coef.to(p.grad.device)
            m.lerp_(grad, omb1)
            v.mul_(beta2).addcmul_(grad, grad, value=omb2)
            den = (v.sqrt() / bias2_sqrt).add_(eps)
            p.addcdiv_(m, den, value=neg_step)

    # ------------------------------------------------------------------ device route
    def _step_device(self, params, rows, scalars, max_norm):
        from . import ops
        if not params:
            return
        dev = params[0].device
        d = self._dev
        numels = [r[4] for r in rows]
        if d is None or d["numels"] != numels or d["device"] != dev:
            chunks = ops.optim_chunk_rows(numels)
            d = self._dev = dict(numels=numels, device=dev, rows=None,
                                 table=torch.zeros((len(params), 5), dtype=torch.int64, device=dev),
                                 chunks=torch.tensor(chunks, dtype=torch.int64).reshape(-1, 2).to(dev),
                                 partial=torch.zeros((len(chunks),), dtype=torch.float64, device=dev),
                                 state=torch.zeros((2,), dtype=torch.float32, device=dev),
                                 one=torch.ones((1,), dtype=torch.float32, device=dev),
                                 staging=_Staging((len(params), 5)))
        if rows != d["rows"]:                           # the caching allocator normally hands the same gradient addresses back
            d["staging"].upload(rows, d["table"])
            d["rows"] = rows
            self.table_uploads += 1
        if max_norm is None:
            ops.optim_step(d["table"], d["chunks"], scalars, coef=d["one"])
            self.last_grad_norm = None
        else:
            ops.optim_grad_norm(d["table"], d["chunks"], partial=d["partial"])
            ops.optim_step(d["table"], d["chunks"], scalars, partial=d["partial"], max_norm=max_norm, state=d["state"])
            self.last_grad_norm = d["state"][0]
