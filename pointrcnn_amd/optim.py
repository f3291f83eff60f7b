"""adam_onecycle -- the optimizer the reference trains with (tools/cfgs/default.yaml TRAIN.OPTIMIZER; tools/train_rcnn.py:95-108 and
:135-138): Adam(betas=(mom, 0.99)) inside fastai's OptimWrapper(wd, true_wd=True, bn_wd=True) under OneCycle(total_steps, LR,
MOMS=[0.95, 0.85], DIV_FACTOR=10, PCT_START=0.4) stepped every iteration, with clip_grad_norm_ in front of every step
(tools/train_utils/train_utils.py:135, :188-190).

    one_cycle(step, ...)      the schedule's (lr, mom) of iteration `step` (learning_schedules_fastai.py:40-73)
    adam_scalars(...)         the seven float scalars of one update, formed in double the way torch.optim.Adam forms them
    OneCycleAdam              clip + decoupled decay + Adam + schedule in ONE step(); two routes, one arithmetic contract
                              (csrc/optim_math.h): composed torch ops on any device, or two launches of csrc/optim.hip over all
                              parameter tensors (ops.optim_grad_norm, ops.optim_step) for CUDA(HIP) parameters.
    ClipAdam, ClipSGD         TRAIN.OPTIMIZER adam and sgd (tools/train_rcnn.py:90-94): torch.optim.Adam / SGD that clip the gradient
                              norm inside step(); stock torch on any device, or the same two launches (ops.optim_step_adam,
                              ops.optim_step_sgd).  State and state_dict() are torch's; see _ClipInStep.

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
import math
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
    clips_in_step = True                               # a trainer must not call clip_grad_norm_ in front of step()

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
        if not params:
            return
        _device_launches(self, _device_tables(self, rows, params[0].device), "optim_step", scalars, max_norm)


def _device_tables(opt, rows, dev):
    """the device route's tables of optimizer `opt` (kept in opt._dev) for these pointer rows [param, grad, exp_avg, exp_avg_sq, numel]:
    chunk rows, partial sums and the {norm, coef} state are built once per list of element counts; the pointer table is uploaded
    again (through the pinned staging; opt.table_uploads counts) only when an address changed"""
    from . import ops
    d = opt._dev
    numels = [r[4] for r in rows]
    if d is None or d["numels"] != numels or d["device"] != dev:
        chunks = ops.optim_chunk_rows(numels)
        d = opt._dev = dict(numels=numels, device=dev, rows=None,
                            table=torch.zeros((len(rows), 5), dtype=torch.int64, device=dev),
                            chunks=torch.tensor(chunks, dtype=torch.int64).reshape(-1, 2).to(dev),
                            partial=torch.zeros((len(chunks),), dtype=torch.float64, device=dev),
                            state=torch.zeros((2,), dtype=torch.float32, device=dev),
                            one=torch.ones((1,), dtype=torch.float32, device=dev),
                            staging=_Staging((len(rows), 5)))
    if rows != d["rows"]:                               # the caching allocator normally hands the same gradient addresses back
        d["staging"].upload(rows, d["table"])
        d["rows"] = rows
        opt.table_uploads += 1
    return d


def _device_launches(opt, d, update, scalars, max_norm):
    """the norm launch and the update launch `update` (a name in ops, looked up at the call); sets opt.last_grad_norm"""
    from . import ops
    if max_norm is None:
        getattr(ops, update)(d["table"], d["chunks"], scalars, coef=d["one"])
        opt.last_grad_norm = None
    else:
        ops.optim_grad_norm(d["table"], d["chunks"], partial=d["partial"])
        getattr(ops, update)(d["table"], d["chunks"], scalars, partial=d["partial"], max_norm=max_norm, state=d["state"])
        opt.last_grad_norm = d["state"][0]


def _f32_cuda(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and not t.is_sparse for t in tensors)


class _ClipInStep:
    """What ClipAdam and ClipSGD share: TRAIN.OPTIMIZER adam / sgd of the reference (tools/train_rcnn.py:88-93) with the
    clip_grad_norm_ of its Trainer._train_it (train_utils.py:135) inside step(), on two routes.

      composed   literally clip_grad_norm_(params, grad_norm_clip) followed by torch's own step(): `.grad` is rescaled in memory.
      device     ops.optim_grad_norm and one update launch over all tensors (csrc/optim.hip, arithmetic csrc/optim_math.h): `.grad`
                 keeps its bits; read the norm from last_grad_norm.  lr is read from param_groups[0]["lr"] at every step, so a
                 scheduler's change is used at once.  The state is torch's own (state_dict() loads into the stock class and back).

    fused, last_grad_norm, table_uploads: as OneCycleAdam's.  clips_in_step tells a trainer not to clip a second time."""
    clips_in_step = True

    def _init_clip(self, grad_norm_clip, fused):
        if grad_norm_clip is not None and not grad_norm_clip > 0:
            raise ValueError("%s: grad_norm_clip must be > 0 or None, got %r" % (type(self).__name__, grad_norm_clip))
        self.grad_norm_clip = grad_norm_clip
        self.fused = fused
        self.last_grad_norm = None
        self.table_uploads = 0
        self._dev = None

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("%s: one parameter group" % type(self).__name__)
        super().add_param_group(param_group)

    def _rows_known(self, rows):
        """the same addresses are the tensors that passed the eligibility check last time"""
        return self._dev is not None and rows == self._dev["rows"]

    def _device_rows(self, params):
        """-> (pointer rows, scalars) of the device route, the state brought to where torch's own step would leave it; or a string:
        why this step cannot take the device route"""
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params = self.param_groups[0]["params"]
        with_grad = [p for p in params if p.grad is not None]
        want = self.fused if self.fused is not None else (FUSED_OPTIM and bool(with_grad) and with_grad[0].is_cuda)
        if want and with_grad:
            got = self._device_rows(params)
            if isinstance(got, str):
                if self.fused:
                    raise RuntimeError("%s(fused=True): %s" % (type(self).__name__, got))
                want = False
        if want:
            if with_grad:
                rows, scalars = got
                _device_launches(self, _device_tables(self, rows, with_grad[0].device), self._update, scalars, self.grad_norm_clip)
            else:
                self.last_grad_norm = None
            return loss
        self.last_grad_norm = None
        if self.grad_norm_clip is not None:
            self.last_grad_norm = torch.nn.utils.clip_grad_norm_(params, self.grad_norm_clip)
        super().step()
        return loss


def _step_count(s):
    return int(s.item()) if torch.is_tensor(s) else int(s)


class ClipAdam(_ClipInStep, torch.optim.Adam):
    """torch.optim.Adam (L2 weight decay added to the gradient) that clips the gradient norm inside step(); see _ClipInStep.
    torch counts `step` per parameter and the kernel takes one bias correction per launch, so the device route runs only when
    all parameters that have a gradient share one `step`; otherwise that step takes the composed route."""
    _update = "optim_step_adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 grad_norm_clip=None, fused=None):
        if amsgrad or maximize:
            raise ValueError("ClipAdam: amsgrad and maximize are not built")
        torch.optim.Adam.__init__(self, params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._init_clip(grad_norm_clip, fused)
        self._steps = None

    def _packed_steps(self, states):
        """torch keeps `step` as one 0-dim float32 CPU tensor per parameter; a hundred scalar increments a step cost more than both
        launches.  The counters of these states are therefore made views of ONE flat tensor (the layout stays torch's: its own
        step() increments the views in place, state_dict() hands them out) -> that tensor, element k the `step` of states[k].
        Packed again when a counter is another object than last time (the first step, load_state_dict)."""
        pack = self._steps
        if pack is None or len(pack[1]) != len(states) or any(st["step"] is not v for st, v in zip(states, pack[1])):
            flat = torch.tensor([float(_step_count(st["step"])) for st in states], dtype=torch.float32)
            views = list(flat.unbind(0))
            for st, v in zip(states, views):
                st["step"] = v
            pack = self._steps = (flat, views)
        return pack[0]

    def _device_rows(self, params):
        g = self.param_groups[0]
        rows, states, check = [], [], []
        for p in params:
            st = self.state[p] if p.grad is not None or p in self.state else {}
            if p.grad is not None:
                if not st:                           # as torch.optim.Adam._init_group
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                check += [p, p.grad, st["exp_avg"], st["exp_avg_sq"]]
                states.append(st)
            rows.append((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr(), st["exp_avg"].data_ptr() if st else 0,
                         st["exp_avg_sq"].data_ptr() if st else 0, p.numel()))
        if not self._rows_known(rows) and not _f32_cuda(*check):
            return "the device route needs contiguous float32 CUDA(HIP) parameters, gradients and moments"
        flat = self._packed_steps(states)
        steps = {int(flat.min()), int(flat.max())}
        if len(steps) != 1:
            return "the parameters that have a gradient do not share one `step` (%s)" % sorted(steps)
        t = steps.pop() + 1
        flat.add_(1)
        beta1, beta2 = g["betas"]
        return rows, (g["weight_decay"], 1 - beta1, beta2, 1 - beta2, math.sqrt(1 - beta2 ** t), g["eps"],
                      -(float(g["lr"]) / (1 - beta1 ** t)))


class ClipSGD(_ClipInStep, torch.optim.SGD):
    """torch.optim.SGD with momentum that clips the gradient norm inside step(); see _ClipInStep.  The device route keeps torch's
    `momentum_buffer` (created as zeros, which gives torch's first step buf = g exactly); momentum 0 keeps none."""
    _update = "optim_step_sgd"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 grad_norm_clip=None, fused=None):
        if nesterov or dampening != 0 or maximize:
            raise ValueError("ClipSGD: nesterov, dampening and maximize are not built")
        torch.optim.SGD.__init__(self, params, lr=lr, momentum=momentum, weight_decay=weight_decay)
        self._init_clip(grad_norm_clip, fused)

    def _device_rows(self, params):
        g = self.param_groups[0]
        rows, check = [], []
        for p in params:
            buf = None
            if p.grad is not None:
                if g["momentum"] != 0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                check += [p, p.grad] + ([] if buf is None else [buf])
            rows.append((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr(), 0 if buf is None else buf.data_ptr(), 0, p.numel()))
        if not self._rows_known(rows) and not _f32_cuda(*check):
            return "the device route needs contiguous float32 CUDA(HIP) parameters, gradients and momentum buffers"
        return rows, (g["weight_decay"], g["momentum"], -float(g["lr"]))
