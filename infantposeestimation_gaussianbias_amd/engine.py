"""Training engine (S1): flat parameter storage, fused AdamW, per-iteration LR schedule, data-parallel gradient exchange.

MI355X-first layout: all parameters live in ONE fp32 buffer, all gradients in another (each `param.data` / `param.grad`
is a view), so
  * the optimiser is one HIP launch over the whole model (pk_adamw_step) instead of ~820 per-tensor updates,
  * the gradient all-reduce runs on a few large contiguous slices (RCCL over xGMI is per-link bound: few, big messages),
    issued from autograd hooks while backward is still producing earlier layers' gradients,
  * averaging over ranks is folded into the optimiser kernel (grad_scale = 1/world).
Semantics follow train.py:55-128: AdamW(lr 5e-4, betas (.9,.999), wd .01 on the "decay" group), parameters whose name
contains 'bias' / 'bn' / 'norm' are not decayed; parameters that never receive a gradient (41 tensors for
HRFormer-small) are left untouched exactly as torch.optim.AdamW skips `grad is None`.
"""
import collections
import contextlib
import math
import os
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import hipops, nnops


def is_no_decay(name: str) -> bool:
    return "bias" in name or "bn" in name or "norm" in name          # train.py:66


def lr_factor(it: int, iters_per_epoch: int, cfg_train) -> float:
    """LambdaLR factor, stepped per iteration: linear warm-up over warmup_epochs, then x gamma at each milestone epoch."""
    warm = cfg_train.warmup_epochs * iters_per_epoch
    if it < warm:
        r = cfg_train.warmup_lr / cfg_train.lr
        return r + (1 - r) * it / warm
    f = 1.0
    for m in cfg_train.lr_milestones:
        if it >= m * iters_per_epoch:
            f *= cfg_train.lr_gamma
    return f


def checkpoint_weights(ckpt, ema=False):
    """The model state dict of a train.py checkpoint: the raw weights, or with `ema` the averaged ones a run with `--ema` saved."""
    key = "ema_state_dict" if ema else "model_state_dict"
    if key not in ckpt:
        hint = " (it was not trained with train.py --ema)" if ema else ""
        raise KeyError(f"the checkpoint has no '{key}'{hint}; its keys: {sorted(ckpt)}")
    return ckpt[key]


class FlatAdamW:
    """Owns the flat buffers of `model` and applies the fused optimiser step."""

    ALIGN = 4            # elements: every tensor starts 16-byte aligned inside the flat buffers

    def __init__(self, model: torch.nn.Module, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, direct_grads=False,
                 clip_grad_norm=0.0, skip_nonfinite=False, ema_decay=0.0, trace_nonfinite=False):
        """`clip_grad_norm` > 0 (torch.nn.utils.clip_grad_norm_'s max_norm) or `skip_nonfinite` select the guarded step: the global
        gradient norm is reduced on the device, the update is scaled by the clip coefficient and dropped as a whole when a gradient is
        inf / NaN (what GradScaler.step does in the reference).  A non-finite norm cannot clip anything, so clipping implies skipping.

        `ema_decay` in (0, 1) keeps an exponential moving average of the masters in `self.ema`, written by the update kernel itself
        (pk_adamw_step_ema): e += (1 - d_t) (p_new - e) with d_t = min(ema_decay, (1 + t) / (10 + t)), t = applied updates.  It moves
        only when the masters do (a skipped step freezes it), and only on the elements the optimiser updates.  0 = off: no buffer, and
        the launches are the ones above.

        `trace_nonfinite` adds the per-tensor gradient statistics (pk_tensor_stats) and their latch to every step, between the guard's
        reduction and the update: when a gradient is inf / NaN the records of that step stay in `trace_latched` until the next such
        step, and `nonfinite_trace()` names the tensors.  Off: no launch, no buffer."""
        if not (math.isfinite(clip_grad_norm) and clip_grad_norm >= 0):
            raise ValueError(f"clip_grad_norm must be finite and >= 0 (0 = off), got {clip_grad_norm}")
        if not (math.isfinite(ema_decay) and 0 <= ema_decay < 1):
            raise ValueError(f"ema_decay must be finite and in [0, 1) (0 = off), got {ema_decay}")
        self.model = model
        self.direct_grads = direct_grads
        self.clip_grad_norm = float(clip_grad_norm)
        self.guarded = self.clip_grad_norm > 0 or bool(skip_nonfinite)
        self.ema_decay = float(ema_decay)
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        if not named:
            raise ValueError("model has no trainable parameters")
        dev = named[0][1].device
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += -(-p.numel() // self.ALIGN) * self.ALIGN
        self.numel = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(off, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(off, dtype=torch.float32, device=dev)
        flags = torch.zeros(off, dtype=torch.uint8)
        for n, p, o in zip(self.names, self.params, self.offsets):
            self.flat[o:o + p.numel()].copy_(p.data.reshape(-1))
            p.data = self.flat[o:o + p.numel()].view_as(p)
            flags[o:o + p.numel()] = 2 | (0 if is_no_decay(n) else 1)
        self.flags = flags.to(dev)
        self.active = [True] * len(self.params)
        self._grads_installed = False
        self._sinks_armed = False          # True once a whole step has run with the gradient sinks installed
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.lr_dev = torch.full((1,), lr, dtype=torch.float32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.step_count = 0          # steps taken; guarded mode: steps ATTEMPTED (step_dev counts the applied ones)
        if self.guarded:
            # static buffers (a captured graph holds their addresses): per-workgroup partial sums, and the record the update reads
            self.guard_partials = torch.zeros(hipops.grad_sumsq_partials(off), 2, dtype=torch.float64, device=dev)
            self.guard_state = torch.zeros(hipops.GUARD_STATE_WORDS, dtype=torch.int32, device=dev)
        # static as well: the averaged weights, starting as a copy of the masters (padding and inactive elements keep that copy)
        self.ema = self.flat.clone() if self.ema_decay > 0 else None
        # per-tensor statistics: nothing exists until tensor_stats / snapshot_params are called or the trace is on
        self._stats_plan = None
        self.snapshot = None
        self.trace_nonfinite = bool(trace_nonfinite)
        if self.trace_nonfinite:
            plan = self._need_stats_plan()
            self.trace_records = torch.zeros_like(plan.records)          # the trace's own: a logged tensor_stats call leaves them alone
            self.trace_latched = torch.zeros_like(plan.records)
            self.trace_state = torch.zeros(hipops.LATCH_STATE_WORDS, dtype=torch.int32, device=dev)

    # -- gradient storage ---------------------------------------------------------------------------------
    def grad_view(self, i):
        p, o = self.params[i], self.offsets[i]
        return self.grad[o:o + p.numel()].view_as(p)

    def install_grad_views(self):
        """Adopt the gradients autograd produced on the first backward: parameters still without a gradient are the
        structurally unused ones -> marked inactive (flag bit1 cleared) so the optimiser never touches them."""
        inactive = []
        for i, p in enumerate(self.params):
            v = self.grad_view(i)
            if p.grad is None:
                self.active[i] = False
                inactive.append(i)
                v.zero_()
            else:
                v.copy_(p.grad)
            p.grad = v
        if inactive:
            fl = self.flags.cpu()
            for i in inactive:
                o, n = self.offsets[i], self.params[i].numel()
                fl[o:o + n] &= 0xFD
            self.flags.copy_(fl)
        self._grads_installed = True
        if self.direct_grads:
            # backward kernels now store parameter gradients straight into these views (no autograd accumulation)
            for i, p in enumerate(self.params):
                p._pk_grad_sink = self.grad_view(i)

    def zero_grad(self):
        if self._grads_installed:
            if not self.direct_grads:          # with the gradient sink every active gradient is overwritten, not accumulated
                self.grad.zero_()
            else:
                nnops.begin_grad_epoch()       # a sink may be stored to once per epoch (checked in nnops.grad_sink_of)
        else:
            for p in self.params:
                p.grad = None

    # -- update ------------------------------------------------------------------------------------------------
    def set_lr(self, lr: float):
        self.lr = lr
        self.lr_dev.fill_(lr)

    def step(self, grad_scale: float = 1.0):
        if self.flat.is_cuda:
            nnops.finalize_deferred()          # postponed parameter-gradient reductions (no-op when the Trainer already ran them)
        if not self._grads_installed:
            self.install_grad_views()
        elif self.direct_grads and self._sinks_armed:
            # direct-store sinks are not zeroed between steps: an active parameter whose sink no backward kernel asked for in
            # this step (a batch that skipped a branch) must not have last step's gradient applied again
            for i, p in enumerate(self.params):
                if self.active[i] and not nnops.sink_written(p):
                    self.grad_view(i).zero_()
        self._sinks_armed = self.direct_grads
        self.step_count += 1
        if self.guarded:
            # the finalize kernel advances step_dev, and only when the update is applied
            hipops.grad_sumsq(self.grad, self.flags, self.guard_partials)
            hipops.grad_guard_finalize(self.guard_partials, grad_scale, self.clip_grad_norm, self.guard_state, self.step_dev)
        else:
            self.step_dev.add_(1)
        if self.trace_nonfinite:
            # static buffers throughout: inside a captured step these three launches are replayed with it
            hipops.tensor_stats(self._stats_plan, self.grad, flags=self.flags, records=self.trace_records)
            hipops.tensor_stats_latch(self.trace_records, len(self.params), self.trace_latched, self.trace_state)
        if self.ema is not None:
            # update and average in one pass; the kernel reads the skip decision and the step count where the update reads them
            hipops.adamw_step_ema(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.flags, None, self.lr_dev, self.step_dev,
                                  self.betas[0], self.betas[1], self.eps, self.weight_decay, self.guard_state if self.guarded else None,
                                  self.ema, self.ema_decay, grad_scale)
        elif self.guarded:
            hipops.adamw_step_guarded(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.flags, None, self.lr_dev, self.step_dev,
                                      self.betas[0], self.betas[1], self.eps, self.weight_decay, self.guard_state, grad_scale)
        else:
            hipops.adamw_step(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.flags, None, self.lr_dev, self.step_dev,
                              self.betas[0], self.betas[1], self.eps, self.weight_decay, grad_scale)
        self._masters_rewritten()

    def _masters_rewritten(self):
        wc = getattr(self.model, "_pk_weight_cache", None)
        if wc is not None:
            wc.mark_dirty()          # the kernel rewrote the fp32 masters behind torch's back: bf16 copies are stale
        tw = getattr(self.model, "_pk_twin", None)
        if tw:
            tw.mark_dirty()          # ... and so is the padded twin's embedded copy

    # -- weight EMA --------------------------------------------------------------------------------------------
    def _need_ema(self, who):
        if self.ema is None:
            raise RuntimeError(f"{who}: the weight EMA is off (ema_decay=0)")

    def reset_ema(self):
        """ema <- flat: after the masters were replaced from outside (initial broadcast, a checkpoint without averaged weights)."""
        self._need_ema("reset_ema")
        self.ema.copy_(self.flat)

    def ema_state_dict(self):
        """The model's state dict with the averaged value of every tensor that lives in the flat buffer.  Everything else (BatchNorm
        running statistics and counters, other buffers, tensors that do not train) is the live model's current value: running
        statistics are moving averages already, so they are copied, not averaged a second time."""
        self._need_ema("ema_state_dict")
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        for n, p, o in zip(self.names, self.params, self.offsets):
            if n in sd:
                sd[n] = self.ema[o:o + p.numel()].view_as(p).clone()
        return sd

    def load_ema_state_dict(self, sd):
        """Fill the EMA buffer from a model-style state dict (ema_state_dict's); entries for tensors outside the flat buffer are ignored
        (they belong to the model's own state dict)."""
        self._need_ema("load_ema_state_dict")
        missing = [n for n in self.names if n not in sd]
        if missing:
            raise KeyError(f"load_ema_state_dict: no entry for {missing[:5]}{' ...' if len(missing) > 5 else ''}")
        for n, p, o in zip(self.names, self.params, self.offsets):
            if tuple(sd[n].shape) != tuple(p.shape):
                raise ValueError(f"load_ema_state_dict: {n} has shape {tuple(sd[n].shape)}, the model's is {tuple(p.shape)}")
            self.ema[o:o + p.numel()].copy_(sd[n].reshape(-1))

    def swap_ema(self):
        """Exchange the CONTENTS of flat and ema: captured graphs and every param.data view hold flat's address, so pointers stay."""
        self._need_ema("swap_ema")
        tmp = self.flat.clone()
        self.flat.copy_(self.ema)
        self.ema.copy_(tmp)
        self._masters_rewritten()

    def guard_stats(self):
        """Last step's gradient norm (after grad_scale, before clipping), clip coefficient, whether it was skipped, and the number of
        skipped steps so far.  One device read: for the log interval, never for the step path."""
        if not self.guarded:
            raise RuntimeError("guard_stats: the guarded step is off (clip_grad_norm=0, skip_nonfinite=False)")
        st = self.guard_state.cpu()
        norm, coef = st[:2].view(torch.float32).tolist()
        return {"grad_norm": norm, "clip_coef": coef, "skipped_last": int(st[2]), "skipped_steps": int(st[3])}

    # -- per-tensor statistics ---------------------------------------------------------------------------------
    STATS_BUFFERS = ("grad", "param", "exp_avg", "exp_avg_sq", "ema", "update")

    def _need_stats_plan(self):
        if self._stats_plan is None:
            # one upload of the plan; the table never changes, so the same launches can sit in a graph
            self._stats_plan = hipops.TensorStatsPlan(self.offsets, [p.numel() for p in self.params], self.flat.device)
        return self._stats_plan

    def _stats_buffer(self, which, who):
        if which == "ema":
            self._need_ema(who)
            return self.ema
        if which not in ("grad", "param", "exp_avg", "exp_avg_sq"):
            raise ValueError(f"{who}: unknown buffer '{which}' (one of {', '.join(self.STATS_BUFFERS)})")
        return {"grad": self.grad, "param": self.flat, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}[which]

    def snapshot_params(self):
        """snapshot <- flat on the current stream (a static buffer, allocated on first use): tensor_stats("update") is then the
        statistics of flat - snapshot, i.e. of everything the steps since have done to the weights."""
        if self.snapshot is None:
            self.snapshot = torch.empty_like(self.flat)
        self.snapshot.copy_(self.flat)

    def tensor_stats(self, which="grad", against=None, tiny=0.0, scale=1.0):
        """Per-tensor statistics of one flat buffer ("grad", "param", "exp_avg", "exp_avg_sq", "ema"), of `which - against`, or with
        "update" of flat - snapshot: {name: {mean, std, min, max, norm, abs_mean, abs_max, numel, nonfinite, small}} in parameter
        order, over the finite elements the optimiser updates (`small`: |x| <= tiny; inactive tensors have numel 0).  `scale`
        multiplies the linear values (comm.grad_scale: the gradients the update sees).  Two launches on the current stream and ONE
        device read of 64 bytes per tensor: for the log interval, never for the step path."""
        if which == "update":
            if against is not None:
                raise ValueError("tensor_stats: 'update' is flat - snapshot already; it takes no `against`")
            if self.snapshot is None:
                raise RuntimeError("tensor_stats: 'update' needs a snapshot (snapshot_params(), or Trainer.step(batch, snapshot=True))")
            a, b = self.flat, self.snapshot
        else:
            a = self._stats_buffer(which, "tensor_stats")
            b = None if against is None else self._stats_buffer(against, "tensor_stats")
        plan = self._need_stats_plan()
        recs = hipops.tensor_stats_records(hipops.tensor_stats(plan, a, b, self.flags, tiny))
        return collections.OrderedDict((n, hipops.derive_tensor_stats(r, scale)) for n, r in zip(self.names, recs))

    def nonfinite_trace(self):
        """None while no step held a non-finite gradient; else {"events": how many steps did, "tensors": {name: non-finite elements}
        of the latest one, "first", "last": the first and last of them in parameter order}.  `last` is the tensor nearest the loss,
        the one to look at once NaN has spread backwards.  One device read."""
        if not self.trace_nonfinite:
            raise RuntimeError("nonfinite_trace: the trace is off (trace_nonfinite=False)")
        events, first, last, _ = self.trace_state.tolist()
        if events == 0:
            return None
        recs = hipops.tensor_stats_records(self.trace_latched)
        tensors = collections.OrderedDict((n, int(r["nonfinite"])) for n, r in zip(self.names, recs) if r["nonfinite"] > 0)
        return {"events": events, "tensors": tensors, "first": self.names[first], "last": self.names[last]}

    # -- checkpoint format of the reference (train.py:351-357): per-parameter state keyed by index ---------------
    def state_dict(self):
        decay = [i for i, n in enumerate(self.names) if not is_no_decay(n)]
        nodecay = [i for i, n in enumerate(self.names) if is_no_decay(n)]
        order = decay + nodecay
        remap = {old: new for new, old in enumerate(order)}
        state = {}
        # guarded mode: "step" is the number of APPLIED updates (the bias correction's t), which only the device knows
        steps = int(self.step_dev) if self.guarded else self.step_count
        for i, p in enumerate(self.params):
            if not self.active[i] or steps == 0:
                continue
            o, n = self.offsets[i], p.numel()
            state[remap[i]] = {"step": torch.tensor(float(steps)),
                               "exp_avg": self.exp_avg[o:o + n].view_as(p).clone(),
                               "exp_avg_sq": self.exp_avg_sq[o:o + n].view_as(p).clone()}
        common = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "amsgrad": False, "maximize": False,
                  "foreach": None, "capturable": False, "differentiable": False, "fused": None, "initial_lr": self.lr}
        groups = [dict(common, weight_decay=self.weight_decay, params=[remap[i] for i in decay]),
                  dict(common, weight_decay=0.0, params=[remap[i] for i in nodecay])]
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        decay = [i for i, n in enumerate(self.names) if not is_no_decay(n)]
        nodecay = [i for i, n in enumerate(self.names) if is_no_decay(n)]
        order = decay + nodecay
        steps = 0
        for new, old in enumerate(order):
            st = sd["state"].get(new)
            if st is None:
                continue
            o, n = self.offsets[old], self.params[old].numel()
            self.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
            steps = max(steps, int(float(st["step"])))
        self.step_count = steps
        self.step_dev.fill_(steps)
        if sd.get("param_groups"):
            self.set_lr(float(sd["param_groups"][0]["lr"]))


def update_to_weight_ratio(update_stats, param_stats):
    """norm(update) / norm(param) per tensor from tensor_stats("update") and tensor_stats("param"); nan where the weights are all zero
    (or the tensor is inactive)."""
    return collections.OrderedDict((n, u["norm"] / param_stats[n]["norm"] if param_stats[n]["norm"] > 0 else float("nan"))
                                   for n, u in update_stats.items())


class WarmupMultiStepLR:
    """Per-iteration schedule of train.py:100-128 with LambdaLR's state_dict fields the reference checkpoints carry."""

    def __init__(self, optimizer: FlatAdamW, cfg_train, iters_per_epoch: int):
        self.opt, self.cfg, self.ipe = optimizer, cfg_train, iters_per_epoch
        self.base_lr = cfg_train.lr
        self.last_epoch = 0
        optimizer.set_lr(self.base_lr * lr_factor(0, iters_per_epoch, cfg_train))

    def step(self):
        self.last_epoch += 1
        self.opt.set_lr(self.base_lr * lr_factor(self.last_epoch, self.ipe, self.cfg))

    def get_last_lr(self):
        return [self.opt.lr, self.opt.lr]

    def state_dict(self):
        return {"base_lrs": [self.base_lr, self.base_lr], "last_epoch": self.last_epoch, "_step_count": self.last_epoch + 1,
                "_last_lr": self.get_last_lr(), "lr_lambdas": [None]}

    def load_state_dict(self, sd):
        self.last_epoch = int(sd["last_epoch"])
        self.opt.set_lr(self.base_lr * lr_factor(self.last_epoch, self.ipe, self.cfg))


class GradientExchange:
    """Data-parallel gradient sum over ranks on the flat gradient buffer (RCCL `nccl` backend on GPUs, gloo on CPU).

    Buckets are contiguous slices of the flat buffer, built from the END (backward produces the last layers first).  A bucket's
    all-reduce is launched asynchronously (RCCL runs it on its own stream) as soon as every ACTIVE parameter in it has its final
    gradient of the step, so the exchange of the head's / late stages' gradients overlaps with the rest of backward:
      * gradient-sink mode (FlatAdamW(direct_grads=True), the Trainer's default): `flush_ready()` is called from backward
        MILESTONES (nnops.backward_milestone: hooks on the stage-boundary tensors, fired when backward has passed them) after the
        postponed slab reductions registered so far have been run; readiness = the parameter's sink was stored to this step;
      * plain autograd mode (`overlap=True`): post-accumulate hooks count a bucket's gradients.
    `finish()` launches whatever is left and waits.  Parameters that never receive a gradient (41 tensors for HRFormer-small,
    SURVEY §8e) are skipped consistently on all ranks (the active set is structural)."""

    def __init__(self, opt: FlatAdamW, bucket_mb: float = 16.0, group=None, overlap: bool = False):
        self.opt, self.group, self.overlap = opt, group, overlap
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.bucket_elems = int(bucket_mb * (1 << 20) / 4)
        self.buckets: List[Dict] = []
        self._hooks = []
        self._pending = []
        self._armed = False
        self.suspended = False          # True while a hipGraph without collectives is being captured: milestones must not launch any
        self.launched_early = 0         # buckets launched from milestones / hooks in the last step (observability, tests)
        # exposed communication: time the COMPUTE stream spends in finish() -- launching the buckets that did not overlap with backward
        # and waiting for all of them -- measured with events on that stream when `record_exposed` is set (bench.py --gpus N reports it)
        self.record_exposed = False
        self._exposed = []

    def broadcast_initial_state(self):
        if self.world == 1:
            return
        dist.broadcast(self.opt.flat, 0, group=self.group)
        for b in self.opt.model.buffers():
            dist.broadcast(b, 0, group=self.group)

    def _build(self):
        opt = self.opt
        hi, cur, members = opt.numel, opt.numel, []
        plan = []
        for i in reversed(range(len(opt.params))):
            members.append(i)
            cur = opt.offsets[i]
            if hi - cur >= self.bucket_elems or i == 0:
                plan.append((cur, hi, members))
                hi, members = cur, []
        self.buckets = [{"lo": lo, "hi": hi_, "members": [i for i in m if opt.active[i]], "need": sum(1 for i in m if opt.active[i]), "got": 0}
                        for lo, hi_, m in plan]
        owner = {}
        for b, (_, _, m) in enumerate(plan):
            for i in m:
                owner[i] = b
        if self.overlap and not opt.direct_grads:
            for i, p in enumerate(opt.params):
                if opt.active[i]:
                    self._hooks.append(p.register_post_accumulate_grad_hook(self._make_hook(owner[i])))
        self._armed = True

    def _make_hook(self, b):
        def hook(_param):
            bk = self.buckets[b]
            bk["got"] += 1
            if bk["got"] == bk["need"] and not self.suspended:
                self.launched_early += 1
                self._launch(bk)
        return hook

    def _launch(self, bk):
        bk["got"] = -1     # launched
        self._pending.append(dist.all_reduce(self.opt.grad[bk["lo"]:bk["hi"]], op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def flush_ready(self):
        """Gradient-sink mode: launch, in backward order, every bucket whose active parameters have all been stored to this step.
        The caller has run nnops.finalize_deferred() first, so a stored-to sink holds its final value."""
        if self.world == 1 or not self._armed or self.suspended or not self.opt.direct_grads:
            return
        from . import nnops as _nn
        for bk in self.buckets:
            if bk["got"] == -1:
                continue
            if not all(_nn.sink_written(self.opt.params[i]) for i in bk["members"]):
                break               # buckets are ordered by backward time: later ones cannot be complete either
            self.launched_early += 1
            self._launch(bk)

    def finish(self):
        """Call after backward: flush buckets that did not fire (first step, or only inactive members), wait for all."""
        if self.world == 1:
            return
        if not self.opt._grads_installed:
            self.opt.install_grad_views()
        if not self._armed:
            self._build()
        timed = self.record_exposed and self.opt.grad.is_cuda and not torch.cuda.is_current_stream_capturing()
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        for bk in self.buckets:
            if bk["got"] != -1:
                self._launch(bk)
        for w in self._pending:
            w.wait()
        self._pending.clear()
        if timed:
            e1.record()
            self._exposed.append((e0, e1))
        for bk in self.buckets:
            bk["got"] = 0

    def exposed_ms(self):
        """Mean time per step the compute stream was held by the gradient exchange since the last call (None: nothing recorded, e.g.
        the collectives live inside a captured graph).  Synchronises."""
        if not self._exposed:
            return None
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in self._exposed]
        self._exposed = []
        return sum(ms) / len(ms)

    @property
    def grad_scale(self):
        return 1.0 / self.world


class Trainer:
    """One optimisation step of train.py::train_one_epoch (:169-187) without its per-step host syncs.

    `use_graph=True` captures zero_grad + forward + backward + gradient exchange + optimiser of a fixed-shape batch into a hipGraph
    after `graph_warmup` eager steps and replays it: ~1 300 kernel launches per step become one graph launch, which removes the
    host as the bottleneck.  With N>1 ranks over RCCL the bucketed all-reduces are captured too: they are issued from backward
    milestones on RCCL's own stream, so inside the replayed graph they run beside the remaining backward kernels, and AdamW follows
    in the same graph.  When the collectives cannot be captured (gloo, or a capture the runtime refuses) the graph holds
    zero_grad + forward + backward only and the exchange + AdamW run between replays.  The LR is written to a device scalar before
    each replay, so the per-iteration schedule advances normally.  Batches are copied into static input buffers."""

    def __init__(self, model, cfg, iters_per_epoch: int, bucket_mb: float = 8.0, use_graph: bool = False, graph_warmup: int = 3,
                 overlap_comm: bool = True, graph_streams: bool = False, clip_grad_norm: float = 0.0, skip_nonfinite: bool = False,
                 ema_decay: float = 0.0, trace_nonfinite: bool = False):
        self.model, self.cfg = model, cfg
        self.overlap_comm = overlap_comm
        # concurrent branch streams: on for eager steps; inside a captured graph only on request (fork/join capture across
        # streams, see scripts/gpu_graph_streams.py)
        self._want_streams = graph_streams if use_graph else True
        self._region = graph_streams               # with use_graph=False: eager launches, same autograd structure as the graph
        t = cfg.train
        if t.optimizer != "AdamW":
            raise ValueError(f"Unknown optimizer: {t.optimizer}")   # the fused kernel implements the reference default only
        # gradients are stored directly by the backward kernels (gradient sinks); the exchange is driven by backward milestones
        # clip_grad_norm / skip_nonfinite: the guarded step lives inside opt.step, so eager steps, the captured whole step and the
        # optimiser between forward+backward-only replays all take it; the LR schedule advances on skipped steps too (as the
        # reference's scheduler.step() does)
        self.opt = FlatAdamW(model, t.lr, tuple(t.betas), 1e-8, t.weight_decay, direct_grads=True, clip_grad_norm=clip_grad_norm,
                             skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, trace_nonfinite=trace_nonfinite)
        self.sched = WarmupMultiStepLR(self.opt, t, iters_per_epoch)
        self.comm = GradientExchange(self.opt, bucket_mb, overlap=overlap_comm)
        self.comm.broadcast_initial_state()
        if self.opt.ema is not None:
            # every rank starts its average from the broadcast weights; from here on the ranks average identical masters with
            # identical arithmetic, so the average needs no collective
            self.opt.reset_ema()
        self._ms_cb = None
        if self.comm.world > 1 and overlap_comm:
            self._ms_cb = self._milestone
        # (Measured and dropped for one GPU: running the postponed slab reductions of the finished stages on an auxiliary stream at
        # the same milestones -- 20.29 -> 20.79 ms per step; the reduction competes with the backward kernels for HBM and queues.
        # Round 3, same experiment on the 17.2 ms step: 17.0-17.4 ms without, 17.5-17.8 ms with, four alternating runs each.)
        # >= 2 eager steps before capture: step 1 installs the gradient sinks, step 2 builds the descriptor tables that depend on
        # them (deferred reductions, padded-twin extraction) -- table uploads are host->device copies and cannot be captured
        self.use_graph, self.graph_warmup = use_graph, max(2, graph_warmup)
        # autograd binds each AccumulateGrad node to the stream that was current when it was created; warm-up and
        # capture therefore run on ONE dedicated side stream, otherwise backward would sync with the (non-capturing)
        # default stream in the middle of the capture
        self._stream = torch.cuda.Stream() if (use_graph and torch.cuda.is_available()) else None
        self._eager_steps = 0
        self._graph = None
        self._static = None
        self._static_out = None
        self._graph_has_opt = self._graph_has_comm = False

    def _milestone(self):
        """Backward has passed a stage boundary: everything registered so far belongs to layers whose backward is complete."""
        if not self.comm._armed:
            return
        # (also while a forward+backward-only graph is being captured: the partial reduction tables must be the ones the eager
        # warm-up steps built -- a new table cannot be uploaded during capture; only the collectives are held back)
        if not self._region:
            # eager branch streams: the hook fires on the stream of whichever boundary producer ran last, while the weight-gradient
            # kernels of the other branches were enqueued on side streams autograd does not order against this one.  (Region mode
            # joins every side stream at the end of each region's backward, so nothing is outstanding there.)
            from . import dispatch
            dispatch.join_side_streams(torch.cuda.current_stream())
        nnops.finalize_deferred()
        self.comm.flush_ready()

    # -- eager path --------------------------------------------------------------------------------------------
    def _fwd_bwd(self, batch):
        nnops.discard_deferred()       # reductions registered by a step that did not finish (exception) must not leak into this one
        self.opt.zero_grad()
        # the device input pipeline hands over the stem's own layout (bf16 NHWC, 8-channel pixels): no conversion launch
        x = batch["img_nhwc8"] if batch.get("img_nhwc8") is not None else batch["img"]
        out = self.model(x, batch["target"], batch["target_weight"], gt_keypoints=batch.get("keypoints"),
                         input_size=self.cfg.data.input_size)
        out["loss"].backward()
        nnops.finalize_deferred()      # ONE launch: all postponed slab reductions of parameter gradients (the rest of them after milestones)
        tw = getattr(self.model, "_pk_twin", None)
        if tw:
            tw.grads_to_real()         # padded twin: no-op when the end-of-backward callback already extracted the gradients
        return out

    def _eager_step(self, batch):
        if not self.model.training:
            self.model.train()
        self.comm.launched_early = 0
        out = self._fwd_bwd(batch)
        self.comm.finish()
        self.opt.step(self.comm.grad_scale)
        self.sched.step()
        return out

    # -- graph path --------------------------------------------------------------------------------------------
    def _comm_capturable(self):
        return (self.comm.world > 1 and dist.get_backend(self.comm.group) == "nccl" and os.environ.get("POSE_GRAPH_COMM", "0") == "1")

    def _capture(self, batch):
        keys = [k for k in ("img_nhwc8" if batch.get("img_nhwc8") is not None else "img", "target", "target_weight", "keypoints")
                if batch.get(k) is not None]
        self._static = {k: batch[k].clone() for k in keys}
        world = self.comm.world
        attempts = [True, False] if self._comm_capturable() else [world == 1]
        for whole_step in attempts:
            torch.cuda.synchronize()
            mode = "global"
            if world > 1:
                # The process group's watchdog thread polls the events of outstanding collectives (cudaEventQuery); under the
                # default global capture mode such a call from another thread invalidates the capture.  All collectives have
                # completed (synchronize above); give the watchdog one polling period to retire them, and only police the
                # capturing threads' own calls.
                import time
                time.sleep(0.5)
                mode = "thread_local"
            self.comm.suspended = world > 1 and not whole_step      # no collectives inside a forward+backward-only capture
            steps_before = self.opt.step_count
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g, stream=self._stream, capture_error_mode=mode):
                    out = self._fwd_bwd(self._static)
                    if whole_step:
                        self.comm.finish()
                        self.opt.step(self.comm.grad_scale)
            except Exception as e:      # noqa: BLE001  (a refused RCCL capture must not end the run: fall back to exchange between replays)
                if not (whole_step and world > 1):
                    raise
                import sys
                print(f"# engine: capturing the step with its RCCL all-reduces failed ({type(e).__name__}: {e}); capturing forward+backward only",
                      file=sys.stderr, flush=True)
                self.opt.step_count = steps_before
                self.comm._pending.clear()
                for bk in self.comm.buckets:
                    bk["got"] = 0
                nnops.discard_deferred()
                continue
            finally:
                self.comm.suspended = False
            if whole_step:
                self.opt.step_count -= 1          # the captured optimiser launch did not execute; _graph_step counts the replays
            self._graph, self._static_out = g, out
            self._graph_has_opt, self._graph_has_comm = whole_step, whole_step and world > 1
            break
        nnops.freeze_workspaces(self.model)   # the graph holds the slab-workspace pointers: they must not be reallocated

    def _graph_step(self, batch):
        for k, v in self._static.items():
            v.copy_(batch[k], non_blocking=True)
        self._graph.replay()
        if self._graph_has_opt:
            # the captured optimiser launches already advanced the device-side counter (guarded mode: unless they skipped the
            # update; step_count then counts attempted steps)
            self.opt.step_count += 1
            # ... and rewrote the fp32 masters behind torch's back: the bf16 compute copies (and a padded twin's embedded
            # parameters) are one step behind until the next forward repacks them
            wc = getattr(self.model, "_pk_weight_cache", None)
            if wc is not None:
                wc.mark_dirty()
            tw = getattr(self.model, "_pk_twin", None)
            if tw:
                tw.mark_dirty()
                twc = getattr(tw.twin, "_pk_weight_cache", None)
                if twc is not None:
                    twc.mark_dirty()
        else:
            self.comm.finish()
            self.opt.step(self.comm.grad_scale)
        self.sched.step()
        return self._static_out

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate under the averaged weights: waits for the step's stream, exchanges the contents of the masters and the average, and
        puts the model in eval mode; on exit (also by an exception) exchanges them back and restores the train/eval mode.  Usable between
        graph replays: the captured graph holds addresses, and only contents move."""
        if self._stream is not None:
            torch.cuda.current_stream().wait_stream(self._stream)
        was_training = self.model.training
        self.opt.swap_ema()
        self.model.eval()
        try:
            yield self.model
        finally:
            self.opt.swap_ema()
            self.model.train(was_training)

    def step(self, batch, snapshot=False):
        """`snapshot`: copy the masters first (FlatAdamW.snapshot_params, eager, between replays), so that tensor_stats("update")
        afterwards describes this step's update."""
        from . import dispatch
        if snapshot:
            self.opt.snapshot_params()
        dispatch.set_streams(self._want_streams)
        dispatch.set_region_mode(self._region)    # capturable fork/join (one autograd node per parallel region)
        nnops.set_milestone_callback(self._ms_cb)  # process-wide hook: the trainer that steps owns it
        if not self.use_graph:
            return self._eager_step(batch)
        if self._graph is None:
            if self._eager_steps < self.graph_warmup:
                self._eager_steps += 1
                self._stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self._stream):
                    out = self._eager_step(batch)
                torch.cuda.current_stream().wait_stream(self._stream)
                return out
            self.model.train()
            self._capture(batch)
            # the capture itself does not execute: run this step through the graph
        if any(k not in batch or batch[k] is None or batch[k].shape != v.shape for k, v in self._static.items()):
            # a batch the captured graph was not recorded for (e.g. the short last batch of an epoch): launch it eagerly on the
            # capture stream, with the same autograd structure and the same optimiser path as the replayed steps
            self._stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._stream):
                out = self._eager_step(batch)
            torch.cuda.current_stream().wait_stream(self._stream)
            return out
        return self._graph_step(batch)
