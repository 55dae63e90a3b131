"""Adam and SGD with momentum, both with coupled L2 weight decay, and LAMB, on the gfx950 fused kernels.

The reference builds one of the two from ``TRAINING.optimizer`` (tools/base.py:44-47): ``optim.SGD(lr, momentum=0.9,
weight_decay=1e-4)`` or ``optim.Adam(lr, betas=(0.9, 0.999), weight_decay=1e-4)`` on every parameter (``make_optimizer``).
Each fused optimiser has the update rule and the ``state_dict`` layout of its torch counterpart, so the reference's
``optimizer_state_dict`` checkpoints interchange.  One kernel launch per parameter tensor, or one per flat bucket when the
parameters were flattened by ``tools.distributed``.

``TRAINING.gradClip`` (absent from the reference's YAML; ``-1`` = off) puts the gradient guard in front of the flat-bucket step:
global-norm clipping (``torch.nn.utils.clip_grad_norm_``'s rule) and the skip of a step whose gradients are not finite, both
decided on the device (``enable_grad_guard``).

``TRAINING.optimizer: lamb`` (new, no reference counterpart) is the large-batch optimiser: Adam's direction rescaled per parameter
tensor by the trust ratio (``FusedLAMB``), with ``TRAINING.lambWeightDecay`` (absent = 0.01) as its decoupled decay.
"""
import torch

from .. import runtime as rt


class _FlatBucketOptimizer(torch.optim.Optimizer):
    """Flat-bucket bookkeeping shared by the fused optimisers: per bucket one flat tensor per state key (``_state_keys``) plus a
    host step count, optionally the {lr, step} pair in device memory for graph-captured steps, and the scatter / gather of the
    flat state through the bucket layout into torch's per-parameter ``state_dict`` layout."""
    _state_keys = ()

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self.grad_scale = 1.0            # e.g. 1/world_size when gradients were sum-all-reduced
        self._flat = None                # optional [(param_flat, grad_flat)] installed by tools.distributed
        self._guard = None               # {coef, norm, skipped, finite} on the device: set by enable_grad_guard()
        self.grad_clip = None            # TRAINING.gradClip as make_optimizer read it (None = off)

    def attach_flat_buckets(self, buckets, layout=None):
        """buckets: list of (flat_param, flat_grad) fp32 GPU tensors covering all parameters in order.
        layout: per bucket, the list of (parameter, offset, numel) it holds — needed to save / restore the state in torch's
        per-parameter ``state_dict`` layout (``GradientBuckets.layout()``)."""
        self._flat = buckets
        self._layout = layout
        # per bucket: {step, <state key>: flat tensor}; step = steps taken (FusedAdam), see _host_step for FusedSGD
        self._flat_state = [dict(step=0, **{k: torch.zeros_like(p) for k in self._state_keys}) for p, _ in buckets]
        self._dev_state = None           # {lr, step} on the device: set by use_device_state() for graph-captured steps

    def use_device_state(self):
        """Keep the learning rate and the step count in device memory (needed when step() is captured in a hipGraph:
        launch arguments are frozen at capture, the step count and LR schedule must keep moving)."""
        if self._dev_state is not None:      # already there (enable_grad_guard): the device copy is the truth
            self.sync_lr()
            return
        dev = self._flat[0][0].device
        self._dev_state = torch.tensor([self.param_groups[0]["lr"], float(self._flat_state[0]["step"])], dtype=torch.float32,
                                       device=dev)
        self._dev_lr = self.param_groups[0]["lr"]

    # -- gradient guard: global-norm clipping and the skip of a non-finite step, on the device -----------------------
    def enable_grad_guard(self, max_norm):
        """From now on ``step()`` takes the L2 norm of all flat gradients times ``grad_scale`` (one ``hupr_grad_sumsq_f32`` per
        bucket + one ``hupr_grad_guard_f32``), scales the gradients by ``min(1, max_norm / (norm + 1e-6))`` inside the update
        and leaves parameters, state and step count untouched when the norm is not finite.  ``max_norm = inf``: guard only.
        Everything is device-side ({lr, step} move to device memory, the guard kernel owns the step increment), so a step
        captured in a hipGraph is guarded too."""
        if self._flat is None:
            raise RuntimeError("enable_grad_guard needs flat gradient buckets (attach_flat_buckets first): the global norm is "
                               "taken over the buckets")
        max_norm = float(max_norm)
        if not max_norm > 0.0:
            raise ValueError("enable_grad_guard: max_norm must be positive (inf = guard only), got %r" % (max_norm,))
        self.use_device_state()
        dev = self._flat[0][0].device
        if self._guard is None:
            self._guard_k = rt.lib().hupr_grad_sumsq_partials()
            self._guard_partials = torch.zeros(len(self._flat) * self._guard_k, dtype=torch.float64, device=dev)
            self._guard = torch.zeros(4, dtype=torch.float32, device=dev)
        self._guard_max_norm = max_norm

    def _guard_launches(self, L, s):
        """The launches of a guarded step in front of the per-bucket updates; afterwards ``_guard`` holds this step's decision and
        ``_dev_state[1]`` this step's count (unchanged when the step is skipped)."""
        if not torch.cuda.is_current_stream_capturing():
            self.sync_lr()                   # a changed param_groups lr (Runner.adjustLR); a captured step reads it on replay
        k = self._guard_k
        for i, (_, g) in enumerate(self._flat):
            rt.check(L.hupr_grad_sumsq_f32(rt.ptr(g), g.numel(), rt.ptr(self._guard_partials) + 8 * k * i, s))
        rt.check(L.hupr_grad_guard_f32(rt.ptr(self._guard_partials), self._guard_partials.numel(), self.grad_scale,
                                       self._guard_max_norm, rt.ptr(self._dev_state), rt.ptr(self._guard), s))

    def guard_stats(self):
        """The last step's {"norm", "coef"} and the number of steps skipped so far (not checkpointed); None without the guard.
        Reads device memory, so it synchronises: per epoch, not per step."""
        if self._guard is None:
            return None
        coef, norm, skipped, _ = self._guard.tolist()
        return {"norm": norm, "coef": coef, "skipped": int(skipped)}

    # -- checkpoint interchange with torch.optim (reference tools/base.py:76-81,113) -----------------------------
    def _host_step(self, i):
        """Bucket i's step count.  0 means no state yet (nothing saved).  FusedAdam's is the true count, restored from the
        checkpoint's ``step``.  torch.optim.SGD saves no count, so FusedSGD restarts at 1 after ``load_state_dict`` and its count
        only tells whether the next step is the first: not a number of steps taken (for an LR schedule or a log)."""
        if self._dev_state is not None:          # during graph replay only the device copy advances
            self._flat_state[i]["step"] = int(round(float(self._dev_state[1].item())))
        return self._flat_state[i]["step"]

    def _param_entry(self, step, slices):
        """torch's per-parameter state entry from the bucket's step count and the parameter's slices of the flat state."""
        return slices

    def _entry_step(self, entry):
        """The step count a loaded per-parameter entry implies."""
        raise NotImplementedError

    def state_dict(self):
        """torch's per-parameter layout: the flat state buffers are scattered into per-parameter tensors (copies), so a
        checkpoint written here resumes under the torch optimiser and vice versa."""
        if self._flat is None:
            return super().state_dict()
        if self._layout is None:
            raise RuntimeError("flat buckets attached without a layout: the optimiser state cannot be serialised")
        saved = self.state
        self.state = type(saved)()
        try:
            for i, entries in enumerate(self._layout):
                step = self._host_step(i)
                if step == 0:
                    continue                      # torch's optimisers have no state before their first step either
                st = self._flat_state[i]
                for p, off, n in entries:
                    self.state[p] = self._param_entry(step, {k: st[k][off:off + n].clone().view_as(p) for k in self._state_keys})
            return super().state_dict()
        finally:
            self.state = saved

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)      # fills self.state per parameter (cast to the parameter's device)
        if self._flat is None:
            return
        if self._layout is None:
            raise RuntimeError("flat buckets attached without a layout: the optimiser state cannot be restored")
        for i, entries in enumerate(self._layout):
            st = self._flat_state[i]
            step = 0
            for k in self._state_keys:
                st[k].zero_()
            for p, off, n in entries:
                ps = self.state.get(p)
                if not ps:
                    continue
                for k in self._state_keys:
                    st[k][off:off + n].copy_(ps[k].reshape(-1))
                step = max(step, self._entry_step(ps))
            st["step"] = step
        self.state.clear()                       # the flat buffers are the state from here on
        if self._dev_state is not None:
            self._dev_lr = self.param_groups[0]["lr"]
            self._dev_state.copy_(torch.tensor([self._dev_lr, float(self._flat_state[0]["step"])], dtype=torch.float32))

    def sync_lr(self):
        """Push a changed param_groups lr to the device state (call outside graph replay, e.g. once per epoch)."""
        if self._dev_state is not None and self.param_groups[0]["lr"] != self._dev_lr:
            self._dev_lr = self.param_groups[0]["lr"]
            self._dev_state[0] = self._dev_lr

    # -- the step: one launch per flat bucket, or one per parameter tensor without buckets ------------------------------
    def _launch_bucket(self, L, s, form, p, g, st, group):
        """One bucket's update.  form: "host" (lr and ``st["step"]`` as launch arguments), "dev" ({lr, step} read from
        ``_dev_state``) or "guard" ("dev" obeying ``_guard``)."""
        raise NotImplementedError

    def _launch_param(self, L, s, p, g, st, group):
        """One parameter tensor's update with torch's per-parameter state ``st`` (created here on the first step)."""
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = rt.lib()
        s = rt.stream()
        from .. import functional as F_
        F_.invalidate_packed()             # parameters change below without bumping torch's version counters
        if self._flat is None:
            for group in self.param_groups:
                for p in group["params"]:
                    if p.grad is not None:
                        self._launch_param(L, s, p, p.grad if p.grad.is_contiguous() else p.grad.contiguous(), self.state[p], group)
            return loss
        form = "guard" if self._guard is not None else "dev" if self._dev_state is not None else "host"
        if form == "guard":
            self._guard_launches(L, s)       # advances the device-side step count unless the step is skipped
        elif form == "dev":
            self._dev_state[1] += 1          # device-side step count (captured as a graph node); SGD: step 1 is the first
        for (p, g), st in zip(self._flat, self._flat_state):
            if form != "guard":
                st["step"] += 1              # host mirror (checkpoints); during replay only the device copy advances
            self._launch_bucket(L, s, form, p, g, st, self.param_groups[0])
        return loss


class FusedAdam(_FlatBucketOptimizer):
    _state_keys = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None)
        super().__init__(params, defaults)

    def _param_entry(self, step, slices):
        return {"step": torch.tensor(float(step)), **slices}      # torch.optim.Adam: {step, exp_avg, exp_avg_sq}

    def _entry_step(self, entry):
        return int(round(float(entry["step"])))

    def _launch_bucket(self, L, s, form, p, g, st, group):
        b1, b2 = group["betas"]
        arrays = (rt.ptr(p), rt.ptr(g), rt.ptr(st["exp_avg"]), rt.ptr(st["exp_avg_sq"]), p.numel())
        hyper = (b1, b2, group["eps"], group["weight_decay"])
        if form == "guard":
            rt.check(L.hupr_adam_step_guard_f32(*arrays, rt.ptr(self._dev_state), rt.ptr(self._guard), *hyper, self.grad_scale, s))
        elif form == "dev":
            rt.check(L.hupr_adam_step_dev_f32(*arrays, rt.ptr(self._dev_state), *hyper, self.grad_scale, s))
        else:
            rt.check(L.hupr_adam_step_f32(*arrays, group["lr"], *hyper, int(st["step"]), self.grad_scale, s))

    def _launch_param(self, L, s, p, g, st, group):
        if len(st) == 0:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["step"] += 1
        self._launch_bucket(L, s, "host", p, g, st, group)


class FusedSGD(_FlatBucketOptimizer):
    """``torch.optim.SGD`` with momentum and coupled L2 weight decay, dampening 0, no Nesterov, not maximising — the
    reference's ``optim.SGD(lr, momentum=0.9, weight_decay=1e-4)``.  State: one momentum buffer per parameter (flat per
    bucket), ``{"momentum_buffer": tensor}`` per parameter in ``state_dict()``, nothing before the first step."""
    _state_keys = ("momentum_buffer",)
    # param_groups keys later torch versions added; the reference pins torch 1.4 (environment.yml), whose SGD saves only lr,
    # momentum, dampening, weight_decay and nesterov: filled in on load as torch.optim.SGD.__setstate__ does
    _LATER_GROUP_KEYS = dict(nesterov=False, maximize=False, foreach=None, differentiable=False, fused=None)

    def __init__(self, params, lr=1e-3, momentum=0.9, dampening=0, weight_decay=0.0, nesterov=False, maximize=False):
        if lr < 0.0 or weight_decay < 0.0:
            raise ValueError("FusedSGD: invalid lr %r or weight_decay %r" % (lr, weight_decay))
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults)           # every group passes _check_group (add_param_group)

    @staticmethod
    def _check_group(group):
        if not (group["momentum"] > 0 and group["dampening"] == 0 and not group["nesterov"] and not group["maximize"]):
            raise ValueError("FusedSGD supports momentum > 0, dampening=0, nesterov=False, maximize=False (the reference's "
                             "SGD(momentum=0.9, weight_decay=1e-4)); got momentum=%r, dampening=%r, nesterov=%r, maximize=%r"
                             % (group["momentum"], group["dampening"], group["nesterov"], group["maximize"]))

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])

    def _entry_step(self, entry):
        return 1              # torch.optim.SGD keeps no step count: a saved buffer only means "not the first step" (_host_step)

    def load_state_dict(self, state_dict):
        for entry in state_dict["state"].values():
            if entry and entry.get("momentum_buffer") is None:
                keys = sorted(entry)
                writer = ("Adam (torch.optim.Adam or FusedAdam)" if "exp_avg" in entry else
                          "SGD without momentum" if "momentum_buffer" in entry else "an optimiser with state keys %s" % keys)
                raise ValueError("FusedSGD cannot load this optimizer state: it was written by %s (entries hold %s, not "
                                 "'momentum_buffer'); TRAINING.optimizer must match the checkpoint's optimiser" % (writer, keys))
        groups = [{**self._LATER_GROUP_KEYS, **group} for group in state_dict["param_groups"]]     # the caller's dict is kept
        for group in groups:
            self._check_group(group)
        super().load_state_dict({**state_dict, "param_groups": groups})

    def _launch_bucket(self, L, s, form, p, g, st, group, first=None):
        arrays = (rt.ptr(p), rt.ptr(g), rt.ptr(st["momentum_buffer"]), p.numel())
        hyper = (group["momentum"], group["weight_decay"])
        if form == "guard":
            rt.check(L.hupr_sgd_step_guard_f32(*arrays, rt.ptr(self._dev_state), rt.ptr(self._guard), *hyper, self.grad_scale, s))
        elif form == "dev":
            rt.check(L.hupr_sgd_step_dev_f32(*arrays, rt.ptr(self._dev_state), *hyper, self.grad_scale, s))
        else:
            first = st["step"] == 1 if first is None else first
            rt.check(L.hupr_sgd_step_f32(*arrays, group["lr"], *hyper, int(first), self.grad_scale, s))

    def _launch_param(self, L, s, p, g, st, group):
        first = "momentum_buffer" not in st
        if first:
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        self._launch_bucket(L, s, "host", p, g, st, group, first)


def lamb_chunk_table(segments, chunk):
    """The chunk table of one flat bucket for the LAMB kernels (``include/hupr.h`` (a13)), as a flat list of ints.
    ``segments``: [(start, length, adapted)] tiling the bucket in order; ``chunk``: elements per chunk (``hupr_lamb_chunk()``).
    Layout: ``[S, K, chunk, n]``, then per segment ``start, length, first chunk, chunk count, adapted``, then per chunk ``segment,
    start relative to the segment``.  Every segment is cut from its own start, so no chunk spans two segments, the chunks of a
    segment are consecutive, and moving a segment inside its bucket changes nothing but its ``start``."""
    chunk = int(chunk)
    if chunk <= 0:
        raise ValueError("lamb_chunk_table: chunk must be positive, got %r" % (chunk,))
    segs, chunks, at = [], [], 0
    for s, (start, length, adapted) in enumerate(segments):
        start, length = int(start), int(length)
        if start != at or length <= 0:
            raise ValueError("lamb_chunk_table: segment %d = (start %d, length %d) does not continue the bucket at %d"
                             % (s, start, length, at))
        count = -(-length // chunk)
        segs += [start, length, len(chunks) // 2, count, 1 if adapted else 0]
        for k in range(count):
            chunks += [s, k * chunk]
        at += length
    if not segs:
        raise ValueError("lamb_chunk_table: no segment")
    return [len(segs) // 5, len(chunks) // 2, chunk, at] + segs + chunks


class FusedLAMB(_FlatBucketOptimizer):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning", 2020) with the update rule of apex's ``FusedLAMB``, over the
    flat buckets only.  Per parameter tensor, ``k`` the 1-based step count and ``g' = g * grad_scale * coef`` (``coef``: the
    gradient guard's clipping coefficient, 1 without the guard)::

        m <- b1 m + (1 - b1) g'          v <- b2 v + (1 - b2) g'^2
        d = (m / (1 - b1^k)) / (sqrt(v) / sqrt(1 - b2^k) + eps)
        p.ndim > 1 :   u = d + wd p ;   r = |p| / |u| if both norms > 0 else 1
        p.ndim <= 1:   u = d ;          r = 1           (biases, BatchNorm, PReLU: no decay, no adaptation)
        p <- p - lr r u

    No clamp on ``r`` and no function other than the identity on ``|p|``; ``|p|`` is taken before the update.  An adapted tensor
    whose gradient is zero at step 1 has ``u = wd p`` and therefore ``r = 1 / wd``: it shrinks by the factor ``1 - lr`` on that
    step.  That is the rule, not a special case.  Three launches per bucket (``csrc/optim.hip``): the new moments and the
    squares per chunk, the norms and ratios per tensor, the update.  ``{lr, step}`` live in device memory from
    ``attach_flat_buckets`` on, so an eager step and a step replayed from a hipGraph are the same launches and the same bits.
    State per parameter in ``state_dict()``: Adam's ``{step, exp_avg, exp_avg_sq}``; ``param_groups[0]`` carries the marker
    ``trust_ratio: True``, by which ``load_state_dict`` tells a LAMB checkpoint from an Adam one."""
    _state_keys = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01):
        if lr < 0.0 or not weight_decay >= 0.0 or weight_decay == float("inf"):
            raise ValueError("FusedLAMB: invalid lr %r or weight_decay %r" % (lr, weight_decay))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, trust_ratio=True))

    def attach_flat_buckets(self, buckets, layout=None):
        if layout is None:
            raise RuntimeError("FusedLAMB needs the bucket layout (GradientBuckets.layout()): its trust ratios are per parameter "
                               "tensor")
        super().attach_flat_buckets(buckets, layout)
        chunk = rt.lib().hupr_lamb_chunk()
        for (p, _), entries, st in zip(buckets, layout, self._flat_state):
            table = torch.tensor(lamb_chunk_table([(off, n, q.ndim > 1) for q, off, n in entries], chunk), dtype=torch.int64)
            rt.check(rt.lib().hupr_lamb_table_check(table.data_ptr(), table.numel(), p.numel()))
            nseg, nchunk = int(table[0]), int(table[1])
            # beside the bucket's state, not a state key: the table in host and device memory, the fp64 pair per chunk and |p|, |u|, r
            # per parameter tensor
            st["lamb"] = dict(host=table, dev=table.to(p.device), words=table.numel(), segments=nseg,
                              partials=torch.zeros(2 * nchunk, dtype=torch.float64, device=p.device),
                              stats=torch.zeros(3 * nseg, dtype=torch.float32, device=p.device))
        self.use_device_state()      # always: the kernels have no form with host arguments

    def _param_entry(self, step, slices):
        return {"step": torch.tensor(float(step)), **slices}      # Adam's entry: {step, exp_avg, exp_avg_sq}

    def _entry_step(self, entry):
        return int(round(float(entry["step"])))

    def load_state_dict(self, state_dict):
        for entry in state_dict["state"].values():
            if entry and "momentum_buffer" in entry:
                raise ValueError("FusedLAMB cannot load this optimizer state: it was written by SGD (torch.optim.SGD or FusedSGD; "
                                 "entries hold %s); TRAINING.optimizer must match the checkpoint's optimiser" % sorted(entry))
            if entry and not all(k in entry for k in ("step",) + self._state_keys):
                raise ValueError("FusedLAMB cannot load this optimizer state: entries hold %s, not 'step', 'exp_avg', 'exp_avg_sq'"
                                 % sorted(entry))
        for group in state_dict["param_groups"]:
            if group.get("trust_ratio") is not True:
                raise ValueError("FusedLAMB cannot load this optimizer state: it was written by Adam (torch.optim.Adam or "
                                 "FusedAdam; its param_groups lack 'trust_ratio').  The state keys are the same, but Adam's eps "
                                 "and coupled weight_decay would replace LAMB's; TRAINING.optimizer must match the checkpoint's "
                                 "optimiser")
        super().load_state_dict(state_dict)

    def _launch_bucket(self, L, s, form, p, g, st, group):
        t = st["lamb"]
        b1, b2 = group["betas"]
        n = p.numel()
        table = (t["host"].data_ptr(), t["words"], rt.ptr(t["dev"]))
        state, guard = rt.ptr(self._dev_state), rt.ptr(self._guard) if form == "guard" else None
        hyper = (b1, b2, group["eps"], group["weight_decay"])
        m, v, partials, stats = rt.ptr(st["exp_avg"]), rt.ptr(st["exp_avg_sq"]), rt.ptr(t["partials"]), rt.ptr(t["stats"])
        rt.check(L.hupr_lamb_stage1_f32(rt.ptr(p), rt.ptr(g), m, v, n, *table, state, guard, *hyper, self.grad_scale, partials, s))
        rt.check(L.hupr_lamb_ratio_f32(partials, n, *table, guard, stats, s))
        rt.check(L.hupr_lamb_stage2_f32(rt.ptr(p), m, v, n, *table, state, guard, *hyper, stats, s))

    @torch.no_grad()
    def step(self, closure=None):
        if self._flat is None:
            raise RuntimeError("FusedLAMB.step needs flat gradient buckets (attach_flat_buckets first): its trust ratios are taken "
                               "per parameter tensor over the buckets")
        if not torch.cuda.is_current_stream_capturing():
            self.sync_lr()                   # a changed param_groups lr (Runner.adjustLR); a captured step reads it on replay
        return super().step(closure)

    def lamb_stats(self):
        """Per bucket ``(|p|, |u|, r)``, one float tensor each with one value per parameter tensor in ``layout()`` order, as the
        last step that was not skipped left them (zeros before the first).  Reads device memory, so it synchronises."""
        if self._flat is None:
            return None
        return [tuple(st["lamb"]["stats"].view(3, st["lamb"]["segments"]).cpu()) for st in self._flat_state]


def lamb_weight_decay_setting(cfg):
    """``TRAINING.lambWeightDecay`` -> None (absent) or the decay as a float (a finite number >= 0).  Anything else is refused."""
    if not hasattr(cfg.TRAINING, "lambWeightDecay"):
        return None
    v = cfg.TRAINING.lambWeightDecay
    if isinstance(v, (int, float)) and not isinstance(v, bool) and 0 <= v < float("inf"):      # False for NaN
        return float(v)
    raise ValueError("TRAINING.lambWeightDecay must be a finite number >= 0 (absent = 0.01), got %r" % (v,))


def grad_clip_setting(cfg):
    """``TRAINING.gradClip`` -> None (absent or -1: off, the YAML's own "-1 = off" idiom) or the max norm as a float (``.inf``:
    guard only, no clipping).  Anything else (0, another negative number, NaN, not a number) is refused."""
    v = getattr(cfg.TRAINING, "gradClip", -1)
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        if v == -1:
            return None
        if v > 0:                            # False for NaN
            return float(v)
    raise ValueError("TRAINING.gradClip must be -1 (off), a positive max norm, or .inf (guard only, no clipping); got %r" % (v,))


def make_optimizer(cfg, params, lr):
    """The optimiser ``TRAINING.optimizer`` selects: ``sgd`` and ``adam`` built as the reference builds them (tools/base.py:44-47),
    ``lamb`` with ``TRAINING.lambWeightDecay`` (absent = 0.01; set together with another optimiser it is an error).  The reference
    leaves ``self.optimizer`` unset for any other name and fails later; this raises here.  ``TRAINING.gradClip`` is read into
    ``optimizer.grad_clip``; the caller enables the guard once the flat buckets are attached (``TrainEngine``)."""
    name = cfg.TRAINING.optimizer
    clip = grad_clip_setting(cfg)
    wd = lamb_weight_decay_setting(cfg)
    if wd is not None and name in ("adam", "sgd"):
        raise ValueError("TRAINING.lambWeightDecay is set but TRAINING.optimizer is %r: the key belongs to 'lamb' (%r decays by "
                         "1e-4, coupled, as the reference does)" % (name, name))
    if name == "lamb":
        opt = FusedLAMB(params, lr=lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01 if wd is None else wd)
    elif name == "adam":
        opt = FusedAdam(params, lr=lr, betas=(0.9, 0.999), weight_decay=1e-4)
    elif name == "sgd":
        opt = FusedSGD(params, lr=lr, momentum=0.9, weight_decay=1e-4)
    else:
        raise ValueError("TRAINING.optimizer must be 'sgd' or 'adam' (tools/base.py:44-47) or 'lamb' (large batches), got %r"
                         % (name,))
    opt.grad_clip = clip
    return opt
