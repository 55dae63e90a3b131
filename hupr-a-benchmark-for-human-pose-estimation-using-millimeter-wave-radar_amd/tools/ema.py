"""Exponential moving average (EMA) of the weights, kept on the device beside the flat parameter buckets.

``TRAINING.emaDecay`` (absent from the reference's YAML; ``-1`` = off) makes ``TrainEngine`` keep ``ema += w (p - ema)`` behind every
optimiser step, ``w = 1 - min(decay, (1 + k) / (10 + k))`` after ``k`` earlier updates (the usual warm-up ramp, so the first updates
are not dominated by the initial weights).  The reference has nothing of the kind: it evaluates, selects and deploys ``self.model``
as trained (tools/run.py:35-63).

Everything a step needs is a launch on the step's stream (``hupr_ema_tick_f32`` + one ``hupr_ema_update_f32`` per bucket,
csrc/optim.hip): the update count and this step's weight live in device memory and the tick reads the gradient guard's decision, so
the average follows a step replayed from a hipGraph and stands still across a step the guard skipped.  ``swap()`` exchanges
parameters and average in place (``hupr_swap_f32``), which is how the engine evaluates with the averaged weights without a second
model.  Allocation, ``state_dict`` and ``load_state_dict`` are host-side bookkeeping on tensors of any device.
"""
import torch

from .. import runtime as rt


def ema_decay_setting(cfg):
    """``TRAINING.emaDecay`` -> None (absent or -1: off, the YAML's own "-1 = off" idiom) or the decay as a float strictly inside
    (0, 1).  Anything else (0, 1, a number outside, NaN, not a number) is refused."""
    v = getattr(cfg.TRAINING, "emaDecay", -1)
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        if v == -1:
            return None
        if 0 < v < 1:                        # False for NaN
            return float(v)
    raise ValueError("TRAINING.emaDecay must be -1 (off) or a decay strictly inside (0, 1), e.g. 0.999; got %r" % (v,))


class WeightEMA:
    """One flat fp32 average per parameter bucket, initialised as a copy of the bucket's parameters, and the 2-float device state
    {updates, weight}.  ``flat_pairs`` / ``layout``: ``GradientBuckets.flat_pairs()`` / ``.layout()``.  ``module``: the network the
    buckets were made from; it gives the parameters their ``state_dict`` names (``state_dict(model)`` does so as well), which
    ``load_state_dict`` needs.  The update count is kept as an fp32 number: exact up to 2^24 updates."""

    def __init__(self, flat_pairs, layout, decay, module=None):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError("WeightEMA: decay must be strictly inside (0, 1), got %r" % (decay,))
        if layout is None or len(layout) != len(flat_pairs):
            raise ValueError("WeightEMA needs the bucket layout (GradientBuckets.layout()): one entry list per flat bucket")
        self.decay = decay
        self._params = [p for p, _ in flat_pairs]
        self._layout = layout
        self.flat = [p.detach().clone() for p in self._params]
        self._state = torch.zeros(2, dtype=torch.float32, device=self._params[0].device)
        self.swapped = False
        self._slot = {id(p): (i, off, n) for i, entries in enumerate(layout) for p, off, n in entries}
        self._names = None
        if module is not None:
            self._learn_names(module)

    def _learn_names(self, module):
        names = {}
        for name, p in module.named_parameters(remove_duplicate=False):
            if id(p) not in self._slot:
                raise RuntimeError("WeightEMA: parameter %s is in no flat bucket (the layout must cover every parameter; a frozen "
                                   "parameter has no slot)" % name)
            names[name] = self._slot[id(p)]
        self._names = names

    # -- the step's launches (GPU only) ------------------------------------------------------------------------------
    def update(self, guard=None):
        """One tick + one update launch per bucket on the current stream.  ``guard``: the optimiser's 4-float gradient guard or
        None; a step the guard skipped leaves the average's bits and the update count alone."""
        if self.swapped:
            raise RuntimeError("WeightEMA.update while the averaged weights are swapped in")
        L, s = rt.lib(), rt.stream()
        state = rt.ptr(self._state)
        rt.check(L.hupr_ema_tick_f32(state, self.decay, rt.ptr(guard), s))
        for e, p in zip(self.flat, self._params):
            rt.check(L.hupr_ema_update_f32(rt.ptr(e), rt.ptr(p), p.numel(), state, s))

    def swap(self):
        """Exchange parameters and average in place, one launch per bucket; ``.swapped`` tells which way round they are.  The
        caller owns what follows from changed parameters (``functional.invalidate_packed``)."""
        L, s = rt.lib(), rt.stream()
        for e, p in zip(self.flat, self._params):
            rt.check(L.hupr_swap_f32(rt.ptr(e), rt.ptr(p), p.numel(), s))
        self.swapped = not self.swapped

    def stats(self):
        """{"updates": updates so far, "weight": the last step's weight (0.0 for a skipped step)}.  Reads device memory, so it
        synchronises: per epoch, not per step."""
        updates, weight = self._state.tolist()
        return {"updates": int(updates), "weight": weight}

    # -- host bookkeeping (any device, no launch) --------------------------------------------------------------------
    def reset(self):
        """Start over from the current parameters at ``updates = 0``."""
        if self.swapped:
            raise RuntimeError("WeightEMA.reset while the averaged weights are swapped in")
        for e, p in zip(self.flat, self._params):
            e.copy_(p.detach())
        self._state.zero_()

    def state_dict(self, model):
        """A complete state dict of ``model`` — its keys, order, shapes and dtypes, so it loads with ``strict=True`` wherever
        ``model.state_dict()`` does — with every parameter taken from the average and every buffer a clone of the model's
        current buffer.  Buffers are not averaged: the BatchNorm running statistics already are moving averages (of the
        activations the live weights produced), and ``num_batches_tracked`` is a count."""
        if self.swapped:
            raise RuntimeError("WeightEMA.state_dict while the averaged weights are swapped in (the flat averages hold the live "
                               "parameters)")
        self._learn_names(model)
        sd = model.state_dict()
        out = type(sd)()
        for key, t in sd.items():
            slot = self._names.get(key)
            if slot is None:
                out[key] = t.detach().clone()
            else:
                i, off, n = slot
                out[key] = self.flat[i][off:off + n].clone().view(t.shape).to(t.dtype)
        if hasattr(sd, "_metadata"):
            out._metadata = sd._metadata
        return out

    def load_state_dict(self, sd, updates):
        """Restore the averaged parameters from a ``state_dict(model)`` and the update count, so the ramp resumes where it was
        (buffers in ``sd`` are the model's business)."""
        if self.swapped:
            raise RuntimeError("WeightEMA.load_state_dict while the averaged weights are swapped in")
        if self._names is None:
            raise RuntimeError("WeightEMA.load_state_dict needs the parameter names: construct with module= (or call state_dict(model))")
        missing = [k for k in self._names if k not in sd]
        if missing:
            raise KeyError("WeightEMA.load_state_dict: missing parameter(s) %s" % ", ".join(missing[:5]))
        updates = int(updates)
        if updates < 0:
            raise ValueError("WeightEMA.load_state_dict: updates must be >= 0, got %r" % (updates,))
        for key, (i, off, n) in self._names.items():
            self.flat[i][off:off + n].copy_(sd[key].detach().reshape(-1))
        self._state.copy_(torch.tensor([float(updates), 0.0], dtype=torch.float32))
