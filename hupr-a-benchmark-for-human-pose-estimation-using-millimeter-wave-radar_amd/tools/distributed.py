"""Data-parallel training over one node: one process per GPU, gradient sum-all-reduce over
RCCL/xGMI on a side HIP stream, overlapped with backward.

The reference has no distributed layer at all (single device string, tools/base.py:14); this is
the new part BASELINE.json asks for.  Design:

  * parameters and gradients live in a few flat fp32 buckets (reverse registration order ==
    roughly the order backward produces gradients: GCN -> decoder -> encoders -> MNets), so one
    collective moves tens of MB instead of 165 small tensors;
  * ``p.grad`` is a *view* into its bucket; the operator kernels write weight/bias gradients straight
    into those views (``functional.GRAD_SINK``: no per-parameter AccumulateGrad add kernels), anything
    autograd still accumulates itself lands in place; either way an arrival counter launches the
    bucket's all-reduce on the communication stream the moment its last gradient lands;
  * ``finish()`` makes the compute stream wait for the collectives; the optimiser then runs one
    fused Adam launch per bucket with grad_scale = 1/world_size (sum -> mean);
  * BatchNorm statistics stay per rank (the reference is single-device, no SyncBN).

Transport.  On GPUs the exchange goes through the C ABI (``hupr_allreduce_bucket`` /
``hupr_broadcast_bucket`` in include/hupr.h: ncclAllReduce on the library's own RCCL communicator, one per
process): the host enqueues it on the communication stream like any other kernel, and — unlike a
``torch.distributed`` work object — it can be captured into the hipGraph of the whole training step.
``torch.distributed`` stays the control plane (rendezvous, exchange of the communicator id, barriers) and
is the transport for CPU tensors (``gloo``: how the ``not gpu`` tests exercise world_size 2).  If the native
communicator cannot be created the launcher says so on stderr and falls back to ``dist.all_reduce`` on the
``nccl`` (= RCCL) process group; ``HUPR_COLLECTIVE=torch`` selects that transport explicitly.

Gradient accumulation (``stash()``): with a fixed global batch a rank may run several micro-batches per
optimiser step (``bench.py --strong``); the buckets of the first m-1 micro-batches are summed into an
accumulator, which is added to the bucket on the communication stream right before the last micro-batch's
all-reduce — one exchange per optimiser step, still overlapped with the last backward.
"""
import ctypes
import os
import sys

import torch
import torch.distributed as dist


class TorchTransport:
    """``torch.distributed`` collectives (gloo on CPU tensors; nccl/RCCL process group as the GPU fallback)."""
    name = "torch.distributed"
    capturable = False

    def __init__(self, group=None):
        self.group = group

    def all_reduce(self, flat, stream=None):
        return dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    def broadcast(self, flat, src):
        dist.broadcast(flat, src=src, group=self.group)


_ID_ERROR = b"HUPR_RCCL_ID_ERROR"          # sentinel rank 0 publishes instead of the id when it could not create one


def _all_ok(ok, group, device):
    """Group decision: True only if EVERY rank reports success (MIN all-reduce over the control plane; a CPU tensor rides
    gloo, and a group without a CPU backend gets a device tensor)."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return bool(ok)
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
    try:
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
    except (RuntimeError, ValueError):
        flag = flag.to(device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
    return bool(int(flag.item()))


class RcclTransport:
    """The C ABI's own RCCL communicator (``hupr_comm_*`` / ``hupr_allreduce_bucket``), bound to the current device.
    The 128-byte communicator id is created on rank 0 and handed to the other ranks through the existing
    ``torch.distributed`` group (any backend); a single-rank communicator needs no process group at all.

    Construction is a group decision in three agreed phases, so that a failure on SOME ranks can neither leave the others
    blocked nor split the job over two transports: (1) every rank binds librccl — agreed; (2) rank 0 creates the id and
    publishes it, or an error sentinel the waiting ranks fail fast on; (3) ncclCommInitRank (collective inside RCCL) —
    agreed; a rank whose peers failed destroys its communicator again.  Any disagreement raises on every rank."""
    name = "rccl (hupr_allreduce_bucket)"
    capturable = True

    def __init__(self, device, group=None):
        from .. import runtime as rt
        self.rt, self.L = rt, rt.lib()
        self.device = device
        self.comm = None
        multi = dist.is_initialized() and dist.get_world_size(group) > 1
        self.rank = dist.get_rank(group) if multi else 0
        self.world = dist.get_world_size(group) if multi else 1
        loaded = self.L.hupr_comm_load(None) == 0
        if not _all_ok(loaded, group, device):
            raise rt.HuprError("librccl could not be bound on every rank (this rank: %s)" % ("ok" if loaded else rt.last_error()))
        uid = ctypes.create_string_buffer(128)
        got = None
        if self.rank == 0:
            got = uid.raw if self.L.hupr_comm_unique_id(uid) == 0 else _ID_ERROR
            err = rt.last_error() if got == _ID_ERROR else ""
        if multi:
            got = self._exchange_id(got, group, device)
        if got == _ID_ERROR:
            raise rt.HuprError("rank 0 could not create an RCCL communicator id" + (": " + err if self.rank == 0 else ""))
        uid = ctypes.create_string_buffer(got, 128)
        comm = ctypes.c_void_p()
        with torch.cuda.device(device):
            ok = self.L.hupr_comm_init_rank(ctypes.byref(comm), uid, self.world, self.rank) == 0
        err = "" if ok else rt.last_error()
        if ok:
            self.comm = comm
        if not _all_ok(ok, group, device):
            self.close()
            raise rt.HuprError("ncclCommInitRank did not succeed on every rank (this rank: %s)" % (err or "ok"))

    _n_comms = 0

    @classmethod
    def _exchange_id(cls, uid_bytes, group, device):
        """Rank 0's 128-byte communicator id (or the error sentinel) to every rank.  Default group: through the rendezvous
        key-value store (no device traffic for the id itself); sub-groups, or a store that cannot be reached ON ANY RANK
        (agreed, so nobody waits on a key the others never write): object broadcast.  ``device`` = the transport's GPU: the
        agreement flag falls back to it when the group has no CPU backend (plain ``init_process_group("nccl")``; ADVICE r3 —
        with ``torch.device("cpu")`` here the fallback was a no-op and the constructor failed on every rank of such a group)."""
        if group is None:
            store = None
            try:
                store = dist.distributed_c10d._get_default_store()
            except Exception as exc:      # noqa: BLE001 — private accessor
                sys.stderr.write("hupr: no rendezvous store for the RCCL id (%s)\n" % exc)
            if _all_ok(store is not None, group, device):
                key = "hupr_rccl_uid_%d" % cls._n_comms
                cls._n_comms += 1
                if uid_bytes is not None:
                    store.set(key, uid_bytes)
                    return uid_bytes
                return bytes(store.get(key))                  # blocks until rank 0 has published the id or the sentinel
        box = [uid_bytes]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        return box[0]

    def ranks(self):
        """(n_ranks, rank) as the live communicator reports them (ncclCommCount / ncclCommUserRank)."""
        n, r = ctypes.c_int(0), ctypes.c_int(0)
        self.rt.check(self.L.hupr_comm_info(self.comm, ctypes.byref(n), ctypes.byref(r)))
        return n.value, r.value

    def all_reduce(self, flat, stream=None):
        """Enqueue on ``stream`` (a torch stream; default: the current one).  Returns None: ordering is the stream's."""
        s = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        self.rt.check(self.L.hupr_allreduce_bucket(self.comm, self.rt.ptr(flat), flat.numel(), 0, s))
        return None

    def broadcast(self, flat, src):
        s = torch.cuda.current_stream(self.device).cuda_stream
        self.rt.check(self.L.hupr_broadcast_bucket(self.comm, self.rt.ptr(flat), flat.numel(), 0, src, s))

    def close(self):
        if self.comm is not None and self.comm.value:
            self.L.hupr_comm_destroy(self.comm)
        self.comm = None


def make_transport(device, group=None):
    """RCCL through the C ABI for GPU buckets (fallback: torch.distributed on the nccl group), gloo for CPU tensors.  The
    constructor's failures are agreed over the control plane, so either every rank holds a native communicator or every
    rank lands in the except branch together — never a mix of transports."""
    if device.type != "cuda" or os.environ.get("HUPR_COLLECTIVE", "rccl") == "torch":
        return TorchTransport(group)
    try:
        return RcclTransport(device, group)
    except Exception as exc:      # noqa: BLE001 — an exchange step on the slower transport beats no exchange step
        sys.stderr.write("hupr: native RCCL communicator unavailable (%s); gradients go through torch.distributed\n" % exc)
        if not dist.is_initialized():
            raise
        return TorchTransport(group)


class _Bucket:
    def __init__(self, params, device):
        self.params = params
        self.numel = sum(p.numel() for p in params)
        self.flat_param = torch.empty(self.numel, dtype=torch.float32, device=device)
        self.flat_grad = torch.zeros(self.numel, dtype=torch.float32, device=device)
        off = 0
        self.views = []
        for p in params:
            n = p.numel()
            self.flat_param[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat_param[off:off + n].view_as(p)
            self.views.append(self.flat_grad[off:off + n].view_as(p))
            off += n
        self.pending = len(params)
        self.work = None
        self.index = {id(p): i for i, p in enumerate(params)}


class GradientBuckets:
    """Flat parameter/gradient buckets with overlapped all-reduce."""

    def __init__(self, module, bucket_bytes=48 << 20, process_group=None, tail_bytes=8 << 20):
        self.group = process_group
        # HUPR_FORCE_ALLREDUCE=1: run the collectives even with one rank (exercises RCCL + the side stream on a 1-GPU box)
        self.world_size = dist.get_world_size(process_group) if dist.is_initialized() else 1
        params = [p for p in module.parameters() if p.requires_grad]
        if not params:
            raise ValueError("module has no trainable parameters")
        self.device = params[0].device
        self.force_collective = os.environ.get("HUPR_FORCE_ALLREDUCE", "0") == "1" and \
            (dist.is_initialized() or self.device.type == "cuda")
        self.active = self.world_size > 1 or self.force_collective      # is there an exchange step at all?
        self.transport = make_transport(self.device, process_group) if self.active else None
        self._timing = None
        self.reduce_this_pass = True      # False while accumulating the leading micro-batches of an optimiser step
        self._accum_live = False
        self.use_streams = self.device.type == "cuda"
        self.comm_stream = torch.cuda.Stream(device=self.device) if self.use_streams else None
        # reverse registration order, split by size.  The all-reduce of the LAST bucket cannot overlap with anything
        # (its final gradient is the end of backward), so the trailing parameters get a small bucket of their own
        # (<= tail_bytes): the exposed collective is then latency- instead of bandwidth-sized.
        # parameters that ask to be ADJACENT in their bucket (module.gradient_groups(): the four 1x1 projection weights of an MSCSA
        # level and map — their fused weight gradient is one (4C, C) GEMM output, written straight into the four slots when they are
        # consecutive): the whole group is placed where its first member (in reverse registration order) falls
        member = {}
        for grp in (module.gradient_groups() if hasattr(module, "gradient_groups") else []):
            grp = [q for q in grp if q.requires_grad]
            for q in grp:
                member[id(q)] = grp
        ordered, placed = [], set()
        for p in reversed(params):
            if id(p) in placed:
                continue
            for q in member.get(id(p), [p]):
                ordered.append(q)
                placed.add(id(q))
        groups = []
        cur, cur_bytes = [], 0
        for p in ordered:
            cur.append(p)
            cur_bytes += p.numel() * 4
            # (a bucket never closes inside an adjacency group)
            if cur_bytes >= bucket_bytes and not (id(p) in member and member[id(p)][-1] is not p):
                groups.append(cur)
                cur, cur_bytes = [], 0
        if cur:
            groups.append(cur)
        last = groups[-1]
        if tail_bytes and sum(p.numel() for p in last) * 4 > tail_bytes and len(last) > 1:
            n_tail, acc = 0, 0
            for p in reversed(last):
                if acc + p.numel() * 4 > tail_bytes and n_tail > 0:
                    break
                acc += p.numel() * 4
                n_tail += 1
            if 0 < n_tail < len(last) and not (id(last[-n_tail]) in member and member[id(last[-n_tail])][0] is not last[-n_tail]):
                groups[-1:] = [last[:-n_tail], last[-n_tail:]]
        self.buckets = [_Bucket(g, self.device) for g in groups]
        self._owner = {}
        self._by_ptr = {}                       # parameter storage address -> (bucket, index): the direct-write sink
        for b in self.buckets:
            for i, p in enumerate(b.params):
                self._owner[id(p)] = b
                self._by_ptr[p.data_ptr()] = (b, i)
                p.register_post_accumulate_grad_hook(self._hook)
        self._names = {id(q): n for n, q in module.named_parameters()}
        self.direct = self.device.type == "cuda"
        self.always_zero = os.environ.get("HUPR_ZERO_GRADS", "0") == "1"
        # debug mode: a bucket that is NOT zero-filled is NaN-filled instead and finish() asserts that nothing of it
        # survived — proof that every kernel writing through the sink overwrites its whole slot (one synchronisation per step)
        self.poison = os.environ.get("HUPR_ZERO_GRADS", "0") == "poison"
        self._deferred = []
        self.prepare()

    # -- direct gradient sink (functional.GRAD_SINK protocol) -----------------------------------
    def take(self, param):
        """View the kernel should write ``param``'s gradient into, or None (unknown tensor / sink inactive)."""
        ent = self._by_ptr.get(param.data_ptr()) if self._armed else None
        if ent is None:
            return None
        b, i = ent
        if b.written[i]:
            raise RuntimeError("parameter received two direct gradient writes in one backward pass "
                               "(shared parameters are not supported by the gradient sink)")
        b.written[i] = True
        return b.views[i]

    # -- deferred final sums (functional.PReLUFn): a parameter whose gradient is a sum of partials that one launch can finish
    # together with others'.  The parameter counts as arrived at once; the sums are launched when the first bucket completes after
    # them (in front of its exchange), before a micro-batch is stashed, and in finish() at the latest.
    def can_defer(self, device):
        from .. import functional as F_
        # (one compute stream only: with the encoder branches on two streams the completing arrival may run on the side stream)
        return self._armed and device.type == "cuda" and not F_.TWO_STREAMS

    def defer_sum(self, param, partial, n, out):
        self._deferred.append((partial, int(n), out))
        self.done(param)

    def _flush_deferred(self):
        if not self._deferred:
            return
        from .. import functional as F_
        items = (F_.rt.SumItem * len(self._deferred))()
        for k, (partial, n, out) in enumerate(self._deferred):
            items[k].partial, items[k].n, items[k].out = partial.data_ptr(), n, out.data_ptr()
        F_.rt.check(F_.rt.lib().hupr_sum_partials_multi(items, len(self._deferred), F_.rt.stream()))
        self._deferred = []

    def _arrive(self, b, i):
        """Parameter i of bucket b has its gradient for this pass: count it ONCE, launch the bucket's exchange on the last arrival.
        (Round 5: autograd runs a parameter's accumulation node — and with it the post-accumulate hook — even when the operator's
        backward returned None after a direct write, so rounds 1-4 counted every directly written parameter twice: ``pending``
        reached zero half-way through a bucket and, with more than one rank, the all-reduce would have started before the bucket's
        last gradients were written.  Never seen on hardware — every run so far had one rank, whose all-reduce is the identity.)"""
        if b.arrived[i]:
            return
        b.arrived[i] = True
        b.pending -= 1
        if b.pending == 0:
            self._flush_deferred()
            self._launch(b)

    def done(self, param):
        b, i = self._by_ptr[param.data_ptr()]
        self._arrive(b, i)

    # -- per-iteration protocol ---------------------------------------------------------------
    def prepare(self, reduce=True):
        """Zero the flat gradients and (re)install the views; call before every backward.  ``reduce=False``: this
        backward is a leading micro-batch of an accumulated step — no exchange, ``stash()`` follows."""
        from .. import functional as F_
        self.reduce_this_pass = reduce
        for b in self.buckets:
            # Every kernel that writes a parameter gradient through the sink OVERWRITES its slot, so a bucket whose parameters were
            # all written directly in the previous pass is not zeroed again (4 fill launches, 142 MB per step).  Guarded: a slot that
            # is not zeroed and then receives an autograd-accumulated gradient raises (``_hook``); one that receives nothing is
            # zeroed in ``finish``.  HUPR_ZERO_GRADS=1 restores the unconditional fill.
            skip = self.direct and not self.always_zero and getattr(b, "written", None) is not None and all(b.written) \
                and getattr(b, "clean", False)
            if not skip:
                b.flat_grad.zero_()
            elif self.poison:
                b.flat_grad.fill_(float("nan"))
            b.zeroed = not skip
            b.clean = False
            b.pending = len(b.params)
            b.written = [False] * len(b.params)
            b.arrived = [False] * len(b.params)
            b.work = None
            b.launched = False
            for p, v in zip(b.params, b.views):
                p.grad = v
        self._deferred = []
        self._armed = self.direct
        F_.GRAD_SINK = self if self.direct else None

    def _hook(self, p):
        b = self._owner[id(p)]
        i = b.index[id(p)]
        v = b.views[i]
        if b.written[i]:                 # a kernel wrote this slot; the engine still visits the (empty) accumulation node
            self._arrive(b, i)
            return
        if not getattr(b, "zeroed", True):
            raise RuntimeError("autograd accumulated a gradient into the flat-bucket slot of %s, which was not zeroed for this pass (the "
                               "parameter received direct kernel writes in the previous pass but not in this one); set HUPR_ZERO_GRADS=1"
                               % self._names.get(id(p), "<unnamed parameter>"))
        if p.grad is not None and p.grad.data_ptr() != v.data_ptr():
            # autograd replaced the view (accumulation into an undefined grad): copy back
            v.copy_(p.grad)
            p.grad = v
        self._arrive(b, i)

    def _launch(self, b):
        if not self.active or not self.reduce_this_pass:
            return
        if self.use_streams:
            from .. import functional as F_
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self.comm_stream):
                self.comm_stream.wait_event(ev)
                for s in F_.side_streams_in_use(self.device):      # gradients of the side-stream branch (host-ordered earlier)
                    # torch hands out streams from a pool of 32 per device in turn, so after 32 more torch.cuda.Stream() calls the
                    # communication stream can BE the side stream.  A stream is ordered after itself; waiting for its own event
                    # while it is a forked stream of a graph capture makes the end of that capture crash, so it is not asked to
                    if s.cuda_stream != self.comm_stream.cuda_stream:
                        self.comm_stream.wait_stream(s)
                if self._accum_live:                               # earlier micro-batches of this optimiser step
                    b.flat_grad.add_(b.accum)
                if self._timing is not None:
                    t0 = torch.cuda.Event(enable_timing=True)
                    t0.record(self.comm_stream)
                b.work = self.transport.all_reduce(b.flat_grad, self.comm_stream)
                if self._timing is not None:
                    t1 = torch.cuda.Event(enable_timing=True)
                    t1.record(self.comm_stream)
                    self._timing["buckets"].append((self.buckets.index(b), t0, t1))
        else:
            if self._accum_live:
                b.flat_grad.add_(b.accum)
            b.work = self.transport.all_reduce(b.flat_grad)
        b.launched = True

    def stash(self):
        """After the backward of a leading micro-batch (``prepare(reduce=False)``): add its gradients to the accumulator."""
        self._flush_deferred()
        self._armed = False
        for b in self.buckets:
            if getattr(b, "accum", None) is None:
                b.accum = torch.zeros_like(b.flat_grad)
            if self._accum_live:
                b.accum.add_(b.flat_grad)
            else:
                b.accum.copy_(b.flat_grad)
        self._accum_live = True

    def finish(self):
        """Block the compute stream on outstanding collectives (call after backward)."""
        from .. import functional as F_
        self._flush_deferred()
        self._armed = False
        if F_.GRAD_SINK is self:
            F_.GRAD_SINK = None
        if self.poison and not self._accum_live:
            torch.cuda.synchronize(self.device)
            bad = [i for i, b in enumerate(self.buckets) if all(b.written) and not bool(torch.isfinite(b.flat_grad).all())]
            if bad:
                raise RuntimeError("HUPR_ZERO_GRADS=poison: buckets %r hold NaN after a pass that wrote every slot through the sink — a "
                                   "kernel writes its gradient slot partially or accumulates into it" % bad)
        for b in self.buckets:
            if not getattr(b, "zeroed", True) and not all(b.written):
                # slots that were left un-zeroed and received nothing in this pass hold the previous pass's gradients: clear them now
                for i, w in enumerate(b.written):
                    if not w:
                        b.views[i].zero_()
            b.clean = all(b.written)            # every slot of the bucket holds a gradient written (not accumulated) in this pass
            if self.active and self.reduce_this_pass and not b.launched:
                # a parameter received no gradient this iteration: reduce what we have
                b.pending = 0
                self._launch(b)
            if b.work is not None:
                b.work.wait()
                b.work = None
            if self._accum_live and self.reduce_this_pass and not self.active:
                b.flat_grad.add_(b.accum)                       # single rank: no exchange, just the micro-batch sum
        if self.use_streams and self.active and self.reduce_this_pass:
            if self._timing is not None:
                # where backward ended on the compute stream vs where the last collective ended on the communication stream: the
                # difference (if positive) is the part of the exchange step that overlapped with nothing
                e_bwd, e_comm = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e_bwd.record(torch.cuda.current_stream(self.device))
                e_comm.record(self.comm_stream)
                self._timing["tails"].append((e_bwd, e_comm))
            torch.cuda.current_stream(self.device).wait_stream(self.comm_stream)
        if self.reduce_this_pass:
            self._accum_live = False

    # -- measurement (bench.py --gpus N): per-bucket all-reduce durations and the exposed tail ---------------------------------
    def enable_timing(self, on=True):
        """Record HIP events around every bucket's all-reduce (communication stream) and at the join before Adam.  Eager steps only
        (events cannot be read back from a graph replay)."""
        self._timing = {"buckets": [], "tails": []} if (on and self.use_streams) else None

    def timing_report(self):
        """-> {"buckets": [{"index", "mbytes", "allreduce_us" (mean), "busbw_GBs"}], "exposed_tail_us": mean, "steps": n} from the
        events recorded since ``enable_timing`` (synchronises the device)."""
        if self._timing is None:
            return None
        torch.cuda.synchronize(self.device)
        per = {}
        for i, t0, t1 in self._timing["buckets"]:
            per.setdefault(i, []).append(t0.elapsed_time(t1) * 1e3)
        tails = [max(a.elapsed_time(b), 0.0) * 1e3 for a, b in self._timing["tails"]]
        n = self.world_size
        out = []
        for i in sorted(per):
            nbytes = self.buckets[i].numel * 4
            us = sum(per[i]) / len(per[i])
            # ring all-reduce: every rank sends and receives 2 (n - 1) / n of the message ("bus bandwidth" in RCCL's tests)
            out.append({"index": i, "mbytes": round(nbytes / 1e6, 1), "allreduce_us": round(us, 1),
                        "busbw_GBs": round(nbytes * 2.0 * (n - 1) / max(n, 1) / (us * 1e-6) / 1e9, 1) if us > 0 and n > 1 else None})
        return {"buckets": out, "exposed_tail_us": round(sum(tails) / len(tails), 1) if tails else None, "steps": len(tails)}

    def close(self):
        """Release the native communicator (engines that are re-created would otherwise leak one each)."""
        tr, self.transport = self.transport, None
        if tr is not None and hasattr(tr, "close"):
            tr.close()
        self.active = False

    def flat_pairs(self):
        return [(b.flat_param, b.flat_grad) for b in self.buckets]

    def layout(self):
        """Per bucket: [(parameter, offset, numel)] in bucket order (FusedAdam's checkpoint scatter/gather map)."""
        out = []
        for b in self.buckets:
            off, ent = 0, []
            for p in b.params:
                ent.append((p, off, p.numel()))
                off += p.numel()
            out.append(ent)
        return out

    def broadcast_parameters(self, src=0):
        """Make every rank start from rank ``src``'s weights (and buffers are left per rank)."""
        if self.world_size == 1:
            return
        for b in self.buckets:
            self.transport.broadcast(b.flat_param, src)
