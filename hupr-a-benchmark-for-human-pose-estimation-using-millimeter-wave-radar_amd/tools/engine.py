"""Training/inference engine shared by the Runner and bench.py: HuPRNet + LossComputer +
flat gradient buckets (+ RCCL all-reduce when world_size > 1) + fused Adam, SGD or LAMB, optionally fed by the
on-GPU FFT loader (int16 ADC cubes -> normalised network input, config "C3" of BASELINE.json)."""

import contextlib
import os

import torch
import torch.distributed as dist

from ..misc.losses import LossComputer
from ..models import HuPRNet
from ..preprocessing.interference import adc_interference, interference_setting
from ..preprocessing.process_iwr1843 import fft_chain_loader, fft_chain_loader_means
from . import augment as aug
from .distributed import GradientBuckets
from .ema import WeightEMA, ema_decay_setting
from .optim import make_optimizer


class TrainEngine:
    def __init__(self, cfg, device="cuda", lr=None, seed=0, bucket_bytes=48 << 20):
        self.cfg = cfg
        # DATASET.tdmCompensation: the FFT chain compensates the Doppler phase between the transmitters' slots (preprocessing,
        # hupr_fft_chain_tdm); off = today's launches.  A mirrored horizontal cube is compensated with the slots of TX0 and TX2 exchanged
        self.tdm = aug.tdm_setting(cfg)
        # DATASET.interference: interference blanking of both raw cubes in front of the FFT chain (preprocessing/interference.py; two
        # launches per cube); off = today's launches.  It runs in front of the mirror, with which it commutes
        self.interference = interference_setting(cfg)
        self.device = torch.device(device)
        self._if_acc = torch.zeros((2, 3), dtype=torch.int64, device=self.device) if self.interference is not None else None
        self.last_interference = None      # the (n, 2) int32 counts per sensor-frame of the cubes filtered last: (hori, vert)
        torch.manual_seed(seed)
        self.model = HuPRNet(cfg).to(self.device)
        self.lossComputer = LossComputer(cfg, self.device)
        self.buckets = GradientBuckets(self.model, bucket_bytes=bucket_bytes)
        self.buckets.broadcast_parameters(0)
        self.world_size = dist.get_world_size() if dist.is_initialized() else 1
        # (data-parallel runs keep the library default of two compute streams: with the stream-ordered hupr_allreduce_bucket the
        # side-stream branch gains 3 % with collectives in flight — 1 368 -> 1 412 frames/s with forced single-rank collectives)
        self.optimizer = make_optimizer(cfg, self.model.parameters(), lr if lr is not None else cfg.TRAINING.lr)
        self.optimizer.attach_flat_buckets(self.buckets.flat_pairs(), self.buckets.layout())
        self.optimizer.grad_scale = 1.0 / self.world_size
        # (TRAINING.optimizer: lamb takes its norms per parameter tensor over these buckets.  Data parallel needs no exchange for
        # them: the parameters are identical on every rank and the gradients all-reduced, so every rank computes the same ratios)
        # TRAINING.gradClip: clip the global gradient norm / skip a non-finite step, decided on the device between finish() and
        # the update (so the norm is that of the mean gradient over ranks and micro-batches, identical on every rank)
        if self.optimizer.grad_clip is not None:
            self.optimizer.enable_grad_guard(self.optimizer.grad_clip)
        # TRAINING.emaDecay: the averaged weights, one flat tensor per bucket, updated on the device behind every optimiser step.
        # Built after broadcast_parameters: every rank starts from the same weights and computes the same average, no exchange
        decay = ema_decay_setting(cfg)
        self.ema = WeightEMA(self.buckets.flat_pairs(), self.buckets.layout(), decay, module=self.model) if decay is not None else None
        self.G = cfg.DATASET.numGroupFrames
        # TRAINING.augMirror / augNoise / augMaskRange / augMaskAngle: one plan per training step, drawn on the device from a counter in
        # device memory (so a replayed step draws a fresh one); the rank is in the generator's key, so data-parallel ranks draw
        # different plans without an exchange.  TEST.flip is read here only to refuse a bad value where the config is read
        settings = aug.augment_settings(cfg)
        aug.flip_setting(cfg)
        self.augment = aug.Augmenter(cfg, settings, self.device, seed=seed, rank=dist.get_rank() if dist.is_initialized() else 0) \
            if settings is not None else None
        self._mirror_pairs = None
        self._all_swapped = None      # the flip test's swap flags under DATASET.tdmCompensation: every frame of the second pass
        self.fuse_elevation_mean = os.environ.get("HUPR_NO_FUSED_MEAN", "0") != "1"
        self._fft_ws = None
        self._seed = None
        self._graph = None
        self.keep_inference_graphs_current = True      # see _replay
        # the num_batches_tracked counters of all BatchNorms as views of one int64 vector: a training step bumps them
        # with ONE launch instead of one tiny add kernel per BatchNorm (30 per step); state_dict I/O is unchanged
        self._bns = [m for m in self.model.modules()
                     if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.num_batches_tracked is not None]
        self._bn_counts = torch.zeros(max(len(self._bns), 1), dtype=torch.long, device=self.device)
        for i, m in enumerate(self._bns):
            self._bn_counts[i] = m.num_batches_tracked
            m._buffers["num_batches_tracked"] = self._bn_counts[i]

    def close(self):
        """Release the exchange step's native communicator (call before building another engine in the same process)."""
        self.buckets.close()

    # -- data -------------------------------------------------------------------------------------
    def _blank(self, adc_hori, adc_vert):
        """DATASET.interference: both cubes through the filter, into new buffers (callers reuse their cubes, and a captured step's
        static inputs are refilled, not regenerated); the counters of ``interference_stats`` move on the device, so a replayed step
        counts too."""
        out, last = [], []
        for sensor, adc in enumerate((adc_hori, adc_vert)):
            cube, stats, _ = adc_interference(adc, self.interference)
            replaced = stats.frames[:, 0]
            self._if_acc[sensor] += torch.stack([torch.full_like(replaced[0], adc.shape[0], dtype=torch.int64), (replaced > 0).sum(),
                                                 replaced.sum()])
            out.append(cube)
            last.append(stats.frames)
        self.last_interference = tuple(last)
        return out

    def preprocess(self, adc_hori, adc_vert, hori_swapped=None, _blanked=False):
        """int16 ADC cubes (B*G, 4, 192, 256, 2) per sensor -> the two network inputs.  Default (``fuse_elevation_mean``): the
        loader tensor already averaged over its elevation axis, (B, G, 16, R, A) planes — 1/8 of the bytes written by the FFT
        chain and read back by the MNet front end, bit-identical results; ``HUPR_NO_FUSED_MEAN=1`` keeps the reference-shaped
        (B,G,F,2,R,A,E) hand-over.  With ``DATASET.tdmCompensation`` both chains compensate the TDM Doppler phase; ``hori_swapped``:
        (B,) uint8 on the device, the samples whose horizontal cube was mirrored (the vertical cube never is).  With
        ``DATASET.interference`` both cubes go through the interference filter first (``_blanked``: the caller already did that, in
        front of its mirror)."""
        if self.interference is not None and not _blanked:
            adc_hori, adc_vert = self._blank(adc_hori, adc_vert)
        n = adc_hori.shape[0]
        B = n // self.G
        if self.tdm:
            hkw = dict(tdm_compensation=True, tx_swapped=hori_swapped, frames_per_flag=self.G)
            if self.fuse_elevation_mean:
                return (fft_chain_loader_means(adc_hori, **hkw).view(B, self.G, 16, 64, 64),
                        fft_chain_loader_means(adc_vert, tdm_compensation=True).view(B, self.G, 16, 64, 64))
            return (fft_chain_loader(adc_hori, **hkw).view(B, self.G, 8, 2, 64, 64, 8),
                    fft_chain_loader(adc_vert, tdm_compensation=True).view(B, self.G, 8, 2, 64, 64, 8))
        if self.fuse_elevation_mean:
            return (fft_chain_loader_means(adc_hori).view(B, self.G, 16, 64, 64),
                    fft_chain_loader_means(adc_vert).view(B, self.G, 16, 64, 64))
        h = fft_chain_loader(adc_hori).view(B, self.G, 8, 2, 64, 64, 8)
        v = fft_chain_loader(adc_vert).view(B, self.G, 8, 2, 64, 64, 8)
        return h, v

    def _augmented_from_adc(self, adc_hori, adc_vert, joints):
        """The augmented training inputs of one (micro-)batch of raw cubes -> (hori, vert, joints): one plan, consumed by the ADC
        mirror of the horizontal cube (out of place: callers reuse their cubes, and a captured step's static inputs are refilled,
        not regenerated; the vertical cube is left as it is, tools/augment.py), by the noise and masks on both network inputs and
        by the labels."""
        a = self.augment
        a.plan(adc_hori.shape[0] // self.G)
        if self.interference is not None:            # the filter runs in front of the mirror (it commutes with it: whole groups move)
            adc_hori, adc_vert = self._blank(adc_hori, adc_vert)
        hori, vert = self.preprocess(a.adc(adc_hori), adc_vert, hori_swapped=a.flags if self.tdm and a.mirrors else None, _blanked=True)
        return a.apply(hori, 0), a.apply(vert, 1), a.labels(joints)

    # -- steps ------------------------------------------------------------------------------------
    def train_step(self, hori, vert, joints, decode=False, _last=True, _micro=1, _augmented=False):
        """One forward + loss + backward (+ exchange + Adam when ``_last``).  ``decode="device"`` also runs the two
        arg-max decodes of the reference's per-iteration ``computeLoss`` (misc/losses.py:43-44) as kernels on the
        step's stream; their results stay on the device (``self.last_decode``).  ``joints`` (B,K,2) are what ``TRAINING.targets``
        asks for: the integer joints by default, the float joints for ``subpixel`` (``tools.run.loss_labels``); they are handed to
        ``LossComputer.computeLoss`` as they come."""
        from .. import functional as F_
        self._refuse_while_swapped("train_step")
        if self.augment is not None and not _augmented:
            # already normalised inputs (stored cubes): noise and masks work on them, the mirror does not.  The engine owns neither
            # tensor here, so the transformed inputs are new ones
            if self.augment.mirrors:
                raise RuntimeError(aug.MIRROR_NEEDS_ADC)
            self.augment.plan(hori.shape[0])
            hori, vert = self.augment.apply(hori.contiguous().clone(), 0), self.augment.apply(vert.contiguous().clone(), 1)
        self.model.train()
        self.buckets.prepare(reduce=_last)
        F_.BN_COUNTER_SINK = due = []
        try:
            preds = self.model(hori, vert)
        finally:
            F_.BN_COUNTER_SINK = None
        if len(due) == len(self._bns) and all(a is b for a, b in zip(sorted(due, key=id), sorted(self._bns, key=id))):
            self._bn_counts.add_(1)                         # every BatchNorm ran exactly once: one launch
        else:
            for m in due:
                m.num_batches_tracked.add_(1)
        loss, loss2, p2d, g2d = self.lossComputer.computeLoss(preds, joints, decode=decode)
        self.last_decode = (p2d, g2d)
        if self._seed is None or self._seed.device != loss.device:
            self._seed = torch.ones((), dtype=loss.dtype, device=loss.device)      # backward()'s own ones_like is a fill launch per step
        loss.backward(gradient=self._seed)
        if self.device.type == "cuda":
            for s in F_.side_streams_in_use(self.device):           # the side-stream branch's backward joins here
                torch.cuda.current_stream(self.device).wait_stream(s)
        if not _last:
            self.buckets.stash()
            return loss, loss2
        self.buckets.finish()
        self.optimizer.grad_scale = 1.0 / (self.world_size * _micro)
        self.optimizer.step()
        if self.ema is not None:                            # a step the guard skipped leaves the average and its count alone
            self.ema.update(guard=self.optimizer._guard)
        return loss, loss2

    def train_step_accumulated(self, micro_batches, from_adc=True, decode=False):
        """One optimiser step over several micro-batches (fixed GLOBAL batch, ``bench.py --strong``): gradients of the
        leading micro-batches are summed locally, the exchange happens once, overlapped with the last backward.
        ``micro_batches``: list of (hori, vert, joints) — ADC cubes when ``from_adc``, joints as ``train_step`` takes them — each a per-rank micro-batch whose
        loss is its own mean, so the step's gradient is the mean over all ``world * len(micro_batches)`` of them.
        BatchNorm statistics are per micro-batch (as they are per rank in data parallel)."""
        m = len(micro_batches)
        out = None
        for i, (a, b, joints) in enumerate(micro_batches):
            augmented = from_adc and self.augment is not None          # each micro-batch draws its own plan
            if augmented:
                h, v, joints = self._augmented_from_adc(a, b, joints)
            else:
                h, v = self.preprocess(a, b) if from_adc else (a, b)
            out = self.train_step(h, v, joints, decode=decode, _last=i == m - 1, _micro=m, _augmented=augmented)
        return out

    def train_step_from_adc(self, adc_hori, adc_vert, joints, decode=False):
        if self._graph is not None:
            self._refuse_while_swapped("train_step")
            return self._replay(adc_hori, adc_vert, joints)
        return self._step_from_adc(adc_hori, adc_vert, joints, decode)

    def _step_from_adc(self, adc_hori, adc_vert, joints, decode):
        if self.augment is not None:
            h, v, joints = self._augmented_from_adc(adc_hori, adc_vert, joints)
            return self.train_step(h, v, joints, decode=decode, _augmented=True)
        h, v = self.preprocess(adc_hori, adc_vert)
        return self.train_step(h, v, joints, decode=decode)

    # -- hipGraph capture of the whole step (single-GPU) --------------------------------------------------------
    def capture(self, adc_hori, adc_vert, joints, warmup=2, decode=False):
        """Capture preprocess + forward + loss + backward (+ the bucket all-reduces on the communication stream) + Adam
        as ONE hipGraph and replay it from then on (``train_step_from_adc``).  ~700 kernel launches per step otherwise
        cost 9-18 ms of host time, which bounds the step once the kernels are faster than that.  Data parallel: the
        exchange is ``hupr_allreduce_bucket`` (ncclAllReduce enqueued on a stream), which is capturable — the fork to the
        communication stream and the join before Adam become edges of the graph; every rank must capture and replay
        in lock step.  Requirements: fixed shapes (the static input buffers are refilled by copy), joints already on
        the device (a pageable host-to-device copy is illegal inside a capture), ``TRAINING.lossDecay == -1`` (the
        alpha/beta loss weights would be frozen at their capture-time values), ``sync_lr()`` after LR changes.
        With ``TRAINING.targets: subpixel`` the joints must be a floating tensor: the static buffer keeps their dtype (an integer
        buffer would truncate every later batch), and a conversion to fp32 is a device kernel inside the captured region.
        The gradient guard (``TRAINING.gradClip``), the weight average (``TRAINING.emaDecay``), the mined loss with its counters
        (``TRAINING.ohkm``, ``TRAINING.jointWeights``) and the coordinate and bone-vector losses with their accumulators
        (``TRAINING.coordLoss``, ``TRAINING.boneLoss``) are device-side and replay with the step; so is the augmentation
        (``TRAINING.aug*``): its plan is drawn by a launch from a counter in device memory, so every replay draws a fresh plan.
        The ``warmup`` eager steps are real optimisation steps."""
        self._refuse_while_swapped("capture")
        tr = self.buckets.transport
        if self.buckets.active and not getattr(tr, "capturable", False):
            raise RuntimeError("graph capture needs the native RCCL transport (got %s)" % getattr(tr, "name", tr))
        if self.cfg.TRAINING.lossDecay != -1:
            raise RuntimeError("graph capture would freeze the loss weights alpha/beta (TRAINING.lossDecay != -1)")
        if not (adc_hori.is_cuda and adc_vert.is_cuda and joints.is_cuda):
            raise RuntimeError("graph capture needs ADC cubes and joints resident on the GPU")
        if self.lossComputer.targets_mode == "subpixel" and not joints.is_floating_point():
            raise RuntimeError("graph capture with TRAINING.targets: subpixel needs floating joints (got %s): the static buffer "
                               "keeps their dtype" % joints.dtype)
        self.optimizer.use_device_state()
        self._g_decode = decode
        self._g_in = (adc_hori.clone(), adc_vert.clone(), joints.clone())
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._step_from_adc(self._g_in[0], self._g_in[1], self._g_in[2], decode)
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._g_out = self._step_from_adc(self._g_in[0], self._g_in[1], self._g_in[2], decode)
        self._graph = g

    def sync_lr(self):
        self.optimizer.sync_lr()

    def guard_stats(self):
        """With ``TRAINING.gradClip`` set: {"norm": the last step's global gradient norm (after ``grad_scale``), "coef": its
        clipping coefficient (0 for a skipped step), "skipped": steps skipped so far}; None otherwise.  Synchronises the
        device: per epoch, not per step.  A skipped step leaves parameters, optimiser state and step count as they were; the
        BatchNorm running statistics of its forward pass have moved all the same (as under torch's GradScaler)."""
        return self.optimizer.guard_stats()

    def lamb_stats(self):
        """With ``TRAINING.optimizer: lamb``: {parameter name: (|p|, |u|, r)} of the last optimiser step that was not skipped —
        the parameter's norm before that step, the norm of its update direction and its trust ratio (1 for every parameter with
        ``ndim <= 1``; all zeros before the first step); None with another optimiser.  Synchronises the device: per epoch, not
        per step."""
        stats = getattr(self.optimizer, "lamb_stats", lambda: None)()
        if stats is None:
            return None
        names = {id(p): name for name, p in self.model.named_parameters()}
        return {names[id(p)]: (float(pn[i]), float(un[i]), float(r[i]))
                for entries, (pn, un, r) in zip(self.buckets.layout(), stats) for i, (p, _, _) in enumerate(entries)}

    def mining_stats(self):
        """With ``TRAINING.ohkm`` or ``TRAINING.jointWeights`` set: {"k": joints kept per head and sample, "counts": (2, K) int64
        ndarray, how often each joint was kept by the first head (row 0) and the PRGCN head (row 1) in the training losses so far,
        "samples": the samples those losses saw, "plane_loss": the last loss's (2, B, K) unweighted plane losses (None before the
        first; between ``capture()`` and the first replay it is the captured step's buffer, which no step has filled yet)}; None
        otherwise.  The counters live on the device and replay with a captured step; they are diagnostics, not part
        of a checkpoint.  Synchronises the device: per epoch, not per step."""
        lc = self.lossComputer
        if not lc.mined:
            return None
        counts = lc.mining_counts.cpu().numpy()
        return {"k": lc.mined_k, "counts": counts, "samples": int(counts[1].sum()) // lc.mined_k,
                "plane_loss": lc.plane_loss.cpu().numpy() if lc.plane_loss is not None else None}

    def coord_stats(self):
        """With ``TRAINING.coordLoss`` set: {"weight": lambda, "sum": (sum of C_0, sum of C_1) over the training losses so far — C_h the
        coordinate loss of the first head and of the PRGCN head in heat-map pixels, before lambda and the head weights —, "steps": how
        many losses those sums hold, "residual": the last loss's (2, B, K, 2) ndarray of centroid offsets from the joints (None
        before the first; between ``capture()`` and the first replay it is the captured step's buffer, which no step has filled
        yet)}; None otherwise.  The accumulator lives on the device and replays with a captured step; it is a diagnostic, not part
        of a checkpoint.  Synchronises the device: per epoch, not per step."""
        lc = self.lossComputer
        if lc.coordLoss is None:
            return None
        acc = lc.coord_acc.cpu().numpy()
        return {"weight": lc.coordLoss, "sum": (float(acc[0]), float(acc[1])), "steps": int(round(acc[2])),
                "residual": lc.coord_residual.cpu().numpy() if lc.coord_residual is not None else None}

    def augment_stats(self):
        """With a ``TRAINING.aug*`` key set: {"steps": plans drawn so far (the generator's counter: it is what a checkpoint keeps as
        ``augment_step``), "samples": the samples they covered, "mirrored": how many of those were mirrored, "mean_sigma": the mean
        noise level drawn, "last_plan": the last plan's (B, 8) int32 table (tools/augment.py; between ``capture()`` and the first
        replay it is the captured step's buffer)}; None otherwise.  The state lives on the device and replays with a captured step.
        Synchronises the device: per epoch, not per step."""
        return self.augment.stats() if self.augment is not None else None

    def interference_stats(self):
        """With ``DATASET.interference`` set: {"filter": the InterferenceFilter, "hori" and "vert": {"frames": sensor-frames the filter
        has seen so far (training and inference, every frame of every window), "touched": how many of them had a sample replaced,
        "samples": samples replaced}}; None otherwise.  The counters live on the device and replay with a captured step; they are
        diagnostics, not part of a checkpoint.  Synchronises the device: per epoch, not per step."""
        if self.interference is None:
            return None
        acc = self._if_acc.cpu().numpy()
        out = {"filter": self.interference}
        for i, name in enumerate(("hori", "vert")):
            out[name] = {"frames": int(acc[i, 0]), "touched": int(acc[i, 1]), "samples": int(acc[i, 2])}
        return out

    def bone_stats(self):
        """With ``TRAINING.boneLoss`` set: {"weight": mu, "sum": (sum of B_0, sum of B_1) over the training losses so far — B_h the
        bone-vector loss of the first head and of the PRGCN head in heat-map pixels, before mu and the head weights —, "steps": how
        many losses those sums hold, "residual": the last loss's (2, B, E, 2) ndarray of bone-vector errors (None before the first;
        between ``capture()`` and the first replay it is the captured step's buffer, which no step has filled yet)}; None
        otherwise.  As ``coord_stats``: the accumulator lives on the device, replays with a captured step and is not part of a
        checkpoint.  Synchronises the device: per epoch, not per step."""
        lc = self.lossComputer
        if lc.boneLoss is None:
            return None
        acc = lc.bone_acc.cpu().numpy()
        return {"weight": lc.boneLoss, "sum": (float(acc[0]), float(acc[1])), "steps": int(round(acc[2])),
                "residual": lc.bone_residual.cpu().numpy() if lc.bone_residual is not None else None}

    # -- averaged weights (TRAINING.emaDecay) -----------------------------------------------------------------------------------
    def ema_stats(self):
        """With ``TRAINING.emaDecay`` set: {"updates": updates of the average so far (skipped steps do not count), "weight": the
        last step's weight 1 - min(decay, (1 + k) / (10 + k)), 0.0 for a skipped step}; None otherwise.  Synchronises the device:
        per epoch, not per step."""
        return self.ema.stats() if self.ema is not None else None

    def _refuse_while_swapped(self, what):
        if self.ema is not None and self.ema.swapped:
            raise RuntimeError("%s inside averaged_weights(): the parameters hold the average, not the trained weights" % what)

    def _swap_weights(self):
        from .. import functional as F_
        self.ema.swap()
        F_.invalidate_packed()      # the parameters changed behind every host-side cache, as after a graph replay (_replay)
        if self.keep_inference_graphs_current:
            F_.refresh_packed(self.device)

    @contextlib.contextmanager
    def averaged_weights(self):
        """``with engine.averaged_weights():`` — the model's parameters are the averaged weights inside the block (``infer``,
        ``Runner.eval``) and the trained ones again behind it: parameters and average are exchanged in place, one launch per
        bucket each way, every bit kept.  Buffers are not touched: the BatchNorm running statistics are the live ones.  No
        training step, no capture and no second ``averaged_weights()`` inside the block."""
        if self.ema is None:
            raise RuntimeError("averaged_weights() needs TRAINING.emaDecay")
        if self.ema.swapped:
            raise RuntimeError("averaged_weights() is already active (no nesting)")
        self._swap_weights()
        try:
            yield self
        finally:
            self._swap_weights()

    def _replay(self, adc_hori, adc_vert, joints):
        for dst, src in zip(self._g_in, (adc_hori, adc_vert, joints)):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src, non_blocking=True)
        self._graph.replay()
        from .. import functional as F_
        F_.invalidate_packed()      # the graph's Adam node changed the parameters behind every host-side cache
        if self.keep_inference_graphs_current:
            # captured INFERENCE graphs (no_grad) read the cached packed / derived weights in place: refill them now, stream-ordered
            # behind the replay, so that such a graph replayed next sees this step's weights (one table launch)
            F_.refresh_packed(self.device)
        return self._g_out

    @torch.no_grad()
    def infer(self, hori, vert):
        self.model.eval()
        return self.model(hori, vert)

    @torch.no_grad()
    def infer_from_adc(self, adc_hori, adc_vert, flip=False):
        """Inference from raw cubes; never augmented.  ``flip``: the flip test — one forward on the input, one on the horizontal cube
        with every frame mirrored (``hupr_adc_mirror_i16``; the same batch size, so the kernels route identically; the vertical
        input is the same tensor, tools/augment.py), and both heads merged with the mirrored, left/right-exchanged maps of the
        second pass (``hupr_flip_merge_f32``).  Twice the work of a plain call.  ``DATASET.interference`` filters both cubes once,
        in front of the mirror."""
        if self.interference is not None:
            adc_hori, adc_vert = self._blank(adc_hori, adc_vert)
        hori, vert = self.preprocess(adc_hori, adc_vert, _blanked=True)
        preds = self.infer(hori, vert)
        if not flip:
            return preds
        if self._mirror_pairs is None:
            self._mirror_pairs = aug.mirror_pairs(self.cfg.DATASET.idxToJoints)
        adc_m = aug.adc_mirror(adc_hori)
        B = adc_m.shape[0] // self.G
        if self.tdm:                             # every frame of the second pass is mirrored: all flags set
            if self._all_swapped is None or self._all_swapped.numel() != B:
                self._all_swapped = torch.ones(B, dtype=torch.uint8, device=adc_m.device)
            kw = dict(tdm_compensation=True, tx_swapped=self._all_swapped, frames_per_flag=self.G)
        else:
            kw = {}
        hori_m = fft_chain_loader_means(adc_m, **kw).view(B, self.G, 16, 64, 64) if self.fuse_elevation_mean else \
            fft_chain_loader(adc_m, **kw).view(B, self.G, 8, 2, 64, 64, 8)
        preds_m = self.infer(hori_m, vert)
        return tuple(aug.flip_merge(p, pm, self._mirror_pairs) for p, pm in zip(preds, preds_m))
