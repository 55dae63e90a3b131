"""Runner — train / eval loops with the reference's surface (tools/run.py:13-86):
``Runner(args, cfg)``, ``.loadModelWeight(mode)``, ``.train()``, ``.eval(visualization, epoch) -> AP``.

Differences that are the point of this build: the step runs through ``TrainEngine`` (HIP kernels,
flat gradient buckets, RCCL all-reduce when launched under torchrun), the FFT preprocessing can run
on the GPU inside the step (synthetic/raw-ADC datasets), and losses are not synchronised every step.
"""
import contextlib
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.utils.data as data

from ..datasets import getDataset
from ..datasets.dataset import HuPRRawADC, SequenceGroupedSampler
from ..misc.losses import TARGETS
from ..misc.oks_eval import evaluate_keypoints, mean_bone_error, mean_position_error
from ..misc.plot import plotHumanPose
from .augment import flip_setting
from .base import BaseRunner
from .engine import TrainEngine
from .smooth import SequenceSmoother, SequenceWalker, jitter, temporal_setting
from .stream import presence_setting


def _collate(batch):
    out = {}
    for k in batch[0]:
        v = [b[k] for b in batch]
        out[k] = torch.stack(v) if isinstance(v[0], torch.Tensor) else torch.as_tensor(v)
    return out


def loss_labels(batch, mode):
    """The joints of ``batch`` that the loss takes under ``TRAINING.targets`` = ``mode``: the integer ``jointsGroup`` itself for
    ``integer``, the float ``jointsFloat`` as fp32 (fractions kept) for ``subpixel``.  A batch without ``jointsFloat`` is an error
    there, not a reason to train on the truncated joints."""
    if mode not in TARGETS:
        raise ValueError("TRAINING.targets must be 'integer' or 'subpixel', got %r" % (mode,))
    if mode == "integer":
        return batch["jointsGroup"]
    if "jointsFloat" not in batch:
        raise KeyError("TRAINING.targets: subpixel needs the float joints of the batch ('jointsFloat'); this dataset yields only %s"
                       % sorted(batch))
    return batch["jointsFloat"].float()


def interference_line(what, counts):
    """DATASET.interference — the line ``Runner.train`` prints per epoch and ``Runner.eval`` per evaluation: per sensor, the share of
    the labelled frames (window position G / 2) in which the filter replaced a sample, and the samples it replaced there.
    ``counts``: a list of int32 (B, 2 sensors, 2) tensors, one per batch."""
    c = torch.cat(counts).cpu().numpy().astype(np.int64) if counts else np.zeros((0, 2, 2), np.int64)
    n = c.shape[0]
    parts = ["%s %.3f (%d samples replaced)" % (name, float((c[:, i, 0] > 0).mean()) if n else float("nan"), int(c[:, i, 0].sum()))
             for i, name in enumerate(("hori", "vert"))]
    return "%s: share of %d labelled frames touched: %s" % (what, n, "  ".join(parts))


def trust_ratio_line(epoch, stats, params):
    """TRAINING.optimizer: lamb — the epoch's line: minimum, median and maximum trust ratio of the last step over the adapted
    tensors (``ndim > 1``; the others have ratio 1 by rule) and the names of the two extremes."""
    r = sorted((v[2], name) for name, v in stats.items() if params[name].ndim > 1)
    if not r:
        return "==========>Trust ratios in epoch %d: no adapted tensor" % epoch
    return "==========>Trust ratios in epoch %d (%d adapted tensors): min %.4g (%s)  median %.4g  max %.4g (%s)" % (
        epoch, len(r), r[0][0], r[0][1], float(np.median([x for x, _ in r])), r[-1][0], r[-1][1])


class Runner(BaseRunner):
    def __init__(self, args, cfg):
        super().__init__(args, cfg)
        if self.device != "cuda":
            raise RuntimeError("the HIP runner needs a GPU (no CPU fallback)")
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.temporal = temporal_setting(cfg)   # TEST.temporal: eval() walks the test set through the Kalman tracker (tools/smooth.py)
        if self.temporal is not None and self.world > 1:
            raise RuntimeError("TEST.temporal: %s needs a single process: the evaluation is sharded over the %d ranks sample by sample, "
                               "which would split every sequence" % (self.temporal.mode, self.world))
        self.presence = presence_setting(cfg)   # TEST.presence: eval() runs the CA-CFAR detector and the presence gate (csrc/cfar.hip)
        if self.presence is not None and self.world > 1:
            raise RuntimeError("TEST.presence needs a single process: the evaluation is sharded over the %d ranks sample by sample, "
                               "which would split every sequence" % self.world)
        if not args.eval:
            self.trainSet = getDataset("train", cfg, args)
            if isinstance(self.trainSet, HuPRRawADC):
                # raw captures: a cache miss costs a whole sequence (0.9 GB of adc_data.bin + its FFT), so the loader walks
                # shuffled GROUPS of sequences and shuffles the windows inside a group (SequenceGroupedSampler)
                sampler = SequenceGroupedSampler(self.trainSet, group=self.trainSet.cache_sequences, seed=args.seed,
                                                 rank=self.rank, world=self.world)
            else:
                sampler = data.distributed.DistributedSampler(self.trainSet, shuffle=True, drop_last=True) if self.world > 1 else None
            self.trainLoader = data.DataLoader(self.trainSet, cfg.TRAINING.batchSize, shuffle=sampler is None,
                                               sampler=sampler, num_workers=0, collate_fn=_collate,
                                               drop_last=self.world > 1)      # ragged last step only single-GPU
        else:
            self.trainLoader = [0]
        self.testSet = getDataset("test" if args.eval else "val", cfg, args)
        # does the GPU FFT chain feed this run (raw captures), or stored .npy cubes?  (tools/base.py: the preprocess.json sidecar)
        self.uses_gpu_fft_loader = isinstance(self.testSet, HuPRRawADC) or isinstance(getattr(self, "trainSet", None), HuPRRawADC)
        # evaluation is sharded over the ranks (rank r takes samples r, r + world, ...) and gathered on rank 0
        shard = data.Subset(self.testSet, range(self.rank, len(self.testSet), self.world)) if self.world > 1 else self.testSet
        self.testLoader = data.DataLoader(shard, cfg.TEST.batchSize, shuffle=False, num_workers=0, collate_fn=_collate)
        warm = cfg.TRAINING.warmupEpoch
        self.stepSize = len(self.trainLoader) * warm
        LR = cfg.TRAINING.lr if warm == -1 else cfg.TRAINING.lr / (cfg.TRAINING.warmupGrowth ** self.stepSize)
        self.engine = TrainEngine(cfg, device=torch.device("cuda", torch.cuda.current_device()), lr=LR, seed=args.seed)
        self.model, self.optimizer, self.lossComputer = self.engine.model, self.engine.optimizer, self.engine.lossComputer
        self.flip = flip_setting(cfg)           # TEST.flip: eval() runs the flip test (raw-ADC batches only)
        for d in (self.dir, self.visDir):
            os.makedirs(d, exist_ok=True)
        if not args.eval:
            print("==========>Train set size:", len(self.trainLoader))
        print("==========>Test set size:", len(self.testLoader))

    def _adc(self, batch):
        dev = self.engine.device
        B, G = batch["adc_hori"].shape[:2]
        return (batch["adc_hori"].to(dev).reshape(B * G, 4, 192, 256, 2), batch["adc_vert"].to(dev).reshape(B * G, 4, 192, 256, 2))

    def _inputs(self, batch):
        dev = self.engine.device
        if "adc_hori" in batch:          # raw ADC cubes: FFT chain + loader glue on the GPU
            return self.engine.preprocess(*self._adc(batch))
        return batch["VRDAEmap_hori"].float().to(dev), batch["VRDAEmap_vert"].float().to(dev)

    def _labelled_interference(self, batch):
        """DATASET.interference: the filter's int32 (B, 2 sensors, 2) counts on the labelled frame of every sample of the batch that
        just went through the engine (raw cubes) or through the dataset's sequence cache (``batch["interference"]``)."""
        if "interference" in batch:
            return batch["interference"].to(self.engine.device)
        G = self.F
        return torch.stack([f.view(-1, G, 2)[:, G // 2] for f in self.engine.last_interference], dim=1)

    def _centre_planes(self, hori):
        """The horizontal network input of a batch, (B, G, 16, R, A) mean planes or the (B, G, F, 2, R, A, E) cube (averaged over its
        elevation axis here, as HuPRNet.forward does first) -> the (B, 16, R, A) mean planes of window position G / 2, the labelled frame."""
        if hori.dim() == 7:
            hori = hori.mean(dim=-1).reshape(hori.shape[0], hori.shape[1], 16, hori.shape[4], hori.shape[5])
        return hori[:, hori.shape[1] // 2].contiguous()

    def eval(self, visualization=True, epoch=-1):
        """-> AP (reference tools/run.py:35-63).  Predictions are decoded from the GCN head, scaled to image pixels,
        written to ``<phase>_results.json`` by rank 0 and scored with the OKS evaluator against the ground truth the
        reference uses: the float joints of ``<phase>_gt.json`` (not the integer-truncated ``jointsGroup`` the loss sees by default;
        with ``TRAINING.targets: subpixel`` the loss sees the float joints too, ``loss_labels``).  When ``TRAINING.targets`` or
        ``TEST.decode`` is ``subpixel``, ``TEST.decode`` is ``integral``, or ``TRAINING.coordLoss`` or ``TEST.flip`` is set, one more line is printed, the mean per-joint position error in image pixels
        (``mean_position_error``): AP's OKS thresholds are too coarse to show a sub-pixel change.  ``TRAINING.boneLoss`` prints that
        line and one more, the mean error of the bones' lengths in image pixels (``mean_bone_error``).
        ``--keypoints`` prints the per-joint APs (``evaluateEach``) instead of the summary line.
        ``TEST.temporal: track``, ``rts`` or ``lag`` (``temporal_setting``): the test set is walked in loader order as sequences (sequence and
        frame from ``imageId``; a new sequence or a frame that is not its predecessor + 1 zeroes the tracker state), every sample's
        second-head maps go through ``SequenceSmoother.track`` one frame per call, and the keypoints written and scored are the
        Kalman-filtered ones (``track``), the Rauch-Tung-Striebel smoothed ones (``rts``) or the fixed-lag smoothed ones (``lag``:
        every frame smoothed over the ``TEST.temporalLag`` frames behind it, ``SequenceSmoother.smooth_lagged``).  After the AP line
        come an ``MPJPE`` line for the raw, the filtered and the smoothed (``rts``) or lagged (``lag``) keypoints and a ``Jitter``
        line (``tools.smooth.jitter``) for each of them and for the ground truth.  With ``TEST.temporalFit: true`` the walk also records
        every frame's measurements, and one more line follows: ``tracker fit:`` the maximum-likelihood ``accel_psd``, ``meas_std`` and
        ``heatmap_gain`` on them (``tools.calibrate.fit_tracking``), the cost per measurement at the configured and at the fitted
        values, and the fitted run's status counts.  Nothing is scored again: the values go under ``TEST.tracking`` for the next run.
        With ``TEST.tracking.accel_psd_moving`` (``track`` only) the walk runs the two-model tracker, the filtered keypoints are the
        mixture of its models, and one more line follows the jitter: ``Moving:`` the mean probability of the moving model over the
        joints and frames with a live track.
        ``TEST.presence`` (``tools.stream.presence_setting``): the test set is walked as sequences in the same way, the CA-CFAR
        detector (``functional.cfar_ra``) runs on the horizontal mean planes of every sample's labelled frame (window position G / 2)
        and the presence gate across each sequence, and one more line is printed: ``Presence: <share> of <n> labelled frames present,
        median <m> detections``.  Every labelled frame has a person in it, so the share's complement is the gate's miss rate.  Raw
        ADC batches and stored cubes both work.  Keypoints and AP are what they are without the key.
        ``DATASET.interference`` (``preprocessing.interference_setting``): both raw cubes go through the interference filter in front
        of the FFT chain, and one more line is printed, the share of the labelled frames in which it replaced a sample, per sensor
        (this rank's share of the test set): nobody knows yet whether the published captures carry interference."""
        self.logger.clear(len(self.testLoader.dataset))
        savePreds, gts = [], []
        blanked = [] if self.engine.interference is not None else None
        temporal = self.temporal
        if temporal is not None:
            smoother = SequenceSmoother(temporal.tracking, self.numKeypoints, self.engine.device,
                                        lag=temporal.lag if temporal.mode == "lag" else None, measurements=temporal.fit)
            walker, boxes, ids = SequenceWalker(), [], []
        gate = self.presence
        if gate is not None:
            from .. import functional as F_
            gate_state = F_.presence_state(1, self.engine.device)
            gate_walker, gate_present, gate_counts = SequenceWalker(), [], []
        for batch in self.testLoader:
            keypoints = batch["jointsGroup"]
            hori = None
            if self.flip:
                # TEST.flip: the mirror of this radar is a permutation of the raw cube (tools/augment.py), so stored cubes cannot take it
                if "adc_hori" not in batch:
                    raise RuntimeError("TEST.flip needs a dataset of raw ADC cubes ('adc_hori'); this one yields only %s" % sorted(batch))
                preds = self.engine.infer_from_adc(*self._adc(batch), flip=True)
            else:
                hori, vert = self._inputs(batch)
                preds = self.engine.infer(hori, vert)
            if blanked is not None:
                blanked.append(self._labelled_interference(batch))
            if gate is not None:
                if hori is None:                    # the flip test ran from the raw cubes
                    hori = self._inputs(batch)[0]
                occ = F_.cfar_ra(self._centre_planes(hori), gate.pfa, gate.guard, gate.train, want_mask=False).summary
                for j in range(keypoints.size(0)):
                    if gate_walker.step(batch["imageId"][j]):
                        gate_state.zero_()
                    gate_present.append(F_.presence_update(occ[j:j + 1], gate_state, gate.min_cells, gate.confirm, gate.hold))
                gate_counts.append(occ[:, 0])
            with torch.no_grad():
                loss, loss2, pred2d, _ = self.lossComputer.computeLoss(preds, loss_labels(batch, self.lossComputer.targets_mode))
            self.logger.display(loss, loss2, keypoints.size(0), epoch)
            if visualization:                       # --visDir given: one skeleton overlay per sample (run.py:50-52)
                plotHumanPose(pred2d * self.imgHeatmapRatio, self.cfg, self.visDir, batch["imageId"], None)
            if temporal is None:
                self.saveKeypoints(savePreds, pred2d * self.imgHeatmapRatio, batch["bbox"], batch["imageId"])
            else:
                maps = preds[1].detach().reshape(-1, self.numKeypoints, self.height, self.width)
                for j in range(keypoints.size(0)):
                    if walker.step(batch["imageId"][j]):
                        smoother.new_sequence()
                    smoother.track(maps[j], self.imgHeatmapRatio, refine=self.lossComputer.decode == "subpixel")
                    boxes.append(batch["bbox"][j])
                    ids.append(batch["imageId"][j])
            gt_joints = batch["jointsFloat"] if "jointsFloat" in batch else keypoints
            for j in range(keypoints.size(0)):
                gts.append({"image_id": int(batch["imageId"][j]), "keypoints": gt_joints[j].numpy().astype(np.float64),
                            "bbox": batch["bbox"][j].numpy().astype(np.float64)})
        if temporal is not None:
            seq = {"rts": smoother.smooth, "lag": smoother.smooth_lagged, "track": smoother.history.record}[temporal.mode]().cpu()
            tracks = {"raw": seq.raw.numpy(), "filtered": seq.filtered.numpy()}
            scored = {"rts": "smoothed", "lag": "lagged", "track": "filtered"}[temporal.mode]
            if scored != "filtered":
                tracks[scored] = seq.keypoints.numpy()
            self.saveKeypoints(savePreds, tracks[scored], boxes, ids)
            visited = np.stack([g["keypoints"] for g in gts])
        if self.world > 1:
            parts = [None] * self.world
            dist.all_gather_object(parts, (savePreds, gts))
            savePreds = [r for p in parts for r in p[0]]
            gts = [g for p in parts for g in p[1]]
        ap = 0.0
        if self.rank == 0:
            self.writeKeypoints(savePreds)
            # ground truth = the whole <phase>_gt.json where the dataset has one (the reference scores against the full file,
            # datasets/dataset.py:68-88: with -sr > 1 the frames the loader never visited count as misses); the synthetic
            # dataset has no file, its ground truth is what the loader visited
            full_gt = getattr(self.testSet, "gt_annotations", None)
            if full_gt is not None:
                gts = full_gt
            names = ["AP", "Ap .5", "AP .75", "AP (M)", "AP (L)", "AR", "AR .5", "AR .75", "AR (M)", "AR (L)"]
            if getattr(self.args, "keypoints", False):            # evaluateEach, THEN the summary (tools/run.py:60-63)
                idx2j = self.cfg.DATASET.idxToJoints
                for k in range(self.numKeypoints):
                    print("%s: %.3f" % (idx2j[k], float(evaluate_keypoints(gts, savePreds, idx_keypoint=k)[0])))
            stats = evaluate_keypoints(gts, savePreds)
            print("  ".join("%s: %.3f" % (n, s) for n, s in zip(names, stats)))
            ap = float(stats[0])
            if ("subpixel" in (self.lossComputer.targets_mode, self.lossComputer.decode) or self.lossComputer.decode == "integral"
                    or self.lossComputer.coordLoss is not None or self.lossComputer.boneLoss is not None or self.flip):
                print("MPJPE: %.3f px (n = %d)" % mean_position_error(gts, savePreds)[::2])
            if self.lossComputer.boneLoss is not None:
                print("Bone error: %.3f px (n = %d)" % mean_bone_error(gts, savePreds)[::2])
            if temporal is not None:
                for name, kp in tracks.items():
                    print("MPJPE %s: %.3f px (n = %d)" % ((name,) + mean_position_error(gts, self.saveKeypoints([], kp, boxes, ids))[::2]))
                for name, kp in list(tracks.items()) + [("truth", visited)]:
                    print("Jitter %s: %.3f px" % (name, jitter([kp[a:b] for a, b in walker.segments()])))
                if temporal.tracking.maneuvers:     # TEST.tracking.accel_psd_moving: how much of the time the moving model carried the pose
                    print("Moving: %.3f mean probability of the moving model (n = %d live joints)" % smoother.history.moving_mean())
                if temporal.fit:                    # TEST.temporalFit: the values to put under TEST.tracking; nothing is scored again
                    print(smoother.fit_tracking().line())
            if blanked is not None:
                print(interference_line("Interference", blanked))
            if gate is not None:
                present = torch.cat(gate_present).cpu().numpy() if gate_present else np.zeros(0, np.int32)
                counts = torch.cat(gate_counts).cpu().numpy() if gate_counts else np.zeros(0, np.float32)
                print("Presence: %.3f of %d labelled frames present, median %g detections" % (
                    float(present.mean()) if present.size else float("nan"), present.size,
                    float(np.median(counts)) if counts.size else float("nan")))
        if self.world > 1:
            box = [ap]
            dist.broadcast_object_list(box, src=0)
            ap = box[0]
        return ap

    def train(self):
        averaged = self.engine.ema is not None
        if averaged and self.rank == 0:
            print("==========>TRAINING.emaDecay = %g: each epoch is evaluated, and model_best.pth chosen, with the averaged weights"
                  % self.engine.ema.decay)
        for epoch in range(self.start_epoch, self.cfg.TRAINING.epochs):
            loss_list = []
            guard0 = self.engine.guard_stats()
            mined0 = self.engine.mining_stats()
            coord0 = self.engine.coord_stats()
            bone0 = self.engine.bone_stats()
            aug0 = self.engine.augment_stats()
            blanked = [] if self.engine.interference is not None else None
            self.logger.clear(len(self.trainLoader.dataset))
            if hasattr(self.trainLoader.sampler, "set_epoch"):
                self.trainLoader.sampler.set_epoch(epoch)
            for idxBatch, batch in enumerate(self.trainLoader):
                labels = loss_labels(batch, self.lossComputer.targets_mode)
                if aug0 is not None and "adc_hori" in batch:
                    # TRAINING.aug*: raw cubes take the whole plan, the mirror in front of the FFT chain included
                    loss, loss2 = self.engine.train_step_from_adc(*self._adc(batch), labels)
                else:
                    hori, vert = self._inputs(batch)
                    loss, loss2 = self.engine.train_step(hori, vert, labels)
                if blanked is not None:
                    blanked.append(self._labelled_interference(batch))
                self.logger.display(loss, loss2, batch["jointsGroup"].size(0), epoch)
                if idxBatch % self.cfg.TRAINING.lrDecayIter == 0:
                    self.adjustLR(epoch)
                loss_list.append(loss.detach())
                if getattr(self.args, "max_steps", 0) and idxBatch + 1 >= self.args.max_steps:
                    break
            if guard0 is not None:           # TRAINING.gradClip: steps of this epoch whose gradients were not finite
                skipped = self.engine.guard_stats()["skipped"] - guard0["skipped"]
                if skipped and self.rank == 0:
                    print("==========>Skipped %d optimizer step(s) with non-finite gradients in epoch %d" % (skipped, epoch))
            if mined0 is not None and self.rank == 0:
                # TRAINING.ohkm / TRAINING.jointWeights: in which share of this epoch's samples the PRGCN head kept each joint
                mined = self.engine.mining_stats()
                kept, n = mined["counts"][1] - mined0["counts"][1], mined["samples"] - mined0["samples"]
                print("==========>Mined joints in epoch %d (PRGCN head, %d of %d kept, %d samples): %s" % (
                    epoch, mined["k"], self.numKeypoints, n,
                    "  ".join("%s: %.3f" % (name, c / max(n, 1)) for name, c in zip(self.cfg.DATASET.idxToJoints, kept))))
            if coord0 is not None and self.rank == 0:
                # TRAINING.coordLoss: this epoch's mean of C_h, the weighted per-axis mean offset of each head's mass centroid from the joint
                coord = self.engine.coord_stats()
                n = coord["steps"] - coord0["steps"]
                print("==========>Coordinate loss in epoch %d: first head %.4f  PRGCN head %.4f heat-map px (weight %g, %d steps)" % (
                    epoch, (coord["sum"][0] - coord0["sum"][0]) / max(n, 1), (coord["sum"][1] - coord0["sum"][1]) / max(n, 1),
                    coord["weight"], n))
            if bone0 is not None and self.rank == 0:
                # TRAINING.boneLoss: this epoch's mean of B_h, the weighted per-axis mean error of each head's bone vectors
                bone = self.engine.bone_stats()
                n = bone["steps"] - bone0["steps"]
                print("==========>Bone loss in epoch %d: first head %.4f  PRGCN head %.4f heat-map px (weight %g, %d steps)" % (
                    epoch, (bone["sum"][0] - bone0["sum"][0]) / max(n, 1), (bone["sum"][1] - bone0["sum"][1]) / max(n, 1),
                    bone["weight"], n))
            if aug0 is not None and self.rank == 0:
                # TRAINING.aug*: what this epoch's plans drew (this rank's; the other ranks draw their own)
                st = self.engine.augment_stats()
                n = st["samples"] - aug0["samples"]
                sig = st["mean_sigma"] * st["samples"] - aug0["mean_sigma"] * aug0["samples"]
                print("==========>Augmentation in epoch %d: %d of %d samples mirrored, mean noise sigma %.4f (%d steps)" % (
                    epoch, st["mirrored"] - aug0["mirrored"], n, sig / max(n, 1), st["steps"] - aug0["steps"]))
            if blanked is not None and self.rank == 0:
                # DATASET.interference: in which share of this epoch's labelled frames the filter replaced a sample (this rank's)
                print("==========>" + interference_line("Interference in epoch %d" % epoch, blanked))
            lamb = self.engine.lamb_stats()
            if lamb is not None and self.rank == 0:
                print(trust_ratio_line(epoch, lamb, dict(self.model.named_parameters())))
            with self.engine.averaged_weights() if averaged else contextlib.nullcontext():
                accAP = self.eval(visualization=False, epoch=epoch)
            if self.rank == 0:
                self.saveModelWeight(epoch, accAP)
                self.saveLosslist(epoch, [float(l) for l in loss_list], "train")
            if getattr(self.args, "max_epochs", 0) and epoch + 1 - self.start_epoch >= self.args.max_epochs:
                break
