"""Derived copies of parameters — the packed convolution layouts, the (4C, C) concatenations of the MSCSA projection weights, the
head filter zero-padded to 16 rows — as entries of ONE pack table: persistent buffers, one entry per (parameter, kind), all refilled by
one table-driven launch (``hupr_pack_conv_weights_table``) per optimiser step instead of ~160 small launches.  ``lookup`` is the only
way in; ``functional._packed`` / ``_proj_cat`` / ``_head_w16_cached`` supply what differs (kinds, buffers, the uncached fallback).

The rules, each of which a review finding once paid for:

* Cacheable: a parameter that is a leaf, requires grad and is contiguous (the head filter also has trailing shape (32, 1, 1) —
  checked by its caller).  Anything else: ``lookup`` returns None and the caller computes the copy in place.
* Capture with grad enabled (a training graph): entries are neither read nor created — the graph's own optimiser node changes the
  weights between replays, so the copy is computed inside the graph.
* Capture under no_grad (an inference graph): a fresh entry is returned and PINNED (the graph baked its address in); a missing or
  stale one makes the caller compute inside the graph; nothing is created or refreshed mid-capture (a new buffer would live in the
  graph's private pool, a stale one means the caller skipped ``refresh``).
* An entry is stamped ``(epoch, tensor._version)``: ``invalidate`` bumps the epoch for updates made behind torch's version counter.
* A recycled address (another tensor now lives where a dead parameter did) is detected by weak-reference identity, for the
  packed layouts by a dead reference or another shape; the entry is then built anew.
* Refresh is always IN PLACE, into buffers that live as long as the parameter: captured graphs hold their addresses.
* The table pass covers the entries READ during the current or the previous epoch plus the pinned ones, not every weight the
  process ever registered (a process holding a dozen models repacked all of them after every step of one).
* An entry that dropped out (its model sat idle for two epochs of another one) is refreshed at its next read, and takes the stale
  entries of its creation epoch (~ its model) along in that one launch — not one launch per weight, not every stale entry of the
  process.  ``refresh(device, params)`` does the same for an idle model IN FRONT of the two-stream fork: a lazy refresh inside the
  fork would run on whichever stream got there first, unordered against the sibling stream's reads.
* The device table is rebuilt only when the list of live entries changes.
* The fresh hit (~160 per training step) is a dictionary lookup, a stamp compare and the touch.
* Entries of dead parameters leave the registry at every 256th table pass (and at once when a table pass meets them).
"""
import weakref

import numpy as np
import torch

from . import runtime as rt

# what the table kernel writes for an entry: both packed convolution layouts as fp32 / as bf16, or the weight's rows copied into a
# row block of a wider matrix, plain / plain into wp[0] and scaled by log2(e) into wp[1] (the query rows of the QS attention kernels)
PACK_F32, PACK_BF16, COPY, COPY_LOG2E = KINDS = (0, 1, 2, 3)

epoch = 0               # bumped by ``invalidate``; read it as ``weight_cache.epoch`` (rebound, so never ``from ... import``)
entries = {}            # (parameter address, kind) -> Entry
_table = None           # (descriptor table, block table, number of blocks, ids of the entries it describes); None: rebuild
_recent = [{}, {}]      # id(entry) -> entry: read during the current / the previous epoch
_pinned = {}            # id(entry) -> entry: read by a captured inference graph, refreshed after every update
_passes = 0


class Entry:
    """wp: the two persistent buffers the table kernel fills for this parameter; out: what ``lookup`` returns for the entry's set;
    members: the entries of that set, in the caller's order; group: the epoch of creation (~ the model)."""
    __slots__ = ("wref", "ptr", "kind", "shape", "wp", "stamp", "group", "out", "members")

    def __init__(self, w, kind, wp, out, filled):
        self.wref, self.ptr, self.kind, self.shape, self.wp, self.out = weakref.ref(w), w.data_ptr(), kind, w.shape, wp, out
        self.stamp = (epoch, w._version) if filled else None
        self.group = epoch


def invalidate():
    """Call after changing parameters behind torch's back (the fused optimisers do, and a replayed training graph)."""
    global epoch
    epoch += 1
    _recent[1] = _recent[0]
    _recent[0] = {}


def _touch(e, capturing):
    """Mark ``e`` as read in this epoch (and pin it for a capture) -> was it among the table pass's candidates already?"""
    k = id(e)
    known = k in _recent[0] or k in _recent[1] or k in _pinned
    _recent[0][k] = e
    if capturing:
        _pinned[k] = e
    return known


def lookup(ws, kinds, alloc):
    """-> the persistent buffers derived from the parameters ``ws`` (entry kinds ``kinds``), current; or None when the caller has to
    compute them in place (not cacheable, or a capture that may not use the cache).
    alloc(ws, kinds) -> (out, [(wp0, wp1) per parameter], filled): allocates the set's buffers on first use; ``filled`` says they
    hold current values already (the packed layouts: two single packs), otherwise the table pass fills them right away."""
    global _table
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing and torch.is_grad_enabled():
        return None
    for w in ws:
        if not (w.is_leaf and w.requires_grad and w.is_contiguous()):
            return None
    first = entries.get((ws[0].data_ptr(), kinds[0]))         # the set is found through its first parameter
    if first is not None and len(first.members) != len(ws):
        first = None
    fresh = first is not None
    if fresh:
        for e, w in zip(first.members, ws):
            r = e.wref()
            if (r is None or e.shape != w.shape) if e.kind <= PACK_BF16 else r is not w:      # address recycled by another tensor
                first, fresh = None, False
                break
            if e.stamp != (epoch, w._version):
                fresh = False
    if capturing:
        if not fresh:
            return None
        for e in first.members:
            _touch(e, True)
        return first.out
    created = first is None
    if created:
        out, wps, fresh = alloc(ws, kinds)
        members = tuple([Entry(w, kind, wp, out, fresh) for w, kind, wp in zip(ws, kinds, wps)])
        for e in members:
            e.members = members
            entries[(e.ptr, e.kind)] = e
        first = members[0]
        _table = None
    known = True
    for e in first.members:
        known = _touch(e, False) and known
    if not fresh:
        _refresh_all(ws[0].device, None if (known or created) else first.group)
        if first.kind <= PACK_BF16 and first.stamp != (epoch, ws[0]._version):
            # stale after a table pass (should not happen): pack singly, in place — captured graphs hold these addresses
            for dst, src in zip(first.wp, alloc(ws, kinds)[1][0]):
                dst.copy_(src)
            first.stamp = (epoch, ws[0]._version)
    return first.out


def refresh(device, params=None):
    """Run the table pass now (on the current stream) if any candidate entry on ``device`` is stale — called before the encoder
    branches fork so that the refresh is ordered in front of both, and before replaying a captured inference graph.
    params: the parameters of a model that sat idle for two or more epochs; their stale entries join the candidates first."""
    if params is not None:
        cur = _recent[0]
        for p in params:
            ptr = p.data_ptr()
            for kind in KINDS:
                e = entries.get((ptr, kind))
                if e is not None and e.wref() is p and e.stamp != (epoch, p._version):
                    cur.setdefault(id(e), e)
    for e in _candidates():
        w = e.wref()
        if w is not None and w.device == device and e.stamp != (epoch, w._version):
            _refresh_all(device)
            break


def _candidates():
    cur, prev = _recent
    return (list(cur.values()) + [e for k, e in prev.items() if k not in cur] +
            [e for k, e in _pinned.items() if k not in cur and k not in prev])


def _refresh_all(dev, group=None):
    """One table launch over the candidates on ``dev``; group: also over the stale entries created in that epoch."""
    global _table, _passes
    _passes += 1
    if group is not None:                            # a dropped-out entry came back: take the stale entries of ITS model along — those
        for e in list(entries.values()):             # created in the same epoch (a model's first forward registers all its weights)
            w = e.wref()
            if e.group == group and w is not None and w.device == dev and w.data_ptr() == e.ptr and e.stamp != (epoch, w._version):
                _recent[0].setdefault(id(e), e)
    if _passes % 256 == 0:                           # now and then: drop the entries (and buffers) of weights that are gone
        for key in [k for k, e in entries.items() if e.wref() is None]:
            del entries[key]
    live = []
    for e in _candidates():
        w = e.wref()
        if w is None:
            if entries.get((e.ptr, e.kind)) is e:
                del entries[(e.ptr, e.kind)]
            _recent[0].pop(id(e), None)
            _recent[1].pop(id(e), None)
            _pinned.pop(id(e), None)
        elif w.data_ptr() == e.ptr and w.device == dev:
            live.append((e, w))
    if not live:
        return
    ids = tuple(id(e) for e, _ in live)
    if _table is None or _table[3] != ids:
        rec = np.zeros(len(live), dtype=np.dtype([("w", "<u8"), ("wp0", "<u8"), ("wp1", "<u8"), ("first", "<i8"), ("co", "<i4"),
                                                   ("ci", "<i4"), ("taps", "<i4"), ("kind", "<i4")]))
        first = 0
        blocks = []
        for i, (e, w) in enumerate(live):
            co, ci = w.shape[0], w.shape[1]
            taps = int(np.prod(w.shape[2:]))
            rec[i] = (w.data_ptr(), e.wp[0].data_ptr(), e.wp[1].data_ptr(), first, co, ci, taps, e.kind)
            cnt = co * ci * taps
            first += cnt
            if e.kind >= COPY:
                # the weight's rows -> its row block of the wider matrices (plain, query-scaled): block layout 3
                blocks.extend((i, 3, st) for st in range(0, cnt, 2048))
            elif e.kind == PACK_BF16 and co % 32 == 0 and ci % 32 == 0 and taps <= 27:
                # 32 x 32 x taps tiles, both layouts per tile through LDS (hupr_k_pack_table, block layout 2)
                blocks.extend((i, 2, (c0 << 32) | i0) for c0 in range(0, co, 32) for i0 in range(0, ci, 32))
            else:
                for layout in (0, 1):
                    blocks.extend((i, layout, st) for st in range(0, cnt, 2048))
        blk = np.zeros(len(blocks), dtype=np.dtype([("entry", "<i4"), ("layout", "<i4"), ("start", "<i8")]))
        blk["entry"], blk["layout"], blk["start"] = zip(*blocks)
        tab = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        btab = torch.from_numpy(blk.view(np.uint8).copy()).to(dev)
        _table = (tab, btab, len(blocks), ids)
    tab, btab, n_blocks, _ = _table
    rt.check(rt.lib().hupr_pack_conv_weights_table(rt.ptr(tab), rt.ptr(btab), n_blocks, rt.stream()))
    for e, w in live:
        e.stamp = (epoch, w._version)
