"""Thin torch-tensor front-ends over the C ABI (one function per entry point).

Everything here is plumbing, and an operator states only what is its own: its argument checks,
its outputs and the arguments of its entry point.  How an entry point is called — tensors as
pointers, the workspace pair directly before the stream, the stream and the guard of one device,
the error raised on a non-zero status — is stated once, in _lib.call.  The entries that take no
stream, or their workspace first (deftet_point_in_tet_grid_dims, deftet_point_in_tet_read_stats),
are called as written out.  The reference-shaped operator surface (torch.autograd.Function /
nn.Module with the reference's names and signatures) lives in deftet_amd/layers/ and
deftet_amd/utils/.
"""
from __future__ import annotations

import collections
import ctypes
import operator
import os
import threading

import numpy as np
import torch

from . import _lib

PIT_AUTO, PIT_BRUTE, PIT_EXACT, PIT_SLAB, PIT_WAVE, PIT_PAIR = 0, 1, 2, 3, 4, 5        # include/deftet_hip.h DEFTET_PIT_*
_PIT_KERNEL = {PIT_WAVE: "k_tet_scan_wave", PIT_EXACT: "k_tet_scan", PIT_BRUTE: "k_brute", PIT_SLAB: "k_tet_scan_slab", PIT_PAIR: "k_tet_scan_pair"}
_ORDERED = (PIT_AUTO, PIT_SLAB, PIT_WAVE, PIT_PAIR)     # the algos whose traversal takes an order (PIT_AUTO resolves to one of them)


def pit_kernel_name(algo, n_tet=None, n_query=None):
    """Name of the traversal kernel an `algo` value launches (what deftet_profile_select / rocprofv3 show).  PIT_AUTO depends
    on the problem size, so n_tet and n_query are required for it (no silent default: a wrong guess selects a kernel that
    never runs, and deftet_profile_read then returns zero samples)."""
    if int(algo) == PIT_AUTO and (n_tet is None or n_query is None):
        raise ValueError("pit_kernel_name(PIT_AUTO, ...) needs n_tet and n_query: the kernel AUTO runs depends on them")
    return _PIT_KERNEL[int(_lib.load().deftet_point_in_tet_resolve_algo(int(algo), int(n_tet or 0), int(n_query or 0)))]


def _f32c(t):
    return t.contiguous().float()


def _bad_flag(check, dev):
    """the int32 [1] flag an entry sets on a bad index; None without check"""
    return torch.zeros(1, device=dev, dtype=torch.int32) if check else None


def _raise_if(bad, error, message):
    """the one read-back of a _bad_flag (a host sync; none for None): raises error(message) when the flag is set"""
    if bad is not None and int(bad.item()):
        raise error(message)


def _expected(caller, what, got):
    """the one form of an argument error: got = the offending tensor (its shape is named), or a dtype / device / text"""
    return RuntimeError("%s: %s expected (got %s)" % (caller, what, tuple(got.shape) if isinstance(got, torch.Tensor) else got))


class _LRU(collections.OrderedDict):
    """At most `maxsize` entries, the least recently used dropped first (like _TOPOLOGIES in layers/DefTet/deftet.py); every
    access holds `lock`.  An entry that leaves is retire()d: the GPU may still be writing into pinned host memory it owns, and
    torch hands a freed pinned block out again at once."""

    def __init__(self, maxsize):
        super().__init__()
        self.maxsize, self.lock = maxsize, threading.RLock()

    def lookup(self, key):
        with self.lock:
            value = self.get(key)
            if value is not None:
                self.move_to_end(key)
            return value

    def add(self, key, value):
        with self.lock:
            self[key] = value
            self.move_to_end(key)
            gone = [self.popitem(last=False)[1] for _ in range(len(self) - self.maxsize)]
        for old in gone:
            old.retire()
        return value

    def clear(self):
        with self.lock:
            gone = list(self.values())
            super().clear()
        for old in gone:
            old.retire()


# --------------------------------------------------------------------------------- A1
class PreparedQueries:
    """The query side of point_in_tet (bounding box + counting sort into grid cells) enqueued ahead
    of the tet side — typically on a second stream while the previous step's backward is running:

        with torch.cuda.stream(side):
            pq = hip_ops.prepare_queries(pts_next, n_tet)          # 4 small kernels, no tets needed
        ...
        cond, w = hip_ops.point_in_tet(tet, pts_next, want_bary=True, prepared=pq)   # waits for pq's event

    It owns its workspace and is consumed by exactly ONE point_in_tet call."""

    def __init__(self, pts, n_tet, algo):
        self.pts, self.n_tet, self.algo = pts, int(n_tet), int(algo)
        self.version = pts._version                    # the sorted copy is a snapshot: in-place updates of pts invalidate it
        self.workspace = None
        self.event = None
        self.consumed = False

    def consume(self, caller, pts, n_tet, algo):
        """The workspace for `caller`'s one call on these points, ordered after the sort on the current stream."""
        if self.consumed or self.algo != algo or self.n_tet != n_tet or self.pts.data_ptr() != pts.data_ptr() or self.pts.shape != pts.shape:
            raise RuntimeError("%s: `prepared` was made for other points / sizes / algo, or was already used" % caller)
        if self.version != pts._version:
            raise RuntimeError("%s: the points were modified in place after prepare_queries (stale sorted copy)" % caller)
        cur = torch.cuda.current_stream(pts.device)
        cur.wait_event(self.event)                     # the sort may have run on another stream
        self.workspace.record_stream(cur)
        self.consumed = True
        return self.workspace


# Query boxes tracked from call to call (query_box="track"): per (device, STREAM, B, Q) two [B,6] tensors used in turns — a call
# hands the box the PREVIOUS call measured to the library (query_box_in: the grid spans it, the measuring launch is skipped) and
# receives the box of its own queries for the next one.  A training loop draws its queries from one distribution
# (dataloader.py:108), so the previous box fits.  Where it does not, the queries outside it are answered exactly by the side
# path — at brute-force cost each, so the tracker must notice: the library counts them per shape into `misses`, an int32 [B]
# tensor in pinned host memory that the kernels write directly and the next calls read WITHOUT synchronising (the value seen
# is a few calls old when the host runs ahead of the GPU).  More than `limit` misses in a shape => the next `backoff` calls
# measure their own box again (always exact, always at full speed, one launch more), and `backoff` quadruples every time that
# happens, so a caller that alternates between two query distributions under the same (B, Q) ends up measuring; a long run of
# clean tracked calls shrinks it again.  DEFTET_PIT_BOX=off switches the tracking off.
# The stream is part of the key (round 6): call N+1 reads the box call N's k_slab_sort wrote, and only the
# order of ONE stream makes that read come after the write — two streams sharing a tracker (bench.py's pipelined path: one
# prepare on the main stream, the next on a side stream) raced, and a box that changes while k_slab_local runs gives its
# workgroups different grids.  Every workgroup of k_slab_local<true> reads the caller's box directly, so this per-stream key is
# what keeps calls on different streams from sharing one.  At most _CACHE_MAX trackers are kept.
_CACHE_MAX = 32
_box_cache = _LRU(_CACHE_MAX)


class _BoxTracker:
    def __init__(self, dev, B, Q):
        self.box = [torch.empty(B, 6, device=dev, dtype=torch.float32) for _ in range(2)]
        pin = torch.cuda.is_available()
        self.misses = torch.zeros(max(B, 1), dtype=torch.int32, pin_memory=pin)
        self._np = self.misses.numpy()                       # the same memory: polling it is a few hundred nanoseconds
        self.limit = max(4, Q >> 14)                         # misses per shape that are not worth a reaction
        self.phase, self.hold, self.backoff, self.clean = -1, 0, 1, 0
        self.counts = {"tracked": 0, "measured": 0, "backoffs": 0}

    def step(self):
        """(query_box_in | None, query_box_out, query_box_misses | None) for the next call."""
        if self.phase >= 0 and int(self._np.max()) > self.limit:
            self._np[:] = 0                                  # (a tracked call still in flight may set it again: one more back-off)
            self.hold, self.clean = self.backoff, 0
            self.backoff = min(self.backoff * 4, 1 << 20)
            self.counts["backoffs"] += 1
        if self.phase < 0 or self.hold > 0:                  # measured box, remembered in box[0] for the next tracked call
            self.hold = max(self.hold - 1, 0)
            self.phase = 0
            self.counts["measured"] += 1
            return None, self.box[0], None
        box_in, box_out = self.box[self.phase], self.box[1 - self.phase]
        self.phase = 1 - self.phase
        self.counts["tracked"] += 1
        self.clean += 1
        if self.clean >= 64 * self.backoff and self.backoff > 1:
            self.backoff, self.clean = self.backoff // 4, 0
        return box_in, box_out, self.misses

    def retire(self):
        if self.box[0].is_cuda:                              # tracked calls in flight write `misses`
            torch.cuda.synchronize(self.box[0].device)


def query_box_key(dev, B, Q):
    """Key of the tracker a query_box="track" call on `dev`'s CURRENT stream uses (see query_box_trackers)."""
    dev = torch.device(dev)
    on_gpu = dev.type == "cuda" and torch.cuda.is_available()
    idx = dev.index if dev.index is not None else (torch.cuda.current_device() if on_gpu else 0)
    return (idx, _lib.current_stream(dev) if on_gpu else 0, B, Q)


def _tracked_boxes(dev, B, Q):
    """(query_box_in | None, query_box_out, query_box_misses | None) for this call."""
    if os.environ.get("DEFTET_PIT_BOX", "track") == "off":
        return None, None, None
    # A call that is being captured into a graph measures its own box and touches no tracker: a tracked call would bake ONE
    # (box_in, box_out, misses) triple into the graph — replays would never alternate the buffers nor ever fall back to
    # measuring (the misses are only polled by eager calls), and the Python phase would no longer describe what the graph does.
    if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
        return None, None, None
    key = query_box_key(dev, B, Q)
    with _box_cache.lock:
        st = _box_cache.lookup(key) or _box_cache.add(key, _BoxTracker(dev, B, Q))
        return st.step()


def clear_query_box_cache():
    _box_cache.clear()


def query_box_trackers():
    """{(device, stream, B, Q): {"tracked", "measured", "backoffs", "hold", "backoff"}} — what query_box="track" has been doing."""
    with _box_cache.lock:
        return {k: dict(v.counts, hold=v.hold, backoff=v.backoff) for k, v in _box_cache.items()}


def _resolve_query_box(query_box, dev, B, Q, algo, misses=None):
    """query_box argument -> (query_box_in, query_box_out, query_box_misses) tensors or Nones."""
    if misses is not None and (misses.dtype != torch.int32 or misses.numel() < B or not misses.is_contiguous()):
        raise RuntimeError("query_box_misses must be a contiguous int32 tensor of at least B entries (device or pinned host memory)")
    if query_box is None or algo == PIT_BRUTE or B == 0 or Q == 0:
        return None, None, None
    if isinstance(query_box, str):
        if query_box != "track":
            raise RuntimeError("query_box must be None, 'track' or a float32 [B,6] tensor (lo xyz, hi xyz)")
        return _tracked_boxes(dev, B, Q)
    _lib.require_gpu(query_box)
    if query_box.dtype != torch.float32 or query_box.shape != (B, 6) or not query_box.is_contiguous() or query_box.device != dev:
        raise RuntimeError("query_box must be a contiguous float32 [B,6] tensor (lo xyz, hi xyz) on the queries' device")
    return query_box, None, misses


def prepare_queries(pts_bxqx3, n_tet, algo=PIT_AUTO, query_box=None, query_box_misses=None):
    _lib.require_gpu(pts_bxqx3)
    if algo == PIT_BRUTE:
        raise RuntimeError("prepare_queries needs a binned algo")
    lib = _lib.load()
    pts = _f32c(pts_bxqx3)
    if pts.dim() != 3 or pts.shape[2] != 3:
        raise RuntimeError("point_pos_bxnx3 must be [B,Q,3], got %s" % (tuple(pts.shape),))
    B, Q, dev = pts.shape[0], pts.shape[1], pts.device
    pq = PreparedQueries(pts, n_tet, algo)
    with _lib.on_device(dev):
        nbytes = max(lib.deftet_point_in_tet_workspace_bytes(B, pq.n_tet, Q, algo), 256)
        pq.workspace = torch.empty(nbytes, device=dev, dtype=torch.uint8)       # private: outlives the cached per-stream workspace
        box_in, box_out, box_miss = _resolve_query_box(query_box, dev, B, Q, algo, query_box_misses)
        _lib.call("deftet_point_in_tet_prepare_ex_f32", dev, pts, B, pq.n_tet, Q, algo, box_in, box_out, box_miss, ws=pq.workspace)
        pq.event = torch.cuda.Event()
        pq.event.record(torch.cuda.current_stream(dev))
    return pq


# An `order` indexes the tet array and the hit records: a duplicate silently skips tets, an entry outside [0, T) reads and writes
# out of bounds (ADVICE rounds 5 and 6).  A caller's order is checked once per tensor OBJECT and version, and the verdict is kept
# on the tensor itself: a view, or a new tensor the caching allocator placed where a checked one was freed, is another object
# and is checked again.  (A write that bypasses the version counter — through .data, or by a kernel — is not seen.)  The orders
# tet_spatial_order computes are permutations by construction (a stable sort of 0..T-1) and are marked without the check.
def _check_order(order, T, dev=None):
    if order.dtype != torch.int32 or order.shape != (T,) or not order.is_contiguous() or (dev is not None and order.device != dev):
        raise RuntimeError("order must be a contiguous int32 [T] tensor on the tets' device")
    if getattr(order, "_deftet_permutation", None) == order._version:
        return
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("order: a permutation must be validated by an eager call before it is used inside a graph capture")
    o = order.to(torch.int64)
    ok = T == 0 or (int(o.min()) >= 0 and int(o.max()) < T and bool((torch.bincount(o, minlength=T) == 1).all()))
    if not ok:
        raise RuntimeError("order must be a permutation of 0..T-1 (duplicates would skip tets, entries outside the range index out of bounds)")
    order._deftet_permutation = order._version


def tet_spatial_order(tet_tx4x3, want_breaks=False):
    """int32 [T] permutation that walks the tets of ONE shape column by column ((x, y) columns one mean tet extent wide,
    ascending z inside a column): the traversal order the *_ex_* entry points take (tet_order).  Static topology => computed once
    (from any positions of the grid) and reused for every step and every shape of a batch.  want_breaks also returns the
    int32 [2] device tensor (breaks of the caller's order, breaks of the computed one) the C entry point describes."""
    _lib.require_gpu(tet_tx4x3)
    lib = _lib.load()
    tet = _f32c(tet_tx4x3)
    if tet.dim() != 3 or tet.shape[1:] != (4, 3):
        raise RuntimeError("tet_tx4x3 must be [T,4,3] (one shape), got %s" % (tuple(tet.shape),))
    T, dev = tet.shape[0], tet.device
    order = torch.empty(T, device=dev, dtype=torch.int32)
    breaks = torch.zeros(2, device=dev, dtype=torch.int32)
    _lib.call("deftet_tet_spatial_order_f32", dev, tet, T, order, breaks, ws=max(lib.deftet_tet_spatial_order_workspace_bytes(T), 256))
    order._deftet_permutation = order._version                          # a permutation by construction (see _check_order)
    return (order, breaks) if want_breaks else order


def tet_order_coherence(tet_tx4x3, order=None, out=None):
    """int32 [2] = (far steps, steps looked at) of a tet numbering of ONE shape: places inside a group of 64 consecutive tets
    — of `order` when given, else of the caller's own numbering — where the next tet's centroid lies more than three mean box
    extents from the one before (include/deftet_hip.h, deftet_tet_order_coherence_f32).  What auto_tet_order decides on.
    out: an int32 tensor of >= 2 entries to write into (device memory, or pinned host memory a caller polls)."""
    _lib.require_gpu(tet_tx4x3, order)
    lib = _lib.load()
    tet = _f32c(tet_tx4x3)
    if tet.dim() != 3 or tet.shape[1:] != (4, 3):
        raise RuntimeError("tet_tx4x3 must be [T,4,3] (one shape), got %s" % (tuple(tet.shape),))
    T, dev = tet.shape[0], tet.device
    if order is not None:
        _check_order(order, T, dev)
    if out is None:
        out = torch.empty(2, device=dev, dtype=torch.int32)
    elif out.dtype != torch.int32 or out.numel() < 2 or not out.is_contiguous():
        raise RuntimeError("out must be a contiguous int32 tensor of at least 2 entries")
    _lib.call("deftet_tet_order_coherence_f32", dev, tet, T, order, out, ws=max(lib.deftet_tet_order_coherence_workspace_bytes(T), 256))
    return out


# Traversal orders chosen automatically (order="auto"), one per (device, number of tets, kernel, TOPOLOGY): decided at the first
# eager call from the numbering's COHERENCE — tet_order_coherence: the fraction of steps inside 64-tet groups that land far
# from the tet before — never from a stopwatch (round 5 timed both orders inside the operator: eight extra forwards and a
# verdict that depended on the box's noise).  The computed column order is taken when more than _FAR_LIMIT of the caller's steps
# are far AND the computed order at least halves that.  Measured (profiles/r06_order_rule.jsonl, tools/probes/order_rule_probe.py,
# order_breaks_probe.py): ONE displaced tet per wave already sends its lane to the global walk — the Kuhn list with 1 % / 4 % /
# 100 % of its positions shuffled (far fraction 0.024 / 0.082 / 0.995) runs 79 / 93 / 195 us against 64 / 66 / 98 through the
# computed order — while the Kuhn grids in any enumeration (0.005-0.007: the column ends) and the shipped QuarTet grid (0.047,
# which the computed order only brings to 0.027: its numbering walks neighbouring columns in turns) are faster as they are (the
# QuarTet grid by 13 %: a permutation costs gathers of 48-byte records, profiles/r05_scan_ab_orders.jsonl).  A stale or unlucky
# choice can never change a result.
#   topology: what identifies the tet LIST (static during training, layers/DefTet/deftet.py:65-68) — a TetTopology (its serial), any
# hashable key, or the index tensor itself (fingerprinted by content once per tensor object and version, kept on the tensor).
# Callers that only have positions (check_condition_f_base's reference signature) pass None: their entry is keyed by the sizes
# alone and is WATCHED — every _WATCH_EVERY-th call the coherence of the caller's numbering (and of the permutation in use) is
# measured asynchronously into pinned host memory and read by a later call without synchronising; when it no longer matches what
# the decision was made on (a second mesh with the same number of tets and another numbering) the entry is dropped and decided
# again.  At most _CACHE_MAX decisions are kept.  DEFTET_PIT_ORDER=off|force overrides the decision.
_FAR_LIMIT = 0.02
_WATCH_EVERY = 64
_order_cache = _LRU(_CACHE_MAX)


class _OrderEntry:
    def __init__(self, choice, fractions):
        self.choice, self.fractions = choice, fractions      # fractions: (far fraction of the caller's numbering, of the computed order) | None
        self.calls, self.mail, self.event = 0, None, None

    def retire(self):
        if self.event is not None:                           # a watch measurement in flight writes `mail`
            self.event.synchronize()


def _far_fraction(pair):
    return float(pair[0]) / max(int(pair[1]), 1)


def _decide_order(f_native, f_sorted):
    """True = traverse in the computed column order; the deterministic rule of auto_tet_order."""
    return f_native > _FAR_LIMIT and f_sorted <= 0.5 * f_native


def _topology_key(topology):
    if topology is None or isinstance(topology, (int, str, tuple)):
        return topology
    serial = getattr(topology, "serial", None)
    if serial is not None:
        return ("topology", int(serial))
    if isinstance(topology, torch.Tensor):
        fp = getattr(topology, "_deftet_fingerprint", None)
        if fp is None or fp[0] != topology._version:
            # content fingerprint (one reduction + sync, once per tensor object and version): two index lists with the same
            # content share a decision, two numberings of one mesh do not
            flat = topology.reshape(-1).to(torch.int64)
            w = (torch.arange(flat.numel(), device=flat.device, dtype=torch.int64) * 2654435761 + 40503) & 0xFFFFFFFF
            fp = (topology._version, int(((flat + 1) * w).sum().item()) & ((1 << 62) - 1), int(flat.numel()))
            topology._deftet_fingerprint = fp
        return ("tensor",) + fp[1:]
    raise RuntimeError("topology must be None, a hashable key, a TetTopology or the index tensor")


def _moved(now, then):
    return abs(now - then) > max(0.01, 0.5 * then)


def _watch_order(entry, key, tets0):
    """Position-only callers: now and then measure what is being traversed, asynchronously, and compare with what the decision
    was made on — the far-step fraction of the caller's numbering, and of the permutation in use if there is one.  Both are
    properties of the tet LIST (a training step deforms the grid by a fraction of a tet: they move in the third digit), so a
    value that moved means another list is being handed in under the same sizes: the entry is dropped and decided again.
    tets0() returns shape 0's tets."""
    entry.calls += 1
    if entry.fractions is None or entry.calls % _WATCH_EVERY or torch.cuda.is_current_stream_capturing():
        return
    if entry.mail is not None and entry.event is not None:
        if not entry.event.query():
            return                                            # the last measurement has not landed yet: look again next time
        m = entry.mail.tolist()
        stale = _moved(_far_fraction(m[0:2]), entry.fractions[0]) or (entry.choice is not None and _moved(_far_fraction(m[2:4]), entry.fractions[1]))
        if stale:
            with _order_cache.lock:
                if _order_cache.get(key) is entry:
                    del _order_cache[key]
            return
    if entry.mail is None:
        entry.mail = torch.zeros(4, dtype=torch.int32, pin_memory=True)
        entry.mail[1] = entry.mail[3] = 1
    tet0 = tets0()
    tet_order_coherence(tet0, None, out=entry.mail[0:2])
    if entry.choice is not None:
        tet_order_coherence(tet0, entry.choice, out=entry.mail[2:4])
    entry.event = torch.cuda.Event()
    entry.event.record(torch.cuda.current_stream(tet0.device))


def auto_tet_order(tet_bxtx4x3, pts_bxqx3, algo=PIT_AUTO, topology=None):
    """The cached traversal order for this grid, or None when its own numbering is coherent enough (or the grid is tiny)."""
    return _auto_order(tet_bxtx4x3.device, tet_bxtx4x3.shape[0], tet_bxtx4x3.shape[1], pts_bxqx3.shape[1], algo, topology,
                       lambda: tet_bxtx4x3[0])


def _auto_order(dev, B, T, Q, algo, topology, tets0):
    """auto_tet_order from the sizes; tets0() returns shape 0's [T,4,3] tets and is only called when they are read (a decision
    or a watch measurement), so the indexed query gathers them for that alone."""
    mode = os.environ.get("DEFTET_PIT_ORDER", "auto")
    if mode == "off" or T < 4096 or B == 0 or Q == 0:
        return None
    kernel = int(_lib.load().deftet_point_in_tet_resolve_algo(int(algo), T, Q))
    if kernel not in _ORDERED:
        return None
    tkey = _topology_key(topology)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), T, kernel, tkey)
    entry = _order_cache.lookup(key)
    if entry is not None:
        if tkey is None:
            _watch_order(entry, key, tets0)
        return entry.choice
    if torch.cuda.is_current_stream_capturing():                     # the decision reads two counters back: not inside a graph capture
        return None
    tet0 = tets0()
    order = tet_spatial_order(tet0)
    if mode == "force":
        choice, fractions = order, None
    else:
        fractions = (_far_fraction(tet_order_coherence(tet0).tolist()), _far_fraction(tet_order_coherence(tet0, order).tolist()))
        choice = order if _decide_order(*fractions) else None
    _order_cache.add(key, _OrderEntry(choice, fractions))
    return choice


def tet_order_decisions():
    """{(device, n_tet, kernel id, topology key): (chosen "sorted" | "native", (far fraction of the caller's numbering, of the
    computed order) | None)} — what auto_tet_order decided."""
    with _order_cache.lock:
        return {k: ("native" if v.choice is None else "sorted", v.fractions) for k, v in _order_cache.items()}


def clear_tet_order_cache():
    _order_cache.clear()


def _pit_begin(caller, lib, pts, T, want_bary, algo, pred_bxt, want_hits, prepared, order, query_box, query_box_misses, auto_order):
    """What point_in_tet and point_in_tet_indexed do before their one library call, on the queries' device: the outputs, the
    traversal order (order="auto" asks auto_order()), and the workspace — `prepared`'s, or the cached one with the query box.
    Returns (cond, bary, pred, occ, hits, order, workspace, (query_box_in, query_box_out, query_box_misses))."""
    B, Q, dev = pts.shape[0], pts.shape[1], pts.device
    cond = torch.empty(B, Q, 1, device=dev, dtype=torch.float32)
    bary = torch.empty(B, Q, 4, device=dev, dtype=torch.float32) if want_bary else None
    pred = _f32c(pred_bxt) if pred_bxt is not None else None
    if pred is not None and pred.shape != (B, T):
        raise RuntimeError("pred_tet_occ must be [B,T], got %s" % (tuple(pred.shape),))
    occ = torch.empty(B, Q, device=dev, dtype=torch.float32) if pred is not None else None
    hits = None
    if want_hits and algo != PIT_BRUTE:
        hits = torch.empty(max(lib.deftet_point_in_tet_hits_ints(B, T, Q), 4), device=dev, dtype=torch.int32)
    if isinstance(order, str):
        if order != "auto":
            raise RuntimeError("order must be None, 'auto' or an int32 [T] permutation")
        order = auto_order() if algo in _ORDERED else None
    if order is not None:
        _lib.require_gpu(order)
        _check_order(order, T, dev)
    if prepared is not None:
        return cond, bary, pred, occ, hits, order, prepared.consume(caller, pts, T, algo), (None, None, None)
    ws = _lib.workspace(dev, lib.deftet_point_in_tet_workspace_bytes(B, T, Q, algo))
    return cond, bary, pred, occ, hits, order, ws, _resolve_query_box(query_box, dev, B, Q, algo, query_box_misses)


def _pit_result(cond, bary, occ, hits, want_hits):
    out = (cond,) + ((bary,) if bary is not None else ()) + ((occ,) if occ is not None else ()) + ((hits,) if want_hits else ())
    return out if len(out) > 1 else cond


def point_in_tet(tet_bxtx4x3, pts_bxqx3, want_bary=False, algo=PIT_AUTO, pred_bxt=None, want_hits=False, prepared=None, order=None,
                 query_box=None, query_box_misses=None, topology=None):
    """cond f32 [B,Q,1] (lowest containing tet index or -1); with want_bary also the barycentric
    weights f32 [B,Q,4] of the hit tet; with pred_bxt also occ f32 [B,Q] = the fused
    DefTet.paste_occ gather pred[b, max(index, 0)].  Returns cond | (cond, bary) | (cond, bary, occ)
    | (cond, occ) depending on what was asked for; want_hits appends the opaque int32 hit-record
    buffer that makes point_in_tet_bwd atomic-free.  order: None (the caller's tet numbering), an int32 [T] permutation from
    tet_spatial_order (checked once per tensor), or "auto" (auto_tet_order: decided once per grid from the numbering's coherence; `topology` identifies the tet list — a
    TetTopology, any hashable key or the index tensor; None = keyed by the sizes and re-checked now and then); never changes a result.
    query_box: None (the grid spans the measured box of this call's queries), a float32 [B,6] hint (lo xyz, hi xyz: e.g. the
    sampler's box) or "track" (the box the previous call with these sizes measured, with a fall-back to measuring when the
    queries stop fitting it); never changes a result either.  query_box_misses: with a [B,6] hint, an int32 [>= B] tensor
    (device or pinned host memory) that receives the number of regular queries per shape outside the hint."""
    _lib.require_gpu(tet_bxtx4x3, pts_bxqx3, pred_bxt)
    lib = _lib.load()
    tet, pts = _f32c(tet_bxtx4x3), _f32c(pts_bxqx3)
    if tet.dim() != 4 or tet.shape[2:] != (4, 3):
        raise RuntimeError("tet_bxfx4x3 must be [B,T,4,3], got %s" % (tuple(tet.shape),))
    if pts.dim() != 3 or pts.shape[2] != 3 or pts.shape[0] != tet.shape[0]:
        raise RuntimeError("point_pos_bxnx3 must be [B,Q,3] with the same B, got %s" % (tuple(pts.shape),))
    B, T, Q = tet.shape[0], tet.shape[1], pts.shape[1]
    dev = pts.device
    with _lib.on_device(dev):
        cond, bary, pred, occ, hits, order, ws, box = _pit_begin("point_in_tet", lib, pts, T, want_bary, algo, pred_bxt, want_hits, prepared,
                                                                 order, query_box, query_box_misses,
                                                                 lambda: _auto_order(dev, B, T, Q, algo, topology, lambda: tet[0]))
        if prepared is not None:
            _lib.call("deftet_point_in_tet_scan_ex_f32", dev, tet, pts, cond, bary, pred, occ, hits, B, T, Q, algo, order, ws=ws)
        else:
            _lib.call("deftet_point_in_tet_ex_f32", dev, tet, pts, cond, bary, pred, occ, hits, B, T, Q, algo, order, *box, ws=ws)
    return _pit_result(cond, bary, occ, hits, want_hits)


def _idx32(tet_idx):
    """int32 [Bi,T,4] contiguous copy of an index list ([T,4] or [Bi,T,4]); a TetTopology hands in its own (built once)."""
    idx = tet_idx if tet_idx.dim() == 3 else tet_idx[None]
    if idx.dtype != torch.int32:
        if idx.numel() and (int(idx.min()) < -(1 << 31) or int(idx.max()) >= (1 << 31)):
            raise RuntimeError("tet_idx: index does not fit int32")
        idx = idx.to(torch.int32)
    return idx.contiguous()


# The tet-mesh argument contract of the vertex-indexed operators ("A tet mesh as an argument"), stated once:
# _topology_parts reads a topology, _mesh_args checks the mesh, _check_csr decides whether a CSR fits, _resolve_csr finds the CSR
# of a call, _csr_or_build is the slow path, _out_or_new the `out=` of the gradients that land on the vertices.
def _topology_parts(topology):
    """(tet_idx, tet_idx32, csr) of a TetTopology (layers/DefTet/deftet.py) or anything shaped like one, None for what it does not
    have; the only place that reads one"""
    return getattr(topology, "tet_idx", None), getattr(topology, "tet_idx32", None), getattr(topology, "csr", None)


def _f32_on(caller, name, t, dev, convert):
    """t as a contiguous f32 tensor once it is seen to be a tensor on dev (None: it names the device), float32 unless `convert`"""
    if not isinstance(t, torch.Tensor) or (t.dtype != torch.float32 and not convert) or (dev is not None and t.device != dev):
        raise _expected(caller, "%s as a float32 tensor%s" % (name, "" if dev is None else " on %s" % dev),
                        "%s on %s" % (t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t).__name__)
    return _f32c(t) if convert else t.contiguous()


def _mesh_args(caller, pos, tet_idx, topology=None, field=None, pts=None, convert=False):
    """(pos, idx, field, pts) of a tet mesh argument: contiguous f32 pos [B,V,3] and int32 idx [Bi,T,4] with Bi in (1, B) — the
    topology's own tet_idx32 when tet_idx is its tet_idx or tet_idx32, else a conversion of tet_idx (int32 / int64 [T,4] or
    [Bi,T,4]) — and, where given, contiguous f32 field [B,V,C >= 1] and pts [B,Q,3]; all checked against each other for rank, last
    dimension, B, V, dtype and device.  pos=None with a field: the field alone names B and V.  convert: the contract of the
    entries that came first, floats of any dtype taken to f32 and tet_idx of any dtype _idx32 converts."""
    if not isinstance(tet_idx, torch.Tensor):
        raise _expected(caller, "tet_idx as a tensor", type(tet_idx).__name__)
    _lib.require_gpu(pos, tet_idx, field, pts)
    dev = None
    if pos is not None:
        pos = _f32_on(caller, "pos", pos, dev, convert)
        if pos.dim() != 3 or pos.shape[2] != 3:
            raise _expected(caller, "pos [B,V,3]", pos)
        dev = pos.device
    if field is not None:
        field = _f32_on(caller, "field", field, dev, convert)
        if field.dim() != 3 or field.shape[2] < 1 or (pos is not None and field.shape[:2] != pos.shape[:2]):
            raise _expected(caller, "field [B,V,C] with a channel dimension of at least 1 and the B, V of pos", field)
    anchor = field if pos is None else pos                            # names B, V and the device
    if anchor is None:
        raise _expected(caller, "pos or field", None)
    B, dev = anchor.shape[0], anchor.device
    if pts is not None:
        pts = _f32_on(caller, "pts", pts, dev, convert)
        if pts.dim() != 3 or pts.shape[2] != 3 or pts.shape[0] != B:
            raise _expected(caller, "pts [%d,Q,3]" % B, pts)
    if not convert and tet_idx.dtype != torch.int32 and tet_idx.dtype != torch.int64:
        raise _expected(caller, "tet_idx int32 or int64", tet_idx.dtype)
    idx = tet_idx
    if topology is not None:
        own, own32, _ = _topology_parts(topology)
        if own32 is not None and (tet_idx is own or tet_idx is own32):
            idx = own32
    idx = _idx32(idx)
    if idx.dim() != 3 or idx.shape[2] != 4 or idx.shape[0] not in (1, B) or idx.device != dev:
        raise _expected(caller, "tet_idx [T,4] or [%d,T,4] on %s" % (B, dev), "%s on %s" % (tuple(tet_idx.shape), idx.device))
    return pos, idx, field, pts


def _check_csr(caller, csr, B, V, T, idx_batch=None, dev=None):
    """Whether csr fits a mesh of B shapes, V vertices and T tets, decided here alone: a sequence (offsets, slots, Bc) as
    tet_vertex_csr returns it, Bc in (1, B) and equal to idx_batch (the index lists of the mesh) where the entry reads the lists
    beside the CSR, slots of Bc * 4 T and offsets of Bc * V + 1 elements, both int32 tensors on dev (the operands' device).  The
    C entries dereference what they are handed, so nothing that fails here reaches one."""
    try:
        offsets, slots, Bc = csr
        ok = (slots.numel() == Bc * 4 * T and offsets.numel() == Bc * V + 1 and (Bc == 1 or Bc == B)
              and (idx_batch is None or Bc == idx_batch) and offsets.dtype == torch.int32 and slots.dtype == torch.int32
              and (dev is None or (offsets.device == dev and slots.device == dev)))
    except (TypeError, ValueError, AttributeError):                   # not a sequence of three, or not tensors
        ok = False
    if not ok:
        seen = [("%s %s on %s" % (t.dtype, tuple(t.shape), t.device)) if isinstance(t, torch.Tensor) else repr(t)
                for t in (csr if isinstance(csr, (tuple, list)) else [csr])]
        raise RuntimeError("%s: the CSR does not match the tet list: it is not tet_vertex_csr(tet_idx, %d) of %s list(s) of %d tets, int32%s "
                           "(got %s)" % (caller, V, "1 or %d" % B if idx_batch is None else idx_batch, T,
                                         "" if dev is None else " on %s" % dev, ", ".join(seen)))


def _resolve_csr(caller, csr, topology, pos, idx):
    """the CSR of a call that takes `csr=` / `topology=`: the given one, else the topology's, checked against the mesh (pos or a
    field [B,V,.], idx); None when there is neither (the slow path, _csr_or_build)"""
    if csr is None and topology is not None:
        csr = _topology_parts(topology)[2]
    if csr is not None:
        _check_csr(caller, csr, pos.shape[0], pos.shape[1], idx.shape[1], idx.shape[0], pos.device)
    return csr


def _csr_or_build(csr, idx, V):
    """csr, or THE SLOW PATH when there is none: tet_vertex_csr(idx, V) built on the spot — a sort of 4 T incidences and a host
    sync, in every backward of an operator that was handed neither `csr=` nor a `topology=`"""
    return csr if csr is not None else tet_vertex_csr(idx, V)


def _out_or_new(caller, out, shape, dev):
    """the result of a gradient on the vertices: `out` must be contiguous f32 [B,V,C] (`shape`) on dev; None: a fresh one"""
    if out is None:
        return torch.empty(*shape, device=dev, dtype=torch.float32)     # (unpacked: a shape tuple costs torch 0.8 us more)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise _expected(caller, "out contiguous f32 %s on %s" % (tuple(shape), dev), "%s %s on %s" % (out.dtype, tuple(out.shape), out.device))
    return out


def point_in_tet_indexed(pos_bxvx3, tet_idx, pts_bxqx3, want_bary=False, algo=PIT_AUTO, pred_bxt=None, want_hits=False, prepared=None,
                         order=None, query_box=None, query_box_misses=None, topology=None, check=False):
    """point_in_tet on the tets (pos_bxvx3, tet_idx) without gathering them: corner c of tet t of shape b is
    pos[b, tet_idx[b or 0, t, c]].  tet_idx: [T,4] (shared by the shapes) or [B,T,4], any integer dtype (a TetTopology's int32
    copy is used when `topology` is one).  Returns exactly what point_in_tet(tet_gather(pos, tet_idx), pts, ...) returns, bit
    for bit, including the hit records (either backward takes them).  An index outside [0, V) reads as a NaN corner, as in
    tet_gather; check=True synchronises and raises on one.  order="auto" without a topology keys the decision by tet_idx."""
    pos, idx, _, pts = _mesh_args("point_in_tet_indexed", pos_bxvx3, tet_idx, topology, pts=pts_bxqx3, convert=True)
    _lib.require_gpu(pred_bxt)
    lib = _lib.load()
    B, V, T, Q, Bi = pos.shape[0], pos.shape[1], idx.shape[1], pts.shape[1], idx.shape[0]
    dev = pts.device
    key = topology if topology is not None else tet_idx
    bad = _bad_flag(check, dev)
    with _lib.on_device(dev):
        cond, bary, pred, occ, hits, order, ws, box = _pit_begin("point_in_tet_indexed", lib, pts, T, want_bary, algo, pred_bxt, want_hits,
                                                                 prepared, order, query_box, query_box_misses,
                                                                 lambda: _auto_order(dev, B, T, Q, algo, key, lambda: tet_gather(pos[:1], idx[:1])[0]))
        if prepared is not None:
            _lib.call("deftet_point_in_tet_indexed_scan_f32", dev, pos, idx, Bi, pts, cond, bary, pred, occ, hits, B, V, T, Q, algo, order,
                      bad, ws=ws)
        else:
            _lib.call("deftet_point_in_tet_indexed_f32", dev, pos, idx, Bi, pts, cond, bary, pred, occ, hits, B, V, T, Q, algo, order,
                      *box, bad, ws=ws)
    _raise_if(bad, RuntimeError, "point_in_tet_indexed: index out of range [0, %d)" % V)
    return _pit_result(cond, bary, occ, hits, want_hits)


def point_in_tet_grid(n_tet, n_query):
    """(y/z cells per axis, x cells) of the query grid the binned algos build for this problem size."""
    g, gx = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().deftet_point_in_tet_grid_dims(int(n_tet), int(n_query), ctypes.byref(g), ctypes.byref(gx)), "deftet_point_in_tet_grid_dims")
    return g.value, gx.value


def point_in_tet_stats(B, T, Q, algo, device):
    """Diagnostics of the LAST un-prepared point_in_tet call on this device/stream (it shares the cached workspace):
    int32 [B,8] = irregular tets, irregular queries, record-overflow flag, 0, 0, tets re-scanned exactly, overflowed tets, 0."""
    lib = _lib.load()
    dev = torch.device(device)
    out = np.zeros((B, 8), np.int32)
    with _lib.on_device(dev):
        ws = _lib.workspace(dev, lib.deftet_point_in_tet_workspace_bytes(B, T, Q, algo))
        _lib.check(lib.deftet_point_in_tet_read_stats(_lib.ptr(ws), ws.numel(), B, T, Q, algo, out.ctypes.data, _lib.current_stream(dev)),
                   "deftet_point_in_tet_read_stats")
    return out


def bwd_uses_records(n_tet, n_query):
    """Whether point_in_tet_bwd reads the forward's hit records for this size.  They are for the sparse case (BASELINE: 0.4 to 1
    query per tet); above 2 queries per tet the library takes per-tet lists whatever it is handed (include/deftet_hip.h,
    deftet_point_in_tet_bwd_f32), so a caller need not ask the forward for records there."""
    return int(n_query) <= 2 * int(n_tet)


def point_in_tet_bwd(tet_bxtx4x3, pts_bxqx3, cond, grad_w, want_grad_pts=False, grad_occ=None, hits=None):
    """(grad_tet [B,T,4,3], grad_pts [B,Q,3] | None) and, when grad_occ [B,Q] is given, also
    grad_pred [B,T] (fused paste_occ backward).  `hits` = the forward's hit-record buffer (same
    tet/pts/cond): selects the atomic-free path; without it per-tet linked lists are built."""
    _lib.require_gpu(tet_bxtx4x3, pts_bxqx3, cond, grad_w, grad_occ)
    lib = _lib.load()
    tet, pts, cond, gw = _f32c(tet_bxtx4x3), _f32c(pts_bxqx3), _f32c(cond), _f32c(grad_w)
    B, T, Q = tet.shape[0], tet.shape[1], pts.shape[1]
    dev = pts.device
    grad_tet = torch.empty_like(tet)
    grad_pts = torch.empty_like(pts) if want_grad_pts else None
    go = _f32c(grad_occ) if grad_occ is not None else None
    grad_pred = torch.empty(B, T, device=dev, dtype=torch.float32) if go is not None else None
    _lib.call("deftet_point_in_tet_bwd_f32", dev, tet, pts, cond, gw, grad_tet, grad_pts, go, grad_pred, hits, B, T, Q, 0,
              ws=lib.deftet_point_in_tet_bwd_workspace_bytes(B, T, Q))
    if go is not None:
        return grad_tet, grad_pts, grad_pred
    return grad_tet, grad_pts


def _to_vertices_begin(caller, csr, Bi, B, V, T, pts, want_grad_pts, grad_occ, out):
    """The checks, outputs and workspace size of the two *_bwd_to_vertices, on the queries' device (Bi: the index lists the tets
    come from, None = the CSR's).  Returns (offsets, slots, Bi, grad_pos, grad_pts, grad_occ as f32, grad_pred, workspace bytes)."""
    dev = pts.device
    _check_csr(caller, csr, B, V, T, Bi, dev)
    offsets, slots, Bc = csr
    grad_pos = _out_or_new(caller, out, (B, V, 3), dev)
    grad_pts = torch.empty_like(pts) if want_grad_pts else None
    go = _f32c(grad_occ) if grad_occ is not None else None
    # (`accumulate` of the C entry covers grad_pos AND grad_pred: a fresh grad_pred must then start from zero)
    grad_pred = (torch.zeros if out is not None else torch.empty)(B, T, device=dev, dtype=torch.float32) if go is not None else None
    return offsets, slots, Bc, grad_pos, grad_pts, go, grad_pred, _lib.load().deftet_point_in_tet_bwd_to_vertices_workspace_bytes(B, T, pts.shape[1])


def point_in_tet_bwd_to_vertices(tet_bxtx4x3, pts_bxqx3, cond, grad_w, csr, n_vertex, want_grad_pts=False, grad_occ=None, hits=None,
                                 out=None):
    """(grad_pos [B,V,3], grad_pts [B,Q,3] | None[, grad_pred [B,T]]): point_in_tet_bwd followed by tet_gather_bwd in one call
    that never writes the dense grad_tet — the gradient of a caller that owns both the gather (layers/DefTet/deftet.py:65-68)
    and the query.  csr = tet_vertex_csr(...) of the topology the tets were gathered with; bit-identical to the two-call form.
    out: existing [B,V,3] tensor to ADD to."""
    _lib.require_gpu(tet_bxtx4x3, pts_bxqx3, cond, grad_w, grad_occ)
    tet, pts, cond, gw = _f32c(tet_bxtx4x3), _f32c(pts_bxqx3), _f32c(cond), _f32c(grad_w)
    B, T, Q, V = tet.shape[0], tet.shape[1], pts.shape[1], int(n_vertex)
    offsets, slots, Bi, grad_pos, grad_pts, go, grad_pred, nbytes = _to_vertices_begin("point_in_tet_bwd_to_vertices", csr, None, B, V, T, pts,
                                                                                       want_grad_pts, grad_occ, out)
    _lib.call("deftet_point_in_tet_bwd_to_vertices_f32", pts.device, tet, pts, cond, gw, go, hits, offsets, slots, Bi, grad_pos, grad_pts,
              grad_pred, B, V, T, Q, 1 if out is not None else 0, ws=nbytes)
    return (grad_pos, grad_pts) if grad_pred is None else (grad_pos, grad_pts, grad_pred)


def point_in_tet_indexed_bwd_to_vertices(pos, tet_idx, pts, cond, grad_w, csr, want_grad_pts=False, grad_occ=None, hits=None, out=None):
    """point_in_tet_bwd_to_vertices for the indexed forward: the tets are read from (pos, tet_idx) instead of a gathered tensor.
    csr = tet_vertex_csr(tet_idx, V) of the same list (same idx_batch).  Returns and `out=` as point_in_tet_bwd_to_vertices, bit
    for bit the same values on the same inputs; hits from either forward."""
    pos, idx, _, pts = _mesh_args("point_in_tet_indexed_bwd_to_vertices", pos, tet_idx, pts=pts, convert=True)
    _lib.require_gpu(cond, grad_w, grad_occ)
    cond, gw = _f32c(cond), _f32c(grad_w)
    B, V, T, Q, Bi = pos.shape[0], pos.shape[1], idx.shape[1], pts.shape[1], idx.shape[0]
    offsets, slots, _, grad_pos, grad_pts, go, grad_pred, nbytes = _to_vertices_begin("point_in_tet_indexed_bwd_to_vertices", csr, Bi, B, V, T,
                                                                                      pts, want_grad_pts, grad_occ, out)
    _lib.call("deftet_point_in_tet_indexed_bwd_to_vertices_f32", pts.device, pos, idx, Bi, pts, cond, gw, go, hits, offsets, slots, grad_pos,
              grad_pts, grad_pred, B, V, T, Q, 1 if out is not None else 0, ws=nbytes)
    return (grad_pos, grad_pts) if grad_pred is None else (grad_pos, grad_pts, grad_pred)


def paste_occ_fwd(pred_bxt, cond_bxqx1, clamp_inplace=True):
    _lib.require_gpu(pred_bxt, cond_bxqx1)
    pred = _f32c(pred_bxt)
    if not (cond_bxqx1.is_contiguous() and cond_bxqx1.dtype == torch.float32):
        raise RuntimeError("condition must be a contiguous float32 tensor (it is clamped in place)")
    B, T = pred.shape
    Q = cond_bxqx1.shape[1]
    out = torch.empty(B, Q, device=pred.device, dtype=torch.float32)
    _lib.call("deftet_paste_occ_fwd_f32", pred.device, pred, cond_bxqx1, out, B, T, Q, int(clamp_inplace))
    return out


def paste_occ_bwd(cond_bxqx1, grad_out_bxq, n_tet):
    _lib.require_gpu(cond_bxqx1, grad_out_bxq)
    cond, go = _f32c(cond_bxqx1), _f32c(grad_out_bxq)
    B, Q = go.shape
    gp = torch.empty(B, n_tet, device=go.device, dtype=torch.float32)
    _lib.call("deftet_paste_occ_bwd_f32", go.device, cond, go, gp, B, n_tet, Q, 1)
    return gp


def radix_sort(keys, values=None, bits=None, n_valid=None):
    """Stable ascending sort with the library's own LSD radix sort (csrc/prims.hpp).  keys: int32/int64 tensor of
    NON-NEGATIVE integers (sorted as unsigned on their low `bits` bits; default all bits); values: optional int32/int64/
    float32 tensor of the same length carried along.  n_valid: optional int32 device tensor with the number of elements
    that really exist.  Returns (sorted_keys, sorted_values or None)."""
    _lib.require_gpu(keys, values, n_valid)
    if n_valid is not None and (n_valid.dtype != torch.int32 or n_valid.device != keys.device or n_valid.numel() < 1):
        raise RuntimeError("radix_sort: n_valid must be an int32 tensor on the keys' device")
    lib = _lib.load()
    k = keys.contiguous()
    if k.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("radix_sort: keys must be int32 or int64")
    kb = k.element_size()
    n = k.numel()
    v = values.contiguous() if values is not None else None
    vb = v.element_size() if v is not None else 0
    if v is not None and (v.numel() != n or vb not in (4, 8)):
        raise RuntimeError("radix_sort: values must have the keys' length and 4- or 8-byte elements")
    ko = torch.empty_like(k)
    vo = torch.empty_like(v) if v is not None else None
    _lib.call("deftet_radix_sort", k.device, k, ko, v, vo, n, kb, vb, int(bits or kb * 8), n_valid,
              ws=lib.deftet_radix_sort_workspace_bytes(n, kb, vb))
    return ko, vo


def scan(x, kind="exclusive"):
    """Prefix scan of a 1-D int32/int64 tensor: "exclusive" / "inclusive" sums or the inclusive running "max"."""
    _lib.require_gpu(x)
    lib = _lib.load()
    t = x.contiguous()
    if t.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("scan: int32 or int64")
    out = torch.empty_like(t)
    _lib.call("deftet_scan", t.device, t, out, t.numel(), t.element_size(), {"exclusive": 0, "inclusive": 1, "max": 2}[kind],
              ws=lib.deftet_scan_workspace_bytes(t.numel(), t.element_size()))
    return out


def rowdot(a, b=None, a2=None, b2=None):
    """out[r] = sum over the trailing dims of a[r]*b[r] (row sums when b is None), plus the same
    for the optional second pair (a2, b2) of its own width, in one launch pair; f32 [R]."""
    _lib.require_gpu(a, b, a2, b2)
    lib = _lib.load()
    a = _f32c(a)
    b = _f32c(b) if b is not None else None
    if b is not None and b.shape != a.shape:
        raise RuntimeError("rowdot: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    R = a.shape[0]
    n2 = 0
    if a2 is not None:
        a2 = _f32c(a2)
        b2 = _f32c(b2) if b2 is not None else None
        if a2.shape[0] != R or (b2 is not None and b2.shape != a2.shape):
            raise RuntimeError("rowdot: second pair shape mismatch")
        n2 = a2.numel() // max(R, 1)
    elif b2 is not None:
        raise RuntimeError("rowdot: b2 without a2")
    out = torch.empty(R, device=a.device, dtype=torch.float32)
    _lib.call("deftet_rowdot2_f32", a.device, a, b, a.numel() // max(R, 1), a2, b2, n2, out, R, ws=lib.deftet_rowdot_workspace_bytes(R))
    return out


class _SqrtRowSum(torch.autograd.Function):
    """out[r] = sum over the trailing dims of sqrt(x[r] + eps): one launch forward, one backward."""

    @staticmethod
    def forward(ctx, x, eps):
        _lib.require_gpu(x)
        lib = _lib.load()
        x = _f32c(x)
        R = x.shape[0]
        if R > 1024:
            raise RuntimeError("sqrt_rowsum: at most 1024 rows, got %d" % R)
        ctx.save_for_backward(x)
        ctx.eps = float(eps)
        if x.numel() == 0:
            return torch.zeros(R, device=x.device, dtype=torch.float32)
        out = torch.empty(R, device=x.device, dtype=torch.float32)
        _lib.call("deftet_sqrt_rowsum_f32", x.device, x, float(eps), out, R, x.numel() // max(R, 1), ws=lib.deftet_rowdot_workspace_bytes(R))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        g = _f32c(grad_out)
        gx = torch.empty_like(x)
        if x.numel() == 0:
            return gx, None
        R = x.shape[0]
        _lib.call("deftet_sqrt_rowsum_bwd_f32", x.device, x, ctx.eps, g, gx, R, x.numel() // max(R, 1))
        return gx, None


def sqrt_rowsum(x, eps):
    """[R] sums of sqrt(x + eps) over everything but the first dimension (differentiable): the tail of the reference's
    point-to-surface term, `sqrt(d^2 + 1e-10)` then the mean over the points (utils/mesh_utils.py:14)."""
    return _SqrtRowSum.apply(x, eps)


# --------------------------------------------------------------------------------- A2-A6 builders
def _i32_tets(tet_list, device):
    t = torch.as_tensor(tet_list)
    if t.dim() != 2 or t.shape[1] != 4:
        raise RuntimeError("tet_list must be [T,4], got %s" % (tuple(t.shape),))
    return t.to(device=device, dtype=torch.int32).contiguous()


def _builder_bytes(n_point, n_tet):
    return _lib.load().deftet_builder_workspace_bytes(int(n_point), int(n_tet))


def tet_adj_share(tet_list, n_point, device):
    """int32 rows [2*n_shared, 3] = [t0,t1,f0],[t1,t0,f1] in ascending face-key order
    (utils/lib/tet_adj_share/run.cpp:40-97)."""
    dev = torch.device(device)
    tet = _i32_tets(tet_list, dev)
    _lib.require_gpu(tet)
    T = tet.shape[0]
    out = torch.empty(max(T * 8, 1), 3, dtype=torch.int32, device=dev)
    n = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("deftet_tet_adj_share_i32", dev, tet, out, n, int(n_point), T, ws=_builder_bytes(n_point, T))
    return out[: int(n.item()) * 2]


def tet_face_adj(tet_list, n_point, device, wrap32=True):
    """int32 rows [n,2] = [fa,fb] (utils/lib/tet_face_adj/run.cpp:18-92); two-phase: count, then fill."""
    dev = torch.device(device)
    tet = _i32_tets(tet_list, dev)
    _lib.require_gpu(tet)
    T = tet.shape[0]
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    nbytes = _builder_bytes(n_point, T)
    _lib.call("deftet_tet_face_adj_i32", dev, tet, None, 0, n, int(n_point), T, int(wrap32), ws=nbytes, what="deftet_tet_face_adj_i32(count)")
    cnt = int(n.item())
    out = torch.empty(max(cnt, 1), 2, dtype=torch.int32, device=dev)
    _lib.call("deftet_tet_face_adj_i32", dev, tet, out, cnt, n, int(n_point), T, int(wrap32), ws=nbytes, what="deftet_tet_face_adj_i32(fill)")
    return out[:cnt]


def tet_point_adj(tet_list, n_point, device):
    """int32 [n,2] unique directed vertex pairs sorted by (a,b) (utils/lib/tet_point_adj/run.cpp:20-56)."""
    dev = torch.device(device)
    tet = _i32_tets(tet_list, dev)
    _lib.require_gpu(tet)
    T = tet.shape[0]
    out = torch.empty(max(T * 12, 1), 2, dtype=torch.int32, device=dev)
    n = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("deftet_tet_point_adj_i32", dev, tet, out, n, int(n_point), T, ws=_builder_bytes(n_point, T))
    return out[: int(n.item())]


def colaps_v(points_nx3):
    """(map_array int32 [N], inverse_idx int32 [k]) — utils/lib/colaps_v/run.cpp:39-59."""
    _lib.require_gpu(points_nx3)
    pts = _f32c(points_nx3)
    N = pts.shape[0]
    dev = pts.device
    m = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    inv = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    n = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("deftet_colaps_v_f32", dev, pts, m, inv, n, N, ws=_builder_bytes(N, 0))
    return m[:N], inv[: int(n.item())]


def tet_to_face(tet_list, n_point, device, with_boundary=False):
    """(face_fx3, tetidx_fx2, tetfaceidx_fx2, boundary_fx3) int64, first-seen order —
    utils/tet_utils.py:208-256 / prepare_for_wz.py:49-104; raises on non-manifold input."""
    dev = torch.device(device)
    tet = _i32_tets(tet_list, dev)
    _lib.require_gpu(tet)
    T = tet.shape[0]
    cap = max(T * 4, 1)
    f3 = torch.empty(cap, 3, dtype=torch.int64, device=dev)
    t2 = torch.empty(cap, 2, dtype=torch.int64, device=dev)
    tf2 = torch.empty(cap, 2, dtype=torch.int64, device=dev)
    b3 = torch.empty(cap, 3, dtype=torch.int64, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    _lib.call("deftet_tet_to_face_i32", dev, tet, f3, t2, tf2, b3, counts, int(n_point), T, int(with_boundary), ws=_builder_bytes(n_point, T))
    nf, nb, nm = (int(x) for x in counts.tolist())
    return f3[:nf], t2[:nf], tf2[:nf], b3[:nb], nm


def tet_neighbours(tet_list, n_point, device, want_face_owners=False):
    """tet_neighbour_idx int64 [T,4] (-1 padded) — the T x 4 table utils_tetsv.tet_adj_share returns
    (diff_render/diftet_6_subdiv/3_model/utils_tetsv.py:16-75) — and, with want_face_owners, also the
    [4T,2] owner table of utils/tet_utils.py:259-300 (tet_to_face_withtet).  Raises ValueError when a face
    has more than two owners, as both reference functions do."""
    lib = _lib.load()
    dev = torch.device(device)
    f3, t2, tf2, _b3, n_multi = tet_to_face(tet_list, n_point, dev, with_boundary=True)
    if n_multi:
        raise ValueError("%d faces are shared by more than two tetrahedra" % n_multi)
    T = int(torch.as_tensor(tet_list).shape[0])
    nbr = torch.empty(T, 4, dtype=torch.int64, device=dev)
    owners = torch.empty(T * 4, 2, dtype=torch.int64, device=dev) if want_face_owners else None
    _lib.call("deftet_tet_neighbours_i64", dev, t2, tf2, int(t2.shape[0]), T, nbr, owners, ws=lib.deftet_tet_neighbours_workspace_bytes(T))
    return (nbr, owners) if want_face_owners else nbr


# --------------------------------------------------------------------------------- A8 / A9 / A10 surface ops
def face_edge_adj(face_fx3x3, n_max_nei=30, brute=False):
    """f32 [F, n_max_nei] neighbour table (-1 padded): tet_face_adj_m_for.cu:72-108.
    brute=True selects the O(F^2) scalar-stream kernel (kept for cross-checks)."""
    _lib.require_gpu(face_fx3x3)
    lib = _lib.load()
    face = _f32c(face_fx3x3)
    F = face.shape[0]
    adj = torch.full((F, n_max_nei), -1.0, device=face.device, dtype=torch.float32)    # utils.py:47
    _lib.call("deftet_face_edge_adj_f32", face.device, face, adj, F, n_max_nei,
              ws=None if brute else lib.deftet_face_edge_adj_workspace_bytes(F))
    return adj


def host_ints(values, device, i32=False, i64=False, f32=False):
    """Device tensors holding a few HOST integers (per-shape counts, offsets), one per requested dtype, in the order
    (int32, int64, float32).  The values travel in a kernel's argument block (deftet_put_host_ints): no copy from pageable
    host memory — torch.tensor(list, device=...) blocks the Python thread until the stream has drained — and one launch for
    all dtypes."""
    vals = [int(v) for v in values]
    n = len(vals)
    outs = [torch.empty(n, device=device, dtype=dt) if want else None
            for want, dt in ((i32, torch.int32), (i64, torch.int64), (f32, torch.float32))]
    if n and any(o is not None for o in outs):
        _lib.call("deftet_put_host_ints", torch.device(device), (ctypes.c_longlong * n)(*vals), n, *outs)
    got = tuple(o for o in outs if o is not None)
    return got[0] if len(got) == 1 else got


def _host_counts(counts, B, hi, what):
    c =[int(x) for x in counts]
    if len(c) != B or any(x < 0 or x > hi for x in c):
        raise RuntimeError("%s: need %d counts in [0, %d], got %s" % (what, B, hi, c))
    return (ctypes.c_int * B)(*c)


def face_edge_adj_ragged(face_bxfx3x3, n_face, n_max_nei=30, brute=False):
    """A8 for a batch of surfaces with different face counts: f32 [B, F_max, n_max_nei] (-1 padded), `n_face` = B host
    integers.  One launch sequence for the whole batch."""
    _lib.require_gpu(face_bxfx3x3)
    lib = _lib.load()
    face = _f32c(face_bxfx3x3)
    B, F = face.shape[0], face.shape[1]
    cnt = _host_counts(n_face, B, F, "face_edge_adj_ragged")
    adj = torch.full((B, F, n_max_nei), -1.0, device=face.device, dtype=torch.float32)
    _lib.call("deftet_face_edge_adj_ragged_f32", face.device, face, adj, B, F, cnt, n_max_nei,
              ws=None if brute else lib.deftet_face_edge_adj_ragged_workspace_bytes(B, F))
    return adj


def nn_index_ragged(queries_bxnx3, points_bxmx3, n_query, brute=False):
    """A10 with a per-shape query count (`n_query` = B host integers <= N): int32 [B,N], rows beyond the count stay 0."""
    _lib.require_gpu(queries_bxnx3, points_bxmx3)
    lib = _lib.load()
    q, p = _f32c(queries_bxnx3), _f32c(points_bxmx3)
    B, N, M = q.shape[0], q.shape[1], p.shape[1]
    cnt = _host_counts(n_query, B, N, "nn_index_ragged")
    out = torch.zeros(B, N, device=q.device, dtype=torch.int32)
    _lib.call("deftet_nn_index_ragged_f32", q.device, q, p, out, B, N, M, cnt, ws=None if brute else lib.deftet_nn_index_workspace_bytes(B, N, M))
    return out


class _ChamferToCloud(torch.autograd.Function):
    """sum over the valid samples of sqrt(|sample - NN_gt(sample)|^2 + 1e-10), per shape; samples = per_face area-uniform
    random points per face.  Gradient to `tri` only (the cloud is data)."""

    @staticmethod
    def forward(ctx, tri, gt, counts, per_face, generator, uv=None):
        B, F, M, K = tri.shape[0], tri.shape[1], gt.shape[1], int(per_face)
        dev = tri.device
        # uv (optional, tests): the two uniform numbers per sample drawn by the caller instead of here
        r = torch.rand(2, B, F, K, device=dev, generator=generator) if uv is None else _f32c(uv).reshape(2, B, F, K)
        samples = torch.empty(B, F * K, 3, device=dev, dtype=torch.float32)
        _lib.call("deftet_face_samples_f32", dev, tri, r, samples, B, F, K)
        n_valid = [int(c) * K for c in counts]
        idx = nn_index_ragged(samples, gt, n_valid)
        nv = host_ints(n_valid, dev, i32=True)                        # (not torch.tensor(..., device=dev): that copy blocks until the stream drains)
        d = torch.empty(B, F * K, device=dev, dtype=torch.float32)
        _lib.call("deftet_chamfer_fwd_f32", dev, samples, gt, idx, nv, d, B, F * K, M)
        ctx.save_for_backward(samples, gt, idx, nv, d, r)
        ctx.dims = (B, F, K, M)
        return rowdot(d)

    @staticmethod
    def backward(ctx, grad_sum):
        samples, gt, idx, nv, d, r = ctx.saved_tensors
        B, F, K, M = ctx.dims
        g = _f32c(grad_sum)
        grad_tri = torch.empty(B, F, 3, 3, device=samples.device, dtype=torch.float32)
        _lib.call("deftet_chamfer_bwd_f32", samples.device, samples, gt, idx, nv, d, r, g, grad_tri, B, F, K, M)
        return grad_tri, None, None, None, None, None


def chamfer_to_cloud(tri_bxfx3x3, gt_bxmx3, counts, per_face=20, generator=None, uv=None):
    """f32 [B]: SUM over shape b's first counts[b] * per_face samples (per_face random points on each of its first
    counts[b] faces) of their distance to the nearest ground-truth point — differentiable w.r.t. tri."""
    _lib.require_gpu(tri_bxfx3x3, gt_bxmx3)
    if gt_bxmx3.shape[1] == 0:
        raise RuntimeError("chamfer_to_cloud: the ground-truth cloud is empty (no nearest neighbour exists)")
    if len(counts) != tri_bxfx3x3.shape[0] or any(int(c) < 0 or int(c) > tri_bxfx3x3.shape[1] for c in counts):
        raise RuntimeError("chamfer_to_cloud: counts must hold one face count in [0, F] per shape")
    # (cast outside the autograd.Function, so that a non-f32 `tri` gets its gradient in its own dtype through the cast)
    return _ChamferToCloud.apply(_f32c(tri_bxfx3x3), _f32c(gt_bxmx3), counts, per_face, generator, uv)


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tri, adj, n_face):
        B, F, K = tri.shape[0], tri.shape[1], adj.shape[2]
        loss = torch.empty(B, device=tri.device, dtype=torch.float32)
        nrm = torch.empty(B, F, 3, device=tri.device, dtype=torch.float32)
        cnt = torch.empty(B, device=tri.device, dtype=torch.float32)
        _lib.call("deftet_normal_consistency_fwd_f32", tri.device, tri, adj, n_face, loss, nrm, cnt, B, F, K)
        ctx.save_for_backward(tri, adj, n_face, nrm, cnt)
        return loss

    @staticmethod
    def backward(ctx, g):
        tri, adj, n_face, nrm, cnt = ctx.saved_tensors
        B, F, K = tri.shape[0], tri.shape[1], adj.shape[2]
        gtri = torch.empty_like(tri)
        acc = torch.empty(B, F, 3, device=tri.device, dtype=torch.float32)
        _lib.call("deftet_normal_consistency_bwd_f32", tri.device, tri, adj, n_face, nrm, cnt, _f32c(g), gtri, acc, B, F, K)
        return gtri, None, None


def normal_consistency(tri_bxfx3x3, adj_bxfxm, n_face_dev):
    """loss f32 [B] = mean over the valid entries of the A8 table of 1 - <n_i, n_j> (unit normals with the 1e-12 guard of
    utils/mesh_utils.py:50-51), differentiable w.r.t. the triangle corners; n_face_dev int32 [B] on the device."""
    _lib.require_gpu(tri_bxfx3x3, adj_bxfxm, n_face_dev)
    return _NormalConsistency.apply(_f32c(tri_bxfx3x3), _f32c(adj_bxfxm), n_face_dev.to(torch.int32).contiguous())


def tri_dist_fwd(pts_bxpx3, face_bxfx3x3, n_face_b, brute=False, want_order=False):
    """(closest_d, closest_f) f32 [B,P,1] — tet_analytic_distance_for.cu:256-307.
    brute=True selects the streaming scan over all faces (kept for cross-checks).
    want_order=True also returns the int32 [B,P] order in which the grid search walked the points (None when the grid
    search did not run: brute, or no faces) — `tri_dist_bwd(order=...)` groups its atomics with it."""
    _lib.require_gpu(pts_bxpx3, face_bxfx3x3, n_face_b)
    lib = _lib.load()
    pts, face, nfb = _f32c(pts_bxpx3), _f32c(face_bxfx3x3), _f32c(n_face_b)
    B, P = pts.shape[0], pts.shape[1]
    d = torch.zeros(B, P, 1, device=pts.device, dtype=torch.float32)                    # utils.py:44-45
    f = torch.zeros(B, P, 1, device=pts.device, dtype=torch.float32)
    order = None
    if want_order and not brute and face.shape[1] > 0 and B * P > 0:
        order = torch.empty(B, P, device=pts.device, dtype=torch.int32)
    _lib.call("deftet_tri_dist_fwd_order_f32", pts.device, pts, face, nfb, d, f, order, B, P, face.shape[1],
              ws=None if brute else lib.deftet_tri_dist_workspace_bytes(B, P, face.shape[1]))
    return (d, f, order) if want_order else (d, f)


def tri_dist_bwd(pts_bxpx3, face_bxfx3x3, closest_f, dl_dd, deterministic=False, order=None):
    """dL/dface f32 [B,F,3,3] — tet_analytic_distance_back.cu:591-715.  order: the forward's point order (see
    tri_dist_fwd); with it the atomic path adds up a wavefront's contributions per distinct face first."""
    _lib.require_gpu(pts_bxpx3, face_bxfx3x3, closest_f, dl_dd)
    pts, face, cf, g = _f32c(pts_bxpx3), _f32c(face_bxfx3x3), _f32c(closest_f), _f32c(dl_dd)
    B, P, F = pts.shape[0], pts.shape[1], face.shape[1]
    out = torch.zeros(B, F, 3, 3, device=pts.device, dtype=torch.float32)               # utils.py:65
    if order is not None and not deterministic:
        _lib.call("deftet_tri_dist_bwd_order_f32", pts.device, pts, face, cf, g, order.contiguous(), out, B, P, F)
    else:
        _lib.call("deftet_tri_dist_bwd_f32", pts.device, pts, face, cf, g, out, B, P, F, int(deterministic))
    return out


def nn_index(queries_bxnx3, points_bxmx3, brute=False):
    """int32 [B,N] index of the first strictly-nearest point (nearest_neighbor_cuda.cu:17-55).
    brute=True selects the O(N*M) scalar-stream kernel (kept for cross-checks)."""
    _lib.require_gpu(queries_bxnx3, points_bxmx3)
    lib = _lib.load()
    q, p = _f32c(queries_bxnx3), _f32c(points_bxmx3)
    B, N, M = q.shape[0], q.shape[1], p.shape[1]
    out = torch.zeros(B, N, device=q.device, dtype=torch.int32)                         # nearest_neighbor.py:32-33
    _lib.call("deftet_nn_index_f32", q.device, q, p, out, B, N, M, ws=None if brute else lib.deftet_nn_index_workspace_bytes(B, N, M))
    return out


# --------------------------------------------------------------------------------- N1 check_sign
def check_sign(verts_bxvx3, faces_fx3, points_bxnx3, brute=False, return_count=False, check=True):
    """bool [B,N]: point inside the (watertight) mesh — kal.ops.mesh.check_sign restated
    (parity unpinned, contract in oracle/deftet_oracle_sign.c)."""
    _lib.require_gpu(verts_bxvx3, faces_fx3, points_bxnx3)
    lib = _lib.load()
    v, p = _f32c(verts_bxvx3), _f32c(points_bxnx3)
    f = faces_fx3.long().contiguous()
    if v.dim() != 3 or p.dim() != 3 or f.dim() != 2 or f.shape[1] != 3 or v.shape[0] != p.shape[0] or v.shape[2] != 3 or p.shape[2] != 3:
        raise RuntimeError("check_sign: verts [B,V,3], faces [F,3], points [B,N,3] expected")
    B, V, N, F, dev = v.shape[0], v.shape[1], p.shape[1], f.shape[0], v.device
    out = torch.empty(B, N, device=dev, dtype=torch.uint8)
    cnt = torch.empty(B, N, device=dev, dtype=torch.int32) if return_count else None
    bad = torch.zeros(1, device=dev, dtype=torch.int32)
    algo = 1 if brute else 0
    _lib.call("deftet_check_sign_f32", dev, v, f, p, out, cnt, bad, B, V, F, N, algo, ws=lib.deftet_check_sign_workspace_bytes(B, F, algo))
    if check and int(bad.item()):
        raise IndexError("check_sign: face index outside [0, %d)" % V)
    inside = out.view(torch.bool)                            # 0 / 1 bytes: a reinterpretation, not a conversion launch
    return (inside, cnt) if return_count else inside


def check_sign_ragged(verts_list, faces_list, points_bxnx3, brute=False, return_count=False, check=False):
    """check_sign for a different mesh per shape in ONE launch sequence: verts_list[b] f32 [V_b,3] (or
    [1,V_b,3]), faces_list[b] int [F_b,3] with indices local to mesh b, points [B,N,3] -> bool [B,N]."""
    _lib.require_gpu(points_bxnx3, *verts_list, *faces_list)
    lib = _lib.load()
    p = _f32c(points_bxnx3)
    B, N, dev = p.shape[0], p.shape[1], p.device
    if len(verts_list) != B or len(faces_list) != B:
        raise RuntimeError("check_sign_ragged: one mesh per shape expected")
    vs = [_f32c(v).reshape(-1, 3) for v in verts_list]
    fs = [f.long().reshape(-1, 3) for f in faces_list]
    f_cnt = [f.shape[0] for f in fs]
    # (both offset lists in one launch of host_ints; torch.tensor(..., device=dev) would block until the stream has drained)
    offs = host_ints([0] + list(np.cumsum([v.shape[0] for v in vs])) + [0] + list(np.cumsum(f_cnt)), dev, i32=True)
    v_off, f_off = offs[:B + 1], offs[B + 1:]
    v_cat, f_cat = torch.cat(vs, 0).contiguous(), torch.cat(fs, 0).contiguous()
    out = torch.empty(B, N, device=dev, dtype=torch.uint8)
    cnt = torch.empty(B, N, device=dev, dtype=torch.int32) if return_count else None
    bad = torch.zeros(1, device=dev, dtype=torch.int32)
    algo = 1 if brute else 0
    ftot, fmax = int(sum(f_cnt)), int(max(f_cnt) if f_cnt else 0)
    _lib.call("deftet_check_sign_ragged_f32", dev, v_cat, v_off, f_cat, f_off, p, out, cnt, bad, B, ftot, fmax, N, algo,
              ws=lib.deftet_check_sign_ragged_workspace_bytes(B, ftot, fmax, algo))
    if check and int(bad.item()):
        raise IndexError("check_sign_ragged: face index outside its mesh")
    inside = out.view(torch.bool)                            # 0 / 1 bytes: a reinterpretation, not a conversion launch
    return (inside, cnt) if return_count else inside


# --------------------------------------------------------------------------------- generalised winding number
WINDING_ALGOS = {"auto": 0, "exact": 1, "fast": 2, "fast_unsorted": 3}


def _winding_call(name, v, v_off, f, f_off, p, B, V, ftot, fmax, algo, beta, check):
    lib = _lib.load()
    if algo not in WINDING_ALGOS:
        raise ValueError("%s: algo %r is not one of %s" % (name, algo, sorted(WINDING_ALGOS)))
    beta = 0.0 if beta is None else float(beta)
    if beta != 0.0 and not (1.0 <= beta <= 1e6):
        raise ValueError("%s: beta=%r: None (the default) or a value in [1, 1e6] expected" % (name, beta))
    N, dev, a = p.shape[1], p.device, WINDING_ALGOS[algo]
    out = torch.empty(B, N, device=dev, dtype=torch.float32)
    bad = torch.zeros(4, device=dev, dtype=torch.int32)
    _lib.call("deftet_winding_number_f32", dev, v, v_off, f, f_off, p, out, bad, B, V, ftot, fmax, N, a, beta,
              ws=lib.deftet_winding_number_workspace_bytes(B, ftot, fmax, N, a))
    if check:
        n_idx, n_corner, n_point = bad[:3].tolist()
        if n_idx:
            raise IndexError("%s: %d faces with a vertex index outside their mesh" % (name, n_idx))
        if n_corner or n_point:
            raise ValueError("%s: non-finite input (%d faces with such a corner, %d such points)" % (name, n_corner, n_point))
    return out


def winding_number(verts_bxvx3, faces_fx3, points_bxnx3, algo="auto", beta=None, check=True):
    """f32 [B,N]: the generalised winding number (Jacobson et al. 2013) of the mesh about every point — the sum over the faces of
    the signed solid angle over 4 pi.  An integer on a closed, consistently oriented mesh (1 inside an outward oriented surface,
    -1 inside a flipped one, 2 inside two nested ones), smooth across holes; see winding_inside for the two ways to read it.
    verts f32 [B,V,3], faces int [F,3] shared by the batch, points f32 [B,N,3].

    algo: "exact" tests every point against every face; "fast" walks an octree of the faces and takes clusters farther than `beta`
    radii as dipoles (beta None = 3: within 0.05 of the exact value); "auto" picks by the face count.  A point's
    value does not depend on the other points of the call and is the same bits on every run.
    check=True raises IndexError for a face index outside [0,V) and ValueError for non-finite vertices of faces or points (one
    read-back); with check=False the points of such a mesh, and such points, are NaN.
    There is no backward: the result is a label, and the tensors it comes from are not tracked."""
    _lib.require_gpu(verts_bxvx3, faces_fx3, points_bxnx3)
    v, p = _f32c(verts_bxvx3.detach()), _f32c(points_bxnx3.detach())
    f = faces_fx3.long().contiguous()
    if v.dim() != 3 or p.dim() != 3 or f.dim() != 2 or f.shape[1] != 3 or v.shape[0] != p.shape[0] or v.shape[2] != 3 or p.shape[2] != 3:
        raise RuntimeError("winding_number: verts [B,V,3], faces [F,3], points [B,N,3] expected")
    B, V, F = v.shape[0], v.shape[1], f.shape[0]
    return _winding_call("winding_number", v, None, f, None, p, B, V, B * F, F, algo, beta, check)


def winding_number_ragged(verts_list, faces_list, points_bxnx3, algo="auto", beta=None, check=True):
    """winding_number for a different mesh per shape in one launch sequence: verts_list[b] f32 [V_b,3] (or [1,V_b,3]), faces_list[b]
    int [F_b,3] with indices local to mesh b, points f32 [B,N,3] -> f32 [B,N].  Every shape gets the tree its own face count asks
    for, so a shape's values are those of its single call, bit for bit ("auto" is resolved once, by the largest mesh).  No backward."""
    _lib.require_gpu(points_bxnx3, *verts_list, *faces_list)
    p = _f32c(points_bxnx3.detach())
    if p.dim() != 3 or p.shape[2] != 3:
        raise RuntimeError("winding_number_ragged: points [B,N,3] expected")
    B, dev = p.shape[0], p.device
    if len(verts_list) != B or len(faces_list) != B:
        raise RuntimeError("winding_number_ragged: one mesh per shape expected")
    vs = [_f32c(v.detach()).reshape(-1, 3) for v in verts_list]
    fs = [f.long().reshape(-1, 3) for f in faces_list]
    f_cnt = [f.shape[0] for f in fs]
    offs = host_ints([0] + list(np.cumsum([v.shape[0] for v in vs])) + [0] + list(np.cumsum(f_cnt)), dev, i32=True)
    v_off, f_off = offs[:B + 1], offs[B + 1:]
    v_cat, f_cat = torch.cat(vs, 0).contiguous(), torch.cat(fs, 0).contiguous()
    return _winding_call("winding_number_ragged", v_cat, v_off, f_cat, f_off, p, B, 0, int(sum(f_cnt)), int(max(f_cnt) if f_cnt else 0),
                         algo, beta, check)


def winding_inside(w, rule="positive"):
    """bool, same shape as w: the inside label of a winding number.  "positive": w > 0.5 (Jacobson et al.: the majority reading, for
    open, nested and self-intersecting meshes).  "parity": round(|w|) is odd — what ray parity answers on a watertight mesh (inside
    two nested surfaces of the same orientation is outside)."""
    if rule == "positive":
        return w > 0.5
    if rule == "parity":
        return torch.round(torch.abs(w)).to(torch.int64) % 2 == 1
    raise ValueError("winding_inside: rule %r is not 'positive' or 'parity'" % (rule,))


# --------------------------------------------------------------------------------- N3 render-side rebuilds
def _i64_tets(tet_tx4):
    t = tet_tx4 if tet_tx4.dtype == torch.int64 else tet_tx4.long()
    if t.dim() != 2 or t.shape[1] != 4:
        raise RuntimeError("tet list [T,4] expected, got %s" % (tuple(t.shape),))
    return t.contiguous()


def tet_edges(tet_tx4, n_point):
    """(edges [E,2] int64 — unique (min,max) rows in lexicographic order, tet_edge [T,6] int64):
    generate_edge + generate_tet_edge_idx of prepare_for_wz.py:184-236."""
    _lib.require_gpu(tet_tx4)
    tet = _i64_tets(tet_tx4)
    T, dev = tet.shape[0], tet.device
    edges = torch.empty(max(6 * T, 1), 2, device=dev, dtype=torch.int64)
    tet_edge = torch.empty(T, 6, device=dev, dtype=torch.int64)
    cnt = torch.zeros(2, device=dev, dtype=torch.int32)
    _lib.call("deftet_tet_edges_i64", dev, tet, edges, tet_edge, cnt, cnt[1:], int(n_point), T, ws=_builder_bytes(n_point, T))
    n, bad = cnt.tolist()
    if bad:
        raise IndexError("tet_edges: vertex index outside [0, %d)" % n_point)
    return edges[:n], tet_edge


def subdivide(tet_tx4, points_px3, feat_pxk, subdiv_sig=None):
    """(points_new [P+E,3], feat_new [P+E,K], tet_new [T',4]): generate_subdivision, prepare_for_wz.py:255-301."""
    _lib.require_gpu(tet_tx4, points_px3, feat_pxk, subdiv_sig)
    tet, pts, feat = _i64_tets(tet_tx4), _f32c(points_px3), _f32c(feat_pxk)
    P, K, T, dev = pts.shape[0], feat.shape[1], tet.shape[0], tet.device
    if feat.shape[0] != P or pts.shape[1] != 3:
        raise RuntimeError("subdivide: points [P,3] and features [P,K] expected")
    edges, tet_edge = tet_edges(tet, P)
    E = edges.shape[0]
    sig = None
    if subdiv_sig is not None:
        if subdiv_sig.numel() != T:
            raise RuntimeError("subdivide: subdiv_sig needs one entry per tet")
        sig = subdiv_sig.to(torch.bool).contiguous().view(torch.uint8)
    pn = torch.empty(P + E, 3, device=dev, dtype=torch.float32)
    fn = torch.empty(P + E, K, device=dev, dtype=torch.float32)
    tn = torch.empty(max(8 * T, 1), 4, device=dev, dtype=torch.int64)
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.call("deftet_subdivide_f32", dev, tet, tet_edge, edges, pts, feat, sig, pn, fn, tn, cnt, P, T, E, K, ws=_builder_bytes(P, T))
    return pn, fn, tn[: int(cnt.item())]


def point_adj_idx(n_point, tet_tx4):
    """(pointadj_idx [P,m] int64 — ascending neighbours, -1 padded; adjsum [P,1] f32):
    generate_point_adj_idx, prepare_for_wz.py:134-146, without the dense P x P matrix."""
    _lib.require_gpu(tet_tx4)
    dev, P = tet_tx4.device, int(n_point)
    pairs = tet_point_adj(tet_tx4.to(torch.int32), P, dev)                 # sorted unique ordered pairs (A4)
    n = pairs.shape[0]
    adjsum = torch.zeros(P, 1, device=dev, dtype=torch.float32)
    mx = torch.zeros(1, device=dev, dtype=torch.int32)
    nbytes = (P + 1) * 4 + 256
    _lib.call("deftet_point_adj_table_i64", dev, pairs, n, P, None, 0, adjsum, mx, ws=nbytes)
    m = int(mx.item())
    table = torch.empty(P, m, device=dev, dtype=torch.int64)
    if m > 0:
        _lib.call("deftet_point_adj_table_i64", dev, pairs, n, P, table, m, None, None, ws=nbytes)
    return table, adjsum


def delete_tet(tet_tx4, tet_weights_txk, thres=0.01):
    """tets whose largest weight is > thres, order kept: delete_tet, prepare_for_wz.py:171-180."""
    _lib.require_gpu(tet_tx4, tet_weights_txk)
    tet, w = _i64_tets(tet_tx4), _f32c(tet_weights_txk)
    T, dev = tet.shape[0], tet.device
    if w.dim() != 2 or w.shape[0] != T:
        raise RuntimeError("delete_tet: weights [T,k] expected")
    out = torch.empty(max(T, 1), 4, device=dev, dtype=torch.int64)
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.call("deftet_delete_tet_i64", dev, tet, w, float(np.float32(thres)), out, cnt, T, w.shape[1], ws=_builder_bytes(0, T))
    return out[: int(cnt.item())]


def tet_neighbour_weights(tet_weights_txk, tet_neighbour_idx_tx4, neilevel=1):
    """tetweights2tetneighbourweights, diff_render/diftet_6_subdiv/3_model/deftet.py:316-331."""
    _lib.require_gpu(tet_weights_txk, tet_neighbour_idx_tx4)
    w = _f32c(tet_weights_txk)
    nei = tet_neighbour_idx_tx4.long().contiguous()
    T = w.shape[0]
    if nei.shape != (T, 4):
        raise RuntimeError("tet_neighbour_weights: neighbour index [T,4] expected")
    for _ in range(int(neilevel)):
        K = w.shape[1]
        out = torch.empty(T, 4 * K, device=w.device, dtype=torch.float32)
        _lib.call("deftet_tet_neighbour_weights_f32", w.device, w, nei, out, T, K)
        w = out
    return w


# --------------------------------------------------------------------------------- conforming selective refinement
RefinedTets = collections.namedtuple("RefinedTets", "points_new feat_new tet_new parent kind edges_split")
_REFINE_MAX_SWEEPS = 64                                 # what one deftet_tet_refine_mark_i64 call enqueues at most


def refine_marks(tet_edge_tx6, select, n_edge, sweeps_per_sync=4):
    """The closed edge marks of a selective refinement: (marks int32 [E] of 0 / 1 on the device, the marks every sweep set, a
    host list).  Every edge of a selected tet is marked; then sweeps_per_sync in-place sweeps of the face rule (two marked edges
    of a tet's face mark the third) are enqueued per read-back until the last sweep of a group set nothing, which proves closure.
    The result is the rule's least fixed point, the same bits whatever the schedule and the grouping.  Raises IndexError on a
    tet_edge entry outside [0, E), RuntimeError after E + 1 sweeps that still changed something (each sets at least one mark, so
    that cannot happen)."""
    _lib.require_gpu(tet_edge_tx6, select)
    te = tet_edge_tx6 if tet_edge_tx6.dtype == torch.int64 else tet_edge_tx6.long()
    if te.dim() != 2 or te.shape[1] != 6:
        raise RuntimeError("refine_marks: tet_edge [T,6] expected, got %s" % (tuple(te.shape),))
    te = te.contiguous()
    T, E, dev = int(te.shape[0]), int(n_edge), te.device
    S = int(sweeps_per_sync)
    if not 1 <= S <= _REFINE_MAX_SWEEPS:
        raise ValueError("refine_marks: sweeps_per_sync=%d outside 1..%d" % (S, _REFINE_MAX_SWEEPS))
    if select.numel() != T or select.device != dev:
        raise RuntimeError("refine_marks: select needs one entry per tet, on %s" % dev)
    if E < 0 or E > 6 * T:
        raise RuntimeError("refine_marks: n_edge=%d outside [0, 6 T]" % E)
    sel = (select if select.dtype == torch.bool else select != 0).reshape(-1).contiguous().view(torch.uint8)
    marks = torch.empty(E, device=dev, dtype=torch.int32)
    state = torch.empty(S + 1, device=dev, dtype=torch.int32)             # the counts of a group's sweeps, then bad
    counts, reset = [], 1
    while True:
        _lib.call("deftet_tet_refine_mark_i64", dev, te, sel, T, E, reset, S, marks, state, state[S:])
        got = state.tolist()                                              # the one read-back per group
        if got[S]:
            raise IndexError("refine_tets: tet_edge entry outside [0, %d)" % E)
        counts += got[:S]
        if got[S - 1] == 0:
            return marks, counts
        if sum(1 for c in counts if c) > E + 1:
            raise RuntimeError("refine_tets: the marks did not close within n_edge + 1 sweeps")
        reset = 0


def refine_tets(tet_tx4, points_px3, feat_pxk, select, edges=None, tet_edge=None, sweeps_per_sync=4):
    """Conforming selective refinement: RefinedTets(points_new f32 [P+M,3], feat_new f32 [P+M,K], tet_new int64 [T',4], parent int64
    [T'], kind uint8 [T'], edges_split int64 [M,2]).  The tets with select [T] set are split 1 -> 8 like subdivide, and the split
    is closed (red-green closure on edge marks, refine_marks) so that a face of the result has the owners its parent face had:
    what tet_neighbours, surface_extract, tet_components and marching_tets assume, and what subdivide(..., subdiv_sig) does not
    give.  M marked edges get a midpoint each, vertex P + r for marked edge number r of tet_edges' order, (x[a] + x[b]) / 2 in
    fp32 for positions and features, its ends in edges_split[r].  Tets stay in parent order, a parent's children contiguous;
    kind = the parent's marked edges: 0 untouched, 1 / 2 / 3 green closure tets (2, 4, 4 children), 6 a regular split (8).
    Refining a result again is legal and conforming, but the children of green tets degrade in shape: kind tells which they are.
    Every tet selected: subdivide's points, features and tets bit for bit; none: the input.  edges, tet_edge: tet_edges(tet, P)
    when the caller has them already (both or neither).  Integers only, the same bits on every run; one read-back per
    sweeps_per_sync sweeps and one for the sizes.  Raises IndexError on an index out of range, RuntimeError on wrong shapes and CPU
    tensors (and on a pattern that is no refinement, which closed marks cannot hold)."""
    _lib.require_gpu(tet_tx4, points_px3, feat_pxk, select, edges, tet_edge)
    lib = _lib.load()
    tet, pts, feat = _i64_tets(tet_tx4), _f32c(points_px3), _f32c(feat_pxk)
    if pts.dim() != 2 or pts.shape[1] != 3 or feat.dim() != 2 or feat.shape[0] != pts.shape[0]:
        raise RuntimeError("refine_tets: points [P,3] and features [P,K] expected")
    P, K, T, dev = int(pts.shape[0]), int(feat.shape[1]), int(tet.shape[0]), tet.device
    if (edges is None) != (tet_edge is None):
        raise RuntimeError("refine_tets: edges and tet_edge come together")
    if edges is None:
        edges, tet_edge = tet_edges(tet, P)
    edges, tet_edge = edges.long().contiguous(), tet_edge.long().contiguous()
    if edges.dim() != 2 or edges.shape[1] != 2 or tuple(tet_edge.shape) != (T, 6):
        raise RuntimeError("refine_tets: edges [E,2] and tet_edge [%d,6] expected" % T)
    E = int(edges.shape[0])
    marks, _counts = refine_marks(tet_edge, select, E, sweeps_per_sync)
    # the count pass leaves the ranks and child offsets in its workspace for the fill pass: a tensor of this call, not the shared one
    ws = torch.empty(lib.deftet_tet_refine_workspace_bytes(T, E), dtype=torch.uint8, device=dev)
    totals = torch.empty(3, device=dev, dtype=torch.int32)
    _lib.call("deftet_tet_refine_count_i64", dev, tet_edge, edges, marks, P, T, E, totals, ws=ws)
    M, Tn, bad = totals.tolist()
    if bad:
        raise RuntimeError("refine_tets: an edge end is outside [0, %d), or the marks are not closed" % P)
    out = RefinedTets(torch.empty(P + M, 3, device=dev, dtype=torch.float32), torch.empty(P + M, K, device=dev, dtype=torch.float32),
                      torch.empty(Tn, 4, device=dev, dtype=torch.int64), torch.empty(Tn, device=dev, dtype=torch.int64),
                      torch.empty(Tn, device=dev, dtype=torch.uint8), torch.empty(M, 2, device=dev, dtype=torch.int64))
    _lib.call("deftet_tet_refine_fill_f32", dev, tet, tet_edge, edges, marks, pts, feat, P, T, E, K, M, Tn, *out, ws=ws)
    return out


# --------------------------------------------------------------------------------- N2 vertex <-> tet gather
def _idx64(tet_idx):
    if tet_idx.dtype != torch.int64:
        tet_idx = tet_idx.long()
    if tet_idx.dim() == 2:
        tet_idx = tet_idx[None]
    return tet_idx.contiguous()


def tet_gather(pos_bxvx3, tet_idx, check=False):
    """tet_bxfx4x3 f32 [B,T,4,3] = gather of vertex positions (layers/DefTet/deftet.py:65-68).
    tet_idx int [T,4] (shared) or [B,T,4].  check=True synchronises and raises on an index
    outside [0,V) like torch.gather does (otherwise such corners are NaN)."""
    _lib.require_gpu(pos_bxvx3, tet_idx)
    pos, idx = _f32c(pos_bxvx3), _idx64(tet_idx)
    B, V, T = pos.shape[0], pos.shape[1], idx.shape[1]
    if idx.shape[0] not in (1, B) or idx.shape[2] != 4 or pos.shape[2] != 3:
        raise RuntimeError("tet_gather: pos [B,V,3] and tet_idx [T,4] or [B,T,4] expected")
    out = torch.empty(B, T, 4, 3, device=pos.device, dtype=torch.float32)
    bad = _bad_flag(check, pos.device)
    _lib.call("deftet_tet_gather_fwd_f32", pos.device, pos, idx, out, bad, B, V, T, idx.shape[0])
    _raise_if(bad, RuntimeError, "tet_gather: index out of range [0, %d)" % V)
    return out


def _incidence_csr(entry, bytes_entry, idx, sizes, error, message):
    """(offsets int32 [Bi*V+1], slots int32 [Bi*corners*E]) of the elements idx (tets, edges, faces) around their vertices, slot =
    corners * e + corner in ascending order per vertex: the one builder behind tet_vertex_csr, TetEdges and FaceTopology (their
    entries are all vtx::incidence_csr).  sizes = (Bi | None, V, E, corners), Bi = None for an entry that takes a single list.
    One read-back (a host sync); raises error(message % V) on an index outside [0, V)."""
    Bi, V, E, corners = sizes
    dims, lists = ((V, E), 1) if Bi is None else ((Bi, V, E), Bi)
    dev = idx.device
    offsets = torch.empty(lists * V + 1, device=dev, dtype=torch.int32)
    slots = torch.empty(lists * E * corners, device=dev, dtype=torch.int32)
    bad = _bad_flag(True, dev)
    _lib.call(entry, dev, idx, offsets, slots, bad, *dims, ws=getattr(_lib.load(), bytes_entry)(*dims))
    _raise_if(bad, error, message % V)
    return offsets, slots


def tet_vertex_csr(tet_idx, n_vertex):
    """(offsets int32 [Bi*V+1], slots int32 [Bi*4T], Bi): incidences (4*t+corner, ascending) per
    vertex — built once per topology for tet_gather_bwd.  Raises on an out-of-range index."""
    _lib.require_gpu(tet_idx)
    idx = _idx64(tet_idx)
    Bi, T, V = idx.shape[0], idx.shape[1], int(n_vertex)
    offsets, slots = _incidence_csr("deftet_tet_vertex_csr_i32", "deftet_tet_vertex_csr_workspace_bytes", idx, (Bi, V, T, 4),
                                    RuntimeError, "tet_vertex_csr: index out of range [0, %d)")
    return offsets, slots, Bi


def tet_gather_bwd(grad_tet_bxtx4x3, csr, n_vertex, out=None):
    """grad_pos f32 [B,V,3] = per-vertex sum of grad_tet in ascending (tet, corner) order
    (deterministic, no atomics).  out: existing [B,V,3] tensor to ADD to."""
    _lib.require_gpu(grad_tet_bxtx4x3)
    g = _f32c(grad_tet_bxtx4x3)
    B, T, V = g.shape[0], g.shape[1], int(n_vertex)
    _check_csr("tet_gather_bwd", csr, B, V, T, dev=g.device)
    offsets, slots, Bi = csr
    acc = out is not None
    gp = _out_or_new("tet_gather_bwd", out, (B, V, 3), g.device)
    _lib.call("deftet_tet_gather_bwd_f32", g.device, g, offsets, slots, gp, B, V, T, Bi, 1 if acc else 0)
    return gp


# --------------------------------------------------------------------------------- vertex Laplacian
VLAP_VALUES, VLAP_ROW_DIVISOR = 0, 1               # include/deftet_hip.h DEFTET_VLAP_*
VLAP_NONE, VLAP_SHAPE = 0, 1
_VADJ_ROW_COL, _VADJ_ROW_INPUT = 0, 1
_VLAP_REDUCTIONS = {"none": VLAP_NONE, "shape": VLAP_SHAPE}


class VertexAdjacency:
    """A sparse vertex adjacency M [V,V] for vertex_laplacian, built once per topology and reused (like TetTopology): the CSR
    (offsets, cols, vals) and its transpose (t_offsets, t_rows, t_vals), int32 / f32 on the GPU.  `weighting` is VLAP_VALUES
    (nei = Σ v_ij x_j) or VLAP_ROW_DIVISOR (nei = (Σ_j x_j) / row_weights[i]).  The object is a snapshot: it holds its own
    copies and does not follow later changes of the tensors it was built from — build a new one when the topology changes."""

    def __init__(self, n_vertex, weighting, offsets, cols, vals, t_offsets, t_rows, t_vals, row_weights=None):
        self.n_vertex, self.weighting = int(n_vertex), int(weighting)
        self.offsets, self.cols, self.vals = offsets, cols, vals
        self.t_offsets, self.t_rows, self.t_vals = t_offsets, t_rows, t_vals
        self.row_weights = row_weights
        self.nnz = int(cols.numel())
        self.device = offsets.device

    @classmethod
    def _build(cls, rows, cols, values, n_vertex, order, weighting, row_weights=None, checked=False):
        _lib.require_gpu(rows, cols, values, row_weights)
        lib = _lib.load()
        V, nnz, dev = int(n_vertex), int(rows.numel()), rows.device
        if rows.dtype not in (torch.int32, torch.int64) or cols.dtype != rows.dtype or cols.numel() != nnz:
            raise RuntimeError("VertexAdjacency: rows and cols must be int32 or int64 of one dtype and one length")
        rows, cols = rows.contiguous(), cols.contiguous()
        if values is not None:
            values = values.to(torch.float32).contiguous()
            if values.numel() != nnz:
                raise RuntimeError("VertexAdjacency: one value per entry expected")
        want_vals = weighting == VLAP_VALUES
        offsets = torch.empty(V + 1, device=dev, dtype=torch.int32)
        t_offsets = torch.empty(V + 1, device=dev, dtype=torch.int32)
        out_cols = torch.empty(nnz, device=dev, dtype=torch.int32)
        t_rows = torch.empty(nnz, device=dev, dtype=torch.int32)
        vals = torch.empty(nnz, device=dev, dtype=torch.float32) if want_vals else None
        t_vals = torch.empty(nnz, device=dev, dtype=torch.float32) if want_vals else None
        bad = torch.empty(1, device=dev, dtype=torch.int32)
        _lib.call("deftet_vertex_adjacency_csr_i32", dev, rows, cols, rows.element_size(), values, nnz, V, order, offsets, out_cols, vals,
                  t_offsets, t_rows, t_vals, bad, ws=lib.deftet_vertex_adjacency_workspace_bytes(nnz, V))
        # (the one host sync: build time only; `checked`: the caller's own kernel has already refused indices outside [0, V))
        if not checked and int(bad.item()):
            raise RuntimeError("VertexAdjacency: vertex index out of range [0, %d)" % V)
        return cls(V, weighting, offsets, out_cols, vals, t_offsets, t_rows, t_vals, row_weights)

    @classmethod
    def from_sparse(cls, adj):
        """From a torch sparse COO [V,V] on the GPU, coalesced or not (duplicates are summed, as torch.sparse.mm does): e.g.
        Tet_point_adj().run(V, tets, normalize=True) moved to the GPU, or the reference's MySparse.construct()."""
        if not adj.is_sparse or adj.dim() != 2 or adj.shape[0] != adj.shape[1]:
            raise RuntimeError("VertexAdjacency.from_sparse: a sparse COO [V,V] tensor expected")
        idx = adj._indices()                                # (uncoalesced input: its entries as stored)
        return cls._build(idx[0], idx[1], adj._values(), adj.shape[0], _VADJ_ROW_COL, VLAP_VALUES)

    @classmethod
    def from_tets(cls, tet_tx4, n_vertex, normalize=True):
        """The vertex adjacency of a tet mesh (tet_point_adj): ones, or D⁻¹A with `normalize` — the matrix
        Tet_point_adj().run(n_vertex, tets, normalize) gives, without going through torch sparse."""
        _lib.require_gpu(tet_tx4)
        V = int(n_vertex)
        pairs = tet_point_adj(tet_tx4, V, tet_tx4.device)               # sorted unique directed pairs, int32 [n,2]
        rows, cols = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
        vals = None
        if normalize:
            # 1/deg(row) rounded once from fp64, as utils/lib/tet_point_adj/interface.py does on the host
            deg = torch.bincount(rows.long(), minlength=V).double()
            vals = (1.0 / deg)[rows.long()].float()
        return cls._build(rows, cols, vals, V, _VADJ_ROW_COL, VLAP_VALUES)

    @classmethod
    def from_table(cls, point_adj_idx_pxm, point_adj_weights_px1, index_base=0):
        """From a padded neighbour table [P,m] and row weights [P,1] (Deftet.get_featlap): index_base=0 for this repository's
        table (point_adj_idx: ascending neighbours, -1 padding), index_base=1 for the reference's stored table (+1, 0 padding).
        Each row sums its neighbours in table order, then divides by its weight."""
        _lib.require_gpu(point_adj_idx_pxm, point_adj_weights_px1)
        if index_base not in (0, 1):
            raise ValueError("from_table: index_base must be 0 or 1")
        table = point_adj_idx_pxm
        if table.dim() != 2:
            raise RuntimeError("from_table: a [P,m] table expected")
        P, m = table.shape
        w = point_adj_weights_px1.reshape(-1).to(torch.float32).contiguous().clone()
        if w.numel() != P:
            raise RuntimeError("from_table: one weight per table row expected")
        t = table.long() - index_base
        keep = t != -1                                      # the padding; anything else outside [0, P) raises in the build
        rows = torch.arange(P, device=t.device).unsqueeze(1).expand(P, m)[keep]      # (row-major: table order)
        return cls._build(rows, t[keep], None, P, _VADJ_ROW_INPUT, VLAP_ROW_DIVISOR, w)

    @classmethod
    def from_faces(cls, faces_fx3, n_vertex, normalize=True):
        """The vertex adjacency of a triangle mesh (kal.ops.mesh.adjacency_matrix): the unique undirected edges (face_edges: a
        radix sort of the edge keys, one entry per run) as ones, or D⁻¹A with `normalize` (1/deg rounded once from fp64, as
        from_tets) — vertex_aggregate then gives the neighbour mean."""
        V = int(n_vertex)
        pairs = face_edges(faces_fx3, V)                                # sorted unique directed pairs, int32 [n,2]
        rows, cols = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
        vals = None
        if normalize:
            deg = torch.bincount(rows.long(), minlength=V).double()
            vals = (1.0 / deg)[rows.long()].float()
        return cls._build(rows, cols, vals, V, _VADJ_ROW_COL, VLAP_VALUES, checked=True)     # face_edges raised on a bad index


class _VertexLaplacian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adjacency, reduction):
        ctx.set_materialize_grads(False)
        lib = _lib.load()
        adj = adjacency
        B, V, C = x.shape
        dev = x.device
        r = torch.empty(B, V, C, device=dev, dtype=torch.float32)
        out = torch.empty((B,) if reduction == VLAP_SHAPE else (B, V, C), device=dev, dtype=torch.float32)
        _lib.call("deftet_vertex_laplacian_fwd_f32", dev, x, adj.offsets, adj.cols, adj.vals, adj.row_weights, adj.weighting, reduction,
                  B, V, C, adj.nnz, r, out, ws=lib.deftet_vertex_laplacian_workspace_bytes(B, V) if reduction == VLAP_SHAPE else None)
        ctx.save_for_backward(r)
        ctx.adj, ctx.reduction = adj, reduction
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if grad_out is None or not ctx.needs_input_grad[0]:
            return None, None, None
        (r,) = ctx.saved_tensors
        adj, reduction = ctx.adj, ctx.reduction
        g = _f32c(grad_out)
        B, V, C = r.shape
        dx = torch.empty_like(r)
        _lib.call("deftet_vertex_laplacian_bwd_f32", r.device, r, g, adj.t_offsets, adj.t_rows, adj.t_vals, adj.row_weights, adj.weighting,
                  reduction, B, V, C, adj.nnz, dx)
        return dx, None, None


def vertex_laplacian(x, adjacency, reduction="shape"):
    """r = M·x − x over a VertexAdjacency M, x f32 [B,V,C] with 1 <= C <= 16 (differentiable w.r.t. x); returns
    Σ_{i,c} r² per shape, f32 [B] (reduction="shape": DefTet.laplacian_sparse) or r², f32 [B,V,C] (reduction="none":
    Deftet.get_featlap).  No host synchronisation: the call can be captured in a graph."""
    _lib.require_gpu(x)
    if not isinstance(adjacency, VertexAdjacency):
        raise TypeError("vertex_laplacian: a hip_ops.VertexAdjacency expected, got %s" % type(adjacency).__name__)
    if reduction not in _VLAP_REDUCTIONS:
        raise ValueError("vertex_laplacian: reduction must be 'shape' or 'none', got %r" % (reduction,))
    if x.dim() != 3 or x.shape[1] != adjacency.n_vertex:
        raise RuntimeError("vertex_laplacian: x [B,%d,C] expected, got %s" % (adjacency.n_vertex, tuple(x.shape)))
    if x.device != adjacency.device:
        raise RuntimeError("vertex_laplacian: x is on %s, the adjacency on %s" % (x.device, adjacency.device))
    return _VertexLaplacian.apply(_f32c(x), adjacency, _VLAP_REDUCTIONS[reduction])


# --------------------------------------------------------------------------------- vertex aggregation
def _vertex_aggregate(x, offsets, idx, vals, nnz):
    """out = M·x for the CSR (offsets, idx, vals): the one library call both directions make"""
    B, V, C = x.shape
    out = torch.empty(B, V, C, device=x.device, dtype=torch.float32)
    _lib.call("deftet_vertex_aggregate_f32", x.device, x, offsets, idx, vals, B, V, C, nnz, out)
    return out


class _VertexAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adjacency):
        ctx.set_materialize_grads(False)
        ctx.adj = adjacency
        return _vertex_aggregate(x, adjacency.offsets, adjacency.cols, adjacency.vals, adjacency.nnz)

    @staticmethod
    def backward(ctx, grad_out):
        if grad_out is None or not ctx.needs_input_grad[0]:
            return None, None
        adj = ctx.adj
        return _vertex_aggregate(_f32c(grad_out), adj.t_offsets, adj.t_rows, adj.t_vals, adj.nnz), None


def vertex_aggregate(x, adjacency):
    """M·x over a VertexAdjacency M with values (from_sparse, from_tets), x f32 [B,V,C] with any C >= 1 (differentiable w.r.t.
    x; M is a constant): out[b,i,c] = Σ_k v_ik x[b,k,c], contiguous f32 [B,V,C] — sparse_batch_matmul of the GCN decoder
    (layers/gcn_decoder.py:55-56).  Every channel is one fmaf chain in CSR order: bit-reproducible, and independent of C.
    No host synchronisation: the call can be captured in a graph."""
    _lib.require_gpu(x)
    if not isinstance(adjacency, VertexAdjacency):
        raise TypeError("vertex_aggregate: a hip_ops.VertexAdjacency expected, got %s" % type(adjacency).__name__)
    if adjacency.weighting != VLAP_VALUES:
        raise ValueError("vertex_aggregate: a VLAP_VALUES adjacency (from_sparse, from_tets) expected; a VLAP_ROW_DIVISOR one "
                         "(from_table) is not supported")
    if x.dim() != 3 or x.shape[1] != adjacency.n_vertex or x.shape[2] < 1:
        raise RuntimeError("vertex_aggregate: x [B,%d,C] with C >= 1 expected, got %s" % (adjacency.n_vertex, tuple(x.shape)))
    if x.device != adjacency.device:
        raise RuntimeError("vertex_aggregate: x is on %s, the adjacency on %s" % (x.device, adjacency.device))
    return _VertexAggregate.apply(_f32c(x), adjacency)


# --------------------------------------------------------------------------------- A7 / A11
def boundary_index(tet_face_fx3, tet_idx_fx2, occ_bxn, mode=1):
    """list of B int64 [Fb_i,3] tensors — DefTet.get_boundary_index (mode 1) /
    get_internal_index (mode 2), layers/DefTet/deftet.py:186-203.
    (Measured and not kept, round 6: the lengths read back on a side stream while the energies are enqueued behind the boundary
    kernels, so that the device has work when the host resumes — the pinned buffer, two events and the stream switch cost the
    host more than the 40 us of overlap return: geometry step 2.29 -> 2.34 ms.)"""
    if tet_face_fx3.dim() != 2 or tet_face_fx3.shape[1] != 3:
        raise _lib.DefTetHipError("boundary_index: face [F,3] expected, got %s" % (tuple(tet_face_fx3.shape),))
    if tet_idx_fx2.dim() != 2 or tuple(tet_idx_fx2.shape) != (tet_face_fx3.shape[0], 2):
        raise _lib.DefTetHipError("boundary_index: tet_idx [%d,2] expected (one pair of tets per face), got %s"
                                  % (tet_face_fx3.shape[0], tuple(tet_idx_fx2.shape)))
    if occ_bxn.dim() != 2:
        raise _lib.DefTetHipError("boundary_index: occ [B,T] expected, got %s" % (tuple(occ_bxn.shape),))
    if mode not in (1, 2):
        raise _lib.DefTetHipError("boundary_index: mode must be 1 (boundary) or 2 (internal), got %r" % (mode,))
    _lib.require_gpu(tet_face_fx3, tet_idx_fx2, occ_bxn)
    lib = _lib.load()
    face = tet_face_fx3.contiguous().long()
    tidx = tet_idx_fx2.contiguous().long()
    occ = _f32c(occ_bxn)
    B, T = occ.shape
    Fi = face.shape[0]
    dev = occ.device
    out = torch.empty(max(B * Fi, 1), 3, dtype=torch.int64, device=dev)
    offs = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    _lib.call("deftet_boundary_index_i64", dev, face, tidx, occ, out, offs, B, T, Fi, int(mode),
              ws=lib.deftet_boundary_index_workspace_bytes(B, Fi))
    o = offs.tolist()                                   # one sync (the reference syncs once per shape)
    return [out[o[b]:o[b + 1]] for b in range(B)]


def _energy_pow(name, p):
    try:
        q = operator.index(p)
    except TypeError:
        q = 0
    if not 1 <= q <= 16:                                   # the kernels multiply pow times: an integer, 16 at the most
        raise _lib.DefTetHipError("tet_energies: %s must be an integer in 1..16, got %r" % (name, p))
    return q


class _TetEnergies(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tet_bxfx4x3, inverse_v, pow_v, pow_e, scale):
        if tet_bxfx4x3.dim() != 4 or tuple(tet_bxfx4x3.shape[2:]) != (4, 3):
            raise _lib.DefTetHipError("tet_energies: tet [B,T,4,3] expected, got %s" % (tuple(tet_bxfx4x3.shape),))
        if inverse_v is not None and tuple(inverse_v.shape) != (tet_bxfx4x3.shape[1], 3, 3):     # the kernels read one 3x3 per tet
            raise _lib.DefTetHipError("tet_energies: inverse_v [%d,3,3] expected (one matrix per tet), got %s"
                                      % (tet_bxfx4x3.shape[1], tuple(inverse_v.shape)))
        pow_v, pow_e = _energy_pow("pow_v", pow_v), _energy_pow("pow_e", pow_e)
        _lib.require_gpu(tet_bxfx4x3, inverse_v)
        lib = _lib.load()
        tet = _f32c(tet_bxfx4x3)
        inv = _f32c(inverse_v) if inverse_v is not None else None
        B, T = tet.shape[0], tet.shape[1]
        dev = tet.device
        out = torch.empty(B, 3, device=dev, dtype=torch.float32)
        stats = torch.empty(B, 8, device=dev, dtype=torch.float64)
        _lib.call("deftet_tet_energies_fwd_f32", dev, tet, inv, out, stats, B, T, int(pow_v), int(pow_e), float(scale),
                  ws=lib.deftet_tet_energies_workspace_bytes2(B, T))
        ctx.save_for_backward(tet, inv if inv is not None else tet.new_empty(0), stats)
        ctx.cfg = (int(pow_v), int(pow_e), float(scale), inv is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        tet, inv, stats = ctx.saved_tensors
        pow_v, pow_e, scale, has_inv = ctx.cfg
        g = _f32c(grad_out)
        B, T = tet.shape[0], tet.shape[1]
        grad_tet = torch.empty_like(tet)
        _lib.call("deftet_tet_energies_bwd_f32", tet.device, tet, inv if has_inv else None, stats, g, grad_tet, B, T, pow_v, pow_e, scale)
        return grad_tet, None, None, None, None


def tet_energies(tet_bxfx4x3, inverse_v=None, pow_v=4, pow_e=4, scale=20.0):
    """f32 [B,3] = (volume_variance, amips_energy, edge_length) — differentiable w.r.t. tet."""
    return _TetEnergies.apply(tet_bxfx4x3, inverse_v, pow_v, pow_e, scale)


# --------------------------------------------------------------------------------- surface extraction
SX_BINARY, SX_THRESHOLD = 0, 1                          # include/deftet_hip.h DEFTET_SX_*
_SX_MODES = {"binary": SX_BINARY, "threshold": SX_THRESHOLD, SX_BINARY: SX_BINARY, SX_THRESHOLD: SX_THRESHOLD}
SurfaceSoup = collections.namedtuple("SurfaceSoup", "face face_attr index faces")


class TetFaceNeighbours:
    """nbr[t][i] = the tet across LOCAL FACE i of tet t, -1 where no other tet owns the face: `table` int64 [T,4] for torch
    indexing, `table32` int32 [T,4] for the kernels (16 bytes per tet).  Built once per topology."""
    __slots__ = ("table", "table32", "n_tet", "device")

    def __init__(self, table, table32):
        self.table, self.table32 = table, table32
        self.n_tet, self.device = int(table32.shape[0]), table32.device


def tet_face_neighbours(tet_list, n_point, device):
    """TetFaceNeighbours of a tet list — row t of the i-th matrix of tet_adj_share (utils/lib/tet_adj_share/run.cpp:40-97,
    diff_render/diftet_6_subdiv/3_model/utils_tetsv.py:16-75) as one table.  Raises ValueError when a face has more than two
    owners, as both reference functions do."""
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.DefTetHipError("deftet_amd operators need a GPU (got device %s); there is no CPU fallback" % dev)
    _f3, t2, tf2, _b3, n_multi = tet_to_face(tet_list, n_point, dev, with_boundary=True)
    if n_multi:
        raise ValueError("%d faces are shared by more than two tetrahedra" % n_multi)
    T = int(torch.as_tensor(tet_list).shape[0])
    if T == 0:
        raise ValueError("tet_face_neighbours: empty tet list")
    n64 = torch.empty(T, 4, dtype=torch.int64, device=dev)
    n32 = torch.empty(T, 4, dtype=torch.int32, device=dev)
    _lib.call("deftet_tet_face_neighbours_i64", dev, t2, tf2, int(t2.shape[0]), T, n64, n32)
    return TetFaceNeighbours(n64, n32)


def adj_list_table(adj_list):
    """numpy int64 [T,4] neighbour table by local face from the reference's list of four [T,T] sparse matrices (scipy, or torch
    sparse COO).  A row holds at most one nonzero (a local face has one partner) and its value is 1; anything else raises."""
    if len(adj_list) != 4:
        raise ValueError("tet_adj: four sparse matrices expected, got %d" % len(adj_list))
    T = int(adj_list[0].shape[0])
    table = -np.ones((T, 4), np.int64)
    for i, adj in enumerate(adj_list):
        if tuple(adj.shape) != (T, T):
            raise ValueError("tet_adj[%d] is %s, expected (%d, %d)" % (i, tuple(adj.shape), T, T))
        if isinstance(adj, torch.Tensor):
            adj = (adj if adj.layout == torch.sparse_coo else adj.to_sparse()).coalesce()
            row, col = (x.cpu().numpy() for x in adj.indices())
            val = adj.values().cpu().numpy()
        else:
            adj = adj.tocoo(copy=True)
            adj.sum_duplicates()
            row, col, val = adj.row, adj.col, adj.data
        keep = val != 0
        row, col, val = row[keep], col[keep], val[keep]
        if row.size and np.bincount(row, minlength=T).max() > 1:
            raise ValueError("tet_adj[%d]: a row holds more than one nonzero" % i)
        if not (val == 1).all():
            raise ValueError("tet_adj[%d]: values other than 1" % i)
        table[row, i] = col
    return table


def neighbours_from_adj_list(adj_list, device):
    """TetFaceNeighbours from a TetFaceNeighbours (returned as it is) or the reference's list of four sparse matrices
    (adj_list_table + one upload).  Nothing is cached behind the caller's back: convert once per topology and hand the returned
    object to the drop-ins as `tet_adj` — a list is converted again on every call."""
    if isinstance(adj_list, TetFaceNeighbours):
        return adj_list
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.DefTetHipError("deftet_amd operators need GPU tensors (got device %s); there is no CPU fallback" % dev)
    t64 = torch.from_numpy(adj_list_table(adj_list)).to(dev)
    return TetFaceNeighbours(t64, t64.to(torch.int32))


def surface_extract(tet_bxfx4x3, occ, nbr, mode, thres=None, attr=None, vertex_weights=None, tet_idx=None, return_index=False,
                    return_faces=False):
    """Triangle soup of a per-tet occupancy: SurfaceSoup(face, face_attr, index, faces), each a list of B tensors (or None) with
    rows in ascending (tet, local face) order — face f32 [F_b,3,3]; face_attr f32 [F_b,3,C] with attr f32 [B,T,4,C];
    index int64 [F_b,2] = (tet, local face); faces int64 [F_b,3] = vertex ids through tet_idx [T,4].
    mode "binary": utils/tet_utils.py:427-471; mode "threshold" with thres = htres: utils_tetsv.py:79-128, 145-225.
    occ f32 [B,T] / [B,T,1], or None with vertex_weights f32 [B,V] (or [V] for one shape) and tet_idx: occ = max of the four
    corner weights (3_model/deftet.py:522-523).  No gradient: gather with `index` for one.  One read-back (the offsets)."""
    lib = _lib.load()
    if mode not in _SX_MODES:
        raise ValueError("surface_extract: mode %r is neither 'binary' nor 'threshold'" % (mode,))
    mode = _SX_MODES[mode]
    if mode == SX_THRESHOLD and thres is None:
        raise ValueError("surface_extract: mode 'threshold' needs thres")
    if not isinstance(nbr, TetFaceNeighbours):
        raise TypeError("surface_extract: nbr must be a TetFaceNeighbours (tet_face_neighbours / neighbours_from_adj_list)")
    if attr is not None and (attr.dim() != 4 or not 1 <= int(attr.shape[3]) <= 8):
        raise _lib.DefTetHipError("surface_extract: attr [B,T,4,C] with 1 <= C <= 8 expected, got %s (DEFTET_EINVAL)" % (tuple(attr.shape),))
    _lib.require_gpu(tet_bxfx4x3, occ, attr, vertex_weights, nbr.table32)
    if (occ is None) == (vertex_weights is None):
        raise ValueError("surface_extract: exactly one of occ and vertex_weights")
    tet = _f32c(tet_bxfx4x3)
    if tet.dim() != 4 or tuple(tet.shape[2:]) != (4, 3):
        raise RuntimeError("surface_extract: tet [B,T,4,3] expected, got %s" % (tuple(tet.shape),))
    B, T = int(tet.shape[0]), int(tet.shape[1])
    dev = tet.device
    if nbr.n_tet != T or nbr.device != dev:
        raise RuntimeError("surface_extract: the neighbour table has %d tets on %s, the input %d on %s" % (nbr.n_tet, nbr.device, T, dev))
    idx32, V = None, 0
    if tet_idx is not None:
        idx32 = torch.as_tensor(tet_idx).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(idx32.shape) != (T, 4):
            raise RuntimeError("surface_extract: tet_idx [%d,4] on %s expected" % (T, dev))
    if (vertex_weights is not None or return_faces) and idx32 is None:
        raise ValueError("surface_extract: vertex_weights / return_faces need tet_idx")
    w = None
    if vertex_weights is not None:
        w = _f32c(vertex_weights)
        w = w.reshape(1, -1) if w.dim() == 1 or (w.dim() == 2 and w.shape[1] == 1 and B == 1) else w.reshape(w.shape[0], -1)
        if w.shape[0] != B:
            raise RuntimeError("surface_extract: vertex_weights for %d shapes, tets for %d" % (w.shape[0], B))
        V = int(w.shape[1])
    else:
        occ = _f32c(occ)
        if occ.numel() != B * T:
            raise RuntimeError("surface_extract: occ [%d,%d] expected, got %s" % (B, T, tuple(occ.shape)))
        occ = occ.reshape(B, T)
    C = 0
    if attr is not None:
        attr = _f32c(attr)
        if attr.dim() != 4 or tuple(attr.shape[:3]) != (B, T, 4):
            raise RuntimeError("surface_extract: attr [%d,%d,4,C] expected, got %s" % (B, T, tuple(attr.shape)))
        C = int(attr.shape[3])
    h = float(thres) if thres is not None else 0.0
    offs = torch.empty(B + 1, dtype=torch.int32, device=dev)
    # the count pass leaves the row bases in its workspace for the fill pass: a tensor of this call, not the shared one
    ws = torch.empty(lib.deftet_surface_extract_workspace_bytes(B, T, int(w is not None)), dtype=torch.uint8, device=dev)
    _lib.call("deftet_surface_extract_count_f32", dev, occ, w, idx32, V, nbr.table32, B, T, mode, h, offs, ws=ws)
    o = offs.tolist()                                   # the one sync (the reference syncs per shape and per local face)
    if o[B] < 0:
        raise RuntimeError("surface_extract: a neighbour or vertex index is out of range")
    F = o[B]
    face = torch.empty(F, 3, 3, dtype=torch.float32, device=dev)
    fattr = torch.empty(F, 3, C, dtype=torch.float32, device=dev) if attr is not None else None
    index = torch.empty(F, 2, dtype=torch.int64, device=dev) if return_index else None
    faces = torch.empty(F, 3, dtype=torch.int64, device=dev) if return_faces else None
    _lib.call("deftet_surface_extract_fill_f32", dev, tet, attr, C, occ if w is None else None, idx32, nbr.table32, B, T, mode, h, F,
              face, fattr, index, faces, ws=ws)

    def split(x):
        return None if x is None else [x[o[b]:o[b + 1]] for b in range(B)]
    return SurfaceSoup(split(face), split(fattr), split(index), split(faces))


def surface_weld(verts_vx3, faces_fx3, attrs=None):
    """Indexed mesh on the vertices its faces use, renumbered in ascending original id: (verts [V',3], attrs [V',C] or None,
    faces int64 [F,3] with the new ids, old_id int64 [V']).  verts[faces] is unchanged bit for bit."""
    _lib.require_gpu(verts_vx3, faces_fx3, attrs)
    lib = _lib.load()
    verts = _f32c(verts_vx3)
    faces = faces_fx3.contiguous().long()
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("surface_weld: verts [V,3] and faces [F,3] expected, got %s and %s" % (tuple(verts.shape), tuple(faces.shape)))
    V, F = int(verts.shape[0]), int(faces.shape[0])
    dev = verts.device
    C = 0
    if attrs is not None:
        attrs = _f32c(attrs)
        if attrs.dim() != 2 or attrs.shape[0] != V:
            raise RuntimeError("surface_weld: attrs [%d,C] expected, got %s" % (V, tuple(attrs.shape)))
        C = int(attrs.shape[1])
        if not 1 <= C <= 8:
            raise _lib.DefTetHipError("surface_weld: attrs has C = %d channels, 1..8 supported (DEFTET_EINVAL)" % C)
    cap = min(V, 3 * F)
    n = torch.empty(2, dtype=torch.int32, device=dev)
    old = torch.empty(cap, dtype=torch.int64, device=dev)
    vout = torch.empty(cap, 3, dtype=torch.float32, device=dev)
    aout = torch.empty(cap, C, dtype=torch.float32, device=dev) if attrs is not None else None
    fout = torch.empty(F, 3, dtype=torch.int64, device=dev)
    _lib.call("deftet_surface_weld_f32", dev, faces, F, verts, attrs, C, V, cap, n, old, vout, aout, fout,
              ws=lib.deftet_surface_weld_workspace_bytes(V))
    n_used, bad = n.tolist()
    if bad:
        raise RuntimeError("surface_weld: a face index is outside [0, %d)" % V)
    return vout[:n_used], (aout[:n_used] if aout is not None else None), fout, old[:n_used]


# --------------------------------------------------------------------------------- connected tet components
TetComponents = collections.namedtuple("TetComponents", "labels sizes open count")


def _inside_u8(caller, inside, nbr):
    """(uint8 [B,T] view or copy of `inside`, whether the input had no batch dimension)"""
    if not isinstance(nbr, TetFaceNeighbours):
        raise TypeError("%s: nbr must be a TetFaceNeighbours (tet_face_neighbours / neighbours_from_adj_list)" % caller)
    _lib.require_gpu(inside, nbr.table32)
    single = inside.dim() == 1
    m = inside.reshape(1, -1) if single else inside
    if m.dim() != 2 or int(m.shape[1]) != nbr.n_tet or m.shape[0] < 1 or m.device != nbr.device:
        raise RuntimeError("%s: inside [B,%d] or [%d] on %s expected, got %s on %s"
                           % (caller, nbr.n_tet, nbr.n_tet, nbr.device, tuple(inside.shape), inside.device))
    if m.dtype not in (torch.bool, torch.uint8):
        m = m != 0                                      # (NaN != 0: inside)
    m = m.contiguous()
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), single


def _bad_neighbour(caller, bad):
    if int(bad.item()):
        raise RuntimeError("%s: a neighbour index is out of range" % caller)


def _components_out(B, T, dev):
    return (torch.empty(B, T, dtype=torch.int32, device=dev), torch.empty(B, T, dtype=torch.int32, device=dev),
            torch.empty(B, T, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev))


def _components_result(parts, single):
    labels, sizes, opn, count = parts
    opn = opn.view(torch.bool)
    return TetComponents(labels[0], sizes[0], opn[0], count) if single else TetComponents(labels, sizes, opn, count)


def _tet_components(inside, nbr):
    """tet_components without the read-back: (TetComponents, bad int32 [1] on the device)"""
    lib = _lib.load()
    m, single = _inside_u8("tet_components", inside, nbr)
    B, T = int(m.shape[0]), int(m.shape[1])
    dev = m.device
    parts = _components_out(B, T, dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("deftet_tet_components_u8", dev, m, nbr.table32, B, T, *parts, bad, ws=lib.deftet_tet_components_workspace_bytes(B, T))
    return _components_result(parts, single), bad


def tet_components(inside, nbr, check=True):
    """Connected components of the inside tets of every shape: TetComponents(labels, sizes, open, count), all on the device.
    inside bool / uint8 / float [B,T] or [T] (non-zero = inside); nbr a TetFaceNeighbours, taken as undirected: two inside tets
    are connected when either stands in the other's row.  labels int32 = -1 outside, otherwise the smallest tet index of the
    component (the same bits on every run, whatever the schedule); sizes int32 = tets of the component at its label's index, 0
    elsewhere; open bool = at the label's index, whether a tet of the component has a -1 entry in its row (the component
    reaches the grid boundary); count int32 [B] ([1] for a [T] input) = components per shape.
    The results themselves are not read back.  The count of neighbour entries outside [-1, T) is: four bytes, in this call,
    because nothing later in it synchronises; a non-zero count raises RuntimeError (such an entry is never followed, so the
    components it does not touch are still right).  check=False skips that read and the error with it."""
    comps, bad = _tet_components(inside, nbr)
    if check:
        _bad_neighbour("tet_components", bad)
    return comps


def _occupancy_cleanup(inside, nbr, keep_largest, min_size, fill_voids, return_components):
    """occupancy_cleanup without the read-back: (keep, TetComponents or None, bad int32 [1] on the device)"""
    lib = _lib.load()
    m, single = _inside_u8("occupancy_cleanup", inside, nbr)
    if int(min_size) < 0:
        raise ValueError("occupancy_cleanup: min_size=%d is negative" % min_size)
    B, T = int(m.shape[0]), int(m.shape[1])
    dev = m.device
    keep = torch.empty(B, T, dtype=torch.uint8, device=dev)
    parts = _components_out(B, T, dev) if return_components else (None, None, None, None)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("deftet_occupancy_cleanup_u8", dev, m, nbr.table32, B, T, int(bool(keep_largest)), int(min_size), int(bool(fill_voids)),
              keep, *parts, bad, ws=lib.deftet_tet_components_workspace_bytes(B, T))
    keep = keep.view(torch.bool)
    return (keep[0] if single else keep), (_components_result(parts, single) if return_components else None), bad


def occupancy_cleanup(inside, nbr, keep_largest=False, min_size=0, fill_voids=False, return_components=False, check=True):
    """Cleans a per-tet occupancy on the device: keep bool [B,T] ([T] for a [T] input).  In this order: fill_voids turns every
    component of the OUTSIDE tets that does not reach the grid boundary into inside; the filled mask is labelled; min_size = m > 0
    drops the components with fewer than m tets; keep_largest keeps the component with the most tets among those left, the one
    with the smaller label among equal sizes (an empty shape stays empty).  With no option set keep is the inside mask.
    return_components=True returns (keep, TetComponents) with the components of the filled mask, the labelling the selection
    was made on.  inside, nbr and the four-byte read of the bad-neighbour count (check) as in tet_components."""
    keep, comps, bad = _occupancy_cleanup(inside, nbr, keep_largest, min_size, fill_voids, return_components)
    if check:
        _bad_neighbour("occupancy_cleanup", bad)
    return (keep, comps) if return_components else keep


def cleaned_occupancy(occ, inside, keep):
    """occ with the outcome of occupancy_cleanup written into it: 0 where an inside tet was dropped, 1 where an outside tet was
    filled, occ everywhere else (all three of one shape)."""
    return torch.where(keep, torch.where(inside, occ, torch.ones_like(occ)), torch.where(inside, torch.zeros_like(occ), occ))


def occupancy_band(inside, nbr_tx4, rings=0):
    """bool [T]: the tets that have a face neighbour in the other state in any shape of inside [B,T] (or [T]; non-zero = inside),
    grown by `rings` face rings — the selection refine_tets wants around a surface.  nbr_tx4 int64 [T,4] (or a TetFaceNeighbours:
    its table); entries of -1 are ignored.  Plain torch ops on the existing neighbour table, no kernel of its own: a handful of
    gathers over [B,T,4], on whatever device the inputs are."""
    nbr = nbr_tx4.table if isinstance(nbr_tx4, TetFaceNeighbours) else nbr_tx4
    if nbr.dim() != 2 or nbr.shape[1] != 4:
        raise RuntimeError("occupancy_band: neighbour table [T,4] expected, got %s" % (tuple(nbr.shape),))
    T = int(nbr.shape[0])
    if inside.dim() not in (1, 2) or inside.shape[-1] != T or inside.device != nbr.device:
        raise RuntimeError("occupancy_band: inside [B,%d] or [%d] on %s expected, got %s on %s" % (T, T, nbr.device, tuple(inside.shape), inside.device))
    ins = inside if inside.dtype == torch.bool else inside != 0
    ins = ins[None] if ins.dim() == 1 else ins
    if int(rings) < 0:
        raise ValueError("occupancy_band: rings=%d is negative" % rings)
    has = nbr >= 0
    to = torch.where(has, nbr, torch.zeros_like(nbr)).long()
    band = ((ins[:, to] != ins[:, :, None]) & has[None]).any(2).any(0)
    for _ in range(int(rings)):
        band = band | (band[to] & has).any(1)
    return band


# --------------------------------------------------------------------------------- marching tetrahedra
IsoMesh = collections.namedtuple("IsoMesh", "verts faces vert_attr edge_id t tet_id")


class TetEdges:
    """The edge topology of a tet list for marching_tets, built once and reused (like FaceTopology / VertexAdjacency): `edges`
    int32 [E,2] — the unique (min,max) rows in lexicographic order — and `tet_edge` int32 [T,6] — the edge ids in local order
    (0,1),(0,2),(0,3),(1,2),(1,3),(2,3) — exactly what tet_edges returns; `tets` int32 [T,4]; and the vertex -> edge-end CSR
    `offsets` int32 [V+1], `slots` int32 [2E] holding 2*e+side (side 0 = the min end) in ascending order per vertex.  Raises
    IndexError on an index outside [0, n_vertex).  A snapshot of the list it was built from: a new tet list means a new object.
    `device`: where to put a host list."""

    def __init__(self, tet_tx4, n_vertex, device=None):
        tets = torch.as_tensor(tet_tx4)
        if device is not None:
            tets = tets.to(device)
        _lib.require_gpu(tets)
        tets = _i64_tets(tets)
        T, V, dev = int(tets.shape[0]), int(n_vertex), tets.device
        if T == 0 or V <= 0:
            raise ValueError("TetEdges: an empty tet list or no vertices")
        edges, tet_edge = tet_edges(tets, V)                          # (IndexError on an index outside [0, V))
        E = int(edges.shape[0])
        offsets, slots = _incidence_csr("deftet_edge_vertex_csr_i32", "deftet_edge_vertex_csr_workspace_bytes", edges, (None, V, E, 2),
                                        IndexError, "TetEdges: vertex index outside [0, %d)")
        self.tets = tets.to(torch.int32).contiguous()
        self.edges, self.tet_edge = edges.to(torch.int32).contiguous(), tet_edge.to(torch.int32).contiguous()
        self.offsets, self.slots = offsets, slots
        self.n_vertex, self.n_tet, self.n_edge, self.device = V, T, E, dev


class _MarchingTets(torch.autograd.Function):
    """flat outputs for the whole batch: (verts [Nv,3], vert_attr [Nv,C] | None, faces, edge_id, t, tet_id, offsets [2,B+1] on the
    host); marching_tets splits them by shape"""

    @staticmethod
    def forward(ctx, pos, field, attr, topology, iso, return_index):
        lib = _lib.load()
        top = topology
        B, V, T, E, dev = pos.shape[0], top.n_vertex, top.n_tet, top.n_edge, pos.device
        C = 0 if attr is None else int(attr.shape[2])
        ev = torch.empty(B, E, dtype=torch.int32, device=dev)
        offs = torch.empty(2, B + 1, dtype=torch.int32, device=dev)
        # the count pass leaves the output rows in its workspace for the fill pass: a tensor of this call, not the shared one
        ws = torch.empty(lib.deftet_marching_tets_workspace_bytes(B, T, E), dtype=torch.uint8, device=dev)
        _lib.call("deftet_marching_tets_count_f32", dev, field, top.edges, top.tets, B, V, T, E, iso, ev, offs, ws=ws)
        o = offs.tolist()                               # the one sync
        Nv, Nf = o[0][B], o[1][B]
        verts = torch.empty(Nv, 3, dtype=torch.float32, device=dev)
        vattr = torch.empty(Nv, C, dtype=torch.float32, device=dev) if C else None
        faces = torch.empty(Nf, 3, dtype=torch.int64, device=dev)
        edge_id = torch.empty(Nv, dtype=torch.int64, device=dev) if return_index else None
        t = torch.empty(Nv, dtype=torch.float32, device=dev) if return_index else None
        tet_id = torch.empty(Nf, dtype=torch.int64, device=dev) if return_index else None
        _lib.call("deftet_marching_tets_fill_f32", dev, pos, field, attr, C, top.edges, top.tets, top.tet_edge, ev, B, V, T, E, iso, Nv, Nf,
                  verts, vattr, faces, edge_id, t, tet_id, ws=ws)
        ctx.save_for_backward(pos, field, attr, ev, offs)
        ctx.topology, ctx.iso, ctx.offsets = top, iso, o
        outs = (verts, vattr, faces, edge_id, t, tet_id)
        ctx.mark_non_differentiable(*[x for x in outs[2:] if x is not None])
        ctx.set_materialize_grads(False)
        return outs + (o,)

    @staticmethod
    def backward(ctx, g_verts, g_vattr, *_unused):
        pos, field, attr, ev, offs = ctx.saved_tensors
        want = ctx.needs_input_grad[:3]
        top, Nv = ctx.topology, ctx.offsets[0][-1]
        B, V, dev = pos.shape[0], top.n_vertex, pos.device
        C = 0 if attr is None else int(attr.shape[2])
        want_attr = want[2] and attr is not None
        if not (want[0] or want[1] or want_attr):
            return (None,) * 6
        if Nv == 0 or (g_verts is None and g_vattr is None):
            return (torch.zeros_like(pos) if want[0] else None, torch.zeros_like(field) if want[1] else None,
                    torch.zeros_like(attr) if want_attr else None, None, None, None)
        g_verts, g_vattr = (None if g is None else _f32c(g) for g in (g_verts, g_vattr))
        gp = torch.empty(B, V, 3, device=dev, dtype=torch.float32) if want[0] else None
        gf = torch.empty(B, V, device=dev, dtype=torch.float32) if want[1] else None
        ga = torch.empty(B, V, C, device=dev, dtype=torch.float32) if want_attr else None
        _lib.call("deftet_marching_tets_bwd_f32", dev, g_verts, g_vattr, Nv, pos, field, attr, C, top.edges, top.offsets, top.slots, ev, offs,
                  B, V, top.n_edge, ctx.iso, gp, gf, ga)
        return gp, gf, ga, None, None, None


def marching_tets(pos, field, topology, iso=0.0, attr=None, return_index=False):
    """Marching tetrahedra on a per-vertex field: IsoMesh(verts, faces, vert_attr, edge_id, t, tet_id), each a list of B tensors
    (or None) — verts f32 [Nv_b,3] in ascending edge id, faces int64 [Nf_b,3] (local to the shape) in ascending tet id, vert_attr
    f32 [Nv_b,C] with attr f32 [B,V,C] (1 <= C <= 8); with return_index also edge_id int64 [Nv_b], t f32 [Nv_b], tet_id int64
    [Nf_b].  pos f32 [B,V,3] (or [V,3] for one shape), field f32 [B,V], topology a TetEdges.  A corner is inside iff field > iso
    (fp32, strict; NaN is outside); every crossing edge gets one vertex at t = (iso - f_min) / (f_max - f_min) between its lower
    and its higher vertex id, so the mesh is welded.  Normals point from the inside to the outside of positively oriented tets
    (a negatively oriented tet comes out flipped; nothing is detected).  Differentiable: the gradients of verts and vert_attr
    flow to pos, attr and field through one CSR reduction (no atomics, the same bits on every run).  One read-back (the offsets)."""
    if attr is not None and (attr.dim() not in (2, 3) or not 1 <= int(attr.shape[-1]) <= 8):
        raise _lib.DefTetHipError("marching_tets: attr [B,V,C] with 1 <= C <= 8 expected, got %s (DEFTET_EINVAL)" % (tuple(attr.shape),))
    _lib.require_gpu(pos, field, attr)
    if not isinstance(topology, TetEdges):
        raise TypeError("marching_tets: topology must be a hip_ops.TetEdges (built once per tet list)")
    iso = float(iso)
    if not np.isfinite(np.float32(iso)):
        raise _lib.DefTetHipError("marching_tets: iso = %r is not a finite float32 (DEFTET_EINVAL)" % iso)
    V = topology.n_vertex
    p = _f32c(pos)
    if p.dim() == 2:
        p = p[None]
    B = int(p.shape[0])
    if p.dim() != 3 or tuple(p.shape[1:]) != (V, 3) or p.device != topology.device:
        raise RuntimeError("marching_tets: pos [B,%d,3] or [%d,3] on %s expected, got %s" % (V, V, topology.device, tuple(pos.shape)))
    f = _f32c(field)
    if f.numel() != B * V:
        raise RuntimeError("marching_tets: field [%d,%d] expected, got %s" % (B, V, tuple(field.shape)))
    f = f.reshape(B, V)
    a = None
    if attr is not None:
        a = _f32c(attr)
        if a.numel() != B * V * int(a.shape[-1]):
            raise RuntimeError("marching_tets: attr [%d,%d,C] expected, got %s" % (B, V, tuple(attr.shape)))
        a = a.reshape(B, V, int(a.shape[-1]))
    verts, vattr, faces, edge_id, t, tet_id, o = _MarchingTets.apply(p, f, a, topology, iso, bool(return_index))

    def split(x, row):
        return None if x is None else [x[o[row][b]:o[row][b + 1]] for b in range(B)]
    return IsoMesh(split(verts, 0), split(faces, 1), split(vattr, 0), split(edge_id, 0), split(t, 0), split(tet_id, 1))


# --------------------------------------------------------------------------------- Loop subdivision
LOOP_SUBDIVIDE, LOOP_LIMIT = 0, 1                                    # the `mode` of deftet_loop_subdivide_fwd_f32 / _bwd_f32


class LoopTopology:
    """The topology of a triangle list for loop_subdivide / loop_limit, built once and reused (like TetEdges / FaceTopology), all
    integers on the GPU: `faces` int64 [F,3]; `edges` int32 [E,2], the unique undirected edges as (min,max) in lexicographic
    order; `face_edge` int32 [F,3], the edge ids of the local edges (f0,f1), (f1,f2), (f2,f0); `edge_nface` int32 [E], the number
    of (face, local edge) incidences; `edge_opp` int32 [E,2], the two opposite corners of an edge with exactly two incidences in
    ascending 3*f+k, (-1,-1) otherwise — such an edge is a CREASE (boundary and non-manifold alike); `vertex_kind` uint8 [V]: 0
    smooth (no crease edge, isolated vertices included), 1 crease (exactly two crease edges), 2 corner; `crease_nbr` int32 [V,2],
    the far ends of a crease vertex's two crease edges in ascending edge id, -1 otherwise; the vertex -> edge-end CSR
    `ev_offsets` int32 [V+1], `ev_slots` int32 [2E] (2*e+side) and the vertex -> face-corner CSR `fv_offsets`, `fv_slots` int32
    [3F] (3*f+corner), both ascending per vertex; `child_faces` int64 [4F,3], rows 4f..4f+3 = (a,mab,mca), (b,mbc,mab),
    (c,mca,mbc), (mab,mbc,mca) with m.. = V + the edge id (winding kept) — the faces of the subdivided mesh, whose V+E vertices
    are the old ones followed by one per edge.  IndexError for an index outside [0, n_vertex); ValueError for a face that names
    a vertex twice, for F = 0, n_vertex <= 0, V+E >= 2^31 or 4F >= 2^31.  One read-back (E and the flags; with `vertex_offsets`,
    the ascending vertex ranges [S+1] of disjoint shapes in one list, also `edge_offsets`, the S+1 first edge ids of the shapes).
    A snapshot of the list it was built from.  `device`: where to put a host list."""

    def __init__(self, faces_fx3, n_vertex, device=None, vertex_offsets=None):
        faces = torch.as_tensor(faces_fx3)
        if device is not None:
            faces = faces.to(device)
        _lib.require_gpu(faces)
        if faces.dim() != 2 or faces.shape[1] != 3:
            raise RuntimeError("LoopTopology: faces [F,3] expected, got %s" % (tuple(faces.shape),))
        faces = faces.to(dtype=torch.int64, copy=True).contiguous()   # ours: later in-place edits of the caller's list do not reach it
        F, V, dev = int(faces.shape[0]), int(n_vertex), faces.device
        if F == 0 or V <= 0:
            raise ValueError("LoopTopology: an empty face list or no vertices")
        if 4 * F >= 2 ** 31 or V >= 2 ** 31:
            raise ValueError("LoopTopology: 4 * n_face = %d or n_vertex = %d does not fit 31 bits" % (4 * F, V))
        lib = _lib.load()
        S = 0 if vertex_offsets is None else len(vertex_offsets) - 1
        voff = host_ints(vertex_offsets, dev, i32=True) if S else None
        counts = torch.empty(3 + (S + 1 if S else 0), dtype=torch.int32, device=dev)
        # the count pass leaves the sorted incidences in its workspace for the fill pass: a tensor of this call, not the shared one
        ws = torch.empty(lib.deftet_loop_topology_workspace_bytes(V, F), dtype=torch.uint8, device=dev)
        _lib.call("deftet_loop_topology_count_i64", dev, faces, F, V, voff, S, counts, ws=ws)
        c = counts.tolist()                                              # the one sync
        E = c[0]
        if c[1]:
            raise IndexError("LoopTopology: vertex index outside [0, %d)" % V)
        if c[2]:
            raise ValueError("LoopTopology: a face names a vertex twice")
        if V + E >= 2 ** 31:
            raise ValueError("LoopTopology: n_vertex + n_edge = %d does not fit 31 bits" % (V + E))

        def i32(*shape):
            return torch.empty(*shape, dtype=torch.int32, device=dev)
        self.edges, self.face_edge, self.edge_nface, self.edge_opp = i32(E, 2), i32(F, 3), i32(E), i32(E, 2)
        self.vertex_kind, self.crease_nbr = torch.empty(V, dtype=torch.uint8, device=dev), i32(V, 2)
        self.ev_offsets, self.ev_slots, self.fv_offsets, self.fv_slots = i32(V + 1), i32(2 * E), i32(V + 1), i32(3 * F)
        self.child_faces = torch.empty(4 * F, 3, dtype=torch.int64, device=dev)
        _lib.call("deftet_loop_topology_fill_i64", dev, faces, F, V, E, self.edges, self.face_edge, self.edge_nface, self.edge_opp,
                  self.vertex_kind, self.crease_nbr, self.ev_offsets, self.ev_slots, self.fv_offsets, self.fv_slots, self.child_faces, ws=ws)
        self.faces, self.n_vertex, self.n_face, self.n_edge, self.n_vertex_out, self.device = faces, V, F, E, V + E, dev
        self.edge_offsets = c[3:] if S else None


def _loop_tables(top):
    return (top.edges, top.edge_nface, top.edge_opp, top.vertex_kind, top.crease_nbr, top.ev_offsets, top.ev_slots)


class _LoopSubdivide(torch.autograd.Function):
    """(verts [B,V,3], attr [B,V,C] | None) -> (verts' [B,R,3], attr' [B,R,C] | None), R = V+E (mode 0) or V (mode 1, the limit)"""

    @staticmethod
    def forward(ctx, verts, attr, topology, mode):
        top = topology
        B, V, E, dev = int(verts.shape[0]), top.n_vertex, top.n_edge, verts.device
        C = 0 if attr is None else int(attr.shape[2])
        R = V + E if mode == LOOP_SUBDIVIDE else V
        out = torch.empty(B, R, 3, dtype=torch.float32, device=dev)
        oattr = torch.empty(B, R, C, dtype=torch.float32, device=dev) if C else None
        _lib.call("deftet_loop_subdivide_fwd_f32", dev, verts, attr, C, *_loop_tables(top), B, V, E, mode, out, oattr)
        ctx.topology, ctx.mode, ctx.shape = top, mode, (B, C)
        ctx.set_materialize_grads(False)
        return out, oattr

    @staticmethod
    def backward(ctx, g_verts, g_attr):
        top, mode, (B, C) = ctx.topology, ctx.mode, ctx.shape
        V, dev = top.n_vertex, top.device
        want_v, want_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and C > 0
        if not want_v:
            g_verts = None
        if not want_a:
            g_attr = None
        gv = ga = None
        if g_verts is not None or g_attr is not None:
            g_verts, g_attr = (None if g is None else _f32c(g) for g in (g_verts, g_attr))
            gv = torch.empty(B, V, 3, dtype=torch.float32, device=dev) if g_verts is not None else None
            ga = torch.empty(B, V, C, dtype=torch.float32, device=dev) if g_attr is not None else None
            _lib.call("deftet_loop_subdivide_bwd_f32", dev, g_verts, g_attr, C, *_loop_tables(top), top.face_edge, top.fv_offsets,
                      top.fv_slots, B, V, top.n_edge, top.n_face, mode, gv, ga)
        if want_v and gv is None:
            gv = torch.zeros(B, V, 3, dtype=torch.float32, device=dev)
        if want_a and ga is None:
            ga = torch.zeros(B, V, C, dtype=torch.float32, device=dev)
        return gv, ga, None, None


def _loop_apply(caller, verts, topology, attr, mode):
    if not isinstance(topology, LoopTopology):
        raise TypeError("%s: topology must be a hip_ops.LoopTopology (built once per face list)" % caller)
    if attr is not None and (attr.dim() not in (2, 3) or not 1 <= int(attr.shape[-1]) <= 8):
        raise _lib.DefTetHipError("%s: attr [B,V,C] with 1 <= C <= 8 expected, got %s (DEFTET_EINVAL)" % (caller, tuple(attr.shape)))
    _lib.require_gpu(verts, attr)
    V = topology.n_vertex
    p = _f32c(verts)
    single = p.dim() == 2
    if single:
        p = p[None]
    if p.dim() != 3 or tuple(p.shape[1:]) != (V, 3) or p.device != topology.device:
        raise RuntimeError("%s: verts [B,%d,3] or [%d,3] on %s expected, got %s" % (caller, V, V, topology.device, tuple(verts.shape)))
    B = int(p.shape[0])
    a = None
    if attr is not None:
        a = _f32c(attr)
        if a.numel() != B * V * int(a.shape[-1]) or a.device != p.device:
            raise RuntimeError("%s: attr [%d,%d,C] on %s expected, got %s" % (caller, B, V, p.device, tuple(attr.shape)))
        a = a.reshape(B, V, int(a.shape[-1]))
    out, oattr = _LoopSubdivide.apply(p, a, topology, mode)
    if single and verts.dim() == 2:
        out, oattr = out[0], None if oattr is None else oattr[0]
    return out, oattr


def loop_subdivide(verts, topology, attr=None):
    """One level of Loop subdivision: (verts' f32 [B,V+E,3], attr' f32 [B,V+E,C] | None) from verts f32 [B,V,3] (or [V,3]: the
    results then come without the batch axis) and attr f32 [B,V,C], 1 <= C <= 8, on a LoopTopology.  Rows 0..V-1 are the
    repositioned old vertices, row V+e is the vertex of edge e; the faces of the result are topology.child_faces.  Warren's
    weights: an interior edge (a,b) with opposite corners (c,d) gives 3/8 (a+b) + 1/8 (c+d), a crease edge 1/2 (a+b); a smooth
    vertex of valence n moves to (1 - n beta) v + beta sum of its neighbours, beta = 3/16 for n = 3 and 3/(8n) otherwise, a
    crease vertex to 3/4 v + 1/8 (its two crease neighbours), a corner stays.  Attributes take the same weights.  Every sum in
    fp32 in one order (own term, then the edge-end slots ascending); differentiable by the transpose, one gather per old vertex
    over both CSRs: no atomics, the same bits on every run, for every batch size."""
    return _loop_apply("loop_subdivide", verts, topology, attr, LOOP_SUBDIVIDE)


def loop_limit(verts, topology, attr=None):
    """The limit positions of the Loop surface at the vertices: (f32 [B,V,3], attr [B,V,C] | None).  Smooth: (1 - n gamma) v +
    gamma sum of the neighbours, gamma = 1 / (n + 3/(8 beta)) (1/12 at n = 6, 1/5 at n = 3); crease: 2/3 v + 1/6 (the two crease
    neighbours); corner: v.  Differentiable like loop_subdivide."""
    return _loop_apply("loop_limit", verts, topology, attr, LOOP_LIMIT)


def loop_subdivide_mesh(verts, faces, attr=None, levels=1, limit=False):
    """`levels` rounds of loop_subdivide on one mesh (a batch [B,V,3] shares the faces): (verts, faces int64, attr | None).  One
    LoopTopology (one read-back) per level; limit=True projects the last level's vertices to their limit positions."""
    levels = operator.index(levels)
    if levels < 0:
        raise ValueError("loop_subdivide_mesh: levels = %d is negative" % levels)
    _lib.require_gpu(verts, faces, attr)
    top = None
    for _ in range(levels):
        top = LoopTopology(faces, int(verts.shape[-2]))
        verts, attr = loop_subdivide(verts, top, attr)
        faces = top.child_faces
    if limit:
        verts, attr = loop_limit(verts, LoopTopology(faces, int(verts.shape[-2])), attr)
    return verts, faces, attr


def loop_subdivide_list(verts_list, faces_list, attr_list=None, levels=1, limit=False):
    """loop_subdivide_mesh for a ragged list of shapes (what marching_tets returns): (list of verts, list of faces, list of attr |
    None), each shape's result bit for bit that of its own call.  The shapes are concatenated into one disjoint mesh with offset
    indices: one topology build, one launch sequence and one read-back per level for the whole list.  Edges sort by (min,max) and
    the shapes occupy ascending index ranges, so a shape's rows are two contiguous runs — its old vertices, its edge vertices —
    and its faces are renumbered to local indices.  A shape without faces comes back as it is."""
    levels = operator.index(levels)
    if levels < 0:
        raise ValueError("loop_subdivide_list: levels = %d is negative" % levels)
    n = len(verts_list)
    if len(faces_list) != n or (attr_list is not None and len(attr_list) != n):
        raise RuntimeError("loop_subdivide_list: %d verts, %d faces%s" % (n, len(faces_list), "" if attr_list is None else ", %d attrs" % len(attr_list)))
    verts_list, faces_list = list(verts_list), [f.long() for f in faces_list]
    attr_list = None if attr_list is None else list(attr_list)
    live = [i for i in range(n) if int(faces_list[i].shape[0]) > 0]
    if not live or (levels == 0 and not limit):
        return verts_list, faces_list, attr_list
    _lib.require_gpu(*[verts_list[i] for i in live])
    dev = verts_list[live[0]].device
    vs, fs = [verts_list[i] for i in live], [faces_list[i] for i in live]
    ats = None if attr_list is None else [attr_list[i] for i in live]

    def offsets(counts):
        out = [0]
        for c in counts:
            out.append(out[-1] + c)
        return out

    def per_element(values, counts):
        """values[s] repeated counts[s] times, int64 on the device (no read-back: the total is known on the host)"""
        return torch.repeat_interleave(host_ints(values, dev, i64=True), host_ints(counts, dev, i64=True), output_size=sum(counts))

    for level in range(levels + (1 if limit else 0)):
        nv, nf = [int(v.shape[0]) for v in vs], [int(f.shape[0]) for f in fs]
        voff, foff = offsets(nv), offsets(nf)
        V = voff[-1]
        # one disjoint mesh: shape s on the vertex range voff[s] .. voff[s+1]
        v, f = torch.cat(vs, 0), torch.cat(fs, 0) + per_element(voff[:-1], nf)[:, None]
        a = None if ats is None else torch.cat(ats, 0)
        top = LoopTopology(f, V, vertex_offsets=voff)
        if level == levels:                                                   # the limit projection of the last level
            v, a = loop_limit(v, top, a)
            vs = [v[voff[s]:voff[s + 1]] for s in range(len(vs))]
            ats = None if a is None else [a[voff[s]:voff[s + 1]] for s in range(len(vs))]
            break
        v, a = loop_subdivide(v, top, a)
        eoff = top.edge_offsets
        ne = [y - x for x, y in zip(eoff, eoff[1:])]
        # row r of the fine mesh -> its index inside its shape: an old vertex r - voff[s], an edge vertex nv[s] + (r - V - eoff[s])
        first = torch.cat([per_element(voff[:-1], nv), per_element([V + eoff[s] - nv[s] for s in range(len(vs))], ne)])
        local = (torch.arange(V + top.n_edge, device=dev) - first)[top.child_faces]

        def rows_of(x, s):
            return torch.cat([x[voff[s]:voff[s + 1]], x[V + eoff[s]:V + eoff[s + 1]]], 0)
        ats = None if a is None else [rows_of(a, s) for s in range(len(vs))]
        vs = [rows_of(v, s) for s in range(len(vs))]
        fs = [local[4 * foff[s]:4 * foff[s + 1]] for s in range(len(fs))]
    for k, i in enumerate(live):
        verts_list[i], faces_list[i] = vs[k], fs[k]
        if attr_list is not None:
            attr_list[i] = ats[k]
    return verts_list, faces_list, attr_list


# --------------------------------------------------------------------------------- components of a triangle surface, its clean-up
MESH_EDGE, MESH_VERTEX = 0, 1                                        # the `connectivity` of deftet_mesh_components_i64
MESH_BY_FACES, MESH_BY_AREA = 0, 1                                   # the `largest_by` of deftet_mesh_cleanup_count_i64
_MESH_CONNECTIVITY = {"edge": MESH_EDGE, "vertex": MESH_VERTEX}
_MESH_LARGEST_BY = {"faces": MESH_BY_FACES, "area": MESH_BY_AREA}


class MeshComponents(collections.namedtuple("MeshComponents", "labels count n_face area volume boundary_edges nonmanifold_edges "
                                                              "misoriented_edges")):
    """The connected components of a triangle list (mesh_components), all on the device: labels int32 [F], the smallest face
    index of every face's component; count int32 [S], components per shape; and at the label's index, 0 elsewhere: n_face,
    boundary_edges, nonmanifold_edges, misoriented_edges int32 [F], area and volume float64 [F] (None without verts)."""
    __slots__ = ()

    @property
    def closed(self):
        """bool [F], at the label's index: the component has no boundary, non-manifold or misoriented edge"""
        return (self.n_face > 0) & (self.boundary_edges == 0) & (self.nonmanifold_edges == 0) & (self.misoriented_edges == 0)


CleanMesh = collections.namedtuple("CleanMesh", "verts faces attr vertex_map face_map components")


def _mesh_choice(caller, what, value, table):
    if value not in table:
        raise ValueError("%s: %s = %r is none of %s" % (caller, what, value, ", ".join(repr(k) for k in table)))
    return table[value]


def _surface_mesh_args(caller, faces, n_vertex, verts, face_offsets, vertex_offsets):
    """(faces int64 [F,3] contiguous, verts f32 [V,3] | None, F, V, face offsets, vertex offsets: host lists of S + 1 entries)"""
    if not isinstance(faces, torch.Tensor):
        raise _expected(caller, "faces: an integer tensor [F,3]", type(faces).__name__)
    _lib.require_gpu(faces, verts)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int64, torch.int32):
        raise _expected(caller, "faces int64 [F,3]", "%s %s" % (faces.dtype, tuple(faces.shape)))
    F, V = int(faces.shape[0]), int(n_vertex)
    if 3 * F >= 2 ** 31 or V >= 2 ** 31:
        raise ValueError("%s: 3 * n_face = %d or n_vertex = %d does not fit 31 bits" % (caller, 3 * F, V))
    if V < 0 or (F > 0 and V == 0):
        raise ValueError("%s: n_vertex = %d with %d faces" % (caller, V, F))
    if verts is not None and (verts.dim() != 2 or tuple(verts.shape) != (V, 3) or verts.dtype != torch.float32 or verts.device != faces.device):
        raise _expected(caller, "verts float32 [%d,3] on %s" % (V, faces.device), "%s %s on %s" % (verts.dtype, tuple(verts.shape), verts.device))
    if (face_offsets is None) != (vertex_offsets is None):
        raise ValueError("%s: face_offsets and vertex_offsets go together" % caller)
    foff = [0, F] if face_offsets is None else [int(x) for x in face_offsets]
    voff = [0, V] if vertex_offsets is None else [int(x) for x in vertex_offsets]
    for name, off, end in (("face_offsets", foff, F), ("vertex_offsets", voff, V)):
        if len(off) < 2 or len(off) != len(foff) or off[0] != 0 or off[-1] != end or any(y < x for x, y in zip(off, off[1:])):
            raise ValueError("%s: %s must ascend from 0 to %d with one entry per shape and one more, got %s" % (caller, name, end, off))
    return faces.to(torch.int64).contiguous(), (None if verts is None else verts.contiguous()), F, V, foff, voff


def _mesh_raise(caller, flags, V):
    """the flags of the labelling, read back: out of range, a vertex named twice, a broken union-find"""
    if flags[0]:
        raise IndexError("%s: vertex index outside [0, %d)" % (caller, V))
    if flags[1]:
        raise ValueError("%s: a face names a vertex twice" % caller)
    if flags[2]:
        raise RuntimeError("%s: the union-find met a broken chain or ran out of its trip bound (%d times)" % (caller, flags[2]))


def _mesh_components_out(F, S, dev, measures):
    def i32(n):
        return torch.empty(n, dtype=torch.int32, device=dev)

    def f64():
        return torch.empty(F, dtype=torch.float64, device=dev) if measures else None
    # in the order of the C entries: labels, n_face, boundary, non-manifold, misoriented, area, volume, count
    return [i32(F), i32(F), i32(F), i32(F), i32(F), f64(), f64(), torch.zeros(S, dtype=torch.int32, device=dev) if F == 0 else i32(S)]


def _mesh_components_result(parts):
    labels, n_face, bnd, nm, mis, area, volume, count = parts
    return MeshComponents(labels, count, n_face, area, volume, bnd, nm, mis)


def mesh_components(faces, n_vertex, verts=None, connectivity="edge", check=True, face_offsets=None, vertex_offsets=None):
    """Connected components of a triangle list: MeshComponents(labels, count, n_face, area, volume, boundary_edges,
    nonmanifold_edges, misoriented_edges), all on the device.  faces int64 [F,3] over n_vertex vertices (F = 0 gives empty
    results).  connectivity "edge": two faces are connected when they share an undirected vertex pair, whatever the number of
    faces that meet on it (the three faces of a book are one piece, a bow-tie is two); "vertex": when they share a vertex (the
    bow-tie is one).  labels int32 [F] = the SMALLEST face index of the component, so the result does not depend on the
    schedule.  At the label's index, 0 elsewhere: n_face; boundary_edges (edges with one incidence), nonmanifold_edges (more
    than two), misoriented_edges (two incidences running the same direction); with verts float32 [V,3] also area = sum 1/2
    |(b-a) x (c-a)| and volume = sum a . (b x c) / 6 as float64, every term in double from the widened positions and summed in
    an order that depends on the component's own ascending face list only (no float atomics: the same bits on every run, next
    to whatever other components).  `closed` = the three edge counts are 0.  count int32 [S] = components per shape:
    face_offsets / vertex_offsets (S + 1 ascending host integers each) describe S disjoint shapes in one list, as
    loop_subdivide_list concatenates them; one shape without them.
    Nothing of the results is read back.  The flags are (twelve bytes, check=True): IndexError for an index outside
    [0, n_vertex) — such a corner is counted and never followed —, ValueError for a face that names a vertex twice,
    RuntimeError for a broken union-find.  ValueError for 3 F >= 2^31 or n_vertex >= 2^31."""
    caller = "mesh_components"
    conn = _mesh_choice(caller, "connectivity", connectivity, _MESH_CONNECTIVITY)
    f, v, F, V, foff, _voff = _surface_mesh_args(caller, faces, n_vertex, verts, face_offsets, vertex_offsets)
    S, dev = len(foff) - 1, f.device
    parts = _mesh_components_out(F, S, dev, v is not None)
    if F == 0:
        return _mesh_components_result(parts)
    lib = _lib.load()
    flags = torch.empty(3, dtype=torch.int32, device=dev)
    _lib.call("deftet_mesh_components_i64", dev, f, F, V, v, host_ints(foff, dev, i32=True), S, conn, *parts, flags,
              ws=lib.deftet_mesh_components_workspace_bytes(V, F, S))
    if check:
        _mesh_raise(caller, flags.tolist(), V)
    return _mesh_components_result(parts)


class _MeshGather(torch.autograd.Function):
    """(verts [V,3], attr [V,C] | None) -> their rows at vertex_map [V'] (ascending, injective)"""

    @staticmethod
    def forward(ctx, verts, attr, vertex_map):
        V, Vk, dev = int(verts.shape[0]), int(vertex_map.shape[0]), verts.device
        C = 0 if attr is None else int(attr.shape[1])
        out = torch.empty(Vk, 3, dtype=torch.float32, device=dev)
        oattr = torch.empty(Vk, C, dtype=torch.float32, device=dev) if C else None
        _lib.call("deftet_mesh_gather_fwd_f32", dev, verts, attr, C, vertex_map, V, Vk, out, oattr)
        ctx.save_for_backward(vertex_map)
        ctx.shape = (V, C)
        ctx.set_materialize_grads(False)
        return out, oattr

    @staticmethod
    def backward(ctx, g_verts, g_attr):
        (vertex_map,) = ctx.saved_tensors
        V, C = ctx.shape
        Vk, dev = int(vertex_map.shape[0]), vertex_map.device
        want_v, want_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and C > 0
        if not want_v:
            g_verts = None
        if not want_a:
            g_attr = None
        gv = ga = None
        if g_verts is not None or g_attr is not None:
            g_verts, g_attr = (None if g is None else _f32c(g) for g in (g_verts, g_attr))
            gv = torch.empty(V, 3, dtype=torch.float32, device=dev) if g_verts is not None else None
            ga = torch.empty(V, C, dtype=torch.float32, device=dev) if g_attr is not None else None
            _lib.call("deftet_mesh_gather_bwd_f32", dev, g_verts, g_attr, C, vertex_map, V, Vk, gv, ga)
        if want_v and gv is None:
            gv = torch.zeros(V, 3, dtype=torch.float32, device=dev)
        if want_a and ga is None:
            ga = torch.zeros(V, C, dtype=torch.float32, device=dev)
        return gv, ga, None


def _mesh_cleanup_flat(caller, verts, faces, attr, face_offsets, vertex_offsets, keep_largest, min_faces, min_area, drop_voids, largest_by,
                       connectivity, return_components):
    """the clean-up of one face list of S disjoint shapes: (verts', faces' numbered inside their shapes, attr', vertex_map,
    face_map — old indices of the whole list —, MeshComponents | None, kept-face offsets, kept-vertex offsets: host lists)"""
    conn = _mesh_choice(caller, "connectivity", connectivity, _MESH_CONNECTIVITY)
    by = _mesh_choice(caller, "largest_by", largest_by, _MESH_LARGEST_BY)
    min_faces, min_area = operator.index(min_faces), float(min_area)
    if min_faces < 0 or not min_area >= 0.0:
        raise ValueError("%s: min_faces = %d or min_area = %r is negative" % (caller, min_faces, min_area))
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2:
        raise _expected(caller, "verts float32 [V,3]", verts if isinstance(verts, torch.Tensor) else type(verts).__name__)
    _lib.require_gpu(verts, attr)
    f, v, F, V, foff, voff = _surface_mesh_args(caller, faces, int(verts.shape[0]), verts, face_offsets, vertex_offsets)
    S, dev = len(foff) - 1, f.device
    a = None
    if attr is not None:
        if attr.dim() != 2 or int(attr.shape[0]) != V or not 1 <= int(attr.shape[1]) <= 8 or attr.dtype != torch.float32 or attr.device != dev:
            raise _expected(caller, "attr float32 [%d,C] with 1 <= C <= 8 on %s" % (V, dev), "%s %s on %s" % (attr.dtype, tuple(attr.shape), attr.device))
        a = attr.contiguous()
    if F == 0:                                                                # nothing to label: the mesh comes back as it is
        comps = _mesh_components_result(_mesh_components_out(0, S, dev, True)) if return_components else None
        every = torch.arange(V, dtype=torch.int64, device=dev)
        return v, f, a, every, torch.empty(0, dtype=torch.int64, device=dev), comps, [0] * (S + 1), list(voff)
    lib = _lib.load()
    measures = bool(drop_voids) or min_area > 0.0 or (bool(keep_largest) and by == MESH_BY_AREA) or bool(return_components)
    parts = _mesh_components_out(F, S, dev, measures)
    counts = torch.empty(3 + 2 * (S + 1), dtype=torch.int32, device=dev)
    foff_d, voff_d = host_ints(foff, dev, i32=True), host_ints(voff, dev, i32=True)
    # the count pass leaves its scans in the workspace for the fill pass: a tensor of this call, not the shared one
    ws = torch.empty(lib.deftet_mesh_components_workspace_bytes(V, F, S), dtype=torch.uint8, device=dev)
    _lib.call("deftet_mesh_cleanup_count_i64", dev, f, F, V, v if measures else None, foff_d, voff_d, S, conn, int(bool(keep_largest)),
              min_faces, min_area, int(bool(drop_voids)), by, *parts, counts, ws=ws)
    c = counts.tolist()                                                       # the one read-back: flags and offsets
    _mesh_raise(caller, c[:3], V)
    fo, vo = c[3:3 + S + 1], c[3 + S + 1:]
    Fk, Vk = fo[-1], vo[-1]
    faces_out = torch.empty(Fk, 3, dtype=torch.int64, device=dev)
    vertex_map = torch.empty(Vk, dtype=torch.int64, device=dev)
    face_map = torch.empty(Fk, dtype=torch.int64, device=dev)
    if Fk:
        _lib.call("deftet_mesh_cleanup_fill_i64", dev, f, F, V, foff_d, voff_d, S, Fk, Vk, faces_out, vertex_map, face_map, ws=ws)
        v_out, a_out = _MeshGather.apply(v, a, vertex_map)
    else:
        v_out, a_out = v[:0], None if a is None else a[:0]
    return v_out, faces_out, a_out, vertex_map, face_map, (_mesh_components_result(parts) if return_components else None), fo, vo


def mesh_cleanup(verts, faces, attr=None, keep_largest=False, min_faces=0, min_area=0.0, drop_voids=False, largest_by="faces",
                 connectivity="edge", return_components=False):
    """Cleans a triangle surface on the device and compacts it: CleanMesh(verts, faces, attr, vertex_map, face_map, components).
    verts float32 [V,3], faces int64 [F,3], attr float32 [V,C] (1 <= C <= 8) or None.  One device sequence in this order, nothing
    read back in between: the faces are labelled and measured (mesh_components); drop_voids drops every CLOSED component with
    volume < 0 — marching_tets orients normals from inside to outside, so the shell of an enclosed cavity encloses negative
    volume; min_faces = m > 0 drops the components with fewer than m faces; min_area = a > 0 those with area < a;
    keep_largest keeps, of what is left, the component with the most faces (largest_by="faces", integers only) or the largest
    area (largest_by="area"), the smaller label among equals; an empty mesh stays empty.  drop_voids alone leaves a floater
    INSIDE a cavity in place: with its cavity gone it becomes a shell inside the solid, which keep_largest or min_faces removes.
    Kept faces stay in ascending old index and are renumbered; vertices that no kept face references are dropped, the others
    stay in ascending old index: the ascending edge-id and tet-id orders of marching_tets survive.  vertex_map int64 [V'] and
    face_map int64 [F'] hold the old indices; verts' = verts[vertex_map] and attr' = attr[vertex_map] come from one launch and
    are differentiable (the backward copies the gradient rows to the kept vertices and writes zeros everywhere else: no atomic,
    no sum).  components (return_components=True): the MeshComponents of the input list, the labelling the selection was made
    on.  One read-back per call: the counts together with the flags (IndexError / ValueError / RuntimeError as in
    mesh_components).  A mesh without faces comes back as it is."""
    v, f, a, vmap, fmap, comps, _fo, _vo = _mesh_cleanup_flat("mesh_cleanup", verts, faces, attr, None, None, keep_largest, min_faces, min_area,
                                                             drop_voids, largest_by, connectivity, return_components)
    return CleanMesh(v, f, a, vmap, fmap, comps)


def mesh_cleanup_list(mesh_or_verts, faces_list=None, attr_list=None, keep_largest=False, min_faces=0, min_area=0.0, drop_voids=False,
                      largest_by="faces", connectivity="edge", return_maps=False):
    """mesh_cleanup for a ragged list of shapes: an IsoMesh as marching_tets returns it, or lists of verts, faces and (optionally)
    attrs.  The shapes are concatenated into one disjoint mesh with offset indices: one launch sequence and ONE read-back for
    the whole batch; then they are cut back out, every shape bit for bit what its own mesh_cleanup call gives (a component's
    sums depend on its own face list only).  Returns an IsoMesh of lists; edge_id, t and tet_id of the input, where present,
    are indexed through the maps.  return_maps=True: (IsoMesh, list of vertex_map, list of face_map), local to the shapes.
    Shapes with no faces pass through unchanged."""
    caller = "mesh_cleanup_list"
    if isinstance(mesh_or_verts, IsoMesh):
        if faces_list is not None or attr_list is not None:
            raise RuntimeError("%s: an IsoMesh brings its own faces and attributes" % caller)
        verts_list, faces_list, attr_list, edge_id, t, tet_id = mesh_or_verts
    else:
        verts_list, edge_id, t, tet_id = mesh_or_verts, None, None, None
    if faces_list is None:
        raise RuntimeError("%s: lists of verts and faces (or an IsoMesh) expected" % caller)
    n = len(verts_list)
    for name, other in (("faces", faces_list), ("attrs", attr_list), ("edge_id", edge_id), ("t", t), ("tet_id", tet_id)):
        if other is not None and len(other) != n:
            raise RuntimeError("%s: %d verts, %d %s" % (caller, n, len(other), name))
    # checked before any shape is skipped: a wrong option is wrong for an empty batch as well
    _mesh_choice(caller, "connectivity", connectivity, _MESH_CONNECTIVITY)
    _mesh_choice(caller, "largest_by", largest_by, _MESH_LARGEST_BY)
    verts_out, faces_out = list(verts_list), list(faces_list)
    attr_out = None if attr_list is None else list(attr_list)
    edge_out, t_out, tet_out = (None if x is None else list(x) for x in (edge_id, t, tet_id))
    live = [i for i in range(n) if int(faces_list[i].shape[0]) > 0]
    vmaps = [None] * n
    fmaps = [None] * n
    if live:
        nv, nf = [int(verts_list[i].shape[0]) for i in live], [int(faces_list[i].shape[0]) for i in live]
        voff, foff = [0], [0]
        for x, y in zip(nv, nf):
            voff.append(voff[-1] + x)
            foff.append(foff[-1] + y)
        _lib.require_gpu(*[verts_list[i] for i in live])
        dev = verts_list[live[0]].device
        first = torch.repeat_interleave(host_ints(voff[:-1], dev, i64=True), host_ints(nf, dev, i64=True), output_size=foff[-1])
        v = torch.cat([verts_list[i] for i in live], 0)
        f = torch.cat([faces_list[i].long() for i in live], 0) + first[:, None]
        a = None if attr_list is None else torch.cat([attr_list[i] for i in live], 0)
        v2, f2, a2, vmap, fmap, _comps, fo, vo = _mesh_cleanup_flat(caller, v, f, a, foff, voff, keep_largest, min_faces, min_area, drop_voids,
                                                                    largest_by, connectivity, False)
        for s, i in enumerate(live):
            vs, fs = slice(vo[s], vo[s + 1]), slice(fo[s], fo[s + 1])
            verts_out[i], faces_out[i] = v2[vs], f2[fs]
            if attr_out is not None:
                attr_out[i] = a2[vs]
            vmaps[i], fmaps[i] = vmap[vs] - voff[s], fmap[fs] - foff[s]
            if edge_out is not None:
                edge_out[i] = edge_id[i][vmaps[i]]
            if t_out is not None:
                t_out[i] = t[i][vmaps[i]]
            if tet_out is not None:
                tet_out[i] = tet_id[i][fmaps[i]]
    out = IsoMesh(verts_out, faces_out, attr_out, edge_out, t_out, tet_out)
    if not return_maps:
        return out
    for i in range(n):
        if vmaps[i] is None:                                                  # a shape without faces: as it is
            dev = verts_list[i].device
            vmaps[i] = torch.arange(int(verts_list[i].shape[0]), dtype=torch.int64, device=dev)
            fmaps[i] = torch.empty(0, dtype=torch.int64, device=dev)
    return out, vmaps, fmaps


# --------------------------------------------------------------------------------- rendering from the vertices
class FaceTopology:
    """A face list for face_gather, built once and reused (like TetTopology / VertexAdjacency): `faces` int64 [F,3] on the GPU
    and the CSR of its (face, corner) incidences per vertex — `offsets` int32 [V+1], `slots` int32 [3F] holding 3*f+corner in
    ascending order per vertex.  Raises on an index outside [0, n_vertex).  The object is a snapshot of the list it was built
    from: a new face list (after a subdivision or a deletion) means a new object.  `device`: where to put a host list."""

    def __init__(self, faces_fx3, n_vertex, device=None):
        faces = torch.as_tensor(faces_fx3)
        if device is not None:
            faces = faces.to(device)
        _lib.require_gpu(faces)
        if faces.dim() != 2 or faces.shape[1] != 3:
            raise RuntimeError("FaceTopology: faces [F,3] expected")
        faces = faces.to(dtype=torch.int64, copy=True).contiguous()   # ours: later in-place edits of the caller's list do not reach it
        F, V, dev = faces.shape[0], int(n_vertex), faces.device
        offsets, slots = _incidence_csr("deftet_face_vertex_csr_i32", "deftet_face_vertex_csr_workspace_bytes", faces, (None, V, F, 3),
                                        RuntimeError, "FaceTopology: face index out of range [0, %d)")
        self.faces, self.n_vertex, self.n_face = faces, V, F
        self.offsets, self.slots, self.device = offsets, slots, dev


def _batched(t, last, what):
    """[V,last] -> [1,V,last]; [B,V,last] stays"""
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or t.shape[2] != last:
        raise RuntimeError("project_vertices: %s [V,%d] or [B,V,%d] expected" % (what, last, last))
    return _f32c(t)


class _ProjectVertices(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, features, rot, cam_pos, proj, multiplier, depth):
        _lib.require_gpu(points, features, rot, cam_pos, proj)
        rot, cam_pos, proj = _f32c(rot), _f32c(cam_pos), _f32c(proj).reshape(-1)
        B = rot.shape[0]
        if rot.shape != (B, 3, 3) or cam_pos.shape != (B, 3) or proj.numel() != 3:
            raise RuntimeError("project_vertices: cameras (rotation [B,3,3], position [B,3], projection [3]) expected")
        pos = _batched(points, 3, "points")
        feat = _batched(features, features.shape[-1], "features")
        V, D = pos.shape[1], feat.shape[2]
        if feat.shape[1] != V or pos.shape[0] not in (1, B) or feat.shape[0] not in (1, B) or D < 1:
            raise RuntimeError("project_vertices: points and features must share V and have batch 1 or %d" % B)
        dev, Do = pos.device, D + (1 if depth else 0)
        z = torch.empty(B, V, device=dev, dtype=torch.float32)
        xy = torch.empty(B, V, 2, device=dev, dtype=torch.float32)
        act = torch.empty(B, V, Do, device=dev, dtype=torch.float32)
        _lib.call("deftet_project_vertices_fwd_f32", dev, pos, feat, rot, cam_pos, proj, multiplier, int(depth), z, xy, act, B, V, D,
                  pos.shape[0], feat.shape[0])
        ctx.save_for_backward(pos, feat, rot, cam_pos, proj)   # the inputs: the backward recomputes the camera space in fp64
        ctx.args = (multiplier, bool(depth), points.shape, features.shape)
        ctx.mark_non_differentiable(z)                          # z reaches the loss through the depth channel of `act` only
        ctx.set_materialize_grads(False)
        return z, xy, act

    @staticmethod
    def backward(ctx, _g_z, g_xy, g_act):
        pos, feat, rot, cam_pos, proj = ctx.saved_tensors
        multiplier, depth, pshape, fshape = ctx.args
        want_p, want_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g_xy is None and g_act is None) or not (want_p or want_f):
            return (None,) * 7
        B, Bp, Bf, V, D, dev = rot.shape[0], pos.shape[0], feat.shape[0], pos.shape[1], feat.shape[2], pos.device
        g_xy, g_act = (None if g is None else _f32c(g) for g in (g_xy, g_act))
        gp = torch.empty(Bp, V, 3, device=dev, dtype=torch.float32) if want_p else None
        gf = torch.empty(Bf, V, D, device=dev, dtype=torch.float32) if want_f else None
        _lib.call("deftet_project_vertices_bwd_f32", dev, g_xy, g_act, pos, feat, rot, cam_pos, proj, multiplier, int(depth), gp, gf,
                  B, V, D, Bp, Bf)
        return (gp.reshape(pshape) if want_p else None, gf.reshape(fshape) if want_f else None, None, None, None, None, None)


def project_vertices(points, features, cameras, multiplier=1.0, depth=False):
    """(z [B,V], xy [B,V,2], act [B,V,Do]) of points [V,3] | [B,V,3] and features [V,D] | [B,V,D] under cameras = (rotation
    [B,3,3], position [B,3], projection [3] or [3,1]): camera-space depth, image coordinates times `multiplier` (`perspective`,
    3_model/cameraop.py:19-33, 3_model/deftet.py:468) and sigmoid(features); with depth=True Do = D + 1 and act[..., 0] is the
    camera-space z, not squashed (3_model/deftet.py:452-455, deftetrneder.py:78-89).  A [V,*] or [1,V,*] input is shared by the B
    views without being repeated; its gradient is the sum over the views in ascending b.  Differentiable in points and features
    (through xy and act; z is not differentiable — the rasterizer has no gradient for it); cameras get no gradient."""
    rot, cam_pos, proj = cameras
    return _ProjectVertices.apply(points, features, rot, cam_pos, proj, float(multiplier), bool(depth))


class _FaceGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, xy, act, topology):
        _lib.require_gpu(z, xy, act)
        z, xy, act = _f32c(z), _f32c(xy), _f32c(act)
        B, V = z.shape[0], topology.n_vertex
        F, Do = topology.n_face, act.shape[-1]
        if z.shape != (B, V) or xy.shape != (B, V, 2) or act.shape != (B, V, Do) or Do < 1 or z.device != topology.device:
            raise RuntimeError("face_gather: z [B,V], xy [B,V,2], act [B,V,Do] on the topology's device with V = %d expected" % V)
        dev = z.device
        face_z = torch.empty(B, F, 3, device=dev, dtype=torch.float32)
        face_xy = torch.empty(B, F, 3, 2, device=dev, dtype=torch.float32)
        face_feat = torch.empty(B, F, 3, Do, device=dev, dtype=torch.float32)
        # (no flag: the topology checked its indices when it was built)
        _lib.call("deftet_face_gather_fwd_f32", dev, z, xy, act, topology.faces, face_z, face_xy, face_feat, None, B, V, F, Do)
        ctx.topology, ctx.sizes = topology, (B, V, F, Do)
        ctx.mark_non_differentiable(face_z)
        ctx.set_materialize_grads(False)
        return face_z, face_xy, face_feat

    @staticmethod
    def backward(ctx, _g_face_z, g_face_xy, g_face_feat):
        if g_face_xy is None and g_face_feat is None:
            return None, None, None, None
        top = ctx.topology
        B, V, F, Do = ctx.sizes
        dev = top.device
        g_face_xy, g_face_feat = (None if g is None else _f32c(g) for g in (g_face_xy, g_face_feat))
        g_xy = torch.empty(B, V, 2, device=dev, dtype=torch.float32)
        g_act = torch.empty(B, V, Do, device=dev, dtype=torch.float32)
        _lib.call("deftet_face_gather_bwd_f32", dev, g_face_xy, g_face_feat, top.offsets, top.slots, g_xy, g_act, B, V, F, Do)
        return None, g_xy, g_act, None


def face_gather(z, xy, act, topology):
    """(face_z [B,F,3], face_xy [B,F,3,2], face_feat [B,F,3,Do]): the rows of z [B,V], xy [B,V,2], act [B,V,Do] at the corners of
    `topology` (a FaceTopology) — the rasterizer's three dense inputs, written by one launch (the three `vertex2face` gathers of
    5_rendereq/deftetrneder.py:93-95).  The backward sums the per-corner gradients of face_xy and face_feat per vertex through the
    topology's CSR, one after the other in slot order: no atomics, the same bits on every run.  face_z is not differentiable."""
    if not isinstance(topology, FaceTopology):
        raise TypeError("face_gather: topology must be a hip_ops.FaceTopology")
    return _FaceGather.apply(z, xy, act, topology)


# ------------------------------------------------------------------------------------
# point-voxel operators (pointvoxel.hip): average voxelization and trilinear sampling of voxel volumes
# ------------------------------------------------------------------------------------
def _pv_need(t, dtype, what):
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s (got %s)" % (what, str(dtype).replace("torch.", ""), str(t.dtype).replace("torch.", "")))
    return t.contiguous()


def _grid_bytes(B, N, size):
    """the workspace bytes of the operator whose grids have the spatial shape `size`: (R, R, R) volumes or (H, W) maps"""
    lib = _lib.load()
    return lib.deftet_pointvoxel_workspace_bytes(B, N, size[0]) if len(size) == 3 else lib.deftet_image_sample_workspace_bytes(B, N, *size)


def avg_voxelize_fwd(features, coords, resolution):
    """(out f32 [B,C,R^3], ind i32 [B,N], cnt i32 [B,R^3]) of features f32 [B,C,N] and coords i32 [B,3,N]: the extension's
    avg_voxelize_forward.  out[b,c,s] adds feat * (1.0f / cnt) over the points of voxel s in ascending point order, from 0 (the
    bits of the reference kernel run serially); a coordinate outside [0,R) gives ind = -1 and takes no part.  No atomics."""
    _lib.require_gpu(features, coords)
    features, coords = _pv_need(features, torch.float32, "avg_voxelize: features"), _pv_need(coords, torch.int32, "avg_voxelize: coords")
    R = int(resolution)
    if features.dim() != 3 or coords.dim() != 3 or coords.shape[1] != 3 or R < 1:
        raise RuntimeError("avg_voxelize: features [B,C,N], coords [B,3,N] and a resolution >= 1 expected")
    B, C, N = features.shape
    if coords.shape[0] != B or coords.shape[2] != N or coords.device != features.device:
        raise RuntimeError("avg_voxelize: coords %s do not match features %s" % (tuple(coords.shape), tuple(features.shape)))
    dev = features.device
    out = torch.empty(B, C, R ** 3, device=dev, dtype=torch.float32)
    ind = torch.empty(B, N, device=dev, dtype=torch.int32)
    cnt = torch.empty(B, R ** 3, device=dev, dtype=torch.int32)
    _lib.call("deftet_avg_voxelize_fwd_f32", dev, features, coords, out, ind, cnt, B, C, N, R, ws=_grid_bytes(B, N, (R, R, R)))
    return out, ind, cnt


def avg_voxelize_bwd(grad_y, ind, cnt):
    """grad_x f32 [B,C,N] = grad_y[b,c,ind] * (1.0f / cnt[ind]) of grad_y f32 [B,C,R^3]: avg_voxelize_backward, as a gather."""
    _lib.require_gpu(grad_y, ind, cnt)
    grad_y = _pv_need(grad_y, torch.float32, "avg_voxelize_bwd: grad_y")
    ind, cnt = _pv_need(ind, torch.int32, "avg_voxelize_bwd: ind"), _pv_need(cnt, torch.int32, "avg_voxelize_bwd: cnt")
    if grad_y.dim() != 3 or ind.dim() != 2 or cnt.dim() != 2:
        raise RuntimeError("avg_voxelize_bwd: grad_y [B,C,R^3], ind [B,N], cnt [B,R^3] expected")
    B, C, S = grad_y.shape
    R = int(round(S ** (1.0 / 3.0)))
    if R ** 3 != S or ind.shape[0] != B or tuple(cnt.shape) != (B, S):
        raise RuntimeError("avg_voxelize_bwd: grad_y %s, ind %s, cnt %s do not agree" % (tuple(grad_y.shape), tuple(ind.shape), tuple(cnt.shape)))
    N, dev = ind.shape[1], grad_y.device
    grad_x = torch.empty(B, C, N, device=dev, dtype=torch.float32)
    _lib.call("deftet_avg_voxelize_bwd_f32", dev, grad_y, ind, cnt, grad_x, B, C, N, R)
    return grad_x


class GridCells:
    """The points of one set sorted by the cell they fall in on one grid size (deftet_voxel_cells_* for (R, R, R) volumes,
    deftet_image_cells_f32 for (H, W) maps): what the backward to the grids gathers through.  Grids of equal size share it."""
    __slots__ = ("perm", "seg", "wsorted", "isorted", "B", "N", "size")


def _grid_cells(B, N, size, dev, pos=None, pos_mode=0, inds=None, wgts=None, uv=None, border=0, align=0):
    """the cells of pos (or of the recorded inds / wgts) in volumes of shape `size`, or of uv in maps of shape `size`"""
    n_cells, corners = (size[0] ** 3, 8) if uv is None else ((size[0] + 1) * (size[1] + 1), 4)
    cells = GridCells()
    cells.B, cells.N, cells.size = B, N, tuple(size)
    cells.perm = torch.empty(B * N, device=dev, dtype=torch.int32)
    cells.seg = torch.empty(B * n_cells + 1, device=dev, dtype=torch.int32)
    cells.wsorted = torch.empty(corners, B * N, device=dev, dtype=torch.float32)
    cells.isorted = torch.empty(8, B * N, device=dev, dtype=torch.int32) if inds is not None else None
    out, nbytes = (cells.perm, cells.seg, cells.wsorted), _grid_bytes(B, N, size)
    if uv is not None:
        _lib.call("deftet_image_cells_f32", dev, uv, *out, B, N, size[0], size[1], border, align, ws=nbytes)
    elif inds is None:
        _lib.call("deftet_voxel_cells_f32", dev, pos, pos_mode, *out, B, N, size[0], ws=nbytes)
    else:
        _lib.call("deftet_voxel_cells_from_inds_i32", dev, inds, wgts, *out, cells.isorted, B, N, size[0], ws=nbytes)
    return cells


def _grid_bwd(gout, cells, C, c_off, C_total):
    """the gradient f32 [B, C, *size] of one grid from the rows [c_off, c_off + C) of gout, gathered through `cells`"""
    B, N, size, dev = cells.B, cells.N, cells.size, gout.device
    ggrid = torch.empty((B, C) + size, device=dev, dtype=torch.float32)
    head, nbytes = (gout, cells.perm, cells.seg, cells.wsorted), _grid_bytes(B, N, size)
    if len(size) == 3:
        _lib.call("deftet_voxel_sample_bwd_vol_f32", dev, *head, cells.isorted, ggrid, B, C, size[0], N, c_off, C_total, ws=nbytes)
    else:
        _lib.call("deftet_image_sample_bwd_map_f32", dev, *head, ggrid, B, C, size[0], size[1], N, c_off, C_total, ws=nbytes)
    return ggrid


def _grid_grads(gout, grids, needs, c_off, C_total, make_cells):
    """The gradients of the grids of a list (None where `needs` says so), grid k reading its rows of gout behind those of the
    grids before it, from c_off: one sort of the points per distinct grid size (make_cells(size)), then the gather."""
    grads, cells = [], {}
    for g, need in zip(grids, needs):
        size = tuple(g.shape[2:])
        if need and size not in cells:
            cells[size] = make_cells(size)
        grads.append(_grid_bwd(gout, cells[size], g.shape[1], c_off, C_total) if need else None)
        c_off += g.shape[1]
    return grads


def _check_volumes(caller, volumes, pos):
    """the volumes f32 [B,C,R,R,R] of `caller`, contiguous, on the device and with the batch of pos"""
    vols = []
    for v in volumes:
        v = _pv_need(v, torch.float32, "%s: volume" % caller)
        if v.dim() != 5 or v.shape[2] != v.shape[3] or v.shape[3] != v.shape[4] or v.shape[4] < 1:
            raise RuntimeError("%s: volumes [B,C,R,R,R] expected (got %s)" % (caller, tuple(v.shape)))
        if v.shape[0] != pos.shape[0] or v.device != pos.device:
            raise RuntimeError("%s: volume %s and pos %s differ in batch or device" % (caller, tuple(v.shape), tuple(pos.shape)))
        vols.append(v)
    return vols


class _VoxelSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, append_pos, pos_mode, *volumes):
        dev = pos.device
        B, N = (pos.shape[0], pos.shape[1]) if pos_mode == 0 else (pos.shape[0], pos.shape[2])
        C_feat = sum(v.shape[1] for v in volumes)
        C_total = C_feat + (3 if append_pos else 0)
        out = torch.empty(B, C_total, N, device=dev, dtype=torch.float32)
        c_off = 0
        with _lib.on_device(dev):
            for v in volumes:
                _lib.call("deftet_voxel_sample_fwd_f32", dev, v, pos, out, None, None, B, v.shape[1], v.shape[-1], N, c_off, C_total, pos_mode, 0)
                c_off += v.shape[1]
        if append_pos:
            out[:, C_feat:, :].copy_(pos.transpose(1, 2) if pos_mode == 0 else pos)
        ctx.save_for_backward(pos, *volumes)
        ctx.args = (bool(append_pos), pos_mode, B, N, C_feat, C_total)
        return out

    @staticmethod
    def backward(ctx, gout):
        pos, volumes = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        append_pos, pos_mode, B, N, C_feat, C_total = ctx.args
        dev = pos.device
        gout = _f32c(gout)
        grads = _grid_grads(gout, volumes, ctx.needs_input_grad[3:], 0, C_total,
                            lambda size: _grid_cells(B, N, size, dev, pos=pos, pos_mode=pos_mode))
        gpos = None
        if ctx.needs_input_grad[0]:
            gpos = torch.zeros_like(pos) if not volumes else torch.empty_like(pos)
            c_off = 0
            with _lib.on_device(dev):
                for k, v in enumerate(volumes):                      # list order; channels ascending inside the kernel
                    _lib.call("deftet_voxel_sample_bwd_pos_f32", dev, v, pos, gout, gpos, B, v.shape[1], v.shape[-1], N, c_off, C_total, pos_mode,
                              int(k > 0))
                    c_off += v.shape[1]
            if append_pos:
                gpos += gout[:, C_feat:, :].transpose(1, 2) if pos_mode == 0 else gout[:, C_feat:, :]
        return (gpos, None, None) + tuple(grads)


def voxel_sample(volumes, pos, append_pos=False, voxel_units=False):
    """f32 [B, sum C_k (+3), N]: the volumes f32 [B,C_k,R_k,R_k,R_k] read trilinearly at pos f32 [B,N,3] and written side by side into
    one result (`sample_f`, pc_model.py:182-194: every volume's launch writes its own channel range, so there is no per-volume
    tensor and no torch.cat; with append_pos the three position rows are one strided torch copy into the same tensor).  Per volume u = clamp((pos + 0.5) R, 0, R-1),
    lo = floor(u), hi = min(lo + 1, R - 1), the eight products added in corner order 000 .. 111 (z fastest).  append_pos: the last
    three channels are pos transposed (decode_pos / decode_occ).  voxel_units=True: `pos` is coords f32 [B,3,N] already in voxel
    units, u = clamp(coords, 0, R - 1) (`trilinear_devoxelize`'s argument; appended as it stands).
    Differentiable in every volume and in pos.  The gradient of a volume is a gather over the points sorted by cell (one sort per
    distinct R): no atomics, the same bits on every run.  The gradient of pos follows grid_sample's border rule: 0 for a coordinate
    the clamp holds (u <= 0 or u >= R - 1), the right-hand cell's slope at an interior integer u."""
    volumes = list(volumes)
    _lib.require_gpu(pos, *volumes)
    pos = _pv_need(pos, torch.float32, "voxel_sample: pos")
    if voxel_units:
        if pos.dim() != 3 or pos.shape[1] != 3:
            raise RuntimeError("voxel_sample: coords [B,3,N] expected with voxel_units")
    elif pos.dim() != 3 or pos.shape[2] != 3:
        raise RuntimeError("voxel_sample: pos [B,N,3] expected")
    return _VoxelSample.apply(pos, bool(append_pos), 1 if voxel_units else 0, *_check_volumes("voxel_sample", volumes, pos))


# --------------------------------------------------------------------------------- pixel-aligned image features
class _ImageSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, uv, glob, app, border, align, *maps):
        dev = uv.device
        B, N = uv.shape[0], uv.shape[1]
        G = glob.shape[1] if glob is not None else 0
        A = app.shape[2] if app is not None else 0
        C_total = G + sum(m.shape[1] for m in maps) + A
        out = torch.empty(B, C_total, N, device=dev, dtype=torch.float32)
        with _lib.on_device(dev):
            c_off = G
            for k, m in enumerate(maps):                             # the first launch also writes the global and the appended rows
                first = k == 0
                _lib.call("deftet_image_sample_fwd_f32", dev, m, uv, glob if first else None, app if first else None, out, B, m.shape[1],
                          m.shape[2], m.shape[3], N, G if first else 0, A if first else 0, c_off, C_total, border, align)
                c_off += m.shape[1]
            if not maps and G + A > 0:
                _lib.call("deftet_image_sample_fwd_f32", dev, None, uv, glob, app, out, B, 0, 1, 1, N, G, A, G, C_total, border, align)
        ctx.save_for_backward(uv, *maps)
        ctx.args = (border, align, B, N, G, A, C_total)
        return out

    @staticmethod
    def backward(ctx, gout):
        uv, maps = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        border, align, B, N, G, A, C_total = ctx.args
        dev = uv.device
        gout = _f32c(gout)
        grads = _grid_grads(gout, maps, ctx.needs_input_grad[5:], G, C_total,
                            lambda size: _grid_cells(B, N, size, dev, uv=uv, border=border, align=align))
        guv = None
        if ctx.needs_input_grad[0]:
            guv = torch.zeros_like(uv) if not maps else torch.empty_like(uv)
            c_off = G
            with _lib.on_device(dev):
                for k, m in enumerate(maps):                         # list order; channels ascending inside the kernel
                    _lib.call("deftet_image_sample_bwd_uv_f32", dev, m, uv, gout, guv, B, m.shape[1], m.shape[2], m.shape[3], N, c_off, C_total,
                              border, align, int(k > 0))
                    c_off += m.shape[1]
        gglob = None
        if G > 0 and ctx.needs_input_grad[1]:
            gglob = torch.empty(B, G, device=dev, dtype=torch.float32)
            _lib.call("deftet_image_sample_bwd_global_f32", dev, gout, gglob, B, G, N, C_total)
        elif ctx.needs_input_grad[1]:
            gglob = torch.zeros(B, 0, device=dev, dtype=torch.float32)
        gapp = gout[:, C_total - A:, :].transpose(1, 2).contiguous() if ctx.needs_input_grad[2] else None
        return (guv, gglob, gapp, None, None) + tuple(grads)


def image_sample(maps, uv, global_features=None, append=None, padding_mode="zeros", align_corners=False):
    """f32 [B, G + sum C_k + A, N], contiguous: the feature maps f32 [B,C_k,H_k,W_k] read bilinearly at uv f32 [B,N,2]
    (grid_sample's convention: uv[...,0] along W, uv[...,1] along H, -1 .. 1 spans the image) and written side by side into one
    result — what DISNDecoder._extract_point_image_features computes (layers/disn.py:278-305), without a per-map tensor, a cat or
    an expand.  Rows [0,G) hold global_features f32 [B,G] for every point, then the maps in list order, then append f32 [B,N,A]
    transposed (the positions).  padding_mode "zeros" or "border", align_corners as in F.grid_sample; the arithmetic is spelled
    out at deftet_image_sample_fwd_f32 (include/deftet_hip.h).  A point fully outside the map under "zeros" (+-1e30, +-inf and NaN
    included) has value 0 and no gradient; under "border" a NaN reads pixel 0.
    Differentiable in every map, in uv, in global_features and in append, each computed only when needed.  The gradient of a map
    is a gather over the points sorted by cell (one sort per distinct (H, W)), the gradient of global_features a fixed-order row
    sum: no atomics, the same bits on every run."""
    maps = list(maps)
    _lib.require_gpu(uv, global_features, append, *maps)
    if padding_mode not in ("zeros", "border"):
        raise RuntimeError("image_sample: padding_mode 'zeros' or 'border' expected (got %r)" % (padding_mode,))
    uv = _pv_need(uv, torch.float32, "image_sample: uv")
    if uv.dim() != 3 or uv.shape[2] != 2:
        raise RuntimeError("image_sample: uv [B,N,2] expected (got %s)" % (tuple(uv.shape),))
    B, N = uv.shape[0], uv.shape[1]
    ms = []
    for m in maps:
        m = _pv_need(m, torch.float32, "image_sample: map")
        if m.dim() != 4 or m.shape[2] < 1 or m.shape[3] < 1:
            raise RuntimeError("image_sample: maps [B,C,H,W] expected (got %s)" % (tuple(m.shape),))
        if m.shape[0] != B or m.device != uv.device:
            raise RuntimeError("image_sample: map %s and uv %s differ in batch or device" % (tuple(m.shape), tuple(uv.shape)))
        ms.append(m)
    if global_features is not None:
        global_features = _pv_need(global_features, torch.float32, "image_sample: global_features")
        if global_features.dim() != 2 or global_features.shape[0] != B or global_features.device != uv.device:
            raise RuntimeError("image_sample: global_features [B,G] expected (got %s for B = %d)" % (tuple(global_features.shape), B))
    if append is not None:
        append = _pv_need(append, torch.float32, "image_sample: append")
        if append.dim() != 3 or append.shape[0] != B or append.shape[1] != N or append.device != uv.device:
            raise RuntimeError("image_sample: append [B,N,A] expected (got %s for uv %s)" % (tuple(append.shape), tuple(uv.shape)))
    return _ImageSample.apply(uv, global_features, append, int(padding_mode == "border"), int(bool(align_corners)), *ms)


# --------------------------------------------------------------------------------- tet-centroid feature sampling
_TCS_MAX_VOLUMES = 8


def _tcs_volume_list(volumes):
    """the host arrays of the C ABI's volume list: (device pointers, channels, resolutions, n); the tensors must stay alive"""
    n = len(volumes)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[v.data_ptr() for v in volumes])
    chans = (ctypes.c_int * max(n, 1))(*[v.shape[1] for v in volumes])
    ress = (ctypes.c_int * max(n, 1))(*[v.shape[-1] for v in volumes])
    return ptrs, chans, ress, n


def tet_centroid_sample_bwd_pos(volumes, centroids, gout, append_pos=True):
    """gcent f32 [B,K,3]: the gradient of tet_centroid_sample's result on its centroids, one launch for the whole volume list.  The
    bits of voxel_sample's chain on the same centroids: per volume the channel sum from 0 in ascending order, the volumes added in
    list order, the position rows of gout last.  A slot with a NaN centroid gets 0."""
    B, K = centroids.shape[0], centroids.shape[1]
    gcent = torch.empty(B, K, 3, device=centroids.device, dtype=torch.float32)
    _lib.call("deftet_tet_centroid_sample_bwd_pos_f32", centroids.device, *_tcs_volume_list(volumes), centroids, gout, gcent, B, K,
              1 if append_pos else 0)
    return gcent


def tet_centroid_sample_bwd_vertices(gcent, csr, n_vertex, n_tet, select=None, first=0, out=None):
    """gpos f32 [B,V,3] = 0.25f * (per vertex, over its incidences in the CSR's order and per incidence over the slots that chose
    that tet in ascending slot, the sum of gcent f32 [B,K,3] in one fp32 accumulator from 0).  select int32 [K] or the range from
    `first`; out: an existing contiguous f32 [B,V,3] to ADD to.  Every element is written: no memset, no atomics."""
    lib = _lib.load()
    B, K, V, T, dev = gcent.shape[0], gcent.shape[1], int(n_vertex), int(n_tet), gcent.device
    _check_csr("tet_centroid_sample_bwd_vertices", csr, B, V, T, dev=dev)
    offsets, slots, Bi = csr
    acc = out is not None
    gpos = _out_or_new("tet_centroid_sample_bwd_vertices", out, (B, V, 3), dev)
    _lib.call("deftet_tet_centroid_sample_bwd_vertices_f32", dev, gcent, offsets, slots, select, int(first), gpos, B, V, T, Bi, K,
              1 if acc else 0, ws=lib.deftet_tet_centroid_sample_workspace_bytes(B, T, K) if select is not None else None)
    return gpos


class _TetCentroidSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, tet_idx, csr, select, first, K, append_pos, check, *volumes):
        dev = pos.device
        B, V, T = pos.shape[0], pos.shape[1], tet_idx.shape[1]
        C_feat = sum(v.shape[1] for v in volumes)
        C_total = C_feat + (3 if append_pos else 0)
        out = torch.empty(B, C_total, K, device=dev, dtype=torch.float32)
        centroids = torch.empty(B, K, 3, device=dev, dtype=torch.float32)
        bad = _bad_flag(check, dev)
        _lib.call("deftet_tet_centroid_sample_fwd_f32", dev, *_tcs_volume_list(volumes), pos, tet_idx, select, first, out, centroids, bad,
                  B, V, T, tet_idx.shape[0], K, 1 if append_pos else 0)
        _raise_if(bad, RuntimeError, "tet_centroid_sample: a chosen tet is outside [0, %d) or one of its vertices outside [0, %d)" % (T, V))
        ctx.save_for_backward(centroids, *volumes)
        ctx.tet_idx, ctx.csr, ctx.select = tet_idx, csr, select
        ctx.args = (bool(append_pos), first, B, V, T, K, C_feat, C_total)
        ctx.mark_non_differentiable(centroids)
        return out, centroids

    @staticmethod
    def backward(ctx, gout, _gcentroids):
        centroids, volumes = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        append_pos, first, B, V, T, K, C_feat, C_total = ctx.args
        dev = centroids.device
        gout = _f32c(gout)
        grads = _grid_grads(gout, volumes, ctx.needs_input_grad[8:], 0, C_total, lambda size: _grid_cells(B, K, size, dev, pos=centroids))
        gpos = None
        if ctx.needs_input_grad[0]:
            gcent = tet_centroid_sample_bwd_pos(volumes, centroids, gout, append_pos)
            gpos = tet_centroid_sample_bwd_vertices(gcent, _csr_or_build(ctx.csr, ctx.tet_idx, V), V, T, select=ctx.select, first=first)
        return (gpos, None, None, None, None, None, None, None) + tuple(grads)


def tet_centroid_sample(volumes, pos_bxvx3, tet_idx, csr=None, select=None, first=0, count=None, append_pos=True, check=False,
                        return_centroids=False):
    """f32 [B, sum C_k (+3), K]: the volumes f32 [B,C_k,R_k,R_k,R_k] (at most 8) read trilinearly at the centroids of K chosen tets of
    the mesh (pos f32 [B,V,3], tet_idx int [T,4] or [B,T,4]), the centroids themselves behind them with append_pos — the input of
    the occupancy decoder (`decode_occ`, pc_model.py:276-306) without the gathered [B,T,4,3] tensor, its mean or the index step.
    The chosen tets: `select`, an int tensor [K] shared by the batch (`center_idx`; repeats allowed), or the range [first,
    first + count) (`split_decode_occ`'s walk; count=None: to the end), never both.  The centroid is (((a + b) + c) + d) * 0.25f
    in fp32; the values are voxel_sample's at that point, bit for bit.
    Differentiable in pos and in every volume, with the same bits on every run and no atomics: the volumes through voxel_sample's
    sort by cell, pos through the incidence CSR — `csr` = tet_vertex_csr(tet_idx, V), built once per tet list (TetTopology keeps
    it).  csr=None with pos requiring grad is the slow path: the CSR is rebuilt in every backward.
    check=True synchronises and raises on a tet index outside [0,T) or a vertex index outside [0,V); otherwise such a slot's
    values are NaN and it adds nothing to the gradient of pos.  return_centroids: also the centroids f32 [B,K,3] (no gradient)."""
    volumes = list(volumes)
    _lib.require_gpu(select, *volumes)
    pos, idx, _, _ = _mesh_args("tet_centroid_sample", pos_bxvx3, tet_idx)
    if len(volumes) > _TCS_MAX_VOLUMES:
        raise RuntimeError("tet_centroid_sample: at most %d volumes (got %d)" % (_TCS_MAX_VOLUMES, len(volumes)))
    T = idx.shape[1]
    vols = _check_volumes("tet_centroid_sample", volumes, pos)
    first = int(first)
    if select is not None:
        if count is not None or first != 0:
            raise RuntimeError("tet_centroid_sample: either select or the range first / count, not both")
        if select.dim() != 1 or select.dtype not in (torch.int32, torch.int64) or select.device != pos.device:
            raise RuntimeError("tet_centroid_sample: select must be an int32 / int64 tensor [K] on the device of pos")
        select = select.to(torch.int32).contiguous()
        K = select.shape[0]
    else:
        K = T - first if count is None else int(count)
        if first < 0 or K < 0 or first + K > T:
            raise RuntimeError("tet_centroid_sample: the range [%d, %d) does not lie in the %d tets" % (first, first + K, T))
    if csr is not None:                                              # (the backward reads the CSR alone: its idx_batch need not be the list's)
        _check_csr("tet_centroid_sample", csr, pos.shape[0], pos.shape[1], T, dev=pos.device)
    out, centroids = _TetCentroidSample.apply(pos, idx, csr, select, first, K, bool(append_pos), bool(check), *vols)
    return (out, centroids) if return_centroids else out


# ------------------------------------------------------------------------------------
# a per-vertex field at query points (tet_field_sample.hip)
# ------------------------------------------------------------------------------------
def _tfs_args(caller, field, tet_idx, cond):
    """(field, idx, cond, (B, V, C, T, Bi, Q)) of the raw entries: _mesh_args of the field and the list, and f32 cond [B,Q,1] or [B,Q]"""
    _lib.require_gpu(cond)
    _, idx, field, _ = _mesh_args(caller, None, tet_idx, field=_pv_need(field, torch.float32, caller + ": field"), convert=True)
    cond = _f32c(cond)
    B, V, C = field.shape
    if cond.dim() not in (2, 3) or cond.shape[0] != B or cond.numel() != B * cond.shape[1]:
        raise _expected(caller, "cond [%d,Q,1]" % B, cond)
    return field, idx, cond, (B, V, C, idx.shape[1], idx.shape[0], cond.shape[1])


def tet_field_sample_fwd(field, tet_idx, cond, bary, fill=0.0, bad=None):
    """out f32 [B,Q,C] = ((w0 f(v0) + w1 f(v1)) + w2 f(v2)) + w3 f(v3) per channel, every step rounded, in the tet cond names
    (v_k its vertices in tet_idx, w = bary); `fill` where cond is -1, NaN where a vertex index lies outside [0,V) (bad: an int32
    [1] tensor set to 1 then).  One launch.  The raw forward of tet_field_sample."""
    _lib.require_gpu(bary, bad)
    field, idx, cond, (B, V, C, T, Bi, Q) = _tfs_args("tet_field_sample", field, tet_idx, cond)
    bary = _f32c(bary)
    if bary.shape != (B, Q, 4):
        raise _expected("tet_field_sample", "bary [%d,%d,4]" % (B, Q), bary)
    dev = field.device
    out = torch.empty(B, Q, C, device=dev, dtype=torch.float32)
    _lib.call("deftet_tet_field_sample_fwd_f32", dev, field, idx, cond, bary, out, bad, float(fill), B, V, T, Bi, Q, C)
    return out


def tet_field_sample_bwd_w(field, tet_idx, cond, gout):
    """grad_w f32 [B,Q,4]: the gradient of tet_field_sample's result on the barycentric weights, grad_w[b,q,k] = the sum over the
    channels in ascending order of gout[b,q,c] * f(v_k,c), one fp32 accumulator from 0; 0 on a miss.  One launch."""
    _lib.require_gpu(gout)
    field, idx, cond, (B, V, C, T, Bi, Q) = _tfs_args("tet_field_sample_bwd_w", field, tet_idx, cond)
    gout = _f32c(gout)
    if gout.shape != (B, Q, C):
        raise _expected("tet_field_sample_bwd_w", "gout [%d,%d,%d]" % (B, Q, C), gout)
    dev = field.device
    gw = torch.empty(B, Q, 4, device=dev, dtype=torch.float32)
    _lib.call("deftet_tet_field_sample_bwd_w_f32", dev, field, idx, cond, gout, gw, B, V, T, Bi, Q, C)
    return gw


def tet_field_sample_bwd_field(gout, cond, bary, csr, n_vertex, n_tet, out=None, accumulate=False):
    """grad_field f32 [B,V,C]: per vertex, over its incidences in the CSR's order and per incidence (t, k) over the queries with
    cond == t in ascending q, the sum of bary[b,q,k] * gout[b,q,c] in one fp32 accumulator from 0.  out: an existing contiguous f32
    [B,V,C] to write into, or with `accumulate` to ADD to.  Every element is written: no memset, no atomics."""
    _lib.require_gpu(gout, cond, bary, out)
    lib = _lib.load()
    gout, cond, bary = _f32c(gout), _f32c(cond), _f32c(bary)
    if gout.dim() != 3 or gout.shape[2] < 1:
        raise _expected("tet_field_sample_bwd_field", "gout [B,Q,C]", gout)
    B, Q, C = gout.shape
    V, T, dev = int(n_vertex), int(n_tet), gout.device
    _check_csr("tet_field_sample_bwd_field", csr, B, V, T, dev=dev)
    offsets, slots, Bi = csr
    if cond.numel() != B * Q or bary.shape != (B, Q, 4):
        raise _expected("tet_field_sample_bwd_field", "cond [%d,%d,1] and bary [%d,%d,4]" % (B, Q, B, Q), "%s and %s" % (tuple(cond.shape), tuple(bary.shape)))
    if accumulate and out is None:
        raise RuntimeError("tet_field_sample_bwd_field: accumulate needs out")
    acc = bool(accumulate)
    gfield = _out_or_new("tet_field_sample_bwd_field", out, (B, V, C), dev)
    _lib.call("deftet_tet_field_sample_bwd_field_f32", dev, gout, cond, bary, offsets, slots, gfield, B, V, T, Bi, Q, C, 1 if acc else 0,
              ws=lib.deftet_tet_field_sample_workspace_bytes(B, T, Q))
    return gfield


class _TetFieldSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, pos, pts, idx, csr, topology, fill, check, want_records):
        rec = bool(want_records) and bwd_uses_records(idx.shape[1], pts.shape[1])
        res = point_in_tet_indexed(pos, idx, pts, want_bary=True, want_hits=rec, order="auto", query_box="track", topology=topology,
                                   check=check)
        cond, bary, hits = res if rec else (res + (None,))
        bad = _bad_flag(check, pos.device)
        out = tet_field_sample_fwd(field, idx, cond, bary, fill=fill, bad=bad)
        _raise_if(bad, RuntimeError, "tet_field_sample: a vertex index outside [0, %d)" % pos.shape[1])
        ctx.save_for_backward(field, pos, pts, cond, bary, hits)
        ctx.idx, ctx.csr = idx, csr
        ctx.mark_non_differentiable(cond, bary)
        return out, cond, bary

    @staticmethod
    def backward(ctx, gout, _gcond, _gbary):
        field, pos, pts, cond, bary, hits = ctx.saved_tensors
        V, T = pos.shape[1], ctx.idx.shape[1]
        gout = _f32c(gout)
        csr = _csr_or_build(ctx.csr, ctx.idx, V)
        g_field = g_pos = g_pts = None
        if ctx.needs_input_grad[0]:
            g_field = tet_field_sample_bwd_field(gout, cond, bary, csr, V, T)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw = tet_field_sample_bwd_w(field.detach(), ctx.idx, cond, gout)
            g_pos, g_pts = point_in_tet_indexed_bwd_to_vertices(pos.detach(), ctx.idx, pts.detach(), cond, gw, csr,
                                                                want_grad_pts=ctx.needs_input_grad[2], hits=hits)
            if not ctx.needs_input_grad[1]:
                g_pos = None
        return g_field, g_pos, g_pts, None, None, None, None, None, None


def tet_field_sample(field, pos_bxvx3, tet_idx, pts_bxqx3, csr=None, topology=None, fill=0.0, return_index=False, check=False):
    """f32 [B,Q,C]: the per-vertex field f32 [B,V,C] (an SDF or occupancy for marching_tets, vertex features, an offset) read at the
    query points pts f32 [B,Q,3] in the tet mesh (pos f32 [B,V,3], tet_idx int [T,4] or [B,T,4]): value = sum_k w_k field[v_k] with
    the barycentric weights w of the point in the lowest tet that holds it (point_in_tet_indexed's cond and bary), `fill` where
    no tet holds it.  Per channel ((w0 f0 + w1 f1) + w2 f2) + w3 f3 in fp32, every step rounded.
    Differentiable in field, pos and pts, each gradient computed only when asked for, without float atomics: field through a sort
    of the queries by tet and the incidence CSR, in one fixed order (the same bits on every run); pos and pts through the gradient
    on the weights and point_in_tet_indexed_bwd_to_vertices, whose order is fixed up to 2 queries per tet (bwd_uses_records).
    `csr` = tet_vertex_csr(tet_idx, V), or a TetTopology as `topology` (it brings its own and keys the traversal-order decision);
    neither, with a gradient asked for, is the slow path: the CSR is rebuilt in every backward.  check=True synchronises and raises on a vertex index outside [0,V); otherwise a row whose tet names
    one is NaN and its grad_w is 0.  return_index: also cond f32 [B,Q,1] and bary f32 [B,Q,4] (no gradient)."""
    pos, idx, field, pts = _mesh_args("tet_field_sample", pos_bxvx3, tet_idx, topology, field=field, pts=pts_bxqx3)
    (B, _, C), Q = field.shape, pts.shape[1]
    csr = _resolve_csr("tet_field_sample", csr, topology, pos, idx)
    if Q == 0:
        out, cond, bary = field.new_empty(B, 0, C), field.new_empty(B, 0, 1), field.new_empty(B, 0, 4)
    else:
        # (without a TetTopology the caller's own index tensor keys the traversal-order decision: its fingerprint is taken once)
        # the hit records serve the gradient on pos and pts alone (point_in_tet_indexed_bwd_to_vertices); cond and bary do not
        # depend on whether they are asked for
        records = torch.is_grad_enabled() and (pos.requires_grad or pts.requires_grad)
        out, cond, bary = _TetFieldSample.apply(field, pos, pts, idx, csr, topology if topology is not None else tet_idx, float(fill),
                                                bool(check), records)
    return (out, cond, bary) if return_index else out


# ------------------------------------------------------------------------------------
# field gradients on the tets, their energies, per-tet values to the vertices (tet_field_grad.hip)
# ------------------------------------------------------------------------------------
TFE_MAX_CHANNELS, _TFE_STATS = 8, 17                    # tet_field_grad.hip kTfeMaxC, kTfeStats


def tet_field_gradient_fwd(field, pos_bxvx3, tet_idx, return_volume=False):
    """grad f32 [B,T,C,3] (and vol f32 [B,T]): per tet the gradient of the linear interpolant of field f32 [B,V,C] over the
    positions f32 [B,V,3], g_c = (n0 df0 + n1 df1 + n2 df2) / det in fp32 (include/deftet_hip.h), 0 with volume 0 on a dead tet
    (det > 0 fails).  One launch.  The raw forward of tet_field_gradient."""
    pos, idx, field, _ = _mesh_args("tet_field_gradient", pos_bxvx3, tet_idx, field=field)
    B, V, C = field.shape
    T, dev = idx.shape[1], field.device
    out = torch.empty(B, T, C, 3, device=dev, dtype=torch.float32)
    vol = torch.empty(B, T, device=dev, dtype=torch.float32) if return_volume else None
    _lib.call("deftet_tet_field_gradient_fwd_f32", dev, field, pos, idx, out, vol, B, V, T, idx.shape[0], C)
    return (out, vol) if return_volume else out


def tet_volumes(pos_bxvx3, tet_idx):
    """vol f32 [B,T] = det E / 6 of every tet, 0 for a dead one: tet_field_gradient's volumes alone (no gradient), e.g. as the
    constant weights of tet_to_vertex.  One launch."""
    pos, idx, _, _ = _mesh_args("tet_volumes", _pv_need(pos_bxvx3.detach(), torch.float32, "tet_volumes: pos"), tet_idx, convert=True)
    B, V, T = pos.shape[0], pos.shape[1], idx.shape[1]
    vol = torch.empty(B, T, device=pos.device, dtype=torch.float32)
    _lib.call("deftet_tet_field_gradient_fwd_f32", pos.device, None, pos, idx, None, vol, B, V, T, idx.shape[0], 1)
    return vol


def tet_field_gradient_bwd(grad_out, grad_vol, field, pos_bxvx3, tet_idx, csr, want_field=True, want_pos=True):
    """(grad_field f32 [B,V,C] | None, grad_pos f32 [B,V,3] | None): grad_out f32 [B,T,C,3] and grad_vol f32 [B,T] (or None) of
    tet_field_gradient_fwd taken to the vertices, per vertex one fp32 accumulator over its incidences in the CSR's order
    (ascending 4 t + corner); no atomics, the same bits on every run.  One launch per gradient asked for."""
    pos, idx, field, _ = _mesh_args("tet_field_gradient_bwd", pos_bxvx3, tet_idx, field=field)
    B, V, C = field.shape
    T, dev = idx.shape[1], field.device
    _check_csr("tet_field_gradient_bwd", csr, B, V, T, idx.shape[0], dev)
    _lib.require_gpu(grad_out, grad_vol)
    g = _f32c(grad_out)
    if tuple(g.shape) != (B, T, C, 3):
        raise _expected("tet_field_gradient_bwd", "grad_out %s" % ((B, T, C, 3),), g)
    gv = None
    if grad_vol is not None:
        gv = _f32c(grad_vol)
        if tuple(gv.shape) != (B, T):
            raise _expected("tet_field_gradient_bwd", "grad_vol %s" % ((B, T),), gv)
    gf = torch.empty(B, V, C, device=dev, dtype=torch.float32) if want_field else None
    gp = torch.empty(B, V, 3, device=dev, dtype=torch.float32) if want_pos else None
    if want_field or want_pos:
        _lib.call("deftet_tet_field_gradient_bwd_f32", dev, g, gv, field, pos, idx, csr[0], csr[1], gf, gp, B, V, T, idx.shape[0], C)
    return gf, gp


class _TetFieldGradient(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, pos, idx, csr, return_volume):
        out, vol = tet_field_gradient_fwd(field, pos, idx, return_volume=True) if return_volume else (tet_field_gradient_fwd(field, pos, idx), None)
        ctx.save_for_backward(field, pos)
        ctx.idx, ctx.csr = idx, csr
        ctx.set_materialize_grads(False)
        return out, vol

    @staticmethod
    def backward(ctx, g_out, g_vol):
        field, pos = ctx.saved_tensors
        want_f, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_f or want_p):
            return None, None, None, None, None
        if g_out is None and g_vol is None:
            return (torch.zeros_like(field) if want_f else None, torch.zeros_like(pos) if want_p else None, None, None, None)
        if g_out is None:
            g_out = field.new_zeros(field.shape[0], ctx.idx.shape[1], field.shape[2], 3)
        csr = _csr_or_build(ctx.csr, ctx.idx, pos.shape[1])
        gf, gp = tet_field_gradient_bwd(g_out, g_vol, field.detach(), pos.detach(), ctx.idx, csr, want_field=want_f, want_pos=want_p)
        return gf, gp, None, None, None


def tet_field_gradient(field, pos_bxvx3, tet_idx, csr=None, topology=None, return_volume=False):
    """f32 [B,T,C,3]: the gradient of a per-vertex field f32 [B,V,C] (an SDF, an occupancy, features) on every tet of the mesh
    (pos f32 [B,V,3], tet_idx int [T,4] or [B,T,4]) — it is constant on a tet: g_c = E^-1 df_c with the rows of E the edges from
    vertex 0 and df_k = f(v_{k+1},c) - f(v0,c), in the adjugate form in fp32.  return_volume: also vol f32 [B,T] = det E / 6.
    A tet is live iff det E > 0 in fp32 (the orientation of every grid here); a NaN, flat or inverted tet has gradient 0 and
    volume 0 and gives nothing to a backward.  Differentiable in field and pos, also through vol: the gradient lands on the
    vertices through the incidence CSR in its order, without float atomics (the same bits on every run).  `csr` =
    tet_vertex_csr(tet_idx, V), or a TetTopology as `topology`; neither, with a gradient asked for, is the slow path: the CSR is
    rebuilt in every backward."""
    pos, idx, field, _ = _mesh_args("tet_field_gradient", pos_bxvx3, tet_idx, topology, field=field)
    csr = _resolve_csr("tet_field_gradient", csr, topology, pos, idx)
    out, vol = _TetFieldGradient.apply(field, pos, idx, csr, bool(return_volume))
    return (out, vol) if return_volume else out


class _TetFieldEnergies(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, pos, idx, csr, target):
        lib = _lib.load()
        B, V, C = field.shape
        T, dev = idx.shape[1], field.device
        out = torch.empty(B, C, 2, device=dev, dtype=torch.float32)
        stats = torch.empty(B, _TFE_STATS, device=dev, dtype=torch.float64)
        _lib.call("deftet_tet_field_energies_fwd_f32", dev, field, pos, idx, out, stats, target, B, V, T, idx.shape[0], C,
                  ws=lib.deftet_tet_field_energies_workspace_bytes(B))
        ctx.save_for_backward(field, pos, stats)
        ctx.idx, ctx.csr, ctx.target = idx, csr, target
        return out

    @staticmethod
    def backward(ctx, g_out):
        field, pos, stats = ctx.saved_tensors
        want_f, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_f or want_p):
            return None, None, None, None, None
        B, V, C = field.shape
        idx, dev = ctx.idx, field.device
        csr = _csr_or_build(ctx.csr, idx, V)
        gf = torch.empty(B, V, C, device=dev, dtype=torch.float32) if want_f else None
        gp = torch.empty(B, V, 3, device=dev, dtype=torch.float32) if want_p else None
        _lib.call("deftet_tet_field_energies_bwd_f32", dev, stats, _f32c(g_out), ctx.target, field, pos, idx, csr[0], csr[1], gf, gp, B, V,
                  idx.shape[1], idx.shape[0], C)
        return gf, gp, None, None, None


def tet_field_energies(field, pos_bxvx3, tet_idx, csr=None, topology=None, target=1.0):
    """f32 [B,C,2], 1 <= C <= 8: the two energies of a per-vertex field's gradient g (tet_field_gradient) over the live tets,
    weighted by their volumes w_t, W = sum w_t:  [...,0] = sum w_t |g_c|^2 / W, the Dirichlet energy (the FEM Laplacian), and
    [...,1] = sum w_t (|g_c| - target)^2 / W, the Eikonal term.  One pass over the tets, [B,T,C,3] never stored, the sums in
    fp64 in one order.  Differentiable in field and pos through the saved per-shape sums and the incidence CSR (csr, topology
    and the slow path as in tet_field_gradient), without float atomics.  Where |g| = 0 the Eikonal term's derivative is taken
    as 0.  W = 0 (no live tet) gives 0 energies and 0 gradients."""
    pos, idx, field, _ = _mesh_args("tet_field_energies", pos_bxvx3, tet_idx, topology, field=field)
    if field.shape[2] > TFE_MAX_CHANNELS:
        raise _lib.DefTetHipError("tet_field_energies: field [B,V,C] with 1 <= C <= %d expected (got %s) (DEFTET_EINVAL)"
                                  % (TFE_MAX_CHANNELS, tuple(field.shape)))
    csr = _resolve_csr("tet_field_energies", csr, topology, pos, idx)
    return _TetFieldEnergies.apply(field, pos, idx, csr, float(target))


def _ttv_topology(tet_idx_or_csr, n_vertex):
    """(csr, int32 idx | None) of tet_to_vertex's second argument: a TetTopology (its csr and list), a csr tuple, or a tet list"""
    _, own32, csr = _topology_parts(tet_idx_or_csr)
    if csr is not None and own32 is not None:
        return csr, _idx32(own32)
    if isinstance(tet_idx_or_csr, (tuple, list)):                    # a csr; or the pair (csr, int32 list) vertex_field_gradient hands in
        return tet_idx_or_csr if len(tet_idx_or_csr) == 2 else (tet_idx_or_csr, None)
    if not isinstance(tet_idx_or_csr, torch.Tensor) or tet_idx_or_csr.dtype not in (torch.int32, torch.int64):
        raise _expected("tet_to_vertex", "a tet list int32 / int64 [T,4] or [B,T,4], a tet_vertex_csr tuple or a TetTopology",
                        getattr(tet_idx_or_csr, "dtype", type(tet_idx_or_csr).__name__))
    _lib.require_gpu(tet_idx_or_csr)
    idx = _idx32(tet_idx_or_csr)
    if idx.dim() != 3 or idx.shape[2] != 4:
        raise _expected("tet_to_vertex", "tet_idx [T,4] or [B,T,4]", tet_idx_or_csr)
    return _csr_or_build(None, idx, int(n_vertex)), idx              # the slow path, in this call


def _csr_tet_list(csr, V, T):
    """int32 [Bi,T,4] of a tet_vertex_csr: position i of the sorted incidences belongs to the vertex whose segment holds it"""
    offsets, slots, Bi = csr
    pos = torch.arange(slots.numel(), device=slots.device, dtype=torch.int32)
    row = torch.bucketize(pos, offsets[1:].contiguous(), right=True)      # b V + v
    idx = torch.empty(Bi * T * 4, device=slots.device, dtype=torch.int32)
    idx[(row // V).long() * (4 * T) + slots.long()] = (row % V).to(torch.int32)
    return idx.reshape(Bi, T, 4)


def tet_to_vertex_fwd(values, weights, csr, n_vertex, fill=0.0):
    """(out f32 [B,V,C], weight_sum f32 [B,V]): per vertex (sum w_t values[t]) / (sum w_t) over its incidences in the CSR's order,
    one fp32 accumulator each from 0, every step rounded; `fill` where the weight sum is not > 0.  One launch."""
    B, T, C = values.shape
    V, dev = int(n_vertex), values.device
    out = torch.empty(B, V, C, device=dev, dtype=torch.float32)
    wsum = torch.empty(B, V, device=dev, dtype=torch.float32)
    _lib.call("deftet_tet_to_vertex_fwd_f32", dev, values, weights, csr[0], csr[1], out, wsum, float(fill), B, V, T, csr[2], C)
    return out, wsum


def tet_to_vertex_bwd(grad_out, weight_sum, weights, tet_idx, n_tet):
    """grad_values f32 [B,T,C] = w_t * (gout[v_0] / W_{v_0} + ... + gout[v_3] / W_{v_3}), one fp32 accumulator from 0 over the
    corners in order, a corner whose weight sum is not > 0 left out: a gather, no reduction.  One launch."""
    g = _f32c(grad_out)
    B, V, C = g.shape
    idx = _idx32(tet_idx)
    gval = torch.empty(B, int(n_tet), C, device=g.device, dtype=torch.float32)
    _lib.call("deftet_tet_to_vertex_bwd_f32", g.device, g, weight_sum, weights, idx, gval, B, V, int(n_tet), idx.shape[0], C)
    return gval


class _TetToVertex(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, weights, csr, idx, V, fill):
        out, wsum = tet_to_vertex_fwd(values, weights, csr, V, fill)
        ctx.save_for_backward(wsum, weights)
        ctx.csr, ctx.idx, ctx.n = csr, idx, (V, values.shape[1])
        ctx.mark_non_differentiable(wsum)
        return out, wsum

    @staticmethod
    def backward(ctx, g_out, _g_wsum):
        wsum, weights = ctx.saved_tensors
        V, T = ctx.n
        idx = ctx.idx if ctx.idx is not None else _csr_tet_list(ctx.csr, V, T)     # (a csr alone: its tet list is read back from it)
        return tet_to_vertex_bwd(g_out, wsum, weights, idx, T), None, None, None, None, None


def tet_to_vertex(values_bxtxc, tet_idx_or_csr, n_vertex, weights=None, fill=0.0):
    """f32 [B,V,C]: per-tet values f32 [B,T,C] (an occupancy, tet_field_gradient's rows flattened) carried to the vertices as the
    weighted mean over each vertex's incident tets, (sum w_t values[t]) / (sum w_t) in the incidence CSR's order (ascending
    4 t + corner), one fp32 accumulator each from 0 with every step rounded.  weights f32 [B,T] (the tet volumes, say) are a
    CONSTANT: they get no gradient; None = 1, the plain mean.  A vertex whose weight sum is not > 0 — no incident tet, or only
    dead ones — gets `fill`.  tet_idx_or_csr: tet_vertex_csr(tet_idx, n_vertex) built once per list, a TetTopology, or the tet
    list itself int [T,4] / [B,T,4] (the slow path: the CSR is built in this call, a sort and a host sync).  Differentiable in
    values: grad[t] = w_t sum_k gout[v_k] / W_{v_k}, a gather over the four corners (with a csr alone the tet list is first read
    back from it)."""
    if not isinstance(values_bxtxc, torch.Tensor) or values_bxtxc.dim() != 3 or values_bxtxc.shape[2] < 1:
        raise RuntimeError("tet_to_vertex: values [B,T,C] with a channel dimension of at least 1 expected (got %s)"
                           % (tuple(getattr(values_bxtxc, "shape", ())),))
    _lib.require_gpu(values_bxtxc, weights)
    val = _pv_need(values_bxtxc, torch.float32, "tet_to_vertex: values")
    B, T, C = val.shape
    V = int(n_vertex)
    csr, idx = _ttv_topology(tet_idx_or_csr, V)
    _check_csr("tet_to_vertex", csr, B, V, T, None if idx is None else idx.shape[0], val.device)
    if idx is not None and (tuple(idx.shape) != (csr[2], T, 4) or idx.device != val.device):
        raise _expected("tet_to_vertex", "a tet list [%d,%d,4] on %s" % (csr[2], T, val.device), "%s on %s" % (tuple(idx.shape), idx.device))
    w = None
    if weights is not None:
        w = _pv_need(weights.detach(), torch.float32, "tet_to_vertex: weights")
        if tuple(w.shape) != (B, T) or w.device != val.device:
            raise _expected("tet_to_vertex", "weights [%d,%d] on %s" % (B, T, val.device), "%s on %s" % (tuple(w.shape), w.device))
    return _TetToVertex.apply(val, w, csr, idx, V, float(fill))[0]


def vertex_field_gradient(field, pos_bxvx3, tet_idx, csr=None, topology=None, fill=0.0):
    """f32 [B,V,C,3]: the field's gradient at the vertices, the volume-weighted mean of tet_field_gradient over each vertex's
    incident tets (tet_to_vertex with the volumes as constant weights); `fill` at a vertex with no live tet.  Differentiable in
    field and pos through the per-tet gradients."""
    pos, idx, field, _ = _mesh_args("vertex_field_gradient", pos_bxvx3, tet_idx, topology, field=field)
    V = field.shape[1]
    csr = _csr_or_build(_resolve_csr("vertex_field_gradient", csr, topology, pos, idx), idx, V)      # (once for both steps)
    g, vol = _TetFieldGradient.apply(field, pos, idx, csr, True)
    B, T, C = g.shape[:3]
    return tet_to_vertex(g.reshape(B, T, C * 3), (csr, idx), V, weights=vol, fill=fill).reshape(B, V, C, 3)


def unit_normals(grad_nx3):
    """-g / |g| row by row, 0 where |g| = 0: the outward normal of a level set whose inside is the higher side"""
    norm = grad_nx3.norm(dim=-1, keepdim=True)
    return torch.where(norm > 0, -grad_nx3 / norm.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(grad_nx3))


# ------------------------------------------------------------------------------------
# iso-solid measures on the tets: inside fraction, area, volume, intersection (tet_iso_measure.hip)
# ------------------------------------------------------------------------------------
def _tim_args(caller, field, pos, tet_idx, iso, topology=None):
    """(field [B,V], pos, idx, iso) of the iso measures: the tet-mesh argument contract with a field [B,V] or [B,V,1] and a
    finite float32 level, all decided before any C entry is reached"""
    iso = float(iso)
    with np.errstate(over="ignore"):
        finite = np.isfinite(np.float32(iso))
    if not finite:
        raise _lib.DefTetHipError("%s: iso = %r is not a finite float32 (DEFTET_EINVAL)" % (caller, iso))
    if isinstance(field, torch.Tensor) and field.dim() == 2:
        field = field[:, :, None]
    pos, idx, field, _ = _mesh_args(caller, pos, tet_idx, topology, field=field)
    if pos is None or field.shape[2] != 1:
        raise _expected(caller, "pos [B,V,3] and field [B,V] or [B,V,1]", field)
    return field.reshape(field.shape[0], field.shape[1]), pos, idx, iso


def _tim_grad(caller, g, B, T, dev):
    """an upstream gradient f32 [B,T] of the iso measures, or None"""
    if g is None:
        return None
    _lib.require_gpu(g)
    g = _f32c(g)
    if tuple(g.shape) != (B, T) or g.device != dev:
        raise _expected(caller, "a gradient [%d,%d] on %s" % (B, T, dev), "%s on %s" % (tuple(g.shape), g.device))
    return g


def tet_iso_fraction_fwd(field, pos_bxvx3, tet_idx, iso=0.0, return_area=False, return_volume=False):
    """(frac f32 [B,T], area f32 [B,T] | None, vol f32 [B,T] | None): per tet the share of its volume with field > iso, the area
    of the iso polygon in it and its volume (the bits of tet_volumes on every live tet, 0 on a dead one).  One launch.  The raw
    forward of tet_iso_fraction."""
    field, pos, idx, iso = _tim_args("tet_iso_fraction", field, pos_bxvx3, tet_idx, iso)
    B, V = field.shape
    T, dev = idx.shape[1], field.device
    frac = torch.empty(B, T, device=dev, dtype=torch.float32)
    area = torch.empty(B, T, device=dev, dtype=torch.float32) if return_area else None
    vol = torch.empty(B, T, device=dev, dtype=torch.float32) if return_volume else None
    _lib.call("deftet_tet_iso_fraction_fwd_f32", dev, field, pos, idx, frac, area, vol, iso, B, V, T, idx.shape[0])
    return frac, area, vol


def tet_iso_fraction_bwd(grad_frac, grad_area, grad_vol, field, pos_bxvx3, tet_idx, csr, iso=0.0, want_field=True, want_pos=True):
    """(grad_field f32 [B,V] | None, grad_pos f32 [B,V,3] | None): grad_frac, grad_area, grad_vol f32 [B,T] (each or None) of
    tet_iso_fraction_fwd taken to the vertices, per vertex one fp64 accumulator per output over its incidences in the CSR's order
    (ascending 4 t + corner), rounded once; no atomics, the same bits on every run.  One launch."""
    field, pos, idx, iso = _tim_args("tet_iso_fraction_bwd", field, pos_bxvx3, tet_idx, iso)
    B, V = field.shape
    T, dev = idx.shape[1], field.device
    _check_csr("tet_iso_fraction_bwd", csr, B, V, T, idx.shape[0], dev)
    g = [_tim_grad("tet_iso_fraction_bwd", x, B, T, dev) for x in (grad_frac, grad_area, grad_vol)]
    gf = torch.empty(B, V, device=dev, dtype=torch.float32) if want_field else None
    gp = torch.empty(B, V, 3, device=dev, dtype=torch.float32) if want_pos else None
    if want_field or want_pos:
        _lib.call("deftet_tet_iso_fraction_bwd_f32", dev, g[0], g[1], g[2], field, pos, idx, csr[0], csr[1], gf, gp, iso, B, V, T, idx.shape[0])
    return gf, gp


class _TetIsoFraction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, pos, idx, csr, iso, return_area, return_volume):
        frac, area, vol = tet_iso_fraction_fwd(field, pos, idx, iso, return_area, return_volume)
        ctx.save_for_backward(field, pos)
        ctx.idx, ctx.csr, ctx.iso = idx, csr, iso
        ctx.set_materialize_grads(False)
        return frac, area, vol

    @staticmethod
    def backward(ctx, g_frac, g_area, g_vol):
        field, pos = ctx.saved_tensors
        want_f, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_f or want_p):
            return (None,) * 7
        if g_frac is None and g_area is None and g_vol is None:
            return (torch.zeros_like(field) if want_f else None, torch.zeros_like(pos) if want_p else None) + (None,) * 5
        csr = _csr_or_build(ctx.csr, ctx.idx, pos.shape[1])
        gf, gp = tet_iso_fraction_bwd(g_frac, g_area, g_vol, field.detach(), pos.detach(), ctx.idx, csr, ctx.iso, want_field=want_f,
                                      want_pos=want_p)
        return (gf, gp) + (None,) * 5


def tet_iso_fraction(field, pos_bxvx3, tet_idx, iso=0.0, csr=None, topology=None, return_area=False, return_volume=False):
    """frac f32 [B,T] (then area f32 [B,T] with return_area, then vol f32 [B,T] with return_volume): the share of every tet of
    the mesh (pos f32 [B,V,3], tet_idx int [T,4] or [B,T,4]) that lies inside the solid {field > iso} of the per-vertex field f32
    [B,V] or [B,V,1] — a soft per-tet occupancy in [0,1], exactly 0 or 1 off the surface, usable wherever a predicted per-tet
    occupancy is — the area of the iso polygon in the tet, and the tet's volume.  It is the solid marching_tets bounds: a corner
    is inside iff field > iso in fp32 (strict), the cuts sit at the same parameters.  The field is linear on a tet, so the
    fraction is a closed form in the four corner values (a small tet, its complement, or a wedge); computed in double from the
    fp32 inputs and rounded once.  A tet is live iff it is live to tet_field_gradient (det E > 0 in fp32) and its four corner
    values are finite; a dead tet has fraction, area and volume 0 and gives nothing to a backward.  (marching_tets differs on
    purpose: there a NaN corner is outside and faces are emitted.)  Differentiable in field and pos — frac in field alone, vol
    in pos alone, area in both — through the incidence CSR in its order with one fp64 accumulator per vertex and no float
    atomics (the same bits on every run); on a kink the derivative of the case the predicate picks.  `csr`, `topology` and the
    slow path as in tet_field_gradient."""
    field, pos, idx, iso = _tim_args("tet_iso_fraction", field, pos_bxvx3, tet_idx, iso, topology)
    csr = _resolve_csr("tet_iso_fraction", csr, topology, pos, idx)
    frac, area, vol = _TetIsoFraction.apply(field, pos, idx, csr, iso, bool(return_area), bool(return_volume))
    out = (frac,) + ((area,) if return_area else ()) + ((vol,) if return_volume else ())
    return out if len(out) > 1 else frac


class _TetIsoMeasures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, pos, idx, csr, iso, weights):
        lib = _lib.load()
        B, V = field.shape
        T, dev = idx.shape[1], field.device
        out = torch.empty(B, 5, device=dev, dtype=torch.float32)
        _lib.call("deftet_tet_iso_measures_fwd_f32", dev, field, pos, idx, weights, out, iso, B, V, T, idx.shape[0],
                  ws=lib.deftet_tet_iso_measures_workspace_bytes(B))
        ctx.save_for_backward(field, pos, weights)
        ctx.idx, ctx.csr, ctx.iso = idx, csr, iso
        return out

    @staticmethod
    def backward(ctx, g_out):
        field, pos, weights = ctx.saved_tensors
        want_f, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_f or want_p):
            return (None,) * 6
        B, V = field.shape
        idx, dev = ctx.idx, field.device
        csr = _csr_or_build(ctx.csr, idx, V)
        gf = torch.empty(B, V, device=dev, dtype=torch.float32) if want_f else None
        gp = torch.empty(B, V, 3, device=dev, dtype=torch.float32) if want_p else None
        _lib.call("deftet_tet_iso_measures_bwd_f32", dev, _f32c(g_out), weights, field, pos, idx, csr[0], csr[1], gf, gp, ctx.iso, B, V,
                  idx.shape[1], idx.shape[0])
        return (gf, gp) + (None,) * 4


def tet_iso_measures(field, pos_bxvx3, tet_idx, iso=0.0, weights=None, csr=None, topology=None):
    """f32 [B,5]: per shape the totals of tet_iso_fraction over the live tets —
        [:,0] = sum frac vol     the volume enclosed by the level set (inside the mesh)
        [:,1] = sum area         the area of the iso surface
        [:,2] = sum w frac vol   its intersection with the per-tet occupancy w
        [:,3] = sum w vol        the volume of that occupancy
        [:,4] = sum vol          the live volume
    weights f32 [B,T] is a ground-truth occupancy per tet, a CONSTANT (no gradient); None = 1.  vol is det E / 6 in double from
    the fp32 positions; the sums run in fp64 in one order and are rounded once.  iso_iou(measures) is the volumetric IoU.
    Differentiable in field and pos from the five upstream scalars alone (no [B,T] tensor in either direction), through the
    incidence CSR without float atomics; `csr`, `topology` and the slow path as in tet_field_gradient."""
    field, pos, idx, iso = _tim_args("tet_iso_measures", field, pos_bxvx3, tet_idx, iso, topology)
    w = None
    if weights is not None:
        w = _f32_on("tet_iso_measures", "weights", weights, field.device, False).detach()
        if tuple(w.shape) != (field.shape[0], idx.shape[1]):
            raise _expected("tet_iso_measures", "weights [%d,%d]" % (field.shape[0], idx.shape[1]), w)
    csr = _resolve_csr("tet_iso_measures", csr, topology, pos, idx)
    return _TetIsoMeasures.apply(field, pos, idx, csr, iso, w)


def iso_iou(measures):
    """[B]: the volumetric IoU of the field's solid with the occupancy, I / (V_in + W - I) on the columns of tet_iso_measures,
    0 where the union is 0.  Plain torch: differentiable through the measures."""
    v_in, inter, w = measures[..., 0], measures[..., 2], measures[..., 3]
    union = v_in + w - inter
    return torch.where(union > 0, inter / torch.where(union > 0, union, torch.ones_like(union)), torch.zeros_like(union))


def trilinear_devoxelize_fwd(r, is_training, coords, features):
    """(outs f32 [B,C,N], inds i32 [B,8,N], wgts f32 [B,8,N]) of coords f32 [B,3,N] in voxel units and features f32 [B,C,r^3]: the
    extension's trilinear_devoxelize_forward, one fixed expression per point (the reference kernel's bits).  hi = lo where
    d == 0, so nothing past r - 1 is read; coordinates are clamped to [0, r-1] first (the reference reads out of bounds there).
    Not training: inds and wgts are [1]-shaped zeros."""
    _lib.require_gpu(coords, features)
    coords, features = _pv_need(coords, torch.float32, "trilinear_devoxelize: coords"), _pv_need(features, torch.float32, "trilinear_devoxelize: features")
    r = int(r)
    if coords.dim() != 3 or coords.shape[1] != 3 or features.dim() != 3 or r < 1:
        raise RuntimeError("trilinear_devoxelize: coords [B,3,N] and features [B,C,r^3] expected")
    B, C, S = features.shape
    if S != r ** 3 or coords.shape[0] != B or coords.device != features.device:
        raise RuntimeError("trilinear_devoxelize: features %s do not match r = %d and coords %s" % (tuple(features.shape), r, tuple(coords.shape)))
    N, dev = coords.shape[2], features.device
    outs = torch.empty(B, C, N, device=dev, dtype=torch.float32)
    if is_training:
        inds = torch.empty(B, 8, N, device=dev, dtype=torch.int32)
        wgts = torch.empty(B, 8, N, device=dev, dtype=torch.float32)
    else:
        inds, wgts = torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.float32)
    _lib.call("deftet_voxel_sample_fwd_f32", dev, features, coords, outs, inds if is_training else None, wgts if is_training else None,
              B, C, r, N, 0, C, 1, 1)
    return outs, inds, wgts


def trilinear_devoxelize_bwd(grad_y, inds, wgts, r):
    """grad_x f32 [B,C,r^3] of grad_y f32 [B,C,N] through the recorded inds i32 / wgts f32 [B,8,N]: trilinear_devoxelize_backward on
    the sampler's atomic-free reduction, keyed by inds[:,0,:].  A term counts where the recorded index is the voxel its corner
    nominally lands in (cell + corner offset); the kernel's own fallen-back hi indices carry weight 0, so nothing is lost for
    inds / wgts that come from trilinear_devoxelize_fwd.  Hand-made inds without that lo / hi structure lose the other terms, and a
    non-finite grad_y does not spread through weight-0 terms as the reference's atomics would (0 * inf)."""
    _lib.require_gpu(grad_y, inds, wgts)
    grad_y, wgts = _pv_need(grad_y, torch.float32, "trilinear_devoxelize_bwd: grad_y"), _pv_need(wgts, torch.float32, "trilinear_devoxelize_bwd: wgts")
    inds, r = _pv_need(inds, torch.int32, "trilinear_devoxelize_bwd: inds"), int(r)
    if grad_y.dim() != 3 or inds.dim() != 3 or inds.shape != wgts.shape or inds.shape[1] != 8 or r < 1:
        raise RuntimeError("trilinear_devoxelize_bwd: grad_y [B,C,N] and inds, wgts [B,8,N] expected")
    B, C, N = grad_y.shape
    if inds.shape[0] != B or inds.shape[2] != N:
        raise RuntimeError("trilinear_devoxelize_bwd: grad_y %s and inds %s do not agree" % (tuple(grad_y.shape), tuple(inds.shape)))
    cells = _grid_cells(B, N, (r, r, r), grad_y.device, inds=inds, wgts=wgts)
    return _grid_bwd(grad_y, cells, C, 0, C).view(B, C, r ** 3)


# --------------------------------------------------------------------------------- ground-truth preparation
VOXELIZE_UNIT_BUDGET = 256                          # include/deftet_hip.h DEFTET_VOXELIZE_UNIT_BUDGET


class VoxelBits:
    """The bit-packed voxel grid the preparation stages hand to each other: `words` int32 [B,R,R,ceil(R/32)] on the GPU, bit
    k % 32 of word k // 32 of row (i, j) is voxel (i, j, k); pad bits are zero.  `stats` (mesh_voxelize only): int32 [4] on the
    GPU = (wave tasks, triangles split over several tasks, bad face index flag, 0)."""

    def __init__(self, words, resolution, stats=None):
        self.words, self.resolution, self.stats = words, int(resolution), stats
        self.n_batch, self.device = int(words.shape[0]), words.device

    def unpack(self):
        """uint8 [B,R,R,R]"""
        B, R, dev = self.n_batch, self.resolution, self.device
        vox = torch.empty(B, R, R, R, device=dev, dtype=torch.uint8)
        _lib.call("deftet_voxel_unpack_u8", dev, self.words, B, R, vox)
        return vox


def _vox_u8(vox, what):
    """[B,R,R,R] of any dtype -> contiguous uint8 (non-zero = occupied)"""
    _lib.require_gpu(vox)
    if vox.dim() != 4 or not (vox.shape[1] == vox.shape[2] == vox.shape[3]) or vox.shape[0] < 1 or vox.shape[1] < 1:
        raise RuntimeError("%s: a voxel grid [B,R,R,R] expected, got %s" % (what, tuple(vox.shape)))
    if vox.dtype == torch.bool:
        return vox.contiguous().view(torch.uint8)
    return vox.contiguous() if vox.dtype == torch.uint8 else (vox != 0).view(torch.uint8)


def voxel_pack(vox):
    """VoxelBits of a grid [B,R,R,R] (non-zero = occupied)."""
    v = _vox_u8(vox, "voxel_pack")
    B, R, dev = int(v.shape[0]), int(v.shape[1]), v.device
    words = torch.empty(B, R, R, (R + 31) // 32, device=dev, dtype=torch.int32)
    _lib.call("deftet_voxel_pack_u8", dev, v, B, R, words)
    return VoxelBits(words, R)


def _as_bits(v, what):
    return v if isinstance(v, VoxelBits) else voxel_pack(v)


def mesh_voxelize(vertices, faces, resolution, origin=None, scale=None, return_bits=False):
    """Conservative surface voxelization (parity unpinned; the rule is this library's own, include/deftet_hip.h): vertices f32
    [B,V,3], faces int [F,3], origin f32 [B,3] (None: the per-shape minimum), scale f32 [B] (None: the largest per-shape extent)
    -> uint8 [B,R,R,R], or the VoxelBits (with .stats) when return_bits.  q = ((v - origin) / scale) * R in fp32; voxel (i,j,k) is
    set iff a triangle overlaps the closed box [i,i+1] x [j,j+1] x [k,k+1] under the 13-axis separating-axis test in fp32.
    No host synchronisation."""
    _lib.require_gpu(vertices, faces, origin, scale)
    lib = _lib.load()
    v = _f32c(vertices)
    f = faces.long().contiguous()
    R = int(resolution)
    if v.dim() != 3 or v.shape[2] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise RuntimeError("mesh_voxelize: vertices [B,V,3] and faces [F,3] expected, got %s and %s" % (tuple(v.shape), tuple(f.shape)))
    B, V, F, dev = int(v.shape[0]), int(v.shape[1]), int(f.shape[0]), v.device
    if origin is not None:
        origin = _f32c(origin)
        if tuple(origin.shape) != (B, 3):
            raise RuntimeError("mesh_voxelize: origin [%d,3] expected, got %s" % (B, tuple(origin.shape)))
    if scale is not None:
        scale = _f32c(scale).reshape(-1)
        if scale.numel() != B:
            raise RuntimeError("mesh_voxelize: scale [%d] expected" % B)
    if R < 1:
        raise _lib.DefTetHipError("mesh_voxelize: resolution=%d must be positive (DEFTET_EINVAL)" % R)
    words = torch.empty(B, R, R, (R + 31) // 32, device=dev, dtype=torch.int32)
    vox = None if return_bits else torch.empty(B, R, R, R, device=dev, dtype=torch.uint8)
    stats = torch.empty(4, device=dev, dtype=torch.int32)
    _lib.call("deftet_mesh_voxelize_f32", dev, v, f, origin, scale, B, V, F, R, words, vox, stats, ws=lib.deftet_mesh_voxelize_workspace_bytes(B, F))
    return VoxelBits(words, R, stats) if return_bits else vox


def extract_odms(vox):
    """Orthographic depth maps int32 [B,6,R,R] of a grid [B,R,R,R] (or VoxelBits).  This library's own order: direction d scans
    axis d // 2, ascending for even d, descending for odd d; a map is indexed by the two other axes in ascending axis order;
    a depth is the number of empty voxels in front of the first occupied one, R for an empty ray."""
    v = vox.unpack() if isinstance(vox, VoxelBits) else _vox_u8(vox, "extract_odms")
    B, R, dev = int(v.shape[0]), int(v.shape[1]), v.device
    odms = torch.empty(B, 6, R, R, device=dev, dtype=torch.int32)
    _lib.call("deftet_extract_odms_u8", dev, v, B, R, odms)
    return odms


def project_odms(odms, voxelgrids=None, votes=1):
    """uint8 [B,R,R,R]: start from a full grid (or `voxelgrids`); direction d carves the voxels in front of its depth; a voxel
    stays iff fewer than `votes` directions carve it (extract_odms' direction order)."""
    _lib.require_gpu(odms)
    if odms.dim() != 4 or odms.shape[1] != 6 or odms.shape[2] != odms.shape[3] or odms.shape[0] < 1 or odms.shape[2] < 1:
        raise RuntimeError("project_odms: odms [B,6,R,R] expected, got %s" % (tuple(odms.shape),))
    o = odms.to(torch.int32).contiguous()
    B, R, dev = int(o.shape[0]), int(o.shape[2]), o.device
    vin = None
    if voxelgrids is not None:
        vin = _vox_u8(voxelgrids, "project_odms")
        if tuple(vin.shape) != (B, R, R, R) or vin.device != dev:
            raise RuntimeError("project_odms: voxelgrids [%d,%d,%d,%d] on %s expected" % (B, R, R, R, dev))
    out = torch.empty(B, R, R, R, device=dev, dtype=torch.uint8)
    _lib.call("deftet_project_odms_i32", dev, o, vin, B, R, int(votes), out)
    return out


def voxel_fill(vox_or_bits):
    """project_odms(extract_odms(v)) at votes = 1 in one launch sequence on the bit grid, without depth maps: a voxel stays iff on
    every axis it lies between the first and the last occupied voxel of its ray.  A VoxelBits gives a VoxelBits, a grid a uint8 grid."""
    bits = _as_bits(vox_or_bits, "voxel_fill")
    lib = _lib.load()
    B, R, dev = bits.n_batch, bits.resolution, bits.device
    out = torch.empty_like(bits.words)
    _lib.call("deftet_voxel_fill_b32", dev, bits.words, B, R, out, ws=lib.deftet_voxel_fill_workspace_bytes(B, R))
    res = VoxelBits(out, R)
    return res if isinstance(vox_or_bits, VoxelBits) else res.unpack()


def voxel_surface_mesh(vox, iso_value=0.5):
    """The faces of the occupied region (cuberille) of a grid [B,R,R,R] (occupied: vox > iso_value) or a VoxelBits:
    (list of B verts f32 [V_b,3], list of B faces int64 [F_b,3]).  Every occupied voxel and each of its six directions (-i, +i,
    -j, +j, -k, +k) whose neighbour is empty or outside emits two triangles with the normal pointing out.  Vertices are the
    lattice corners in use, integer coordinates 0..R, numbered in ascending (i (R+1) + j) (R+1) + k: welded by construction.
    Faces come in (voxel linear index, direction, triangle) order.  One read-back (the per-shape counts).
    Kaolin runs marching cubes here (parity unpinned): on a binary grid both surfaces lie on the voxel faces and differ by the
    chamfer at the corners; dataloader.py:55-60 rescales the result to the input's box, so offset and unit do not matter."""
    if isinstance(vox, VoxelBits):
        bits = vox
    else:
        _lib.require_gpu(vox)
        bits = voxel_pack(vox > iso_value)
    lib = _lib.load()
    B, R, dev = bits.n_batch, bits.resolution, bits.device
    offs = torch.empty(2 * (B + 1), device=dev, dtype=torch.int32)
    # the count pass leaves its tables here for the fill pass
    ws = torch.empty(lib.deftet_voxel_surface_workspace_bytes(B, R), dtype=torch.uint8, device=dev)
    _lib.call("deftet_voxel_surface_count_b32", dev, bits.words, B, R, offs, ws=ws)
    o = offs.tolist()                                                    # the one sync
    fo, vo = o[:B + 1], o[B + 1:]
    faces = torch.empty(fo[B], 3, device=dev, dtype=torch.int64)
    verts = torch.empty(vo[B], 3, device=dev, dtype=torch.float32)
    _lib.call("deftet_voxel_surface_fill_b32", dev, bits.words, B, R, fo[B], vo[B], verts if vo[B] else None, faces if fo[B] else None, ws=ws)
    return [verts[vo[b]:vo[b + 1]] for b in range(B)], [faces[fo[b]:fo[b + 1]] for b in range(B)]


def face_edges(faces_fx3, n_vertex):
    """The unique directed vertex pairs (a, b), a != b, of a triangle list, ascending by (a, b): int32 [n,2].  One read-back."""
    _lib.require_gpu(faces_fx3)
    lib = _lib.load()
    f = faces_fx3.long().contiguous()
    if f.dim() != 2 or f.shape[1] != 3:
        raise RuntimeError("face_edges: faces [F,3] expected, got %s" % (tuple(f.shape),))
    F, V, dev = int(f.shape[0]), int(n_vertex), f.device
    pairs = torch.empty(6 * F, 2, device=dev, dtype=torch.int32)
    n = torch.empty(2, device=dev, dtype=torch.int32)
    _lib.call("deftet_face_edges_i32", dev, f, F, V, pairs if F else None, n, ws=lib.deftet_face_edges_workspace_bytes(F))
    count, bad = n.tolist()
    if bad:
        raise RuntimeError("face_edges: a face index is outside [0, %d)" % V)
    return pairs[:count]

