"""StreamSet: S independent GKArray streams on one MI355X, batched.

Every stream behaves exactly like one reference ``GKArray`` (gkarray.py,
``gk:N``) fed the same values in the same order.  All work runs in the HIP
kernels of ``libgkarray_hip.so`` through the C ABI of ``include/gk_capi.h``;
PyTorch only allocates device tensors and supplies the current HIP stream.
"""
import contextlib
import ctypes
import os

import torch

from . import _lib as L

__all__ = ["StreamSet", "peek"]


def peek(path, cpu=False):
    """(eps, num_streams) from a GKSTATE file's header."""
    lib = L.load_cpu() if cpu else L.load()
    eps = ctypes.c_double()
    S = ctypes.c_int64()
    L.check(lib.gk_peek(os.fsencode(path), ctypes.byref(eps), ctypes.byref(S)), lib)
    return eps.value, S.value


def _stream_ptr(device):
    if device.type != "cuda":
        return None
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class StreamSet:
    """A batch of ``num_streams`` GKArray sketches sharing one ``eps``.

    ``ingest(values, offsets)`` is the batched ``add`` (gk:49-61): stream ``s``
    receives ``values[offsets[s]:offsets[s+1]]`` in order.
    """

    def __init__(self, num_streams, eps, device=None, cap_hint=0):
        """``device``: a cuda (HIP) device -- the MI355X engine, the default --
        or ``"cpu"`` for the host engine (libgkarray_cpu.so, same C ABI and
        results, multi-threaded over streams).  There is no implicit fallback
        from the GPU to the host engine."""
        if device is not None and torch.device(device).type == "cpu":
            self._lib = L.load_cpu()
            device = torch.device("cpu")
            dev_index = -1
        else:
            if not torch.cuda.is_available():
                raise L.GKBackendError(L.GK_E_HIP, "no GPU visible (the host engine is StreamSet(..., device='cpu'))")
            self._lib = L.load()
            if device is None:
                device = torch.device("cuda", torch.cuda.current_device())
            device = torch.device(device)
            if device.type != "cuda":
                raise ValueError("StreamSet needs a cuda (HIP) device or 'cpu', got %s" % device)
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            dev_index = device.index
        self.device = device
        self.num_streams = int(num_streams)
        self.eps = eps
        h = ctypes.c_void_p()
        with self._ctx():
            self._check(self._lib.gk_create(self.num_streams, float(eps), int(cap_hint), dev_index, ctypes.byref(h)))
        self._h = h

    @property
    def is_cpu(self):
        return self.device.type == "cpu"

    def _ctx(self):
        # (no device switch when the set's device is already current: the
        # context manager's get/set round trip is host time on every call)
        if self.device.type == "cpu" or torch.cuda.current_device() == self.device.index:
            return contextlib.nullcontext()
        return torch.cuda.device(self.device)

    def _check(self, rc):
        return L.check(rc, self._lib)

    def set_threads(self, threads):
        """Host threads of the CPU engine (0 = every CPU this process may use)."""
        if not self.is_cpu:
            raise ValueError("set_threads applies to the CPU engine only")
        self._check(self._lib.gk_cpu_set_threads(self._h, int(threads)))

    # ------------------------------------------------------------------ basics
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gk_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def flush_period(self):
        return self._lib.gk_flush_period(self._h)

    def capacity(self, cls=0):
        return self._lib.gk_capacity(self._h, cls)

    @property
    def num_promoted(self):
        return self._lib.gk_num_promoted(self._h)

    def class_usage(self):
        """What the set holds per capacity class (``gk_class_usage``): a list
        with one dict per class -- ``capacity`` (table entries of a slot),
        ``streams`` (streams whose class it is), ``slots_used`` / ``slots_alloc``
        (of the class's arena; class 0: both num_streams), ``arena_bytes`` and
        ``workspace_bytes``.  The host engine has one unbounded class.  The
        set's earlier work is settled first."""
        out = []
        with self._ctx():
            cls = 0
            while self._lib.gk_capacity(self._h, cls) > 0:
                v = [ctypes.c_int64(0) for _ in range(5)]
                self._check(self._lib.gk_class_usage(self._h, cls, *[ctypes.byref(x) for x in v], self._sp()))
                out.append(dict(capacity=self._lib.gk_capacity(self._h, cls), streams=v[0].value,
                                slots_used=v[1].value, slots_alloc=v[2].value, arena_bytes=v[3].value,
                                workspace_bytes=v[4].value))
                cls += 1
        return out

    def compact(self):
        """Every stream into the smallest capacity class that holds its table
        (``gk_compact``): streams that were reset or replaced by smaller ones
        leave the large classes, member lists and slots become dense, and the
        arena memory nobody needs goes back to the device.  No stream's state
        changes by a bit.  Returns ``{"demoted": streams whose class dropped,
        "bytes_freed": arena + workspace bytes returned}``.  Never called
        implicitly.  On the host engine it returns the unused capacity of the
        streams' buffers (``demoted`` is 0)."""
        dem = ctypes.c_int64(0)
        freed = ctypes.c_int64(0)
        with self._ctx():
            try:
                self._check(self._lib.gk_compact(self._h, ctypes.byref(dem), ctypes.byref(freed), self._sp()))
            finally:
                self._inflight = None  # (the call synchronised)
        return {"demoted": dem.value, "bytes_freed": freed.value}

    def _sp(self):
        return _stream_ptr(self.device)

    def _dev(self, t, dtype):
        t = torch.as_tensor(t, dtype=dtype)
        if t.device != self.device:
            t = t.to(self.device)
        return t.contiguous()

    # ------------------------------------------------------------------ ingest
    def reset(self):
        """Every stream back to ``GKArray(eps)`` (gk:21-29)."""
        with self._ctx():
            self._check(self._lib.gk_reset(self._h, self._sp()))

    def sync(self):
        """Wait for this set's work on the current stream; raise an
        asynchronous error of an earlier call (a stream that outgrew every
        table capacity class keeps its previous state: GK_E_OVERFLOW)."""
        with self._ctx():
            try:
                self._check(self._lib.gk_sync(self._h, self._sp()))
            finally:
                self._inflight = None  # the last call's inputs are no longer read

    def ingest(self, values, offsets, quantiles=None, single=False, sync=True):
        """Batched ``GKArray.add`` (gk:49-61) over all streams.

        values: float64 [N] (device tensor preferred); offsets: int64 [S+1].
        With ``quantiles=qs`` the call continues with ``quantiles(qs)``
        (gk:187-232) for every stream in the same kernel pass (the leftover
        pending values are flushed, as the reference's quantiles() does) and
        returns the [S, len(qs)] float64 device tensor.
        ``sync=False`` only enqueues the work on the current HIP stream (the
        C ABI itself never blocks here); errors then surface at a later call
        or ``sync()``.
        """
        v = self._dev(values, torch.float64)
        o = self._dev(offsets, torch.int64)
        if o.numel() != self.num_streams + 1:
            raise ValueError("offsets must have num_streams+1 entries")
        if v.numel() == 0:
            v = torch.zeros(1, dtype=torch.float64, device=self.device)
        if quantiles is None:
            with self._ctx():
                self._check(self._lib.gk_ingest(self._h, _ptr(v), _ptr(o), self._sp()))
            # gk_capi.h: the inputs stay valid until the set's next call or
            # gk_sync (a deferred stream is re-run from them)
            self._inflight = (v, o)
            if sync:
                self.sync()
            return None
        qs = [float(q) for q in quantiles]
        nq = len(qs)
        out = torch.empty((self.num_streams, max(nq, 1)), dtype=torch.float64, device=self.device)
        arr = (ctypes.c_double * max(nq, 1))(*qs)
        mode = L.GK_Q_SINGLE if single else L.GK_Q_LIST
        with self._ctx():
            self._check(self._lib.gk_ingest_quantiles(self._h, _ptr(v), _ptr(o), arr, nq, _ptr(out), mode,
                                                  self._sp()))
        self._inflight = (v, o, out)
        if sync:
            self.sync()
        return out[:, :nq]

    # ------------------------------------------------------------ keyed ingest
    def _keyed_args(self, ids, values):
        """(ids int32, values float64) on the set's device, checked."""
        i = torch.as_tensor(ids)
        v = torch.as_tensor(values)
        if i.dim() != 1 or v.dim() != 1:
            raise ValueError("ids and values must be one-dimensional")
        if i.numel() != v.numel():
            raise ValueError("ids and values must have the same length (%d vs %d)" % (i.numel(), v.numel()))
        if i.numel() > 2 ** 31 - 1:
            raise ValueError("at most 2^31-1 samples per call")
        return self._ids_i32(i), self._dev(v, torch.float64)

    def _ids_i32(self, i):
        """A one-dimensional id tensor as int32 on the set's device."""
        if i.dtype == torch.int32:
            pass
        elif i.dtype == torch.int64 or (i.numel() == 0 and not i.dtype.is_floating_point):
            # the C ABI takes int32 ids: one range check (an id beyond int32
            # would wrap into a valid stream) and one conversion pass
            if i.numel() and (int(i.max().item()) > 2 ** 31 - 1 or int(i.min().item()) < -2 ** 31):
                raise ValueError("an id does not fit int32")
            i = i.to(torch.int32)
        else:
            raise ValueError("ids must be int32 or int64, got %s" % i.dtype)
        return self._dev(i, torch.int32)

    def group_by_key(self, ids, values):
        """Stable group-by of samples in arrival order (``gk_group_by_key``):
        returns ``(values_grouped, offsets)`` such that stream s owns
        ``values_grouped[offsets[s]:offsets[s+1]]``, the values whose id is s
        in ascending sample index, copied bit for bit -- the CSR batch
        ``ingest`` takes.  Negative ids are skipped; an id >= num_streams
        raises ``GKBackendError`` (GK_E_ARG).  ``ids`` is int32, or int64 at
        the cost of a range check and a conversion pass."""
        i, v = self._keyed_args(ids, values)
        n = i.numel()
        out = torch.empty(max(n, 1), dtype=torch.float64, device=self.device)
        offs = torch.empty(self.num_streams + 1, dtype=torch.int64, device=self.device)
        with self._ctx():
            self._check(self._lib.gk_group_by_key(self._h, _ptr(i) if n else None, _ptr(v) if n else None, n,
                                                  _ptr(out), _ptr(offs), self._sp()))
        self._inflight = (i, v, out, offs)
        self.sync()
        return out[:int(offs[-1].item())], offs

    def ingest_keyed(self, ids, values, quantiles=None, single=False, sync=True):
        """``for i in range(len(ids)): self[ids[i]].add(values[i])`` (gk:49-61)
        in one call on unsorted device arrays (``gk_ingest_keyed``): the
        samples are grouped by a stable sort on the device and go through the
        path of ``ingest``.  Negative ids are skipped.  An id >= num_streams
        voids the call (no value is added; a fused query answers from the
        state before the call) and raises ``GKBackendError`` (GK_E_ARG), at
        ``sync()`` at the latest.  ``quantiles``, ``single`` and ``sync`` as
        ``ingest``; ``ids`` as ``group_by_key``."""
        i, v = self._keyed_args(ids, values)
        n = i.numel()
        pi, pv = (_ptr(i), _ptr(v)) if n else (None, None)
        if quantiles is None:
            with self._ctx():
                self._check(self._lib.gk_ingest_keyed(self._h, pi, pv, n, None, 0, None, L.GK_Q_LIST, self._sp()))
            self._inflight = (i, v)
            if sync:
                self.sync()
            return None
        qs = [float(q) for q in quantiles]
        nq = len(qs)
        out = torch.empty((self.num_streams, max(nq, 1)), dtype=torch.float64, device=self.device)
        arr = (ctypes.c_double * max(nq, 1))(*qs)
        mode = L.GK_Q_SINGLE if single else L.GK_Q_LIST
        with self._ctx():
            self._check(self._lib.gk_ingest_keyed(self._h, pi, pv, n, arr, nq, _ptr(out), mode, self._sp()))
        self._inflight = (i, v, out)
        if sync:
            self.sync()
        return out[:, :nq]

    def ingest_lists(self, seqs):
        """Convenience: ``seqs[s]`` is the list of values for stream s."""
        if len(seqs) != self.num_streams:
            raise ValueError("need one sequence per stream")
        lens = [len(x) for x in seqs]
        offs = [0]
        for n in lens:
            offs.append(offs[-1] + n)
        flat = [float(x) for s in seqs for x in s]
        self.ingest(torch.tensor(flat, dtype=torch.float64), torch.tensor(offs, dtype=torch.int64))

    def flush(self):
        """``merge_compress()`` where values are pending (gk:45-46, 166, 197)."""
        with self._ctx():
            self._check(self._lib.gk_flush(self._h, self._sp()))
        self.sync()

    # ------------------------------------------------------------------ query
    def quantiles(self, qs, single=False):
        """Batched ``GKArray.quantiles(qs)`` (gk:187-232); ``single=True``
        gives ``quantile(q)`` semantics for every q (gk:156-185).

        Returns a float64 device tensor [S, len(qs)].  Flushes pending values.
        """
        qs = [float(q) for q in qs]
        nq = len(qs)
        out = torch.empty((self.num_streams, max(nq, 1)), dtype=torch.float64, device=self.device)
        if nq == 0:
            return out[:, :0]
        arr = (ctypes.c_double * nq)(*qs)
        mode = L.GK_Q_SINGLE if single else L.GK_Q_LIST
        with self._ctx():
            self._check(self._lib.gk_quantiles(self._h, arr, nq, _ptr(out), mode, self._sp()))
        self.sync()
        return out

    def stats(self):
        """num_values/_min/_max/sum/avg (gk:25-42) and table / pending sizes,
        without flushing.  Dict of device tensors of length S."""
        S = max(self.num_streams, 1)
        d = dict(
            n=torch.empty(S, dtype=torch.int64, device=self.device),
            min=torch.empty(S, dtype=torch.float64, device=self.device),
            max=torch.empty(S, dtype=torch.float64, device=self.device),
            sum=torch.empty(S, dtype=torch.float64, device=self.device),
            avg=torch.empty(S, dtype=torch.float64, device=self.device),
            size=torch.empty(S, dtype=torch.int32, device=self.device),
            pending=torch.empty(S, dtype=torch.int32, device=self.device),
        )
        with self._ctx():
            self._check(self._lib.gk_stats(self._h, _ptr(d["n"]), _ptr(d["min"]), _ptr(d["max"]),
                                       _ptr(d["sum"]), _ptr(d["avg"]), _ptr(d["size"]),
                                       _ptr(d["pending"]), self._sp()))
        if self.num_streams == 0:
            d = {k: v[:0] for k, v in d.items()}
        return d

    # ------------------------------------------------------- per-stream selection
    def _select_ids(self, ids):
        """ids as int32 on the set's device, checked as ``_keyed_args`` checks them."""
        i = torch.as_tensor(ids)
        if i.dim() != 1:
            raise ValueError("ids must be one-dimensional")
        if i.numel() > 2 ** 31 - 1:
            raise ValueError("at most 2^31-1 ids per call")
        return self._ids_i32(i)

    def quantiles_select(self, ids, qs, single=False):
        """``self[ids[k]].quantiles(qs)`` for every k (``gk_quantiles_select``;
        ``single=True``: ``quantile(q)`` for every q): a float64 device tensor
        [len(ids), len(qs)], row k for ``ids[k]``.  Only the listed streams
        with pending values are flushed (gk:166-167, 197-198); every other
        stream of the set stays bit-identical.  Ids may repeat and come in any
        order; an id outside [0, num_streams) raises ``GKBackendError``
        (GK_E_ARG) before anything is changed.  ``ids`` is int32, or int64 at
        the cost of a range check and a conversion."""
        i = self._select_ids(ids)
        K = i.numel()
        qs = [float(q) for q in qs]
        nq = len(qs)
        out = torch.empty((max(K, 1), max(nq, 1)), dtype=torch.float64, device=self.device)
        arr = (ctypes.c_double * max(nq, 1))(*qs)
        mode = L.GK_Q_SINGLE if single else L.GK_Q_LIST
        with self._ctx():
            self._check(self._lib.gk_quantiles_select(self._h, _ptr(i) if K else None, K, arr, nq, _ptr(out), mode,
                                                      self._sp()))
        self._inflight = None  # (the call synchronised)
        return out[:K, :nq]

    def flush_select(self, ids):
        """``merge_compress()`` of the listed streams that hold pending values
        (``gk_flush_select``; what ``size()`` does first, gk:45-46)."""
        i = self._select_ids(ids)
        K = i.numel()
        with self._ctx():
            self._check(self._lib.gk_flush_select(self._h, _ptr(i) if K else None, K, self._sp()))
        self._inflight = None

    def reset_select(self, ids):
        """The listed streams back to ``GKArray(eps)`` (gk:21-29), the set's
        ``sketches[k] = GKArray(eps)`` (``gk_reset_select``).  On the GPU a
        reset stream keeps its capacity class: no memory is returned until
        ``compact()``."""
        i = self._select_ids(ids)
        K = i.numel()
        with self._ctx():
            self._check(self._lib.gk_reset_select(self._h, _ptr(i) if K else None, K, self._sp()))
        self._inflight = None

    def stats_select(self, ids):
        """``stats()`` of the listed streams (``gk_stats_select``): a dict with
        the keys of ``stats()``, each a device tensor of length len(ids), entry
        k for ``ids[k]``.  Does not flush."""
        i = self._select_ids(ids)
        K = i.numel()
        n = max(K, 1)
        d = dict(
            n=torch.empty(n, dtype=torch.int64, device=self.device),
            min=torch.empty(n, dtype=torch.float64, device=self.device),
            max=torch.empty(n, dtype=torch.float64, device=self.device),
            sum=torch.empty(n, dtype=torch.float64, device=self.device),
            avg=torch.empty(n, dtype=torch.float64, device=self.device),
            size=torch.empty(n, dtype=torch.int32, device=self.device),
            pending=torch.empty(n, dtype=torch.int32, device=self.device),
        )
        with self._ctx():
            self._check(self._lib.gk_stats_select(self._h, _ptr(i) if K else None, K, _ptr(d["n"]), _ptr(d["min"]),
                                                  _ptr(d["max"]), _ptr(d["sum"]), _ptr(d["avg"]), _ptr(d["size"]),
                                                  _ptr(d["pending"]), self._sp()))
        self._inflight = None
        return {k: v[:K] for k, v in d.items()}

    # ------------------------------------------------------------ rank queries
    def _rank_out(self, want, rows, nx, name):
        """An output of ``ranks``: (tensor handed back, tensor whose pointer the
        call gets) -- (None, None) for an output that is not wanted."""
        if want is None or want is False:
            return None, None
        if want is True:
            t = torch.empty((max(rows, 1), max(nx, 1)), dtype=torch.int64, device=self.device)
            return t[:rows, :nx], t
        if not isinstance(want, torch.Tensor) or want.dtype != torch.int64 or want.device != self.device \
                or not want.is_contiguous() or tuple(want.shape) != (rows, nx):
            raise ValueError("%s must be True, False or a contiguous int64 tensor of shape (%d, %d) on %s"
                             % (name, rows, nx, self.device))
        return want, (want if want.numel() else torch.empty(1, dtype=torch.int64, device=self.device))

    def ranks(self, xs, lo=True, hi=True):
        """Bounds on every stream's count of values <= x (``gk_ranks``), the
        inverse of ``quantiles``: ``(lo, hi)``, int64 device tensors
        [S, len(xs)] with ``lo <= #{values <= x} <= hi`` and ``hi - lo <=
        2 eps n`` for a stream built by ``add`` alone (after a merge or a
        roll-up the pair is still the formula on the table, gk_capi.h, but the
        true count may lie outside).  Pending values are flushed first, as
        ``quantiles`` does.  ``xs``: any order, repeats allowed, no NaN.
        ``lo`` / ``hi``: False leaves that output out (None is returned in its
        place); an int64 tensor [S, len(xs)] on the set's device is written in
        place."""
        xs = [float(x) for x in xs]
        nx = len(xs)
        S = self.num_streams
        lo_t, lo_p = self._rank_out(lo, S, nx, "lo")
        hi_t, hi_p = self._rank_out(hi, S, nx, "hi")
        arr = (ctypes.c_double * max(nx, 1))(*xs)
        with self._ctx():
            try:
                self._check(self._lib.gk_ranks(self._h, arr, nx, _ptr(lo_p), _ptr(hi_p), self._sp()))
            finally:
                self._inflight = None  # (the call synchronised)
        return lo_t, hi_t

    def ranks_select(self, ids, xs, lo=True, hi=True):
        """``ranks(xs)`` of the listed streams (``gk_ranks_select``): int64
        tensors [len(ids), len(xs)], row k for ``ids[k]``.  Only the listed
        streams with pending values are flushed; ids as ``quantiles_select``."""
        i = self._select_ids(ids)
        K = i.numel()
        xs = [float(x) for x in xs]
        nx = len(xs)
        lo_t, lo_p = self._rank_out(lo, K, nx, "lo")
        hi_t, hi_p = self._rank_out(hi, K, nx, "hi")
        arr = (ctypes.c_double * max(nx, 1))(*xs)
        with self._ctx():
            self._check(self._lib.gk_ranks_select(self._h, _ptr(i) if K else None, K, arr, nx, _ptr(lo_p), _ptr(hi_p),
                                                  self._sp()))
        self._inflight = None
        return lo_t, hi_t

    @staticmethod
    def _cdf(lo, hi, n):
        # (lo + hi) / (2 n); 0 / 0 = NaN where n == 0
        return (lo + hi).to(torch.float64) / (2.0 * n.to(torch.float64)).unsqueeze(1)

    def cdf(self, xs):
        """Point estimate of every stream's share of values <= x: float64
        [S, len(xs)], ``(lo + hi) / (2 n)`` of ``ranks(xs)``; NaN where n == 0."""
        lo, hi = self.ranks(xs)
        return self._cdf(lo, hi, self.stats()["n"])

    def cdf_select(self, ids, xs):
        """``cdf(xs)`` of the listed streams: float64 [len(ids), len(xs)]."""
        i = self._select_ids(ids)
        lo, hi = self.ranks_select(i, xs)
        return self._cdf(lo, hi, self.stats_select(i)["n"])

    def _keyed_out(self, want, count, name):
        """An output of ``ranks_keyed``, as ``_rank_out`` for one dimension."""
        if want is None or want is False:
            return None, None
        if want is True:
            t = torch.empty(max(count, 1), dtype=torch.int64, device=self.device)
            return t[:count], t
        if not isinstance(want, torch.Tensor) or want.dtype != torch.int64 or want.device != self.device \
                or not want.is_contiguous() or tuple(want.shape) != (count,):
            raise ValueError("%s must be True, False or a contiguous int64 tensor of shape (%d,) on %s"
                             % (name, count, self.device))
        return want, (want if want.numel() else torch.empty(1, dtype=torch.int64, device=self.device))

    def ranks_keyed(self, ids, xs, lo=True, hi=True, n=False):
        """Rank bounds per sample (``gk_ranks_keyed``): row i is
        ``ranks_select([ids[i]], [xs[i]])`` -- where ``xs[i]`` sits in the
        distribution of stream ``ids[i]`` -- and, with ``n``, that stream's
        count.  Returns ``(lo, hi, n)``, int64 device tensors [len(ids)]; None
        for an output not asked for; an int64 tensor [len(ids)] on the set's
        device is written in place.  Ids may repeat and come in any order; a
        negative id is "no stream" (``KeyDirectory.lookup`` of an unknown key):
        its row is (0, 0, 0) and its x may be NaN.  An id >= num_streams or a
        NaN x on a live row raises ``GKBackendError`` (GK_E_ARG) with nothing
        changed.  The occurring streams with pending values are flushed first,
        as ``ranks_select`` does.  ``ids`` is int32, or int64 at the cost of a
        range check and a conversion pass; ``xs`` becomes float64 on the set's
        device."""
        i = torch.as_tensor(ids)
        # (a Python list goes straight to float64, not through torch's float32 default)
        x = xs if isinstance(xs, torch.Tensor) else torch.as_tensor(xs, dtype=torch.float64)
        if i.dim() != 1 or x.dim() != 1:
            raise ValueError("ids and xs must be one-dimensional")
        if i.numel() != x.numel():
            raise ValueError("ids and xs must have the same length (%d vs %d)" % (i.numel(), x.numel()))
        if i.numel() > 2 ** 31 - 1:
            raise ValueError("at most 2^31-1 samples per call")
        i, x = self._ids_i32(i), self._dev(x, torch.float64)
        K = i.numel()
        lo_t, lo_p = self._keyed_out(lo, K, "lo")
        hi_t, hi_p = self._keyed_out(hi, K, "hi")
        n_t, n_p = self._keyed_out(n, K, "n")
        with self._ctx():
            try:
                self._check(self._lib.gk_ranks_keyed(self._h, _ptr(i) if K else None, _ptr(x) if K else None, K,
                                                     _ptr(lo_p), _ptr(hi_p), _ptr(n_p), self._sp()))
            finally:
                self._inflight = None  # (the call synchronised)
        return lo_t, hi_t, n_t

    def cdf_keyed(self, ids, xs):
        """Point estimate per sample of stream ``ids[i]``'s share of values <=
        ``xs[i]``: float64 [len(ids)], ``(lo + hi) / (2 n)`` of ``ranks_keyed``;
        NaN where n == 0, so also for a negative id."""
        lo, hi, n = self.ranks_keyed(ids, xs, n=True)
        return (lo + hi).to(torch.float64) / (2.0 * n.to(torch.float64))

    # ------------------------------------------------- keyed score-and-ingest
    def rank_ingest_keyed(self, ids, values, lo=True, hi=True, n=False, quantiles=None, single=False, sync=True):
        """``ranks_keyed(ids, values, lo, hi, n)`` followed by
        ``ingest_keyed(ids, values, quantiles, single, sync)`` in one call
        (``gk_rank_ingest_keyed``): every sample is ranked against its stream
        BEFORE any value of the batch is added, then the batch is added in
        arrival order -- answers and stream states are bit for bit those of
        the two calls, at one group-by of the samples instead of two.  Returns
        ``(lo, hi, n)``, or ``(lo, hi, n, q)`` with ``quantiles``; outputs as
        ``ranks_keyed`` (all three may be left out: the call is then
        ``ingest_keyed``), ``q``, ``single`` and ``sync`` as ``ingest_keyed``.
        A negative id is "no stream": row (0, 0, 0), value not added.  An
        id >= num_streams or a NaN value on a live row raises
        ``GKBackendError`` (GK_E_ARG) from the call itself with nothing changed,
        so NaN cannot be added this way.  With ``sync=False`` the outputs are
        ordered on the current HIP stream."""
        # (a Python list goes straight to float64, as in ranks_keyed)
        v = values if isinstance(values, torch.Tensor) else torch.as_tensor(values, dtype=torch.float64)
        i, v = self._keyed_args(ids, v)
        K = i.numel()
        lo_t, lo_p = self._keyed_out(lo, K, "lo")
        hi_t, hi_p = self._keyed_out(hi, K, "hi")
        n_t, n_p = self._keyed_out(n, K, "n")
        pi, pv = (_ptr(i), _ptr(v)) if K else (None, None)
        if quantiles is None:
            nq, arr, out = 0, None, None
        else:
            qs = [float(q) for q in quantiles]
            nq = len(qs)
            out = torch.empty((self.num_streams, max(nq, 1)), dtype=torch.float64, device=self.device)
            arr = (ctypes.c_double * max(nq, 1))(*qs)
        mode = L.GK_Q_SINGLE if single else L.GK_Q_LIST
        with self._ctx():
            self._check(self._lib.gk_rank_ingest_keyed(self._h, pi, pv, K, _ptr(lo_p), _ptr(hi_p), _ptr(n_p), arr, nq,
                                                       _ptr(out), mode, self._sp()))
        self._inflight = (i, v, lo_p, hi_p, n_p, out)
        if sync:
            self.sync()
        if quantiles is None:
            return lo_t, hi_t, n_t
        return lo_t, hi_t, n_t, out[:, :nq]

    def score_ingest_keyed(self, ids, values, quantiles=None, single=False, sync=True):
        """``cdf_keyed(ids, values)`` -- ``(lo + hi) / (2 n)`` against the state
        before the batch, NaN where n == 0 -- and then ``ingest_keyed``, through
        ``rank_ingest_keyed``.  Returns the scores, or ``(scores, q)`` with
        ``quantiles``."""
        r = self.rank_ingest_keyed(ids, values, n=True, quantiles=quantiles, single=single, sync=sync)
        score = (r[0] + r[1]).to(torch.float64) / (2.0 * r[2].to(torch.float64))
        return score if quantiles is None else (score, r[3])

    # ------------------------------------------------------------------ export
    def tables(self):
        """All tables in CSR form: (offs int64[S+1], v f64, g i32, d i32)."""
        S = self.num_streams
        sizes = torch.empty(max(S, 1), dtype=torch.int32, device=self.device)
        with self._ctx():
            self._check(self._lib.gk_export_sizes(self._h, _ptr(sizes), self._sp()))
        sizes = sizes[:S]
        offs = torch.zeros(S + 1, dtype=torch.int64, device=self.device)
        if S:
            offs[1:] = torch.cumsum(sizes.to(torch.int64), 0)
        tot = int(offs[-1].item()) if S else 0
        v = torch.empty(max(tot, 1), dtype=torch.float64, device=self.device)
        g = torch.empty(max(tot, 1), dtype=torch.int32, device=self.device)
        d = torch.empty(max(tot, 1), dtype=torch.int32, device=self.device)
        with self._ctx():
            self._check(self._lib.gk_export(self._h, _ptr(offs), _ptr(v), _ptr(g), _ptr(d), self._sp()))
        return offs, v[:tot], g[:tot], d[:tot]

    def pending(self):
        """All pending (incoming) values in CSR form: (poffs int64[S+1], pv f64)."""
        S = self.num_streams
        sizes = torch.empty(max(S, 1), dtype=torch.int32, device=self.device)
        with self._ctx():
            self._check(self._lib.gk_export_pending_sizes(self._h, _ptr(sizes), self._sp()))
        sizes = sizes[:S]
        offs = torch.zeros(S + 1, dtype=torch.int64, device=self.device)
        if S:
            offs[1:] = torch.cumsum(sizes.to(torch.int64), 0)
        tot = int(offs[-1].item()) if S else 0
        pv = torch.empty(max(tot, 1), dtype=torch.float64, device=self.device)
        with self._ctx():
            self._check(self._lib.gk_export_pending(self._h, _ptr(offs), _ptr(pv), self._sp()))
        return offs, pv[:tot]

    def table(self, s):
        """Stream s's table as a list of (v, g, d) (the reference's entries)."""
        offs, v, g, d = self.tables()
        a, b = int(offs[s]), int(offs[s + 1])
        vv, gg, dd = v[a:b].cpu().tolist(), g[a:b].cpu().tolist(), d[a:b].cpu().tolist()
        return list(zip(vv, gg, dd))

    def export_state(self):
        """Full state (checkpoint / RCCL payload) as a dict of device tensors."""
        offs, v, g, d = self.tables()
        poffs, pv = self.pending()
        st = self.stats()
        return dict(eps=self.eps, offs=offs, v=v, g=g, d=d, poffs=poffs, pv=pv,
                    n=st["n"], min=st["min"], max=st["max"], sum=st["sum"], avg=st["avg"])

    def import_state(self, state):
        """Inverse of export_state (replaces every stream's state)."""
        if state["eps"] != self.eps:
            raise ValueError("eps mismatch on import")
        t = {k: self._dev(state[k], dt) for k, dt in (
            ("offs", torch.int64), ("v", torch.float64), ("g", torch.int32), ("d", torch.int32),
            ("poffs", torch.int64), ("pv", torch.float64), ("n", torch.int64),
            ("min", torch.float64), ("max", torch.float64), ("sum", torch.float64),
            ("avg", torch.float64))}
        for k in ("v", "g", "d", "pv"):
            if t[k].numel() == 0:
                t[k] = torch.zeros(1, dtype=t[k].dtype, device=self.device)
        with self._ctx():
            self._check(self._lib.gk_import(self._h, _ptr(t["offs"]), _ptr(t["v"]), _ptr(t["g"]),
                                        _ptr(t["d"]), _ptr(t["poffs"]), _ptr(t["pv"]),
                                        _ptr(t["n"]), _ptr(t["min"]), _ptr(t["max"]),
                                        _ptr(t["sum"]), _ptr(t["avg"]), self._sp()))

    # ------------------------------------------------------------------ files
    def save(self, path):
        """Write every stream's state (tables, pending values, n/min/max/sum/avg)
        to a versioned GKSTATE file (csrc/gk_format.h) without flushing."""
        with self._ctx():
            self._check(self._lib.gk_save(self._h, os.fsencode(path), self._sp()))

    def load_state(self, path):
        """Replace every stream's state with a GKSTATE file's (same stream
        count and eps as this set)."""
        with self._ctx():
            rc = self._lib.gk_load(self._h, os.fsencode(path), self._sp())
        if rc == L.GK_E_EPS_MISMATCH:
            from .gkarray import UnequalEpsilonException
            raise UnequalEpsilonException(L.last_error(self._lib))
        self._check(rc)

    @classmethod
    def load(cls, path, device=None):
        """A new StreamSet holding the state saved in ``path``."""
        eps, S = peek(path, cpu=device is not None and torch.device(device).type == "cpu")
        ss = cls(S, eps, device=device)
        ss.load_state(path)
        return ss

    def import_arrays(self, offs, v, g, d, poffs, pv, n, mn, mx, sm, av):
        """``gk_import`` on device tensors as they are (no copies): stream s's
        table is ``v/g/d[offs[s]:offs[s+1]]`` -- offsets may be absolute into
        a larger array (a slice of another set's export) -- and its pending
        values ``pv[poffs[s]:poffs[s+1]]``; header arrays have S entries."""
        with self._ctx():
            self._check(self._lib.gk_import(self._h, _ptr(offs), _ptr(v), _ptr(g), _ptr(d), _ptr(poffs), _ptr(pv),
                                            _ptr(n), _ptr(mn), _ptr(mx), _ptr(sm), _ptr(av), self._sp()))

    def export_sizes(self):
        """Device tensors (table sizes int32[S], pending counts int32[S]) -- no host sync."""
        S = max(self.num_streams, 1)
        e = torch.empty(S, dtype=torch.int32, device=self.device)
        p = torch.empty(S, dtype=torch.int32, device=self.device)
        with self._ctx():
            self._check(self._lib.gk_export_sizes(self._h, _ptr(e), self._sp()))
            self._check(self._lib.gk_export_pending_sizes(self._h, _ptr(p), self._sp()))
        return e[:self.num_streams], p[:self.num_streams]

    def export_into(self, offs, v, g, d, poffs, pv):
        """Tables / pending values into caller buffers at the given offsets (device, no host sync)."""
        with self._ctx():
            self._check(self._lib.gk_export(self._h, _ptr(offs), _ptr(v), _ptr(g), _ptr(d), self._sp()))
            self._check(self._lib.gk_export_pending(self._h, _ptr(poffs), _ptr(pv), self._sp()))

    # ------------------------------------------------------------------ merge
    def merge_from(self, others):
        """Left fold ``self.merge(others[0]); self.merge(others[1]); ...``
        stream by stream (gk:111-154).  Each source is flushed (mutated)."""
        if isinstance(others, StreamSet):
            others = [others]
        for o in others:
            if o.eps != self.eps:
                from .gkarray import UnequalEpsilonException
                raise UnequalEpsilonException("Cannot merge two GKArrays with different epsilon values")
        for o in others:
            if o.is_cpu != self.is_cpu:
                raise ValueError("cannot merge a CPU-engine set with a GPU-engine set (export / import the state)")
        arr = (ctypes.c_void_p * max(len(others), 1))(*[o._h for o in others])
        with self._ctx():
            rc = self._lib.gk_merge(self._h, arr, len(others), self._sp())
        if rc == L.GK_E_EPS_MISMATCH:
            from .gkarray import UnequalEpsilonException
            raise UnequalEpsilonException("Cannot merge two GKArrays with different epsilon values")
        self._check(rc)

    # ---------------------------------------------------------------- roll-up
    def rollup_from(self, src, group_offsets, members):
        """Group-by roll-up (``gk_rollup``): for every stream j of this set, in
        order of k, ``self[j].merge(src[members[k]])`` for k in
        ``group_offsets[j] .. group_offsets[j+1]-1`` (gk:111-154).

        ``src`` is another set with the same eps (any stream count);
        ``group_offsets`` is int64[num_streams+1] starting at 0, non-decreasing;
        ``members`` are indices into ``src``, each at most once.  This set keeps
        its state from before the call, so a roll-up can be continued by a
        later call; a stream with an empty group is not touched.  Members are
        flushed (mutated) as the reference flushes ``other``; every other
        stream of ``src`` is left as it is."""
        if not isinstance(src, StreamSet):
            raise ValueError("src must be a StreamSet")
        if src.eps != self.eps:
            from .gkarray import UnequalEpsilonException
            raise UnequalEpsilonException("Cannot merge two GKArrays with different epsilon values")
        if src.is_cpu != self.is_cpu:
            raise ValueError("cannot roll up a CPU-engine set into a GPU-engine set or back "
                             "(export / import the state)")
        if not self.is_cpu and src.device != self.device:
            raise ValueError("both sets must live on one device")
        go = self._dev(group_offsets, torch.int64)
        mem = self._dev(members, torch.int64)
        if go.dim() != 1 or go.numel() != self.num_streams + 1:
            raise ValueError("group_offsets must have num_streams+1 entries")
        if mem.dim() != 1:
            raise ValueError("members must be one-dimensional")
        if mem.numel() == 0:
            mem = torch.zeros(1, dtype=torch.int64, device=self.device)
        with self._ctx():
            rc = self._lib.gk_rollup(self._h, src._h, _ptr(go), _ptr(mem), self._sp())
        if rc == L.GK_E_EPS_MISMATCH:
            from .gkarray import UnequalEpsilonException
            raise UnequalEpsilonException("Cannot merge two GKArrays with different epsilon values")
        self._check(rc)

    def rollup_by_key(self, src, keys):
        """Roll-up by destination key: ``keys`` is int64[src.num_streams],
        ``keys[s]`` the stream of this set that source stream s is merged into,
        -1 for "not rolled up".  The members of a group are taken in ascending
        source index."""
        if not isinstance(src, StreamSet):
            raise ValueError("src must be a StreamSet")
        k = self._dev(keys, torch.int64)
        if k.dim() != 1 or k.numel() != src.num_streams:
            raise ValueError("keys must have one entry per source stream")
        G = self.num_streams
        if k.numel() and (int(k.max().item()) >= G or int(k.min().item()) < -1):
            raise ValueError("keys must lie in [-1, num_streams)")
        # CSR by a stable sort: equal keys keep ascending source index
        sk, order = torch.sort(k, stable=True)
        members = order[sk >= 0]
        counts = torch.bincount(sk[sk >= 0], minlength=G) if G else torch.zeros(0, dtype=torch.int64, device=k.device)
        go = torch.zeros(G + 1, dtype=torch.int64, device=k.device)
        if G:
            go[1:] = torch.cumsum(counts, 0)
        self.rollup_from(src, go, members)

    # ---- packed state (gk_pack_bytes / gk_pack / gk_fold_packed) -------------
    def pack_bytes(self):
        """Size of this set's packed state (one contiguous buffer: header
        words, tables, pending values; layout in csrc/gk_pack.h)."""
        b = ctypes.c_int64(0)
        with self._ctx():
            self._check(self._lib.gk_pack_bytes(self._h, ctypes.byref(b), self._sp()))
        return b.value

    def pack(self, buf=None):
        """The packed state as a uint8 tensor on the set's device (host for
        the CPU engine).  ``buf``: a uint8 tensor of at least pack_bytes()
        bytes to write into (e.g. an equal-sized all-gather slot)."""
        if buf is None:
            buf = torch.empty(self.pack_bytes(), dtype=torch.uint8, device=self.device)
        if buf.dtype != torch.uint8 or not buf.is_contiguous():
            raise ValueError("buf must be a contiguous uint8 tensor")
        with self._ctx():
            self._check(self._lib.gk_pack(self._h, _ptr(buf), buf.numel(), self._sp()))
        return buf

    def fold_packed(self, bufs):
        """self := bufs[0], then self.merge(bufs[r]) for r = 1.. (gk:111-154,
        every stream): the rank-ordered fold of packed states."""
        bufs = [b if b.device == torch.device(self.device) else b.to(self.device) for b in bufs]
        arr = (ctypes.c_void_p * max(len(bufs), 1))(*[b.data_ptr() for b in bufs])
        with self._ctx():
            rc = self._lib.gk_fold_packed(self._h, arr, len(bufs), self._sp())
        if rc == L.GK_E_EPS_MISMATCH:
            from .gkarray import UnequalEpsilonException
            raise UnequalEpsilonException("Cannot merge two GKArrays with different epsilon values")
        self._check(rc)

    # ---- stream transfer (gk_pack_select / gk_unpack_select) ----------------
    def pack_select_bytes(self, ids):
        """Size of ``pack_select(ids)``."""
        i = self._select_ids(ids)
        K = i.numel()
        b = ctypes.c_int64(0)
        with self._ctx():
            self._check(self._lib.gk_pack_select_bytes(self._h, _ptr(i) if K else None, K, ctypes.byref(b),
                                                       self._sp()))
        self._inflight = None  # (the call synchronised)
        return b.value

    def pack_select(self, ids, buf=None):
        """The complete state of the listed streams -- tables, pending values,
        n / min / max / sum / avg, nothing flushed -- as one packed state of
        ``len(ids)`` streams (``gk_pack_select``; layout in csrc/gk_pack.h),
        row k for ``ids[k]``: a uint8 tensor on the set's device.  The set is
        not changed.  Ids may repeat and come in any order.  ``buf``: a
        contiguous uint8 tensor of at least ``pack_select_bytes(ids)`` bytes on
        the set's device to write into."""
        i = self._select_ids(ids)
        K = i.numel()
        if buf is None:
            buf = torch.empty(self.pack_select_bytes(i), dtype=torch.uint8, device=self.device)
        if buf.dtype != torch.uint8 or not buf.is_contiguous() or buf.device != self.device:
            raise ValueError("buf must be a contiguous uint8 tensor on %s" % self.device)
        with self._ctx():
            self._check(self._lib.gk_pack_select(self._h, _ptr(i) if K else None, K, _ptr(buf), buf.numel(),
                                                 self._sp()))
        self._inflight = None
        return buf

    def unpack_select(self, ids, buf):
        """``self[ids[k]] := stream k of buf`` (``gk_unpack_select``): the
        complete state of each listed stream is replaced by the packed one, so
        that it continues exactly as the packed stream would have.  ``buf`` is
        a packed state of ``len(ids)`` streams (``pack_select`` / ``pack``; it
        is moved to the set's device if it lives elsewhere).  Every refusal --
        an id outside the set or listed twice, a stream count or eps that does
        not match, a malformed buffer -- comes before anything is changed."""
        i = self._select_ids(ids)
        K = i.numel()
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.dim() != 1:
            raise ValueError("buf must be a one-dimensional uint8 tensor")
        if buf.device != self.device:
            buf = buf.to(self.device)
        buf = buf.contiguous()
        if buf.numel() < 64:
            raise ValueError("buf is shorter than a packed state's header")
        with self._ctx():
            rc = self._lib.gk_unpack_select(self._h, _ptr(i) if K else None, K, _ptr(buf), self._sp())
        self._inflight = None
        if rc == L.GK_E_EPS_MISMATCH:
            from .gkarray import UnequalEpsilonException
            raise UnequalEpsilonException(L.last_error(self._lib))
        self._check(rc)

    def take(self, ids, device=None):
        """A new set of ``len(ids)`` streams and the same eps holding copies of
        the listed streams (``pack_select`` + ``fold_packed``); this set is not
        changed.  ``device``: where the new set lives -- this set's device by
        default, another GPU, or ``"cpu"`` for the host engine."""
        i = self._select_ids(ids)
        buf = self.pack_select(i)
        out = StreamSet(i.numel(), self.eps, device=self.device if device is None else device)
        if buf.device != out.device:
            buf = buf.to(out.device)
        out.fold_packed([buf])
        return out

    def put(self, ids, other):
        """``self[ids[k]] := other[k]`` for every k: ``other`` is a set of
        ``len(ids)`` streams (either engine, any device) and is not changed
        (``other.pack()`` + ``unpack_select``)."""
        if not isinstance(other, StreamSet):
            raise ValueError("other must be a StreamSet")
        i = self._select_ids(ids)
        if other.num_streams != i.numel():
            raise ValueError("other holds %d streams, %d ids are listed" % (other.num_streams, i.numel()))
        self.unpack_select(i, other.pack())

    def resized(self, num_streams):
        """A new set of ``num_streams`` streams on this set's device: streams
        [0, min(S, num_streams)) are copies of this set's, the rest are empty;
        this set is not changed.  How a keyed-ingest user grows a set."""
        num_streams = int(num_streams)
        if num_streams < 0:
            raise ValueError("num_streams must be >= 0")
        keep = torch.arange(min(self.num_streams, num_streams), dtype=torch.int32)
        out = StreamSet(num_streams, self.eps, device=self.device)
        if keep.numel():
            out.unpack_select(keep, self.pack_select(keep))
        return out

    def merge_compress(self, v=None, g=None, d=None, eoffs=None):
        """``merge_compress(entries)`` (gk:63-109) on every stream; stream s
        merges records [eoffs[s], eoffs[s+1]) (sorted by value).  With no
        records this is the unconditional ``merge_compress()``."""
        S = self.num_streams
        if eoffs is None:
            eoffs = torch.zeros(S + 1, dtype=torch.int64)
            v = torch.zeros(1, dtype=torch.float64)
            g = torch.zeros(1, dtype=torch.int32)
            d = torch.zeros(1, dtype=torch.int32)
        t_o = self._dev(eoffs, torch.int64)
        t_v = self._dev(v, torch.float64)
        t_g = self._dev(g, torch.int32)
        t_d = self._dev(d, torch.int32)
        if t_v.numel() == 0:
            t_v = torch.zeros(1, dtype=torch.float64, device=self.device)
            t_g = torch.zeros(1, dtype=torch.int32, device=self.device)
            t_d = torch.zeros(1, dtype=torch.int32, device=self.device)
        with self._ctx():
            self._check(self._lib.gk_merge_compress(self._h, _ptr(t_v), _ptr(t_g), _ptr(t_d),
                                                _ptr(t_o), self._sp()))

    # ------------------------------------------------------------------ timing
    def timing(self, on=True, stats=False):
        """HIP events around the ingest launch (and, stats=True, around the
        call's stats fork: two more event markers per call)."""
        self._check(self._lib.gk_timing_enable(self._h, (1 | (2 if stats else 0)) if on else 0))

    def read_timing(self):
        f = ctypes.c_double()
        s = ctypes.c_double()
        n = ctypes.c_int64()
        self._check(self._lib.gk_timing_read(self._h, ctypes.byref(f), ctypes.byref(s), ctypes.byref(n)))
        return f.value, s.value, n.value
