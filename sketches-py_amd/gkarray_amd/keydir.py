"""KeyDirectory and KeyedStreamSet: the dict in "a dict of GKArray objects".

``KeyDirectory`` maps int64 keys to the dense int32 stream ids every
``StreamSet`` call takes, assigning ids to keys it has not seen, a batch per
call (``gk_dir_*`` of ``include/gk_capi.h``: a hash table on the device).
``KeyedStreamSet`` puts one directory in front of one ``StreamSet``: samples
go in as (key, value), answers come out by key, and nothing runs per sample
on the host.
"""
import contextlib
import ctypes
import os

import numpy as np
import torch

from . import _lib as L
from .streamset import StreamSet, _ptr, _stream_ptr, peek

__all__ = ["KeyDirectory", "KeyedStreamSet", "NO_KEY"]

NO_KEY = -2 ** 63  # GK_DIR_NONE: "no key", always answers id -1


class KeyDirectory:
    """At most ``capacity`` int64 keys, each bound to an id below ``bound``:
    a new key takes the smallest id a removed key has left free and, when
    there is none, ``bound`` itself, which then grows by one.  Ids depend on
    the directory's contents and the order of first occurrence alone; the GPU
    and the host engine give the same ones.  ``len(dir)`` counts the keys held."""

    def __init__(self, capacity, device=None):
        """``device`` as ``StreamSet``: a cuda (HIP) device, the default, or
        ``"cpu"`` for the host engine; no implicit fallback."""
        if device is not None and torch.device(device).type == "cpu":
            self._lib = L.load_cpu()
            device = torch.device("cpu")
            dev_index = 0
        else:
            if not torch.cuda.is_available():
                raise L.GKBackendError(L.GK_E_HIP, "no GPU visible (the host engine is KeyDirectory(..., device='cpu'))")
            self._lib = L.load()
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            if device.type != "cuda":
                raise ValueError("KeyDirectory needs a cuda (HIP) device or 'cpu', got %s" % device)
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            dev_index = device.index
        self.device = device
        self.last_new = 0
        self.last_removed = 0
        h = ctypes.c_void_p()
        with self._ctx():
            self._check(self._lib.gk_dir_create(int(capacity), dev_index, ctypes.byref(h)))
        self._h = h

    @property
    def is_cpu(self):
        return self.device.type == "cpu"

    def _ctx(self):
        if self.device.type == "cpu" or torch.cuda.current_device() == self.device.index:
            return contextlib.nullcontext()
        return torch.cuda.device(self.device)

    def _check(self, rc):
        return L.check(rc, self._lib)

    def _sp(self):
        return _stream_ptr(self.device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gk_dir_destroy(self._h)
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
    def capacity(self):
        return self._lib.gk_dir_capacity(self._h)

    def __len__(self):
        return self._lib.gk_dir_size(self._h)

    @property
    def bound(self):
        """One past the largest id handed out (``gk_dir_bound``):
        ``len(self)`` plus the number of free ids."""
        return self._lib.gk_dir_bound(self._h)

    def _keys(self, keys):
        """A one-dimensional int64 key tensor on the directory's device."""
        k = torch.as_tensor(keys)
        if k.dim() != 1:
            raise ValueError("keys must be one-dimensional")
        if k.dtype != torch.int64:
            if k.dtype.is_floating_point or k.dtype == torch.bool:
                raise ValueError("keys must be int64, got %s" % k.dtype)
            k = k.to(torch.int64)
        if k.numel() > 2 ** 31 - 1:
            raise ValueError("at most 2^31-1 keys per call")
        if k.device != self.device:
            k = k.to(self.device)
        return k.contiguous()

    def assign(self, keys):
        """``gk_dir_assign``: the ids of ``keys`` (int32 tensor); new keys, in
        order of first occurrence, take the free ids in ascending order and
        then ``bound``, ``bound + 1``, ...; ``NO_KEY`` answers -1.  ``self.last_new`` is the number of keys added.  A batch
        whose new keys do not fit raises ``GKBackendError`` (GK_E_OVERFLOW) and
        leaves the directory exactly as it was."""
        k = self._keys(keys)
        n = k.numel()
        out = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        new = ctypes.c_int64(0)
        with self._ctx():
            self._check(self._lib.gk_dir_assign(self._h, _ptr(k) if n else None, n, _ptr(out) if n else None,
                                                ctypes.byref(new), self._sp()))
        self.last_new = new.value
        return out[:n]

    def remove(self, keys):
        """``gk_dir_remove``: the ids the listed keys held (int32 tensor), -1
        for a key the directory does not hold, for ``NO_KEY`` and for every
        occurrence of a key after its first.  The ids are free for later new
        keys; ``self.last_removed`` is the number of keys removed.  No set is
        touched: reset the streams of the returned ids before new keys
        inherit them (``KeyedStreamSet.remove`` does)."""
        k = self._keys(keys)
        n = k.numel()
        out = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        gone = ctypes.c_int64(0)
        with self._ctx():
            self._check(self._lib.gk_dir_remove(self._h, _ptr(k) if n else None, n, _ptr(out) if n else None,
                                                ctypes.byref(gone), self._sp()))
        self.last_removed = gone.value
        return out[:n]

    def lookup(self, keys):
        """``gk_dir_lookup``: the ids of ``keys``, -1 for a key the directory
        does not hold (and for ``NO_KEY``).  Changes nothing."""
        k = self._keys(keys)
        n = k.numel()
        out = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        with self._ctx():
            self._check(self._lib.gk_dir_lookup(self._h, _ptr(k) if n else None, n, _ptr(out) if n else None,
                                                self._sp()))
        return out[:n]

    def keys(self):
        """The inverse array: int64 tensor of length ``bound``, ``keys()[id]``
        holds ``id``; ``NO_KEY`` at free ids."""
        n = self.bound
        out = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        with self._ctx():
            self._check(self._lib.gk_dir_keys(self._h, _ptr(out), self._sp()))
        return out[:n]

    def import_keys(self, keys, sparse=False):
        """``gk_dir_import``: the contents become ``keys[i] -> i``.  More keys
        than ``capacity``, a ``NO_KEY`` entry or a key listed twice raise
        ``GKBackendError`` (GK_E_ARG) and leave the old contents in place.
        ``sparse=True`` (``gk_dir_import_sparse``): a ``NO_KEY`` entry is a
        free id instead, so that ``keys()`` of a directory with free ids
        restores it."""
        k = self._keys(keys)
        n = k.numel()
        call = self._lib.gk_dir_import_sparse if sparse else self._lib.gk_dir_import
        with self._ctx():
            self._check(call(self._h, _ptr(k) if n else None, n, self._sp()))

    def resized(self, capacity):
        """A new directory of ``capacity`` keys on this device with the same
        bindings and free ids; this one is not changed.  A capacity below
        ``bound`` is refused."""
        out = KeyDirectory(capacity, device=self.device)
        try:
            out.import_keys(self.keys(), sparse=True)
        except Exception:
            out.close()
            raise
        return out


class KeyedStreamSet:
    """``sketches = {}; sketches.setdefault(key, GKArray(eps)).add(value)`` for
    whole batches: a ``KeyDirectory`` in front of a ``StreamSet``.  Key ``k``
    owns stream ``directory.lookup([k])`` of ``streams``; both halves grow by
    doubling when a batch brings more new keys than fit.  ``remove`` is
    ``del sketches[k]``: the stream is reset and its id goes to the next new
    key, so keys that come and go at a steady count never grow either half.
    Removal resets the stream but, on the GPU, the stream keeps its capacity
    class: the key that inherits the id inherits the class and its slot, until
    ``compact()`` puts every stream back into the smallest class that holds it
    and returns the arena memory.  Nothing compacts implicitly."""

    def __init__(self, eps, capacity=1024, device=None, max_streams=None):
        capacity = int(capacity)
        if max_streams is not None:
            max_streams = int(max_streams)
            if max_streams < 1:
                raise ValueError("max_streams must be >= 1")
            capacity = min(capacity, max_streams)
        self.eps = eps
        self.max_streams = max_streams
        self.directory = KeyDirectory(capacity, device=device)
        self.streams = StreamSet(capacity, eps, device=self.directory.device)
        self.device = self.directory.device

    def close(self):
        self.directory.close()
        self.streams.close()

    # ---------------------------------------------------------------- ingest
    def _assign_growing(self, k):
        """ids of ``k``, after doubling both halves as often as the batch needs.
        The grown directory is tried first, so that a batch ``max_streams``
        refuses leaves this object as it was."""
        d = self.directory
        while True:
            try:
                ids = d.assign(k)
                break
            except L.GKBackendError as e:
                if e.code != L.GK_E_OVERFLOW:
                    raise
            cap = d.capacity
            if self.max_streams is not None and cap >= self.max_streams:
                if d is not self.directory:
                    d.close()
                raise L.GKBackendError(L.GK_E_OVERFLOW, "the batch's new keys would pass max_streams=%d"
                                       % self.max_streams)
            new_cap = 2 * cap if self.max_streams is None else min(2 * cap, self.max_streams)
            grown = self.directory.resized(new_cap)
            if d is not self.directory:
                d.close()
            d = grown
        if d is not self.directory:
            streams = self.streams.resized(d.capacity)
            self.directory.close()
            self.streams.close()
            self.directory, self.streams = d, streams
        return ids

    def add(self, keys, values, quantiles=None, single=False):
        """``for i: sketches[keys[i]].add(values[i])`` with new keys bound on
        the way (``gk_dir_assign`` + ``gk_ingest_keyed``); ``NO_KEY`` samples
        are skipped.  With ``quantiles=qs``: ``quantiles(qs)`` of every key
        after the batch, float64 [directory.bound, len(qs)], row ``id`` for
        ``keys()[id]``; the row of a free id (``NO_KEY``) holds the answers of
        an empty stream.  Raises ``GKBackendError`` (GK_E_OVERFLOW), with
        nothing changed, when the new keys would pass ``max_streams``."""
        k = self.directory._keys(keys)
        v = torch.as_tensor(values)
        if v.dim() != 1 or v.numel() != k.numel():
            raise ValueError("keys and values must be one-dimensional and of one length")
        ids = self._assign_growing(k)
        out = self.streams.ingest_keyed(ids, v, quantiles=quantiles, single=single)
        return None if out is None else out[:self.directory.bound]

    # ----------------------------------------------------------------- query
    def _ids(self, keys):
        k = self.directory._keys(keys)
        ids = self.directory.lookup(k)
        if ids.numel():
            bad = (ids < 0).nonzero()
            if bad.numel():
                raise KeyError(int(k[int(bad[0, 0])].item()))
        return ids

    def quantiles(self, keys, qs, single=False):
        """``sketches[keys[j]].quantiles(qs)`` for every j: float64
        [len(keys), len(qs)].  ``KeyError`` names the first unknown key."""
        return self.streams.quantiles_select(self._ids(keys), qs, single=single)

    def ranks(self, keys, xs):
        """``(lo, hi)`` of ``StreamSet.ranks_select`` for the keys' streams."""
        return self.streams.ranks_select(self._ids(keys), xs)

    def cdf(self, keys, xs):
        return self.streams.cdf_select(self._ids(keys), xs)

    def _sample_args(self, keys, values):
        """(ids, values) of per-sample queries: ``directory.lookup``, never an
        assignment -- an unknown key and ``NO_KEY`` are id -1, "no stream"."""
        k = self.directory._keys(keys)
        v = values if isinstance(values, torch.Tensor) else torch.as_tensor(values, dtype=torch.float64)
        if v.dim() != 1 or v.numel() != k.numel():
            raise ValueError("keys and values must be one-dimensional and of one length")
        return self.directory.lookup(k), v

    def ranks_keyed(self, keys, values):
        """``(lo, hi)`` of ``StreamSet.ranks_keyed``: row i bounds the count of
        values <= ``values[i]`` in the sketch of ``keys[i]``.  No key is bound:
        an unknown key or ``NO_KEY`` gives (0, 0), the answer of an empty
        sketch, never a ``KeyError``."""
        ids, v = self._sample_args(keys, values)
        lo, hi, _ = self.streams.ranks_keyed(ids, v)
        return lo, hi

    def score(self, keys, values):
        """Where each sample sits in the distribution of its own key: float64
        [len(keys)], ``StreamSet.cdf_keyed`` -- ``(lo + hi) / (2 n)``, NaN for
        an unknown key, ``NO_KEY`` or an empty sketch.  Scoring a batch against
        the history BEFORE it joins it is ``score_add(keys, v)``, one call
        with the answers of ``s = k.score(keys, v); k.add(keys, v)``.  Like
        ``quantiles``, ``score`` flushes the pending values of the streams it
        touches."""
        ids, v = self._sample_args(keys, values)
        return self.streams.cdf_keyed(ids, v)

    def score_add(self, keys, values, quantiles=None, single=False):
        """``s = score(keys, values); add(keys, values)`` in one call
        (``gk_dir_assign`` + ``gk_rank_ingest_keyed``): every sample is scored
        against its key's history before any value of the batch joins it, then
        the batch is added.  A key that is new in this batch is bound first;
        its history is empty, so every one of its samples in the batch scores
        NaN.  ``NO_KEY`` samples score NaN and are skipped.  A NaN value on a
        sample with a key raises ``GKBackendError`` (GK_E_ARG); the new keys of
        that batch stay bound, with empty sketches.  Returns the scores, float64
        [len(keys)], or ``(scores, q)`` with ``quantiles`` -- ``q`` as ``add``
        returns it.  The ``max_streams`` refusal leaves the object unchanged,
        as in ``add``."""
        k = self.directory._keys(keys)
        v = values if isinstance(values, torch.Tensor) else torch.as_tensor(values, dtype=torch.float64)
        if v.dim() != 1 or v.numel() != k.numel():
            raise ValueError("keys and values must be one-dimensional and of one length")
        ids = self._assign_growing(k)
        out = self.streams.score_ingest_keyed(ids, v, quantiles=quantiles, single=single)
        return out if quantiles is None else (out[0], out[1][:self.directory.bound])

    def stats(self, keys):
        return self.streams.stats_select(self._ids(keys))

    def flush(self, keys):
        self.streams.flush_select(self._ids(keys))

    def reset(self, keys):
        """``sketches[k] = GKArray(eps)`` for the listed keys; each keeps its binding."""
        self.streams.reset_select(self._ids(keys))

    # --------------------------------------------------------------- removal
    def _release(self, ids):
        """Streams ``ids`` (no -1, no repeats) back to ``GKArray(eps)``, first:
        a sticky error of the set surfaces before the directory changes."""
        if ids.numel():
            self.streams.reset_select(ids)

    def remove(self, keys):
        """``for k in keys: del sketches[k]``: the keys leave the directory,
        their streams are reset and their ids are free for new keys.
        ``KeyError`` names the first unknown key, with nothing changed; a key
        listed twice is removed once.  A reset stream keeps its capacity class
        (GPU engine) until ``compact()``."""
        k = self.directory._keys(keys)
        self._release(torch.unique(self._ids(k)))
        self.directory.remove(k)

    def compact(self):
        """``streams.compact()``: after keys with large tables have gone, their
        streams -- and the keys that inherited them -- leave the large capacity
        classes and the memory goes back.  ``{"demoted": .., "bytes_freed": ..}``."""
        return self.streams.compact()

    def discard(self, keys):
        """``remove`` that ignores keys the object does not hold (and ``NO_KEY``)."""
        k = self.directory._keys(keys)
        ids = self.directory.lookup(k)
        self._release(torch.unique(ids[ids >= 0]))
        self.directory.remove(k)

    def pop(self, keys, device=None):
        """``[sketches.pop(k) for k in keys]``: a new ``StreamSet`` whose stream
        j is the complete state of ``keys[j]`` (``streams.take``; ``device`` as
        there: this device, another GPU or ``"cpu"``), after which the keys
        are removed.  Eviction in one call.  ``KeyError`` as ``remove``."""
        k = self.directory._keys(keys)
        ids = self._ids(k)
        out = self.streams.take(ids, device=device)
        self._release(torch.unique(ids))
        self.directory.remove(k)
        return out

    def keys(self):
        """``directory.keys()``: length ``directory.bound``, ``NO_KEY`` at free ids."""
        return self.directory.keys()

    def __len__(self):
        return len(self.directory)

    def __contains__(self, key):
        return int(self.directory.lookup([int(key)])[0].item()) >= 0

    # ----------------------------------------------------------------- files
    def save(self, path):
        """The streams as a GKSTATE file at ``path`` and the keys beside it as
        ``path + ".keys.npy"`` (int64, ``keys()``: ``NO_KEY`` at free ids)."""
        self.streams.save(path)
        np.save(os.fspath(path) + ".keys.npy", self.keys().cpu().numpy())

    @classmethod
    def load(cls, path, device=None, max_streams=None):
        """The object ``save(path)`` wrote: same keys, ids, free ids and stream states."""
        cpu = device is not None and torch.device(device).type == "cpu"
        eps, S = peek(path, cpu=cpu)
        keys = torch.from_numpy(np.load(os.fspath(path) + ".keys.npy").astype(np.int64))
        if keys.numel() > S:
            raise ValueError("%d keys for %d saved streams" % (keys.numel(), S))
        out = cls(eps, capacity=max(S, 1), device=device, max_streams=max_streams)
        if out.directory.capacity != S:
            raise ValueError("%d saved streams do not fit max_streams=%s" % (S, max_streams))
        out.streams.load_state(path)
        out.directory.import_keys(keys, sparse=True)
        return out
