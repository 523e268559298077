"""One store for the tensors that the serving paths derive from the parameters: merged LoRA weights, the fused decoder's fp8
weights, packed weight images, adaRMS modulations.

A captured graph (serve.GraphedSampler, serve.GraphedTokenDecoder) holds the ADDRESSES of these tensors.  So a record is built
once, rebuilt IN PLACE whenever the parameter version has moved, never rebuilt while a stream is being captured, and `refresh()`
reaches every record there is.  The store checks the first rule after every rebuild instead of trusting each builder with it.

A record is `[version, value, unit, build]` under a key `(kind, name...)`.  `value` is a tensor or a (nested) tuple / list of
tensors.  `unit` is what `wait` is given before the source weights are read (None: the builder waits itself, or nothing has
to).  `build(old)` returns the value; with `old` not None it writes into old's storage and returns tensors at the same addresses.
A record is inserted when its first `build` has returned, so whatever that build looked up (the merged weight that fp8 codes are
quantised from) stands ahead of it and `refresh()`, which walks in insertion order, rebuilds sources before their dependents.
"""
from __future__ import annotations

import torch

STALE_IN_CAPTURE = "serving caches are stale inside a stream capture: call refresh_serve_caches() first"


def _tensors(value):
    return [value] if isinstance(value, torch.Tensor) else [t for v in value for t in _tensors(v)]


class ServeCache:
    def __init__(self, params, device, wait, capturing=None):
        """params: whatever carries the parameter `version`; wait(unit); capturing(): is a stream capture in progress."""
        self._params, self._wait = params, wait
        device = torch.device(device)
        self._capturing = capturing or (lambda: device.type == "cuda" and torch.cuda.is_current_stream_capturing())
        self._recs: dict = {}

    def get(self, key, unit, build):
        rec = self._recs.get(key)
        if rec is not None and rec[0] == self._params.version:
            return rec[1]
        return self._build(key, rec, unit, build)

    def _build(self, key, rec, unit, build):
        if self._capturing():
            raise RuntimeError(STALE_IN_CAPTURE)
        if unit is not None:
            self._wait(unit)
        version = self._params.version
        if rec is None:
            value = build(None)
            self._recs[key] = [version, value, unit, build]
            return value
        ptrs = [t.data_ptr() for t in _tensors(rec[1])]
        value = build(rec[1])
        if [t.data_ptr() for t in _tensors(value)] != ptrs:
            raise RuntimeError(f"serving cache {key!r} was rebuilt at another address: a captured graph would read the old one")
        rec[0], rec[1] = version, value
        return value

    def refresh(self):
        """Bring every record there is to the current parameter version, in insertion order; creates none."""
        for key, rec in list(self._recs.items()):
            if rec[0] != self._params.version:
                self._build(key, rec, rec[2], rec[3])

    def entries(self, kind=None) -> dict:
        """{name: value} of the records `(kind, name...)` (name: the one further key element, or the tuple of them); kind None:
        {key: value} of all records."""
        if kind is None:
            return {k: r[1] for k, r in self._recs.items()}
        return {(k[1] if len(k) == 2 else k[1:]): r[1] for k, r in self._recs.items() if k[0] == kind}

    def stale(self) -> list:
        """Keys of the records that are not at the current parameter version."""
        return [k for k, r in self._recs.items() if r[0] != self._params.version]
