"""The train step's side streams.

Second stream (`suffix_stream`, `handoff`): the action expert's kernels (1,600 rows: poorly filled grids, launch-latency bound) are
issued on it and run under the prefix stream's GEMMs; the two meet before and after each layer's attention (lap_amd/joint_layers.py;
`LAP_DUAL_STREAM=0`: everything on one stream).

Third stream (`OffPathStream`, held as `model.wg`): nothing in the backward waits for a weight / bias gradient except the optimizer, so
the prefix stream's and SigLIP's are issued there: the data-gradient chain (the critical path) keeps the compute stream, and the
weight-gradient GEMMs fill the CUs its poorly filled last rounds leave idle.  The compute stream joins before it updates a dy in
place and before a unit's gradients are declared complete (`LAP_WGRAD_STREAM=0`: inline).
"""
from __future__ import annotations

import contextlib

import torch


def suffix_stream(model, *tensors):
    """The second HIP stream for the suffix (action-expert) side of a joint layer loop, or None when both streams of
    activations go down the current one (one of them absent, CPU tensors, stream capture, LAP_DUAL_STREAM=0).  It starts
    behind everything the current stream has been given so far; `tensors` are marked as used on it."""
    if not model.dual_stream or any(t is None or not t.is_cuda for t in tensors) or torch.cuda.is_current_stream_capturing():
        return None
    if model.sfx is None:
        model.sfx = torch.cuda.Stream(model.device, priority=-1)   # short kernels: never let them queue behind a full grid
    model.sfx.wait_stream(torch.cuda.current_stream())
    for t in tensors:
        t.record_stream(model.sfx)
    return model.sfx


def handoff(src, dst, *tensors):
    """`dst` waits for what `src` has been given so far; `tensors` (allocated on src) are about to be used on dst."""
    if src is not None and dst is not None:
        dst.wait_stream(src)
        for t in tensors:
            if t is not None:
                t.record_stream(dst)


class OffPathStream:
    """The weight-gradient stream of one model: open between `begin()` and `end()` of a backward pass, on the stream that began it."""

    def __init__(self, device):
        self.device = device
        self.stream = None      # the HIP stream (created on first use)
        self._open = None       # ... while a backward pass has it open
        self._main = None       # the compute stream of that pass
        self._dirty = False     # work issued since the last full join
        self._ev: dict = {}     # data_ptr of a dy -> events behind its off-path readers

    def begin(self, enabled):
        """Start of a backward pass on the current stream: weight gradients go off the path from here on."""
        if enabled and self.device.type == "cuda" and not torch.cuda.is_current_stream_capturing():
            if self.stream is None:
                self.stream = torch.cuda.Stream(self.device)
            self._open, self._main, self._dirty = self.stream, torch.cuda.current_stream(), False

    def end(self):
        self.join()
        self._open = None

    @contextlib.contextmanager
    def run(self, *tensors):
        """Issue the body on the third stream, behind the compute stream; `tensors[0]` is the dy the path may rewrite (`join`)."""
        wg = self._open
        cur = torch.cuda.current_stream()
        if wg is None or cur != self._main:
            yield
            return
        wg.wait_stream(self._main)
        for t in tensors:
            t.record_stream(wg)
        with torch.cuda.stream(wg):
            yield
        ev = torch.cuda.Event()
        ev.record(wg)
        self._ev.setdefault(tensors[0].data_ptr(), []).append(ev)     # keyed by dy: the tensor the path may rewrite
        self._dirty = True

    def pending(self):
        """The third stream if gradients issued from the current stream may still be in flight on it, else None."""
        if self._open is not None and self._dirty and torch.cuda.current_stream() == self._main:
            return self._open
        return None

    def join(self, dy=None):
        """The compute stream waits for the off-path readers of `dy` (about to be updated in place), or for all of them."""
        if self.pending() is None:
            return
        if dy is not None:
            for ev in self._ev.pop(dy.data_ptr(), ()):
                self._main.wait_event(ev)
        else:
            self._main.wait_stream(self._open)
            self._ev.clear()
            self._dirty = False


def unit_done(model, name, sfx=None):
    """comm.grads_ready for a unit whose gradients may still be in flight on the second (`sfx`) or third stream: the
    communication / optimizer stream waits for those too, the compute stream does not."""
    also = [sfx] if sfx is not None else []
    wg = model.wg.pending()
    if wg is not None:
        also.append(wg)
    model.comm.grads_ready(name, also=also or None)
