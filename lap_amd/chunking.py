"""Real-time chunking by inpainting, the host side (numpy only; not in the reference, whose sampler has no such option).

A client that executes chunk n while chunk n + 1 is computed needs the head of chunk n + 1 to EQUAL the actions it has already
committed to: `shift_chunk` turns the previous chunk into the `(known, mask)` pair that `LAP.sample_actions(inpaint=...)` takes,
and `RealTimeChunker` keeps that previous chunk.  Everything here is in MODEL space (normalised, padded to action_dim): the
chunk is kept as the sampler returned it, before unnormalisation and the output transforms, so no inverse transform is needed.

Shifting a previous chunk is meaningful only when the action representation does not depend on the new observation's frame
(absolute targets, or deltas against a fixed frame): actions expressed relative to the state at the START of their own chunk
mean something else once that state has moved, and must be re-expressed by the caller before they are passed as `known`.
"""
from __future__ import annotations

import numpy as np


def shift_chunk(prev, executed: int, freeze: int):
    """The inpainting inputs of the next chunk from the previous one.

    prev [S, ad] (or [B, S, ad]): the previous chunk in model space; `executed` of its rows will have been executed when the new
    chunk starts, and the `freeze` rows after them are committed.  Returns (known f32 like prev, mask uint8 [S] or [B, S]) with
    known[h] = prev[h + executed] where that row exists, else 0, and mask[h] = h < freeze.  Requires 0 <= executed <= S and
    0 <= freeze <= S - executed (a frozen row must have a previous action); ValueError otherwise."""
    prev = np.asarray(prev, dtype=np.float32)
    if prev.ndim not in (2, 3):
        raise ValueError(f"shift_chunk: prev has shape {prev.shape}, expected [S, action_dim] or [B, S, action_dim]")
    S = prev.shape[-2]
    for name, v in (("executed", executed), ("freeze", freeze)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"shift_chunk: {name} must be an integer, got {v!r}")
    if not 0 <= executed <= S:
        raise ValueError(f"shift_chunk: executed = {executed} outside [0, {S}]")
    if not 0 <= freeze <= S - executed:
        raise ValueError(f"shift_chunk: freeze = {freeze} outside [0, S - executed = {S - executed}]")
    known = np.zeros_like(prev)
    known[..., :S - executed, :] = prev[..., executed:, :]
    mask = np.zeros(prev.shape[:-1], dtype=np.uint8)
    mask[..., :freeze] = 1
    return known, mask


class RealTimeChunker:
    """The previous model-space chunk of one policy.  `next(executed, freeze)` gives the `(known, mask)` of the coming request, or
    None when there is no previous chunk (the first request, or after `reset`: the request then samples freely); `update(chunk)`
    stores what the sampler returned."""

    def __init__(self):
        self.prev = None

    def reset(self):
        self.prev = None

    def update(self, chunk):
        chunk = np.array(chunk, dtype=np.float32)      # (a copy: the caller's array may be a view of a reused buffer)
        if chunk.ndim not in (2, 3):
            raise ValueError(f"RealTimeChunker.update: chunk has shape {chunk.shape}, expected [S, action_dim] or [B, S, action_dim]")
        self.prev = chunk

    def next(self, executed: int, freeze: int):
        if self.prev is None:
            return None
        return shift_chunk(self.prev, executed, freeze)
