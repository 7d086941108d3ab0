"""Captured HIP graphs: the capture mode, a bounded LRU cache of captures, and the capture itself.

Every site that captures (Trainer's step and validation_step, CFM's Euler solve, the HiFi-GAN generator, Griffin-Lim)
keeps what is its own -- the key, its static input buffers and how they are refilled, what it returns -- and takes
the rest from here."""
from __future__ import annotations

import collections

import torch
import torch.distributed as dist


def capture_mode() -> str:
    """torch.cuda.graph's capture_error_mode for this process."""
    # with a process group up, its watchdog thread polls the events of earlier collectives (e.g. the eager
    # all-reduce of the torch.distributed transport) at any time; in the default "global" capture mode such a
    # query from another thread invalidates the capture and aborts the process.  "thread_local" restricts only
    # this thread (the autograd thread's launches still go to the capturing stream and its allocations to the
    # graph pool)
    return "thread_local" if (dist.is_available() and dist.is_initialized()) else "global"


class GraphCache(collections.OrderedDict):
    """key -> captured entry, least recently used first; at most max(1, limit) entries."""

    def __init__(self, limit: int):
        super().__init__()
        self.limit = max(1, int(limit))

    def lookup(self, key, build):
        """The entry of `key`, now the most recently used; a miss inserts build() and evicts down to the limit
        (a build() that raises leaves the cache as it was)."""
        if key in self:
            self.move_to_end(key)
            return self[key]
        entry = self[key] = build()
        while len(self) > self.limit:
            self.popitem(last=False)
        return entry


def capture(fn, device, *, warmup=None, passes: int = 1, pool=None):
    """`passes` calls of `warmup` (default: `fn`) on a fresh side stream fenced against the current one -- lazy
    code-object loads, pack plans, allocator pools --, then `fn()` captured.  Returns (graph, fn's result)."""
    cur = torch.cuda.current_stream(device)
    side = torch.cuda.Stream(device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        for _ in range(passes):
            (warmup or fn)()
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=pool, capture_error_mode=capture_mode()):
        out = fn()
    return graph, out
