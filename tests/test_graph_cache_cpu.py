"""matcha/_graphs.py off the device: the bounded LRU cache every captured path keeps its graphs in, and the
capture-mode decision (thread_local while a process group is up)."""
from __future__ import annotations

import os
import socket

import pytest
import torch.distributed as dist

from matcha._graphs import GraphCache, capture_mode


def _never():
    raise AssertionError("build() called on a hit")


def test_hit_returns_the_entry_without_building():
    c = GraphCache(2)
    entry = object()
    assert c.lookup("a", lambda: entry) is entry
    assert c.lookup("a", _never) is entry
    assert len(c) == 1


def test_eviction_is_least_recently_used_not_oldest_inserted():
    c = GraphCache(2)
    for k in "abac":
        c.lookup(k, lambda k=k: k.upper())
    assert list(c) == ["a", "c"] and list(c.values()) == ["A", "C"]


def test_limit_is_at_least_one():
    c = GraphCache(0)
    c.lookup("a", lambda: 1)
    assert list(c) == ["a"]
    c.lookup("b", lambda: 2)
    assert list(c) == ["b"]


def test_a_raising_build_leaves_the_cache_unchanged():
    c = GraphCache(2)
    c.lookup("a", lambda: 1)
    c.lookup("b", lambda: 2)

    def boom():
        raise RuntimeError("capture failed")

    with pytest.raises(RuntimeError):
        c.lookup("c", boom)
    assert len(c) == 2 and list(c) == ["a", "b"]
    c.lookup("a", _never)  # a hit: a is now the most recently used
    with pytest.raises(RuntimeError):
        c.lookup("d", boom)
    assert list(c) == ["b", "a"]


def test_behaves_as_a_dict():
    c = GraphCache(3)
    for i, k in enumerate("xyz"):
        c.lookup(k, lambda i=i: {"overlap": i})
    assert len(c) == 3 and bool(c) and not GraphCache(3)
    assert [k for k in c] == ["x", "y", "z"] and set(c) == {"x", "y", "z"} and "y" in c
    assert next(iter(c.values()))["overlap"] == 0
    assert dict(c.items()) == {"x": {"overlap": 0}, "y": {"overlap": 1}, "z": {"overlap": 2}}
    c.clear()
    assert len(c) == 0


def test_capture_mode_follows_the_process_group():
    assert capture_mode() == "global"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        assert capture_mode() == "thread_local"
    finally:
        dist.destroy_process_group()
    assert capture_mode() == "global"
