"""Which training passes of an engine are alive: the bookkeeping behind the pass slots of ``seq_train``.

A training engine keeps the activations of a forward pass in buffers of its own (a *plan*) until the pass's backward has read
them.  ``experiments/behavior_net.py:611-686`` holds three passes of one shape at once -- the one the loss is formed on (:616), a
dead one (:627) and the one behind ``classifier_beta`` (:681) -- so an engine keeps several plans per shape, numbered 0, 1, ...:
a pass takes the lowest free number for its shape key and gives it back when its autograd node dies (not when its backward has
run: ``retain_graph=True`` runs it again).  Nothing here touches the GPU: the engines allocate the plan of slot k when a pass first
gets k, i.e. when k + 1 passes of that shape are alive.
"""
from __future__ import annotations

import weakref
from typing import Dict, Hashable, Set


class PassLease:
    """The owner of one slot: lives on the autograd node of its pass (``ctx``); the slot is free again when it is collected."""

    __slots__ = ("key", "slot", "_finalizer", "__weakref__")

    def __init__(self, key: Hashable, slot: int):
        self.key, self.slot = key, slot
        self._finalizer = None

    def release(self):
        """Give the slot back now (idempotent; what the finalizer does when the node dies)."""
        if self._finalizer is not None:
            self._finalizer()


class PassPool:
    """Slots per shape key, at most ``max_passes`` of them alive per key.  Nothing is ever evicted: a pass that finds every slot
    of its shape taken raises."""

    def __init__(self, max_passes: int = 4, what: str = "the net"):
        self.max_passes = int(max_passes)
        self.what = what
        self._live: Dict[Hashable, Set[int]] = {}

    def alive(self, key: Hashable) -> int:
        return len(self._live.get(key, ()))

    def acquire(self, key: Hashable) -> int:
        """The lowest free slot of ``key``."""
        live = self._live.setdefault(key, set())
        for slot in range(self.max_passes):
            if slot not in live:
                live.add(slot)
                return slot
        if not live:
            del self._live[key]
        raise RuntimeError(
            f"{len(live)} passes of {self.what} with shape {key} are alive and the engine keeps at most max_passes = {self.max_passes} "
            f"per shape: every pass holds its saved activations until its outputs (its autograd graph) are gone.  Drop the outputs of a "
            f"pass that is done with, or raise the engine's max_passes attribute")

    def release(self, key: Hashable, slot: int):
        live = self._live.get(key)
        if live is not None:
            live.discard(slot)
            if not live:
                del self._live[key]

    def lease(self, key: Hashable) -> PassLease:
        """``acquire`` + an owner object whose death releases the slot."""
        lease = PassLease(key, self.acquire(key))
        lease._finalizer = weakref.finalize(lease, self.release, key, lease.slot)
        return lease


class KeepsPasses:
    """For an engine that holds its pool as ``_passes``: the engine's ``max_passes`` attribute."""

    @property
    def max_passes(self) -> int:
        """How many forward passes of one shape may be alive (under autograd) at the same time, each in a plan of its own."""
        return self._passes.max_passes

    @max_passes.setter
    def max_passes(self, n: int):
        self._passes.max_passes = int(n)
