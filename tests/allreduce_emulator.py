"""In-process sum all-reduce for the table-sharded DeepFM's training tests — the companion of
a2a_emulator.InProcessAllToAll.  P shards live in one process, one Python thread each; every shard's
`reduce_fn` is bound to one InProcessAllReduce.  A call is collective: all ranks deposit their flat
tensor, meet at a barrier, each adds the P deposits in rank order into a buffer of its own (so every
rank computes the same bits), and only after every rank has finished reading do the ranks overwrite
their tensors with the sum.  On a GPU the reads and writes are stream-ordered through one event per
rank, as in the all-to-all emulator."""
from __future__ import annotations

import threading


class InProcessAllReduce:
    def __init__(self, world: int, timeout: float = 120.0):
        self.world = world
        self.barrier = threading.Barrier(world, timeout=timeout)
        self.slots = [None] * world
        self.events = [None] * world
        self.calls = 0

    def bind(self, rank: int):
        def reduce(flat):
            self._reduce(rank, flat)
            return flat
        return reduce

    def _record(self, rank, cuda):
        if cuda:
            import torch
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self.events[rank] = ev

    def _wait_all(self, cuda):
        if cuda:
            import torch
            st = torch.cuda.current_stream()
            for e in list(self.events):
                st.wait_event(e)

    def _reduce(self, rank, flat):
        cuda = flat.is_cuda
        self.slots[rank] = flat
        self._record(rank, cuda)      # after this rank's producers
        self.barrier.wait()
        self._wait_all(cuda)
        if any(s.shape != flat.shape or s.dtype != flat.dtype for s in self.slots):
            raise ValueError(f"rank {rank}: the ranks' tensors differ in shape or dtype")
        total = self.slots[0].clone()
        for s in range(1, self.world):
            total += self.slots[s]
        self.barrier.wait()           # every rank has read the deposit events
        self._record(rank, cuda)      # after this rank's reads of every deposit
        self.barrier.wait()
        self._wait_all(cuda)
        flat.copy_(total)
        if rank == 0:
            self.calls += 1
        self.barrier.wait()           # every rank has read the events before the next call replaces them

    def abort(self):
        self.barrier.abort()
