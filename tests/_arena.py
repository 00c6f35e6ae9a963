"""A guarded, poisoned arena for memory-contract tests (tests/test_gpu_memory_contract.py).

``include/miaudio.h`` promises that the caller owns all memory and that a size function (or a prose formula)
gives the bytes one call needs.  torch's caching allocator hides a kernel that breaks that promise: it rounds
requests up and carves tensors out of larger blocks, so a short overrun lands in padding or in a live neighbour
and nothing faults.  ``GuardedArena.take`` hands out a view of EXACTLY ``nbytes`` whose last byte is followed
immediately by guard bytes the arena owns (and a leading guard in front); the interior and both guards hold one
poison byte.  After the kernels ran (and ``torch.cuda.synchronize()``), ``check()`` raises if any guard byte
changed.

Poison 0xFF makes every f32 / bf16 / f64 word a NaN, poison 0x00 makes it zero: a result that differs between
the two was read from memory the call never wrote.

Reach: a write is seen only if it lands within ``guard`` bytes of the buffer (1 MiB by default, 64 KiB in the
chunked arena of the whole-model steps).  These are conditions of the test, not measurements; an overrun longer
than the guard is outside this harness's reach.  Every byte within a guard length of a taken pointer belongs to a
tensor this arena owns, so such an overrun damages only the test's own memory.  A write that stores the poison
value itself is invisible; running both poisons covers that.
"""
from __future__ import annotations

import torch

POISONS = (0xFF, 0x00)
GUARD = 1 << 20
CHUNK_GUARD = 64 << 10


class GuardDamage(AssertionError):
    pass


class _Entry:
    __slots__ = ("name", "store", "start", "nbytes", "lead0", "trail1")

    def __init__(self, name, store, start, nbytes, lead0, trail1):
        self.name, self.store, self.start, self.nbytes, self.lead0, self.trail1 = name, store, start, nbytes, lead0, trail1


class GuardedArena:
    """``chunk_bytes`` None: every ``take`` is an allocation of its own (leading guard, buffer, trailing guard).
    ``chunk_bytes`` set: buffers are carved out of chunks of at least that size, each between two guards of its
    own (for whole model steps, which take hundreds of workspaces)."""

    def __init__(self, device, poison: int, guard: int | None = None, chunk_bytes: int | None = None):
        if poison not in POISONS:
            raise ValueError(f"poison must be one of {[hex(p) for p in POISONS]}, got {poison!r}")
        self.device = torch.device(device)
        self.poison = poison
        self.guard = int(guard if guard is not None else (CHUNK_GUARD if chunk_bytes else GUARD))
        if self.guard < 1:
            raise ValueError("guard must be at least one byte")
        self.chunk_bytes = chunk_bytes
        self.entries: list[_Entry] = []
        self._chunk = None
        self._used = 0

    # ------------------------------------------------------------------ allocation
    def _alloc(self, n: int) -> torch.Tensor:
        return torch.full((n,), self.poison, dtype=torch.uint8, device=self.device)

    def _region(self, need: int) -> tuple[torch.Tensor, int]:
        """(storage, first free offset) with ``need`` poisoned bytes free behind it."""
        if self.chunk_bytes is None:
            return self._alloc(need), 0
        if self._chunk is None or self._used + need > self._chunk.numel():
            self._chunk = self._alloc(max(int(self.chunk_bytes), need))
            self._used = 0
        off = self._used
        self._used += need
        return self._chunk, off

    def take(self, name: str, nbytes: int, align: int = 256, offset: int = 0) -> torch.Tensor:
        """A ``uint8`` view of exactly ``nbytes`` bytes: first byte aligned to ``align`` (``offset`` bytes past an
        ``align`` boundary when given: a deliberately misaligned buffer), guard bytes immediately behind the last
        one and in front of the first, everything poisoned.  ``nbytes == 0`` gives a zero-length view between two
        guards."""
        nbytes = int(nbytes)
        if nbytes < 0:
            raise ValueError(f"{name}: negative size {nbytes}")
        if align < 1 or align & (align - 1):
            raise ValueError(f"{name}: align {align} is not a power of two")
        if not 0 <= offset < align:
            raise ValueError(f"{name}: offset {offset} outside [0, {align})")
        need = self.guard + align + nbytes + self.guard
        store, off = self._region(need)
        base = store.data_ptr() + off + self.guard
        start = off + self.guard + (offset - base) % align
        self.entries.append(_Entry(name, store, start, nbytes, off, off + need))
        return store[start:start + nbytes]

    def take_as(self, name: str, shape, dtype: torch.dtype, align: int = 256, offset: int = 0) -> torch.Tensor:
        """``take`` of exactly the bytes of a contiguous ``shape`` tensor of ``dtype``, viewed as such."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        numel = 1
        for s in shape:
            numel *= int(s)
        item = torch.empty((), dtype=dtype).element_size()
        return self.take(name, numel * item, max(align, item), offset).view(dtype).view(shape)

    def f32(self, name, shape, align=256):
        return self.take_as(name, shape, torch.float32, align)

    def bf16(self, name, shape, align=256):
        return self.take_as(name, shape, torch.bfloat16, align)

    def f64(self, name, shape, align=256):
        return self.take_as(name, shape, torch.float64, align)

    def u8(self, name, shape, align=256):
        return self.take_as(name, shape, torch.uint8, align)

    def i32(self, name, shape, align=256):
        return self.take_as(name, shape, torch.int32, align)

    # ------------------------------------------------------------------ checking
    def _sides(self, e: _Entry):
        # (side, region, offset of region[0] relative to the buffer edge it guards)
        yield "before the start", e.store[e.lead0:e.start], -(e.start - e.lead0)
        yield "past the end", e.store[e.start + e.nbytes:e.trail1], 0

    def check(self) -> None:
        """Raise GuardDamage if a guard byte changed.  Call after ``torch.cuda.synchronize()``.  The message names
        the buffer, the damaged side, the first and last damaged byte relative to that buffer edge (past the end:
        0 is the first byte behind the buffer; before the start: -1 is the byte in front of it) and the count."""
        if not self.entries:
            return
        counts = torch.stack([torch.count_nonzero(r != self.poison) for e in self.entries for _, r, _ in self._sides(e)])
        counts = counts.cpu().tolist()
        msgs = []
        for k, e in enumerate(self.entries):
            for j, (side, region, rel) in enumerate(self._sides(e)):
                if not counts[2 * k + j]:
                    continue
                idx = (region != self.poison).nonzero().flatten()
                first, last = int(idx[0]) + rel, int(idx[-1]) + rel
                msgs.append(f"buffer '{e.name}' ({e.nbytes} bytes): guard damaged {side}: {counts[2 * k + j]} byte(s), "
                            f"first at offset {first:+d}, last at offset {last:+d} from that edge "
                            f"(poison 0x{self.poison:02X})")
        if msgs:
            raise GuardDamage("; ".join(msgs))

    def release(self) -> None:
        self.entries.clear()
        self._chunk = None
        self._used = 0
