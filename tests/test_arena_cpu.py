"""tests/_arena.py on CPU tensors: what the GPU memory-contract cases rely on."""
import re

import pytest
import torch

from tests._arena import GUARD, GuardDamage, GuardedArena

CPU = torch.device("cpu")
SMALL = 4096  # guard size of these tests (the GPU cases use the 1 MiB default)


@pytest.mark.parametrize("poison", [0xFF, 0x00])
@pytest.mark.parametrize("chunk", [None, 1 << 16])
@pytest.mark.parametrize("nbytes,align", [(1, 1), (7, 4), (1000, 256), (4096, 4096), (12, 16)])
def test_alignment_exact_length_and_poison(poison, chunk, nbytes, align):
    a = GuardedArena(CPU, poison, guard=SMALL, chunk_bytes=chunk)
    bufs = [a.take(f"b{i}", nbytes, align) for i in range(3)]
    for b, e in zip(bufs, a.entries):
        assert b.dtype == torch.uint8 and b.numel() == nbytes and b.is_contiguous()
        assert b.data_ptr() % align == 0
        assert bool((b == poison).all())
        # the guards touch the buffer on both sides, are at least a guard long and hold the poison
        assert e.store.data_ptr() + e.start == b.data_ptr()
        assert e.start - e.lead0 >= SMALL and e.trail1 - (e.start + nbytes) >= SMALL
        assert bool((e.store[e.lead0:e.start] == poison).all())
        assert bool((e.store[e.start + nbytes:e.trail1] == poison).all())
    a.check()
    # writing the whole interior is not damage
    for b in bufs:
        b.fill_(0x5A)
    a.check()


def test_default_guard_is_one_mib():
    a = GuardedArena(CPU, 0xFF)
    a.take("x", 16)
    e = a.entries[0]
    assert a.guard == GUARD == 1 << 20
    assert e.start - e.lead0 >= GUARD and e.trail1 - (e.start + 16) >= GUARD
    assert GuardedArena(CPU, 0xFF, chunk_bytes=1 << 20).guard == 64 << 10


def test_poison_ff_is_nan_in_every_float_type():
    a = GuardedArena(CPU, 0xFF, guard=SMALL)
    assert bool(torch.isnan(a.f32("f", (3, 5))).all())
    assert bool(torch.isnan(a.bf16("b", (3, 5)).float()).all())
    assert bool(torch.isnan(a.f64("d", 7)).all())
    z = GuardedArena(CPU, 0x00, guard=SMALL)
    assert bool((z.f32("f", (3, 5)) == 0).all()) and bool((z.i32("i", 4) == 0).all())


def test_typed_helpers_shape_and_alignment():
    a = GuardedArena(CPU, 0x00, guard=SMALL)
    t = a.f64("d", (3, 5), align=4)  # the element size is the least alignment
    assert t.shape == (3, 5) and t.dtype == torch.float64 and t.data_ptr() % 8 == 0
    assert a.entries[-1].nbytes == 3 * 5 * 8
    u = a.u8("u", 13)
    assert u.shape == (13,) and a.entries[-1].nbytes == 13


def test_offset_from_an_alignment_boundary():
    a = GuardedArena(CPU, 0xFF, guard=SMALL)
    t = a.take_as("p", 1003, torch.float32, align=256, offset=4)
    assert t.data_ptr() % 256 == 4 and t.numel() == 1003 and a.entries[-1].nbytes == 4012
    a.check()
    with pytest.raises(ValueError):
        a.take("q", 8, align=16, offset=16)


def _neighbour(a, k=0):
    e = a.entries[k]
    return e.store, e.start, e.nbytes


@pytest.mark.parametrize("poison", [0xFF, 0x00])
@pytest.mark.parametrize("chunk", [None, 1 << 16])
def test_one_byte_past_the_end_is_detected(poison, chunk):
    a = GuardedArena(CPU, poison, guard=SMALL, chunk_bytes=chunk)
    a.take("first", 64)
    a.take("partial slab", 100, align=4)
    store, start, n = _neighbour(a, 1)
    store[start + n] = 0x5A
    with pytest.raises(GuardDamage) as ei:
        a.check()
    msg = str(ei.value)
    assert "'partial slab' (100 bytes)" in msg and "past the end" in msg and "1 byte(s)" in msg
    assert "first at offset +0, last at offset +0" in msg
    assert f"poison 0x{poison:02X}" in msg
    assert "'first'" not in msg


@pytest.mark.parametrize("poison", [0xFF, 0x00])
def test_one_byte_before_the_start_is_detected(poison):
    a = GuardedArena(CPU, poison, guard=SMALL)
    a.take("ws", 256)
    store, start, _ = _neighbour(a)
    store[start - 1] = 0x5A
    with pytest.raises(GuardDamage) as ei:
        a.check()
    msg = str(ei.value)
    assert "'ws' (256 bytes)" in msg and "before the start" in msg and "1 byte(s)" in msg
    assert "first at offset -1, last at offset -1" in msg


def test_message_reports_extent_and_count_of_a_longer_overrun():
    a = GuardedArena(CPU, 0xFF, guard=SMALL)
    a.take("out", 32, align=16)
    store, start, n = _neighbour(a)
    store[start + n + 16:start + n + 32] = 0  # one 16-byte vector store, one group past the end
    store[start - 8:start - 4] = 0
    with pytest.raises(GuardDamage) as ei:
        a.check()
    msg = str(ei.value)
    m = re.search(r"past the end: (\d+) byte\(s\), first at offset ([+-]\d+), last at offset ([+-]\d+)", msg)
    assert m and (int(m[1]), int(m[2]), int(m[3])) == (16, 16, 31)
    m = re.search(r"before the start: (\d+) byte\(s\), first at offset ([+-]\d+), last at offset ([+-]\d+)", msg)
    assert m and (int(m[1]), int(m[2]), int(m[3])) == (4, -8, -5)


@pytest.mark.parametrize("chunk", [None, 1 << 16])
def test_zero_length_buffer_sits_between_two_guards(chunk):
    a = GuardedArena(CPU, 0x00, guard=SMALL, chunk_bytes=chunk)
    b = a.take("empty", 0)
    assert b.numel() == 0 and b.dtype == torch.uint8
    assert a.f32("empty f32", 0).numel() == 0
    a.check()
    store, start, n = _neighbour(a)
    assert n == 0
    store[start] = 1  # the first byte "past the end" of a zero-length buffer
    with pytest.raises(GuardDamage, match=r"'empty' \(0 bytes\).*past the end.*offset \+0"):
        a.check()
    store[start] = 0
    store[start - 1] = 1
    with pytest.raises(GuardDamage, match=r"'empty' \(0 bytes\).*before the start.*offset -1"):
        a.check()


def test_chunked_arena_starts_a_new_chunk_and_keeps_checking_the_old_one():
    a = GuardedArena(CPU, 0xFF, guard=256, chunk_bytes=4096)
    a.take("a", 1000)
    a.take("b", 3000)  # does not fit behind "a": a new chunk
    a.take("c", 100_000)  # larger than a chunk
    assert a.entries[0].store is not a.entries[1].store
    store, start, n = _neighbour(a, 0)
    store[start + n + 3] = 0
    with pytest.raises(GuardDamage, match=r"'a' \(1000 bytes\).*past the end.*offset \+3"):
        a.check()


def test_bad_arguments():
    with pytest.raises(ValueError):
        GuardedArena(CPU, 0xAB)
    a = GuardedArena(CPU, 0xFF, guard=SMALL)
    with pytest.raises(ValueError):
        a.take("x", -1)
    with pytest.raises(ValueError):
        a.take("x", 8, align=3)
