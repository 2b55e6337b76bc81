"""Poisoning of PyTorch's caching allocator for tests/test_gpu_dirty_memory.py: after poison_caching_allocator() every free byte
the allocator holds is a NaN pattern, so the product's torch.empty calls get what they get in production -- memory somebody else
used -- with the worst plausible content."""
from __future__ import annotations

from tests.backends import POISON_WORD

MiB = 1 << 20
PROBE_BYTES = (64, 4 << 10, 600 << 10, 3 * MiB, 64 * MiB)
# the allocator's size classes: requests of at most 1 MiB come from the small pool (2 MiB segments), larger ones from the large pool
# (20 MiB segments for requests under 10 MiB, own segments rounded to 2 MiB above); sizes round to 512 bytes, free blocks are split
# (in the large pool only while more than 1 MiB remains)
_LARGE_FILL = (64 * MiB, 16 * MiB, 4 * MiB, MiB + 512)
_SMALL_FILL = tuple(MiB >> k for k in range(12))  # 1 MiB, 512 KiB, ... 512 bytes


def _nan_block(torch, nbytes):
    return torch.empty(nbytes // 4, dtype=torch.int32, device="cuda").fill_(POISON_WORD)


def _fill_gaps(torch, held, sizes):
    """Blocks of each size (largest first) until one makes the allocator reserve a new segment: no free gap of that size was left.  The
    new segment's own remainder is a gap for the smaller sizes.  Returns the remainder left behind the last block."""
    rest = 0
    for size in sizes:
        for _ in range(100000):
            before = torch.cuda.memory_reserved()
            held.append(_nan_block(torch, size))
            grown = torch.cuda.memory_reserved() - before
            if grown:
                rest = grown - size
                break
        else:
            raise AssertionError(f"still filling {size}-byte gaps after 100000 blocks")
    return rest


def poison_caching_allocator(torch, peak_bytes):
    """Leave the caching allocator holding only poisoned free memory.  The gaps inside the segments that live tensors keep alive are
    filled size class by size class, then whole new segments are added -- large blocks totalling at least twice `peak_bytes`, and 64 MiB
    of small-pool segments; every block is filled with POISON_WORD, and all are freed together.  Then PROVES it: torch.empty at
    PROBE_BYTES must come back as the poison word throughout (all-NaN as fp32), else AssertionError: a vacuous test must not pass."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    held = []
    rest = _fill_gaps(torch, held, _LARGE_FILL)
    if rest > MiB:                                   # the last new 20 MiB segment: the one free block of that size
        held.append(_nan_block(torch, rest))
    rest = _fill_gaps(torch, held, _SMALL_FILL)      # ends with a new 2 MiB segment holding one 512-byte block:
    for size in _SMALL_FILL:                         # 1 MiB + 512 KiB + ... + 512 bytes fill the rest of it exactly
        if rest >= size:
            held.append(_nan_block(torch, size))
            rest -= size
    held.append(_nan_block(torch, 128 * MiB))
    total = 0
    while total < 2 * peak_bytes:
        held.append(_nan_block(torch, 64 * MiB))
        total += 64 * MiB
    held.extend(_nan_block(torch, MiB) for _ in range(64))
    torch.cuda.synchronize()
    del held
    # (the proof must not write into the memory it examines: min / max leave a scalar each, itself the poison word, and at most a few
    # hundred bytes of reduction scratch, where isnan() would leave a mask a quarter of the block's size behind)
    probes = [torch.empty(n // 4, dtype=torch.int32, device="cuda") for n in PROBE_BYTES]
    for nbytes, probe in zip(PROBE_BYTES, probes):
        lo, hi = int(probe.min()), int(probe.max())
        assert lo == hi == POISON_WORD, f"vacuous: torch.empty({nbytes} bytes) after poisoning is not all-NaN (words {lo:#x} .. {hi:#x})"
    del probes
