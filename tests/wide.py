"""Shared layout for the tests that put offsets at and beyond 2^31 and 2^32 (DESIGN.md §6,
"Offsets beyond 4 GiB").  A plain module: a test module makes its own module-scoped fixture
with ``widebuf = wide.fixture()``.

  big     uint8 [BIG_BYTES], zeros: the one source buffer every offset is relative to
  bigout  uint8 [BIG_BYTES], GUARD: the one destination buffer

  W31 = [B31 - 1 MiB, B31 + 1 MiB)      the signed-32-bit line
  W32 = [B32 - 1 MiB, B32 + 3 MiB)      the unsigned-32-bit line
  A0  = [0, 3 MiB)                      what [B32, B32 + 3 MiB) reads as once the high word is lost

Every payload byte at an address a >= B32 has a decoy byte at a - B32: well-formed data of the same
kind with other content, so that code which drops the high word gives a plausible other answer,
not zeros.  In bigout, A0 stays GUARD and assert_untouched() looks at it.

A block of length n stands at six starts around a boundary B (placements()); tests count what they
placed with census() so that a refactor cannot move every case below the line unnoticed.
"""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest

B31 = 1 << 31
B32 = 1 << 32
MIB = 1 << 20
BIG_BYTES = B32 + (4 << 20)
GUARD = 0xA5
W31 = (B31 - MIB, B31 + MIB)
W32 = (B32 - MIB, B32 + 3 * MIB)
A0 = (0, 3 * MIB)
BOUNDARIES = (B31, B32)
NEED_FREE = 16 << 30
SLICE = 256 << 20          # the most assert_untouched() looks at in one device operation
KINDS = ("ends_at", "straddles", "last_below", "starts_at", "starts_above", "well_above")


def placements(n: int, B: int) -> list[int]:
    """The six starts of a block of n > 0 bytes at boundary B (KINDS): it ends exactly at B,
    straddles it, has only its first byte below, starts at B, at an odd address above, well above."""
    assert n > 0
    return [B - n, B - (n + 1) // 2, B - 1, B, B + 1, B + 65537]


def all_placements(n: int) -> list[int]:
    """placements() at both boundaries: twelve starts."""
    return [s for B in BOUNDARIES for s in placements(n, B)]


def census(blocks) -> dict:
    """Of (start, n) blocks, per boundary: how many start below B and end above it ("cross"),
    start exactly at B ("at") and start above it inside its window ("above")."""
    c = Counter()
    for s, n in blocks:
        for name, B, hi in (("31", B31, W31[1]), ("32", B32, W32[1])):
            if s < B < s + n and s >= B - MIB:
                c["cross" + name] += 1
            elif s == B:
                c["at" + name] += 1
            elif B < s < hi:
                c["above" + name] += 1
    return dict(c)


def full_census(lengths) -> dict:
    """What census() gives when every length stands at all_placements(): a block of one byte
    crosses nothing (its straddle and last-below starts are B - 1, its end B)."""
    lengths = list(lengths)
    k, cross = len(lengths), sum(2 if n > 1 else 0 for n in lengths)
    return {"cross31": cross, "at31": k, "above31": 2 * k, "cross32": cross, "at32": k, "above32": 2 * k}


def decoy_tail(at: int, payload: bytes, decoy: bytes):
    """What stands in A0 for a payload at `at`: None when the payload ends at or below B32, else
    (address, bytes): the decoy from the index of the payload's first byte at or above B32, at
    that byte's address minus 2^32.  A payload that starts at or above B32 so gets the whole
    decoy, of whatever length; a decoy that ends before that index gives filler bytes."""
    k = max(0, B32 - at)
    if k >= len(payload):
        return None
    tail = decoy[k:] if k < len(decoy) else bytes([0x5A]) * (len(payload) - k)
    assert at + k - B32 + len(tail) <= A0[1], "the decoy leaves A0"
    assert tail[:len(payload) - k] != payload[k:], "the decoy equals the payload above 2^32"
    return at + k - B32, tail


def rounds(jobs, gap: int = 64):
    """Split jobs into rounds in which no two spans of the same buffer come nearer than `gap`.
    A job is (key, [(buffer name, start, length), ...]); greedy, in order, so it is stable."""
    out = []          # per round: (list of jobs, {buffer name: [(lo, hi)]})
    for job in jobs:
        spans = job[1]
        assert all(a[0] != b[0] or a[1] + a[2] <= b[1] or b[1] + b[2] <= a[1]
                   for i, a in enumerate(spans) for b in spans[:i]), ("a job's own spans overlap", job[0])
        for members, used in out:
            if all(hi + gap <= s or s + n + gap <= lo for b, s, n in spans for lo, hi in used.get(b, ())):
                break
        else:
            members, used = [], {}
            out.append((members, used))
        members.append(job)
        for b, s, n in spans:
            used.setdefault(b, []).append((s, s + n))
    return [m for m, _ in out]


class Wide:
    """The two buffers of a module and what a test wrote into them."""

    def __init__(self, device, out_bytes: int = BIG_BYTES):
        import torch
        self.torch = torch
        self.device = device
        self.big = torch.zeros(BIG_BYTES, dtype=torch.uint8, device=device)
        self.bigout = torch.full((out_bytes,), GUARD, dtype=torch.uint8, device=device)
        self._dirty = []     # (buffer, lo, hi, fill)

    def _fill_of(self, buf) -> int:
        return GUARD if buf is self.bigout else 0

    def place(self, buf, at: int, payload) -> None:
        """buf[at : at + len(payload)] = payload (bytes or a uint8 ndarray); restore() undoes it."""
        a = np.array(np.frombuffer(payload, np.uint8) if isinstance(payload, (bytes, bytearray)) else payload, np.uint8)
        assert 0 <= at and at + len(a) <= buf.numel(), (at, len(a))
        if len(a):
            buf[at:at + len(a)] = self.torch.from_numpy(a).to(self.device)
            self._dirty.append((buf, at, at + len(a), self._fill_of(buf)))

    def place_with_decoy(self, at: int, payload: bytes, decoy: bytes) -> None:
        """payload into big at `at`, and what decoy_tail() gives for it into A0."""
        self.place(self.big, at, payload)
        alias = decoy_tail(at, payload, decoy)
        if alias is not None:
            self.place(self.big, *alias)

    def wrote(self, buf, at: int, n: int) -> None:
        """A kernel is about to write buf[at : at + n]: restore() refills it."""
        if n:
            self._dirty.append((buf, at, at + n, self._fill_of(buf)))

    def fetch(self, buf, at: int, n: int) -> bytes:
        return buf[at:at + n].cpu().numpy().tobytes()

    def restore(self, only=None) -> None:
        """Put back what place() and wrote() registered, in every buffer or in `only`."""
        keep = []
        for buf, lo, hi, fill in self._dirty:
            if only is None or buf is only:
                buf[lo:hi] = fill
            else:
                keep.append((buf, lo, hi, fill))
        self._dirty = keep

    def free(self) -> None:
        self._dirty = []
        del self.big, self.bigout
        self.torch.cuda.empty_cache()


def assert_untouched(bigout, spans) -> None:
    """Every byte of bigout outside `spans` ((start, length) pairs) still holds GUARD: compared
    on the device in slices of at most SLICE bytes, one read-back of the verdict."""
    import torch
    total = bigout.numel()
    merged = []
    for s, n in sorted((int(s), int(n)) for s, n in spans if n):
        if merged and s <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], s + n)
        else:
            merged.append([s, s + n])
    gaps, pos = [], 0
    for lo, hi in merged:
        if pos < lo:
            gaps.append((pos, lo))
        pos = max(pos, hi)
    if pos < total:
        gaps.append((pos, total))
    pieces = [(a, min(a + SLICE, hi)) for lo, hi in gaps for a in range(lo, hi, SLICE)]
    bad = torch.zeros((), dtype=torch.bool, device=bigout.device)
    for a, b in pieces:
        bad |= (bigout[a:b] != GUARD).any()
    if bool(bad.item()):
        for a, b in pieces:        # the failure path: name the first byte
            hit = torch.nonzero(bigout[a:b] != GUARD)
            if hit.numel():
                at = a + int(hit[0].item())
                raise AssertionError(f"bigout[{at:#x}] = {int(bigout[at].item()):#x}, written outside the blocks "
                                     f"(B31 {at - B31:+d}, B32 {at - B32:+d})")


def fixture(out_bytes: int = BIG_BYTES):
    """The module-scoped fixture of a wide test module: the Wide of that module, freed at its
    teardown; the module is skipped when the device has less than NEED_FREE bytes free."""
    @pytest.fixture(scope="module")
    def widebuf(cuda):
        import torch
        free = torch.cuda.mem_get_info()[0]
        if free < NEED_FREE:
            pytest.skip(f"wide-offset tests need 16 GiB of free device memory, {free >> 20} MiB are free")
        w = Wide(cuda, out_bytes)
        yield w
        w.free()
        del w
        torch.cuda.empty_cache()
    return widebuf


def per_test():
    """The function-scoped view of widebuf: what a test placed is put back when it ends."""
    @pytest.fixture
    def w(widebuf):
        yield widebuf
        widebuf.restore()
    return w
