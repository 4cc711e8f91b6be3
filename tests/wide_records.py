"""The .data layout of tests/test_gpu_wide_records.py and the rules that derive what the reader
owes for a 4 GiB buffer from the oracle's answers on its three windows (tests/test_wide_rules.py
checks the rules against the oracle itself, at a small scale).  Host code only.

A layout puts one chunk of records around 2^31, another around 2^32 and decoy records into A0:
at the address of every record at or above 2^32, minus 2^32, stands a valid record of the same
sizes with another key and another value, so a reader that drops an offset's high word finds a
record there -- the wrong one.

Records start on 256-byte slots and 2^31 and 2^32 are slot boundaries, so a 24-byte header never
straddles a line; what can straddle is a key or a body.  One chunk cannot have both a record that
starts at a line and one that straddles it, so there are two layouts:

  "straddle"   a compressed record's body straddles 2^32; a record starts exactly at 2^31
  "starts_at"  a record starts exactly at 2^32 (the one before ends there); a compressed body
               straddles 2^31
"""
from __future__ import annotations

import functools
import random

import numpy as np

import hint_model as H
import wide
from oracle import oracle as O
from oracle import replay as R
from wide import B31, B32

M32 = 0xFFFFFFFF
WIN31 = wide.W31
WIN32 = (wide.W32[0], wide.BIG_BYTES)      # to the buffer's end: offsets near `size` are judged in it
WINA0 = wide.A0


def chunk(seed: int, n: int, max_body: int = 3000) -> bytes:
    """tests/test_gpu_gc_batch.py's _chunk (the generator of tests/test_gc.py)."""
    rnd = random.Random(seed)
    out = bytearray()
    for i in range(n):
        key = b"key_%016x" % (seed * 1000 + i)
        body = O.gen_text(seed, i, rnd.randint(0, max_body)) if rnd.random() < 0.7 else \
            bytes(rnd.getrandbits(8) for _ in range(rnd.randint(0, 600)))
        flag = 0
        if len(body) > 300 and rnd.random() < 0.6:
            body, flag = O.compress(body), R.FLAG_COMPRESS
        out += R.make_record(key, body, flag=flag, ver=rnd.randint(-2, 5), ts=1700000000 + i)
    return bytes(out)


def _base(recs, B: int, how: str) -> int:
    """Where the chunk of `recs` starts so that, at boundary B, a record of its second half
    starts exactly at B, or a compressed one has the middle of its body in [B, B + 256)."""
    later = recs[len(recs) // 2:]
    if how == "starts_at":
        return B - later[0].offset
    r = next(r for r in later if r.flag & R.FLAG_COMPRESS and len(r.body) >= 600)
    return B - (r.offset + R.HDR + len(r.key) + len(r.body) // 2) // 256 * 256


@functools.lru_cache(maxsize=None)
def layout(kind: str, corrupt: bool = False):
    """{window start: uint8 array} for A0, WIN31 and WIN32, plus the facts the tests assert.
    corrupt=True flips a body byte of the last record that starts below 2^32, so the reader's
    resync from it crosses the line."""
    assert kind in ("straddle", "starts_at")
    how32, how31 = ("straddle", "starts_at") if kind == "straddle" else ("starts_at", "straddle")
    c32, c31 = chunk(41, 120), chunk(42, 120)
    r32, r31 = R.stream_all(c32)[0], R.stream_all(c31)[0]
    p32, p31 = _base(r32, B32, how32), _base(r31, B31, how31)
    win = {lo: np.zeros(hi - lo, np.uint8) for lo, hi in (WINA0, WIN31, WIN32)}
    for lo, p, c in ((WIN31[0], p31, c31), (WIN32[0], p32, c32)):
        assert p % 256 == 0 and lo <= p and p + len(c) <= lo + len(win[lo])
        win[lo][p - lo:p - lo + len(c)] = np.frombuffer(c, np.uint8)
    rnd = random.Random(43)
    for i, r in enumerate(r32):                      # the decoys
        at = p32 + r.offset - B32
        if at >= 0:
            d = R.make_record((b"dcy_%016x" % i)[:len(r.key)].ljust(len(r.key), b"~"), rnd.randbytes(len(r.body)),
                              ver=r.ver + 7, ts=r.ts)
            assert len(d) == r.rsize and at + len(d) <= WINA0[1]
            win[0][at:at + len(d)] = np.frombuffer(d, np.uint8)
    if corrupt:
        last_below = max((r for r in r32 if p32 + r.offset < B32), key=lambda r: r.offset)
        assert len(last_below.body) > 2
        win[WIN32[0]][p32 + last_below.offset + R.HDR + len(last_below.key) + 1 - WIN32[0]] ^= 0x10
    return win, {"p31": p31, "p32": p32, "n31": len(r31), "n32": len(r32)}


def window_bytes(win, lo: int) -> bytes:
    return win[lo].tobytes()


def facts(win):
    """Per window the oracle's records with absolute offsets, and the layout's census: how many
    records start below / exactly at / above each line, which record's key or body straddles it
    and whether that record is compressed."""
    recs = {lo: [(lo + r.offset, r) for r in R.stream_all(window_bytes(win, lo))[0]] for lo in win}
    census = {}
    for name, B, lo in (("31", B31, WIN31[0]), ("32", B32, WIN32[0])):
        offs = [o for o, _ in recs[lo]]
        census["below" + name] = sum(o < B for o in offs)
        census["at" + name] = sum(o == B for o in offs)
        census["above" + name] = sum(o > B for o in offs)
        census["straddle" + name] = [(bool(r.flag & R.FLAG_COMPRESS), o + R.HDR + len(r.key) < B)
                                     for o, r in recs[lo] if o + R.HDR < B < o + R.HDR + len(r.key) + len(r.body)]
        census["ends_at" + name] = sum(o + r.rsize == B for o, r in recs[lo])
    return recs, census


def assert_decoys(win, recs) -> int:
    """Under every record at or above 2^32 lies, 2^32 lower, a valid record with another key and
    another value; returns how many."""
    a0 = window_bytes(win, 0)
    k = 0
    for o, r in recs[WIN32[0]]:
        if o >= B32:
            d = R.read_record_at(a0, o - B32)
            assert d is not None and d.key != r.key and d.body != r.body and d.rsize == r.rsize, o
            k += 1
    return k


# ---------------------------------------------------------------- the derivation rules

def replay_rows(win, lo: int):
    """oracle.replay of one window from its start, offsets absolute: (rows, end error)."""
    rows, err = R.replay(window_bytes(win, lo))
    return [(lo + row[0],) + tuple(row[1:]) for row in rows], err


def join_replays(parts):
    """The replay rule.  parts: (window start, rows with absolute offsets, padded size of the
    window's last record) in address order, the windows separated by zeros and each ending in
    zeros.  What the reader returns from the first window's start over the whole buffer: every
    window's rows, and the first row after a gap carries in sizeBroken the zeros the resync
    crossed: from the end of the record before the gap to this window's start, plus what the
    window's own replay skipped before its first record."""
    out, prev_end = [], None
    for lo, rows, last_rsize in parts:
        rows = list(rows)
        if rows and prev_end is not None:
            first = rows[0]
            rows[0] = (first[0], first[1] + (lo - prev_end)) + tuple(first[2:])
        out += rows
        if rows:
            prev_end = rows[-1][0] + last_rsize
    return out


def last_rsize(win, lo: int) -> int:
    recs = R.stream_all(window_bytes(win, lo))[0]
    return recs[-1].rsize


def slot_counts(win, size: int, max_key=R.MAX_KEY_LEN, body_max=R.BODY_MAX):
    """(candidates, valid records) over every 256-byte slot of the windows -- everything else in
    the buffer is zeros, no candidate: a candidate has readRecordAt's sizes and fits in `size`."""
    ncand = nvalid = 0
    for lo, a in win.items():
        data = a.tobytes()
        for off in range(0, len(data) - R.HDR + 1, 256):
            if not any(data[off + 16:off + 20]):      # ksz == 0: no candidate
                continue
            _, _, _, _, k, v = R._hdr(data, off)
            if 0 < k <= max_key and v <= body_max and lo + off + R.HDR + k + v <= size:
                ncand += 1
                nvalid += R.read_record_at(data, off, max_key, body_max) is not None
    return ncand, nvalid


def hint_records(rows, recs):
    """hint_model's input for replayed rows with absolute offsets: the offset reduced mod 2^32,
    as the hint item stores it (include/qlzx.h: uint32(rec_off[j]))."""
    assert len(rows) == len(recs)
    return [(H.keyhash(row[2]), row[2], row[0] & M32, r.rsize, row[3], row[6]) for row, (_, r) in zip(rows, recs)]


def gc_with_repeats(image: bytes, times: int, tail_chunks, tail_pos):
    """The GC concatenation rule.  A record listed `times` times ahead of other records, all kept,
    one destination chunk from head 0: its padded image `times` times, then what
    oracle.gc.gc_rewrite gives for the others with dst_head = times * len(image) (tail_chunks,
    tail_pos).  Returns (chunks, positions)."""
    assert len(tail_chunks) == 1 and len(image) % 256 == 0
    return [image * times + tail_chunks[0]], [(0, k * len(image)) for k in range(times)] + list(tail_pos)


def hint_datasize(model_records, max_offset: int = 0) -> int:
    """include/qlzx.h's datasize of one split that takes every record: the largest of max_offset
    and uint32(rec_off) + the padded record size, in 32-bit arithmetic."""
    return max([max_offset] + [((o & M32) + rs) & M32 for _, _, o, rs, _, _ in model_records])
