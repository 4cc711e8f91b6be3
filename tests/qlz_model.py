"""An instrumented model of the level-3 compressor -- TEST INFRASTRUCTURE ONLY.

A plain restatement of qlz_compress_core level 3 (quicklz.c:197-494) and of the header rule
(3 bytes below 216, else 9; Go: always 9), with nothing taken from oracle/.  It is never the
expected value of a test: tests/test_encoder_cases.py asserts that it equals the oracle byte for
byte and uses it only to say WHICH decisions of the compressor a plaintext forces, so that the
GPU parity tests over tests/qlz_cases.py cannot pass vacuously.

Every position ip <= n - 11 is inserted into its bucket in order, so the table a position sees
is a function of the input before it: with r earlier positions in its bucket, the slots read are
the min(r mod 256, 16) most recent of them (the counter is one byte, quicklz.c:316-331).

  parse(data)             -> (core or None, Report)  the core loop, once
  finish(data, core, margins, bias) -> stream        header rule and bail-out bias (9 = Go's rule)
  compress(data, bias=0)  -> (stream, Report)        the two together
  Report.ev       Counter of events at item starts (names below); item starts at three zero
                  bytes are left out of ev, limits and viable
  Report.limits   the limits n - 4 - ip < 255 at which a taken match ended
  Report.viable   the numbers of candidates that could match (same 3 bytes, far enough back)
  Report.at       item start -> (rank in its bucket, candidates that could match, its events)
  Report.margins  (ip - (ip >> 5)) - op at every tested control word, the failing one included
  Report.stored, Report.repeat_share
  walker_rounds(data)     -> (rounds, notes)         the segment-walker scheme of k_encode_wg

Events:
  wrap_hides       the counter has wrapped (r >= 256), fewer than 16 slots are read and a slot
                   not read holds a longer match than the one taken; wrap_hides_0: none is read
  tie              two or more read candidates share the best length (the later one wins)
  evicted          the first occurrence of these 3 bytes has left the 16-slot ring;
                   evicted_literal: and nothing read matches, so a literal is emitted
  collision        a read slot holds other 3 bytes
  minoffset        a read candidate with the same 3 bytes is refused by o + 2 >= ip
  far_reject       the best candidate lies 131071 or more back, so a literal is emitted;
                   far_reject_nearer: while a nearer, shorter one was read
  limit_cut        a taken match ended at limit = n - 4 - ip < 255 with the source going on
  long_recent_wins two or more candidates agree through byte 6 and the most recent of them wins
  long_older_wins  ... and an older, strictly longer one wins
  long_over_short  the winner agrees through byte 6 and a more recent candidate does not
"""
from __future__ import annotations

from collections import Counter

import numpy as np

BUCKETS, SLOTS, TAIL, MAX_OFFSET = 4096, 16, 10, 131071


class Table:
    """The buckets of a plaintext: positions in insertion order, and each position's rank."""

    def __init__(self, data: bytes):
        n = len(data)
        self.P = P = max(0, n - TAIL)           # main-loop positions: ip <= n - 11
        a = np.frombuffer(data, np.uint8).astype(np.uint32)
        f = a[:P] | (a[1:P + 1] << 8) | (a[2:P + 2] << 16) if P else np.zeros(0, np.uint32)
        h = ((f >> 12) ^ f) & (BUCKETS - 1)
        order = np.argsort(h, kind="stable")
        start = np.searchsorted(h[order], np.arange(BUCKETS))
        rank = np.empty(P, np.int64)
        rank[order] = np.arange(P) - start[h[order]]
        self.f, self.h, self.rank = f.tolist(), h.tolist(), rank.tolist()
        self.order, self.start = order.tolist(), start.tolist()
        _, first = np.unique(f, return_index=True)
        self.first = {self.f[i]: i for i in first.tolist()}
        self.repeat_share = 1.0 - len(first) / P if P else 0.0


def _mlen(data: bytes, o: int, ip: int, limit: int) -> int:
    a, b = data[o + 3:o + limit], data[ip + 3:ip + limit]
    if a == b:
        return limit
    x = int.from_bytes(a, "little") ^ int.from_bytes(b, "little")
    return 3 + (((x & -x).bit_length() - 1) >> 3)


def search(data: bytes, tb: Table, ip: int, ev: Counter | None = None, rep=None):
    """(length, position) of the match the loop finds at ip (0, 0: none), events into ev."""
    n = len(data)
    f, h, r = tb.f[ip], tb.h[ip], tb.rank[ip]
    quiet = ev is None or f == 0                 # runs of zeros are the carrier of the planted cases:
    c = r & 255                                  # their events would drown the planted ones
    vis = min(c, SLOTS)
    limit = min(255, n - 4 - ip)
    base = tb.start[h] + r
    order, grams = tb.order, tb.f
    best, bpos, hidden_best = 0, 0, 0
    cands, evs = [], []                          # (length, position), most recent first; event names
    for d in range(1, min(r, SLOTS) + 1):
        o = order[base - d]
        same = grams[o] == f
        if d > vis:
            if not quiet and same and o + 2 < ip:
                hidden_best = max(hidden_best, _mlen(data, o, ip, limit))
            continue
        if not same:
            evs.append("collision")
            continue
        if o + 2 >= ip:
            evs.append("minoffset")
            continue
        m = _mlen(data, o, ip, limit)
        cands.append((m, o))
        if m > best or (m == best and o > bpos):
            best, bpos = m, o
    if quiet:
        return best, bpos
    rep.viable.add(len(cands))
    if r >= 256 and c < SLOTS and hidden_best > best:
        evs.append("wrap_hides")
        if c == 0:
            evs.append("wrap_hides_0")
    if sum(m == best for m, _ in cands) >= 2:
        evs.append("tie")
    if tb.rank[tb.first[f]] < r - SLOTS:
        evs.append("evicted")
        if not best:
            evs.append("evicted_literal")
    if best and ip - bpos >= MAX_OFFSET:
        evs.append("far_reject")
        if any(ip - o < MAX_OFFSET for _, o in cands):
            evs.append("far_reject_nearer")
    elif best:
        if best == limit and limit < 255 and data[bpos + limit] == data[ip + limit]:
            evs.append("limit_cut")
            rep.limits.add(limit)
        if limit > 7 and best >= 7:
            longs = [o for m, o in cands if m >= 7]
            if len(longs) >= 2:
                evs.append("long_recent_wins" if bpos == longs[0] else "long_older_wins")
            if any(m < 7 and o > bpos for m, o in cands):
                evs.append("long_over_short")
    ev.update(evs)
    rep.at[ip] = (r, len(cands), sorted(set(evs)))
    return best, bpos


class Report:
    def __init__(self):
        self.ev, self.limits, self.viable, self.margins = Counter(), set(), set(), []
        self.stored, self.repeat_share = False, 0.0
        self.at = {}                             # item start -> (rank, candidates that could match, events)


def _token(ml: int, off: int) -> bytes:
    if ml == 3 and off <= 63:
        return bytes([off << 2])
    if ml == 3 and off <= 16383:
        return ((off << 2) | 1).to_bytes(2, "little")
    if ml <= 18 and off <= 1023:
        return (((ml - 3) << 2) | (off << 6) | 2).to_bytes(2, "little")
    if ml <= 33:
        return (((ml - 2) << 2) | (off << 7) | 3).to_bytes(3, "little")
    return (((ml - 3) << 7) | (off << 15) | 3).to_bytes(4, "little")


def _header(hdr: int, compressed: bool, csize: int, dsize: int) -> bytes:
    b0 = (1 << 6) | (3 << 2) | int(compressed)
    if hdr == 3:
        return bytes([b0, csize, dsize])
    return bytes([b0 | 2]) + csize.to_bytes(4, "little") + dsize.to_bytes(4, "little")


def finish(data: bytes, core, margins, bias: int = 0) -> bytes:
    """The stream of a parse under the C rule (bias 0) or Go's (bias 9, quicklz.go:119).  The bias
    only moves the bail-out test, so one parse serves both rules: Go's stream is the plain core
    under a 9-byte header unless a margin below 9 occurred, and then the block is stored."""
    n = len(data)
    go = bias != 0
    hdr = 9 if go or n >= 216 else 3
    if core is None or any(m < bias for m in margins):
        return _header(hdr, False, n + hdr, n) + data
    if go and n < 5:
        core = core[:n + 4]                      # Go has no 9-byte core minimum
    return _header(hdr, True, len(core) + hdr, n) + core


def compress(data: bytes, bias: int = 0):
    """(stream, Report)."""
    if not data:
        return b"", Report()
    core, rep = parse(data)
    return finish(data, core, rep.margins, bias), rep


def parse(data: bytes):
    """(core or None when the block is left stored, Report): quicklz.c:197-494."""
    n = len(data)
    rep = Report()
    tb = Table(data)
    rep.repeat_share = tb.repeat_share
    out = bytearray(4)
    ip, cwpos, cw, nbits = 0, 0, 0, 0
    while ip < n:
        if nbits == 31:
            if ip < tb.P and ip > 3 * (n >> 2):   # quicklz.c:216-219
                margin = (ip - (ip >> 5)) - len(out)
                rep.margins.append(margin)
                if margin < 0:
                    rep.stored = True
                    return None, rep
            out[cwpos:cwpos + 4] = (cw | 0x80000000).to_bytes(4, "little")
            cwpos, cw, nbits = len(out), 0, 0
            out += bytes(4)
        ml = 0
        if ip < tb.P:
            ml, pos = search(data, tb, ip, rep.ev, rep)
            if ml < 3 or ip - pos >= MAX_OFFSET:
                ml = 0
        if ml:
            out += _token(ml, ip - pos)
            cw |= 1 << nbits
            ip += ml
        else:
            out.append(data[ip])
            ip += 1
        nbits += 1
    out[cwpos:cwpos + 4] = (cw | 0x80000000).to_bytes(4, "little")
    out += bytes(max(0, 9 - len(out)))           # quicklz.c:493
    return bytes(out), rep


def best_lengths(data: bytes) -> list:
    """The best length of every main-loop position (0: a literal), as phase 2 of k_encode_wg
    leaves it; only for blocks of the workgroup encoder (no offset limit below 65536)."""
    tb = Table(data)
    out = []
    for ip in range(tb.P):
        m, _ = search(data, tb, ip)
        out.append(m if m >= 3 else 0)
    return out


def walker_rounds(data: bytes, seg: int = 64):
    """Phase 3 of k_encode_wg restated: one walker per 64-position segment, each started at its
    segment's first position; then every segment whose entry (the exit of the segment before)
    changed is walked again from there, until no exit changes.  Returns (rounds, notes): rounds
    counts the passes in which an exit changed (the first pass included), notes holds 'cover'
    (an entry beyond the whole segment) and 'merge' (a new entry that the earlier walk of the
    segment had already passed through)."""
    n = len(data)
    L8 = best_lengths(data)
    P = len(L8)
    nseg = (n + seg - 1) // seg

    def walk(a, e0):
        seen, p = set(), a
        while p < e0:
            seen.add(p)
            p += (L8[p] if p < P else 0) or 1
        return p, seen

    frm = [seg * s for s in range(nseg)]
    res = [walk(seg * s, min(n, seg * s + seg)) for s in range(nseg)]
    ex, bits = [r[0] for r in res], [r[1] for r in res]
    rounds, notes = 1, set()
    while True:
        changed, new = False, list(ex)
        for s in range(1, nseg):
            entry = ex[s - 1]
            if entry == frm[s]:
                continue
            e0 = min(n, seg * s + seg)
            if entry >= e0:
                notes.add("cover")
                nx, bits[s] = entry, set()
            elif entry > frm[s] and entry in bits[s]:
                notes.add("merge")
                nx, bits[s] = ex[s], {p for p in bits[s] if p >= entry}
            else:
                nx, bits[s] = walk(entry, e0)
            frm[s] = entry
            if nx != ex[s]:
                new[s], changed = nx, True
        ex = new
        if not changed:
            return rounds, notes
        rounds += 1
