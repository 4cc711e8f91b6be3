"""TEST INFRASTRUCTURE ONLY: quicklz.go level 1, transliterated line for line into plain Python.

Nothing here comes from oracle/ or from the kernels.  `decompress` is quicklz.go:291-431 and
`compress` is quicklz.go:80-191 plus the shared tail 266-288, with the level-3 arms left out.
Every `source[...]` and `destination[...]` access of the decoder goes through `_Slice`, which
raises where the index lies outside [0, len) as a Go slice does: a panic is the wrapper's
IndexError, not a check placed here.  The statements keep Go's shape (fastRead as its own loop,
the three unrolled copies, then i = 3..matchlen-1), so the panic happens at the same access.

The model is never the expected value of a GPU test.  tests/test_go_l1_cases.py proves it equal
to the oracle over the whole collection of tests/go_l1_cases.py; its `Report` then says which
panic site or which decision a case reaches, so that a pass on the GPU cannot be vacuous.

`fill` is not Go: it is the byte the destination holds before decoding (Go: 0).  Decoding with
another value shows whether a stream's result depends on make([]byte, size) zero-filling.
"""
from __future__ import annotations

from collections import Counter
from dataclasses import dataclass, field

OK, E_CORRUPT, E_LEVEL, E_HEADER = 0, 2, 3, 6      # include/qlzx.h status codes

HASH_VALUES = 4096
MINOFFSET = 2
UNCONDITIONAL_MATCHLEN = 6
UNCOMPRESSED_END = 4
CWORD_LEN = 4
DEFAULT_HEADERLEN = 9

# decoder panic sites, in the order of quicklz.go:291-431
SITES = ("header", "cword", "fetch_cword", "len_byte", "match_copy", "rehash_first", "rehash_loop",
         "fetch_match", "literal", "literal_ahead", "tail")

DEC_EVENTS = ("short_len_3", "short_len_17", "long_len_0", "long_len_1", "long_len_2", "long_len_3",
              "long_len_17", "long_len_18", "long_len_255", "unwritten_bucket", "overlap",
              "rehash_past_dst", "fetch_never_loaded", "stale_fetch", "tail_cword_skip",
              "stored_short_body", "header3")

ENC_EVENTS = ("counter0", "collision", "minoffset_1", "minoffset_2", "rle_taken", "rle_lits01", "rle_lits2",
              "rle_src3", "rle_m3", "rle_m2", "rle_m1", "rle_p1", "rle_p2", "len_3", "len_4", "len_5",
              "len_6", "len_17", "len_18", "len_255", "cut_by_remaining", "last_cword_full", "stored")


@dataclass
class Report:
    site: str | None = None                        # the site that panicked, None when none did
    events: Counter = field(default_factory=Counter)
    # encoder, at every full control word: (src - 3*(len>>2), (src - (src>>5)) - dst)
    margins: list = field(default_factory=list)
    cut: list = field(default_factory=list)        # encoder: len-4-src of every match it cut
    rle: list = field(default_factory=list)        # encoder, where src == o+1: (lits, src, the five byte tests)


class _Slice:
    """A Go []byte: indexing outside [0, len) panics."""

    def __init__(self, data):
        self.a = bytearray(data)

    def __len__(self):
        return len(self.a)

    def __getitem__(self, i):
        if i < 0 or i >= len(self.a):
            raise IndexError(i)
        return self.a[i]

    def __setitem__(self, i, v):
        if i < 0 or i >= len(self.a):
            raise IndexError(i)
        self.a[i] = v & 0xFF


def headerLen(source):
    if (source[0] & 2) == 2:
        return 9
    return 3


def fastRead(a, i, numbytes):
    l = 0
    for j in range(numbytes):
        l |= a[i + j] << (j * 8)
    return l


def SizeDecompressed(source):
    if headerLen(source) == 9:
        return fastRead(source, 5, 4)
    return fastRead(source, 2, 1)


def decompress(stream: bytes, fill: int = 0):
    """Go Decompress(stream) -> (status, bytes | None, Report)."""
    rep = Report()
    source = _Slice(stream)
    at = ["header"]                                # the site the next slice access belongs to
    try:
        out = _decompress(source, rep, at, fill)
    except IndexError:
        rep.site = at[0]
        return (E_HEADER if rep.site == "header" else E_CORRUPT), None, rep
    if out is None:
        return E_LEVEL, None, rep
    return OK, bytes(out), rep


def _decompress(source, rep, at, fill):
    ev = rep.events
    size = SizeDecompressed(source)
    src = headerLen(source)
    if src == 3:
        ev["header3"] += 1
    dst = 0
    cwordVal = 1
    destination = _Slice(bytes([fill]) * size)
    hashtable = [0] * 4096
    hashCounter = [0] * 4096
    lastMatchStart = size - UNCONDITIONAL_MATCHLEN - UNCOMPRESSED_END - 1
    lastHashed = -1
    fetch = 0
    fetch_at = None                                # the src whose bytes `fetch` holds; None: never loaded

    level = (source[0] >> 2) & 0x3

    if level != 1 and level != 3:
        return None                                # panic("Go version only supports level 1 and 3")

    if (source[0] & 1) != 1:
        body = source.a[headerLen(source):]
        if len(body) < size:
            ev["stored_short_body"] += 1
        k = min(size, len(body))                   # copy(d2, source[headerLen(source):])
        destination.a[:k] = body[:k]
        destination.a[k:] = bytes(size - k)        # d2 is a fresh make([]byte, size)
        return destination.a

    if level != 1:
        return None                                # a compressed level-3 stream is not this codec's

    while True:
        if cwordVal == 1:
            at[0] = "cword"
            cwordVal = fastRead(source, src, 4)
            src += 4
            if dst <= lastMatchStart:
                at[0] = "fetch_cword"
                fetch = fastRead(source, src, 3)
                fetch_at = src

        if (cwordVal & 1) == 1:
            cwordVal = cwordVal >> 1

            if fetch_at is None:
                ev["fetch_never_loaded"] += 1
            elif fetch_at != src:
                ev["stale_fetch"] += 1
            hash = (fetch >> 4) & 0xfff
            offset2 = hashtable[hash]
            if hashCounter[hash] == 0:
                ev["unwritten_bucket"] += 1

            if (fetch & 0xf) != 0:
                matchlen = (fetch & 0xf) + 2
                src += 2
                if matchlen in (3, 17):
                    ev["short_len_%d" % matchlen] += 1
            else:
                at[0] = "len_byte"
                matchlen = source[src + 2] & 0xff
                src += 3
                if matchlen in (0, 1, 2, 3, 17, 18, 255):
                    ev["long_len_%d" % matchlen] += 1
            if offset2 + matchlen > dst:
                ev["overlap"] += 1

            at[0] = "match_copy"
            destination[dst + 0] = destination[offset2 + 0]
            destination[dst + 1] = destination[offset2 + 1]
            destination[dst + 2] = destination[offset2 + 2]

            for i in range(3, matchlen):
                destination[dst + i] = destination[offset2 + i]
            dst += matchlen

            at[0] = "rehash_first"
            if lastHashed + 3 >= dst and lastHashed + 3 < size:
                ev["rehash_past_dst"] += 1
            fetch = fastRead(destination, lastHashed + 1, 3)
            while lastHashed < dst - matchlen:
                lastHashed += 1
                hash = ((fetch >> 12) ^ fetch) & (HASH_VALUES - 1)
                hashtable[hash] = lastHashed
                hashCounter[hash] = 1
                at[0] = "rehash_loop"
                if lastHashed + 3 >= dst and lastHashed + 3 < size:
                    ev["rehash_past_dst"] += 1
                fetch = (fetch >> 8 & 0xffff) | (destination[lastHashed + 3] << 16)
            at[0] = "fetch_match"
            fetch = fastRead(source, src, 3)
            fetch_at = src
            lastHashed = dst - 1
        else:
            if dst <= lastMatchStart:
                at[0] = "literal"
                destination[dst] = source[src]
                dst += 1
                src += 1
                cwordVal = cwordVal >> 1

                while lastHashed < dst - 3:
                    lastHashed += 1
                    fetch2 = fastRead(destination, lastHashed, 3)
                    hash = ((fetch2 >> 12) ^ fetch2) & (HASH_VALUES - 1)
                    hashtable[hash] = lastHashed
                    hashCounter[hash] = 1
                at[0] = "literal_ahead"
                fetch = fetch >> 8 & 0xffff | source[src + 2] << 16
                if fetch_at is not None:
                    fetch_at = src
            else:
                at[0] = "tail"
                while dst <= size - 1:
                    if cwordVal == 1:
                        src += CWORD_LEN
                        cwordVal = 0x80000000
                        ev["tail_cword_skip"] += 1

                    destination[dst] = source[src]
                    dst += 1
                    src += 1
                    cwordVal = cwordVal >> 1
                return destination.a


def _writeHeader(dst, level, compressible, sizeCompressed, sizeDecompressed):
    dst[0] = 2 | (1 if compressible else 0)
    dst[0] |= level << 2
    dst[0] |= 1 << 6
    _fastWrite(dst, 1, sizeDecompressed, 4)
    _fastWrite(dst, 5, sizeCompressed, 4)


def _fastWrite(a, i, value, numbytes):
    for j in range(numbytes):
        a[i + j] = (value >> (j * 8)) & 0xFF


def compress(data: bytes):
    """Go Compress(data, 1) -> (stream | None, Report)."""
    rep = Report()
    ev = rep.events
    source = _Slice(data)
    n = len(source)
    src = 0
    dst = DEFAULT_HEADERLEN + CWORD_LEN
    cwordVal = 0x80000000
    cwordPtr = DEFAULT_HEADERLEN
    destination = _Slice(bytes(n + 400))
    hashtable = [0] * HASH_VALUES
    cachetable = [0] * HASH_VALUES
    hashCounter = [0] * HASH_VALUES
    fetch = 0
    lastMatchStart = n - UNCONDITIONAL_MATCHLEN - UNCOMPRESSED_END - 1
    lits = 0

    if n == 0:
        return None, rep

    if src <= lastMatchStart:
        fetch = fastRead(source, src, 3)

    while src <= lastMatchStart:
        if (cwordVal & 1) == 1:
            # at src <= 3*(len>>2) Go's && never looks at dst; the margin is recorded all the same
            rep.margins.append((src - 3 * (n >> 2), (src - (src >> 5)) - dst))
            if src > 3 * (n >> 2) and dst > src - (src >> 5):
                d2 = _Slice(bytes(n + DEFAULT_HEADERLEN))
                _writeHeader(d2, 1, False, n, n + DEFAULT_HEADERLEN)
                d2.a[DEFAULT_HEADERLEN:] = source.a
                ev["stored"] += 1
                return bytes(d2.a), rep

            _fastWrite(destination, cwordPtr, (cwordVal >> 1) | 0x80000000, 4)
            cwordPtr = dst
            dst += CWORD_LEN
            cwordVal = 0x80000000

        hash = ((fetch >> 12) ^ fetch) & (HASH_VALUES - 1)
        o = hashtable[hash]
        cache = cachetable[hash] ^ fetch

        cachetable[hash] = fetch
        hashtable[hash] = src

        # the condition of quicklz.go:140, with each refusal counted where Go's && / || stops
        take = False
        if cache != 0:
            if hashCounter[hash] != 0:
                ev["collision"] += 1
        elif hashCounter[hash] == 0:
            ev["counter0"] += 1
        elif src - o > MINOFFSET:
            take = True
        else:
            ev["minoffset_%d" % (src - o)] += 1
            if src == o + 1:
                rep.rle.append((lits, src, tuple(src + k >= 0 and source[src] == source[src + k]
                                                 for k in (-3, -2, -1, 1, 2))))
                if not lits >= 3:
                    ev["rle_lits2" if lits == 2 else "rle_lits01"] += 1
                elif not src > 3:
                    ev["rle_src3"] += 1
                elif source[src] != source[src - 3]:
                    ev["rle_m3"] += 1
                elif source[src] != source[src - 2]:
                    ev["rle_m2"] += 1
                elif source[src] != source[src - 1]:
                    ev["rle_m1"] += 1
                elif source[src] != source[src + 1]:
                    ev["rle_p1"] += 1
                elif source[src] != source[src + 2]:
                    ev["rle_p2"] += 1
                else:
                    ev["rle_taken"] += 1
                    take = True
        if take:
            cwordVal = (cwordVal >> 1) | 0x80000000
            if source[o + 3] != source[src + 3]:
                f = 3 - 2 | (hash << 4)
                destination[dst + 0] = f >> (0 * 8)
                destination[dst + 1] = f >> (1 * 8)
                src += 3
                dst += 2
                ev["len_3"] += 1
            else:
                oldSrc = src
                remaining = 255
                ln = n - UNCOMPRESSED_END - src + 1 - 1
                if ln <= 255:
                    remaining = ln

                src += 4
                if source[o + src - oldSrc] == source[src]:
                    src += 1
                    if source[o + src - oldSrc] == source[src]:
                        src += 1
                        while source[o + (src - oldSrc)] == source[src] and (src - oldSrc) < remaining:
                            src += 1
                        if source[o + (src - oldSrc)] == source[src] and remaining < 255:
                            ev["cut_by_remaining"] += 1
                            rep.cut.append(ln)

                matchlen = src - oldSrc
                if matchlen in (4, 5, 6, 17, 18, 255):
                    ev["len_%d" % matchlen] += 1

                hash <<= 4
                if matchlen < 18:
                    f = hash | (matchlen - 2)
                    destination[dst + 0] = f >> (0 * 8)
                    destination[dst + 1] = f >> (1 * 8)
                    dst += 2
                else:
                    f = hash | (matchlen << 16)
                    _fastWrite(destination, dst, f, 3)
                    dst += 3
            lits = 0
            fetch = fastRead(source, src, 3)
        else:
            lits += 1
            hashCounter[hash] = 1
            destination[dst] = source[src]
            cwordVal = cwordVal >> 1
            src += 1
            dst += 1
            fetch = (fetch >> 8) & 0xffff | source[src + 2] << 16

    while src <= n - 1:
        if (cwordVal & 1) == 1:
            _fastWrite(destination, cwordPtr, (cwordVal >> 1) | 0x80000000, 4)
            cwordPtr = dst
            dst += CWORD_LEN
            cwordVal = 0x80000000

        destination[dst] = source[src]
        src += 1
        dst += 1
        cwordVal = cwordVal >> 1
    if (cwordVal & 1) == 1:
        ev["last_cword_full"] += 1
    while (cwordVal & 1) != 1:
        cwordVal = cwordVal >> 1
    _fastWrite(destination, cwordPtr, (cwordVal >> 1) | 0x80000000, CWORD_LEN)
    _writeHeader(destination, 1, True, n, dst)

    return bytes(destination.a[:dst]), rep
