"""A hand assembler for QuickLZ level-3 streams -- TEST INFRASTRUCTURE ONLY.

Pure Python, no code shared with oracle/: the five token encodings of quicklz.c:579-610 are
written out here from the format, items are packed 31 to a control word, and the assembler
keeps the plaintext it builds.  That plaintext is the expected output of every decoder and
depends on none of them.

  Asm(name)            one stream under construction; its random bytes come from the name
    .lit(byte)         a literal
    .match(form, off, ml)   a match, form 'A'..'E'
    .finish(dsize)     literals up to dsize
    .stream(short_header=False, junk=0, pad=b"\0")   the bytes; refuses a stream that breaks C3 or C4
  pack(items, dsize, ...)   the same packing without any check: what the mutations use
  MUTATIONS            one edit each to a valid stream, giving an invalid one
  collection()         every valid stream of the families below, built once
  invalid_collection() the invalid ones
  disassemble(stream)  (dsize, items, bail-out margins) of a valid stream: what an encoder decided
  replay(stream, items)   the plaintext from a disassembly

The forms (t is the little-endian token, tl its bytes):
  A  tl 1  t & 3 == 0                  off = t >> 2         (0..63)      ml = 3
  B  tl 2  t & 3 == 1                  off = t >> 2         (0..16383)   ml = 3
  C  tl 2  t & 3 == 2                  off = t >> 6         (0..1023)    ml = (t >> 2 & 15) + 3   (3..18)
  D  tl 3  t & 3 == 3, t & 127 != 3    off = t >> 7         (0..131071)  ml = (t >> 2 & 31) + 2   (3..33)
  E  tl 4  t & 127 == 3                off = t >> 15        (0..131071)  ml = (t >> 7 & 255) + 3  (3..258)

A stream is valid (checks C1-C5 of oracle/qlz_oracle.c:166-179) when every match has
3 <= off <= op and op + ml + 4 <= dsize (C3), no match follows the first literal at
op >= dsize - 11 (C4), and the stream ends with the item that completes dsize, but for the zero
padding up to the 9-byte core minimum (C5).
"""
from __future__ import annotations

import functools
from collections import namedtuple

M64 = (1 << 64) - 1

# form: (token bytes, largest offset, smallest length, largest length)
FORMS = {"A": (1, 63, 3, 3), "B": (2, 16383, 3, 3), "C": (2, 1023, 3, 18), "D": (3, 131071, 3, 33),
         "E": (4, 131071, 3, 258)}
LEN_EDGES = {"A": [3], "B": [3], "C": [3, 4, 17, 18], "D": [3, 18, 19, 33], "E": [3, 33, 34, 255, 256, 257, 258]}
TAIL = 11  # a literal at op >= dsize - TAIL starts the literal tail


class XorShift64:
    """Marsaglia's xorshift64 (13, 7, 17): the same streams on every Python."""

    def __init__(self, seed: int):
        self.s = (seed & M64) or 0x9E3779B97F4A7C15

    def next(self) -> int:
        s = self.s
        s ^= (s << 13) & M64
        s ^= s >> 7
        s ^= (s << 17) & M64
        self.s = s
        return s

    def below(self, n: int) -> int:
        return self.next() % n

    def between(self, lo: int, hi: int) -> int:
        return lo + self.next() % (hi - lo + 1)

    def bytes(self, n: int) -> bytes:
        return b"".join(self.next().to_bytes(8, "little") for _ in range((n + 7) // 8))[:n]

    def log_between(self, lo: int, hi: int) -> int:
        """An integer of [lo, hi], its bit length drawn uniformly (no floating point)."""
        k = self.between(lo.bit_length(), hi.bit_length())
        return self.between(max(lo, 1 << (k - 1)), min(hi, (1 << k) - 1))


def name_seed(name: str) -> int:
    h = 0xCBF29CE484222325  # FNV-1a 64
    for c in name.encode():
        h = ((h ^ c) * 0x100000001B3) & M64
    return h


def encode(form: str, off: int, ml: int) -> bytes:
    """The token of a match; only the form's own field ranges are asserted."""
    tl, off_max, ml_min, ml_max = FORMS[form]
    assert 0 <= off <= off_max and ml_min <= ml <= ml_max, (form, off, ml)
    if form == "A":
        t = off << 2
    elif form == "B":
        t = (off << 2) | 1
    elif form == "C":
        t = ((ml - 3) << 2) | (off << 6) | 2
    elif form == "D":
        t = ((ml - 2) << 2) | (off << 7) | 3
    else:
        t = ((ml - 3) << 7) | (off << 15) | 3
    return t.to_bytes(tl, "little")


# tok: the item's stream bytes; op: where its output starts; ml: output bytes (1 for a literal)
Item = namedtuple("Item", "tok is_match op ml form off")


def lit_item(byte: int, op: int) -> Item:
    return Item(bytes([byte]), False, op, 1, None, 0)


def match_item(form: str, off: int, ml: int, op: int) -> Item:
    return Item(encode(form, off, ml), True, op, ml, form, off)


def pack(seq, dsize: int, short_header: bool = False, junk: int = 0, trailer: bytes = b"",
         csize: int | None = None, pad: bytes = b"\0") -> bytes:
    """Header + control words + items, with no validity check.  `seq` holds Items and runs of
    literal bytes.  31 items per control word, bit 31 set on each; the last word's bits above its
    last item come from `junk`; zeros (or `pad`, repeated) pad the core to 9 bytes; `trailer`
    follows the last item; `csize` cuts (and declares) the stream there."""
    core = bytearray()
    pos, cw, k = -1, 0, 31

    def new_word():
        nonlocal pos, cw, k
        if pos >= 0:
            core[pos:pos + 4] = cw.to_bytes(4, "little")
        pos, cw, k = len(core), 0x80000000, 0
        core.extend(bytes(4))

    for e in seq:
        if isinstance(e, Item):
            if k == 31:
                new_word()
            cw |= int(e.is_match) << k
            core += e.tok
            k += 1
            continue
        i = 0
        while i < len(e):                       # a run of literals: bit 0 each
            if k == 31:
                new_word()
            n = min(31 - k, len(e) - i)
            core += e[i:i + n]
            k += n
            i += n
    if pos >= 0:
        cw |= junk & 0x7FFFFFFF & ~((1 << k) - 1)
        core[pos:pos + 4] = cw.to_bytes(4, "little")
    core += trailer
    core += (pad * 9)[:max(0, 9 - len(core))]
    hdr = 3 if short_header else 9
    n = hdr + len(core) if csize is None else csize
    if short_header:
        assert n <= 255 and dsize <= 255, (n, dsize)
        head = bytes([0x4D, n, dsize])           # 01 00 11 0 1: level 3, compressed
    else:
        head = bytes([0x4F]) + n.to_bytes(4, "little") + dsize.to_bytes(4, "little")
    return (head + bytes(core))[:n]


class Asm:
    def __init__(self, name: str):
        self.name = name
        self.rng = XorShift64(name_seed(name))
        self.seq: list = []          # match Items and bytearray runs of literals, in stream order
        self.nitems = 0
        self.plain = bytearray()

    @property
    def op(self) -> int:
        return len(self.plain)

    @property
    def items(self) -> list[Item]:
        """One Item per item of the stream (the runs of literals spelled out)."""
        out, op = [], 0
        for e in self.seq:
            if isinstance(e, Item):
                out.append(e)
                op += e.ml
            else:
                out += [lit_item(b, op + k) for k, b in enumerate(e)]
                op += len(e)
        return out

    def _run(self, data: bytes):
        if not data:
            return
        if not self.seq or isinstance(self.seq[-1], Item):
            self.seq.append(bytearray())
        self.seq[-1] += data
        self.plain += data
        self.nitems += len(data)

    def lit(self, byte: int):
        self._run(bytes([byte]))

    def lits(self, n: int):
        self._run(self.rng.bytes(n))

    def match(self, form: str, off: int, ml: int):
        op = self.op
        if not 3 <= off <= op:
            raise ValueError(f"{self.name}: offset {off} at op {op} breaks C3")
        self.seq.append(match_item(form, off, ml, op))
        self.nitems += 1
        seg = self.plain[op - off:op - off + ml]
        if off < ml:                            # overlapping: the forward byte copy repeats the last `off` bytes
            seg = (seg * (ml // off + 1))[:ml]
        self.plain += seg

    def fill_to(self, target: int):
        """Filler up to op == target: short literal runs and form-E matches of random offset and
        length, so the text stays aperiodic while the stream stays small."""
        rng = self.rng
        while self.op < target:
            rem = target - self.op
            if self.op < 3 or rem < 3:
                self.lits(min(rem, 3))
                continue
            self.lits(min(rem, rng.between(1, 6)))
            rem = target - self.op
            if rem >= 3:
                self.match("E", rng.log_between(3, min(self.op, 131071)), min(rem, rng.between(3, 258)))

    def finish(self, dsize: int):
        assert dsize >= self.op, (self.name, dsize, self.op)
        self.lits(dsize - self.op)

    def check(self):
        dsize, tail, op = self.op, False, 0
        if dsize < 1:
            raise ValueError(f"{self.name}: empty")
        for e in self.seq:
            if isinstance(e, Item):
                if tail:
                    raise ValueError(f"{self.name}: match at op {e.op} after the tail began (C4)")
                if e.op != op or not 3 <= e.off <= op or op + e.ml + 4 > dsize:
                    raise ValueError(f"{self.name}: match at op {op} breaks C3")
                op += e.ml
            else:
                op += len(e)
                tail = tail or op - 1 >= dsize - TAIL
        assert op == dsize

    def stream(self, short_header: bool = False, junk: int = 0, pad: bytes = b"\0") -> bytes:
        self.check()
        return pack(self.seq, self.op, short_header, junk, pad=pad)


# ------------------------------------------------------------------ valid families ----
# name: unique; family: the row of the table below; stream / plain: bytes; asm: the Asm (items)
Case = namedtuple("Case", "name family stream plain asm")


def _case(family: str, a: Asm, **kw) -> Case:
    return Case(a.name, family, a.stream(**kw), bytes(a.plain), a)


S_OFFSETS = [3, 4, 63, 64, 255, 256, 257, 1023, 1024]


def forms_s():
    """dsize <= 4 KiB.  Every form at every offset of S_OFFSETS it can hold and every length edge:
    after a literal, twice in a row (a token of <= 3 bytes shares a dword with the next token's
    first byte) and behind a 1-byte token (so a 4-byte token is the second of such a pair)."""
    out, i = [], 0
    for form in "ABCDE":
        for off in S_OFFSETS:
            if off > FORMS[form][1]:
                continue
            for ml in LEN_EDGES[form]:
                a = Asm(f"forms_S/{form}_off{off}_len{ml}")
                a.lits(off + i % 7)
                a.match(form, off, ml)
                a.lits(1 + i % 3)
                a.match(form, off, ml)
                a.match(form, off, ml)
                a.lits(1)
                a.match("A", 3, 3)
                a.match(form, off, ml)
                a.match("A", 3, 3)
                a.lits(2)
                a.match(form, off, ml)
                a.finish(a.op + 12 + i % 5)
                assert a.op <= 4096
                out.append(_case("forms_S", a))
                i += 1
    return out


M_OFFSETS = [3583, 3584, 3585, 3840, 4095, 4096, 4097, 16383, 16384, 65000]


def forms_m():
    """dsize exactly 65536.  Forms B, D, E at the offsets around K2's 4 KiB window less its
    256-byte marker ring (3840), around the window (4096) and the 2-byte form's limit, at 65000
    and at the largest offset that fits; lengths 3 and the form's largest.  Each match stands once
    at op == off (the C3 boundary) and once later.  The largest offset is off == op with the
    match ending 4..26 bytes before the block end: op within 64 bytes of the end, except for a
    258-byte match, which cannot start closer than 262 bytes before it."""
    out, i = [], 0
    for form in "BDE":
        for ml in sorted({3, FORMS[form][3]}):
            for off in M_OFFSETS + ["max"]:
                if off != "max" and off > FORMS[form][1]:
                    continue
                a = Asm(f"forms_M/{form}_off{off}_len{ml}")
                if off == "max":
                    if FORMS[form][1] < 65536:
                        continue
                    at = 65536 - 4 - ml - (i * 7) % 23
                    a.fill_to(at - 40)
                    a.match("E", 7, 40)                # no literal from dsize - 11 on ahead of the match
                    a.match(form, at, ml)
                else:
                    a.fill_to(off)
                    a.match(form, off, ml)
                    reps = min(2, (65536 - 24 - a.op) // ml)   # none behind a 258-byte match at 65000
                    a.fill_to(min(off + 300 + (65536 - 700 - off) * (i % 5) // 5, 65536 - 24 - reps * ml))
                    for _ in range(reps):
                        a.match(form, off, ml)
                    a.fill_to(65536 - 24)
                    a.match("E", 5, 8)
                a.finish(65536)
                out.append(_case("forms_M", a))
                i += 1
    return out


L_OFFSETS = [65535, 65536, 65537, 131070, 131071]
L_DSIZE = 143360


def forms_l():
    """About 140 KiB.  Forms D and E at the offsets around 2^16 and at the format's largest."""
    out, i = [], 0
    for form in "DE":
        for ml in (3, FORMS[form][3]):
            for off in L_OFFSETS:
                a = Asm(f"forms_L/{form}_off{off}_len{ml}")
                a.fill_to(off)
                a.match(form, off, ml)                 # off == op
                a.fill_to(off + 700 + 1000 * (i % 7))
                a.match(form, off, ml)
                a.match(form, off, ml)
                a.fill_to(L_DSIZE - 24)
                a.match("E", 5, 8)
                a.finish(L_DSIZE)
                out.append(_case("forms_L", a))
                i += 1
    return out


C_DMODS = [0, 1, 254, 255]


def chunk_cover():
    """Form E, lengths 256-258 (no encoder emits them): the only items that cover a whole aligned
    256-byte chunk of K2 with no marker inside.  Starts at d mod 256 in C_DMODS; sources 3, 255,
    256, 257 bytes back (inside the LDS window) and more than 4096 back (from HBM)."""
    out = []

    def next_at(op, dmod, least):
        d = max(op, least)
        return d + (dmod - d) % 256

    for ml in (256, 257, 258):
        for dmod in C_DMODS:
            for off in (3, 255, 256, 257):
                a = Asm(f"chunk_cover/1536_len{ml}_d{dmod}_off{off}")
                a.fill_to(next_at(0, dmod, max(off, 1)))
                a.match("E", off, ml)
                a.fill_to(1536 - 16)
                a.finish(1536)
                out.append(_case("chunk_cover", a))
    for bs in (20480, 65536):
        for ml in (256, 257, 258):
            for off in (3, 255, 256, 257, 4097) + ((40000,) if bs == 65536 else ()):
                a = Asm(f"chunk_cover/{bs}_len{ml}_off{off}")
                rounds = 0
                while a.op < bs - 4096 and (bs == 65536 or rounds < 3):
                    for dmod in C_DMODS:
                        a.fill_to(next_at(a.op + (rounds % 2), dmod, off))
                        a.match("E", off, ml)
                    rounds += 1
                a.fill_to(next_at(a.op, 0, off))       # back to back: a marker at slot 0 only
                for _ in range(3):
                    a.match("E", off, 256)
                a.fill_to(next_at(a.op, 255, off))     # ... and at slot 255 only
                for _ in range(3):
                    a.match("E", off, 256)
                assert a.op < bs - 16
                a.fill_to(bs - 16)
                a.finish(bs)
                out.append(_case("chunk_cover", a))
    return out


def groups():
    """Control words of 31 four-byte tokens (128 stream bytes, the longest group) and of 31
    one-byte tokens (35, the shortest a group of matches can be; 31 literals are as long), and
    streams of exactly 31 and 62 items: no partial last word."""
    out = []
    for tag, dsize, lens in (("E258", 65536, (258, 258)), ("E3_258", 32768, (3, 258)), ("E3", 3000, (3, 3)),
                             ("E258_s", 16384, (258, 258))):
        a = Asm(f"groups/{tag}")
        a.lits(31)
        while a.op + 258 + 4 + 31 <= dsize:
            a.match("E", a.rng.log_between(3, a.op), a.rng.between(*lens))
        a.lits(-a.nitems % 31)                     # the tail starts a control word
        a.finish(dsize)
        out.append(_case("groups", a))
    for tag, dsize in (("A", 2000), ("A_l", 16384)):
        a = Asm(f"groups/{tag}")
        a.lits(31)
        while a.op + 3 + 4 + 31 <= dsize:
            a.match("A", a.rng.between(3, min(63, a.op)), 3)
        a.finish(dsize)
        out.append(_case("groups", a))
    for n in (31, 62):
        for form, off, ml in (("A", 3, 3), ("C", 7, 18), ("E", 9, 258)):
            a = Asm(f"groups/items{n}_{form}")
            a.lits(9)
            while a.nitems < n - 12:
                a.match(form, off, ml)
                if a.nitems % 3 == 0 and a.nitems < n - 12:
                    a.lits(1)
            a.lits(n - a.nitems)
            assert a.nitems == n == len(a.items)
            out.append(_case("groups", a))
            if a.op <= 255 and len(a.stream()) - 6 <= 255:
                out.append(Case(a.name + "_short", "groups", a.stream(short_header=True), bytes(a.plain), a))
    return out


JUNKS = (0x7FFFFFFF, 0x55555555)
PADS = (b"\xff", b"\x03", b"\x01", b"\x00\xff")   # first bytes of a 3-, 4- and 2-byte token; a 1-byte one, then a cut one


def lastword():
    """Set bits in the last control word above the item that completes dsize: never looked at by
    a decoder that stops at op == dsize.  Last groups of 1, 5 and 30 items, behind zero, one and
    two full groups; and the streams of dsize 1, 3 and 4, whose core is padded with zeros to 9
    bytes, so the junk bits stand over the padding.  The padding is whatever the encoder's
    destination held (quicklz.c:493 only moves the end), so besides zeros the padded streams come
    with the bytes of PADS there: read as tokens, they run past csize."""
    out = []
    for junk in JUNKS:
        for short in (False, True):
            tag = f"junk{junk:08x}_{'short' if short else 'long'}"
            for dsize in (1, 3, 4):                    # padded: 4 + dsize < 9
                a = Asm(f"lastword/padded_d{dsize}_{tag}")
                a.lits(dsize)
                out.append(_case("lastword", a, short_header=short, junk=junk))
                for pad in PADS:
                    b = Asm(f"lastword/padded_d{dsize}_pad{pad.hex()}_{tag}")
                    b.lits(dsize)
                    out.append(_case("lastword", b, short_header=short, junk=junk, pad=pad))
            for n in (5, 30, 32, 36, 61, 63, 67, 92):  # not padded
                a = Asm(f"lastword/items{n}_{tag}")
                if n > 22:                             # room for two matches ahead of the tail
                    a.lits(8)
                    a.match("C", 5, 9)
                    a.match("A", 3, 3)
                a.lits(n - a.nitems)
                assert a.nitems == n == len(a.items)
                out.append(_case("lastword", a, short_header=short, junk=junk))
    return out


def tail():
    """C3 and C4 at their edges: a match ending at dsize - 4; a literal at dsize - 12 (not yet the
    tail) followed by a match of 3..7 bytes; and every dsize 1..15 as a compressed stream under
    both headers (a match is possible from dsize 14 on)."""
    out = []
    for form in "ABCDE":
        for ml in sorted({3, FORMS[form][3]}):
            a = Asm(f"tail/end4_{form}_len{ml}")
            a.lits(40)
            a.match("E", 30, 90)                       # no literal from dsize - 11 on but the last four
            a.match(form, 37, ml)                      # op + ml + 4 == dsize
            a.finish(a.op + 4)
            out.append(_case("tail", a))
    for form in "ABCDE":
        for ml in range(3, 8):
            if ml > FORMS[form][3]:
                continue
            a = Asm(f"tail/lit12_{form}_len{ml}")
            a.lits(50)
            a.match("D", 20, 33)
            a.lits(1)                                  # at dsize - 12
            a.match(form, 11, ml)                      # at dsize - 11
            a.finish(a.op + 11 - ml)
            assert [(it.op, it.is_match) for it in a.items if it.op >= a.op - 12][:2] == [(a.op - 12, False), (a.op - 11, True)]
            out.append(_case("tail", a))
    for short in (False, True):
        for dsize in range(1, 16):
            a = Asm(f"tail/d{dsize}_{'short' if short else 'long'}")
            a.lits(dsize)
            out.append(_case("tail", a, short_header=short))
        for dsize, ml in ((14, 3), (14, 7), (15, 3), (15, 8)):
            a = Asm(f"tail/d{dsize}_match{ml}_{'short' if short else 'long'}")
            a.lits(3)
            a.match("C", 3, ml)
            a.finish(dsize)
            out.append(_case("tail", a, short_header=short))
    return out


N_RANDOM = 200


def random_streams():
    """N_RANDOM streams: dsize in five classes (<= 300, <= 4 KiB, <= 32 KiB, exactly 65536,
    70-140 KiB); forms uniform, offsets log-uniform in [3, min(op, form max)], lengths uniform
    over the form's range, literal runs of 0..40 items."""
    out = []
    for i in range(N_RANDOM):
        a = Asm(f"random/{i:03d}")
        rng = a.rng
        cls = i % 5
        dsize = (rng.between(1, 300), rng.between(301, 4096), rng.between(4097, 32768), 65536,
                 rng.between(70 << 10, 140 << 10))[cls]
        while True:
            run = rng.below(41)
            if a.op + run > dsize - TAIL:              # a literal of the run would start the tail
                break
            a.lits(run)
            form = "ABCDE"[rng.below(5)]
            _, off_max, ml_min, ml_max = FORMS[form]
            room = dsize - 4 - a.op
            if a.op < 3 or room < 3:
                a.lits(1)
                continue
            a.match(form, rng.log_between(3, min(a.op, off_max)), min(room, rng.between(ml_min, ml_max)))
        a.finish(dsize)
        short = bool(i & 1) and dsize <= 255 and len(a.stream()) - 6 <= 255
        out.append(_case("random", a, short_header=short))
    return out


FAMILIES = {"forms_S": forms_s, "forms_M": forms_m, "forms_L": forms_l, "chunk_cover": chunk_cover,
            "groups": groups, "lastword": lastword, "tail": tail, "random": random_streams}


@functools.lru_cache(maxsize=None)
def collection() -> tuple:
    """Every valid case, family by family; names are unique."""
    out = []
    for fn in FAMILIES.values():
        out += fn()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# ---------------------------------------------------------------- invalid streams ----
# Each mutation makes ONE edit to a valid long-header stream and returns the invalid stream, or
# None when the stream has no place for that edit.  The status every decoder owes is E_CORRUPT.
def _matches(items):
    return [j for j, it in enumerate(items) if it.is_match]


def _replace(items, dsize, j: int, it: Item) -> bytes:
    return pack(items[:j] + [it] + items[j + 1:], dsize)


def mut_off_op_plus_1(items, dsize):
    """C3: a match reaching one byte before the block start (offset op + 1)."""
    for j in reversed(_matches(items)):               # the last match whose form can hold it
        it = items[j]
        if it.op + 1 <= FORMS[it.form][1]:
            return _replace(items, dsize, j, match_item(it.form, it.op + 1, it.ml, it.op))
    return None


def _mut_off_small(form: str, off: int):
    def mut(items, dsize):
        for j in _matches(items):
            it = items[j]
            if it.form == form:
                return _replace(items, dsize, j, match_item(form, off, it.ml, it.op))
        return None
    mut.__doc__ = f"C3: offset {off} in the first match of form {form}."
    return mut


def mut_end_plus_1(items, dsize):
    """C3: op + len + 4 == dsize + 1 -- a match, then three literals and the end.  The last match
    with no literal in the 11 bytes before the new end ahead of it (C4 stays kept), else the last."""
    ms = _matches(items)
    j = ms[-1]
    for k in reversed(ms):
        it = items[k]
        lo = it.op + it.ml + 3 - TAIL
        if all(p.is_match for p in items[max(0, k - 12):k] if p.op >= lo):
            j = k
            break
    it = items[j]
    return pack(items[:j + 1] + [lit_item(0x41 + k, it.op + it.ml + k) for k in range(3)], it.op + it.ml + 3)


def mut_match_in_tail(items, dsize):
    """C4: the literal at dsize - 11 starts the tail; the three literals after it become one
    match (form A, offset 3), which obeys C3 and leaves every length as it was."""
    if len(items) < 12 or any(it.is_match for it in items[-11:]) or items[-11].op != dsize - 11:
        return None
    return pack(items[:-10] + [match_item("A", 3, 3, dsize - 10)] + items[-7:], dsize)


def mut_trailing_byte(items, dsize):
    """C5: one byte after the item that completes dsize."""
    return pack(items, dsize, trailer=b"\0")


def mut_trailing_word(items, dsize):
    """C5: an empty control word (bit 31 only) after the last item."""
    return pack(items, dsize, trailer=(0x80000000).to_bytes(4, "little"))


def mut_second_word_no_sentinel(items, dsize):
    """C1: the second control word without bit 31."""
    if len(items) <= 31:
        return None
    s = bytearray(pack(items, dsize))
    x = 9 + 4 + sum(len(it.tok) for it in items[:31])
    s[x + 3] &= 0x7F
    return bytes(s)


def mut_cut_last_token(items, dsize):
    """C2: csize ends the stream inside the last match token (before it when it has one byte)."""
    j = _matches(items)[-1]
    x = 9 + 4 * (j // 31 + 1) + sum(len(it.tok) for it in items[:j])
    return pack(items, dsize, csize=x + len(items[j].tok) - 1)


MUTATIONS = {"off_op+1": mut_off_op_plus_1, "end+1": mut_end_plus_1, "match_in_tail": mut_match_in_tail,
             "trailing_byte": mut_trailing_byte, "trailing_word": mut_trailing_word,
             "word2_no_bit31": mut_second_word_no_sentinel, "cut_last_token": mut_cut_last_token}
for _f in "ABCDE":
    for _o in (0, 1, 2):
        MUTATIONS[f"off{_o}_{_f}"] = _mut_off_small(_f, _o)

INVALID_FAMILIES = ("forms_S", "forms_M", "forms_L")


@functools.lru_cache(maxsize=None)
def invalid_collection() -> tuple:
    """(name, kind, family, stream, dsize) of every invalid case: each mutation applied to the
    first and the last stream of every form in forms_S, forms_M and forms_L, where it has a place."""
    out = []
    for fam in INVALID_FAMILIES:
        by_form = {}
        for c in collection():
            if c.family == fam:
                by_form.setdefault(c.name.split("/")[1][0], []).append(c)
        bases = [c for cs in by_form.values() for c in (cs[0], cs[-1])]
        for c in bases:
            items = c.asm.items
            for kind, mut in MUTATIONS.items():
                s = mut(items, len(c.plain))
                if s is not None:
                    out.append(Invalid(f"{c.name}~{kind}", kind, fam, s, int.from_bytes(s[5:9], "little")))
    return tuple(out)


Invalid = namedtuple("Invalid", "name kind family stream dsize")


# ------------------------------------------------------------------ disassembler ----
def disassemble(stream: bytes):
    """(dsize, items, tests) of a valid level-3 stream -- what an encoder decided, read back.

    items: (ip, form_bytes, length, offset) per item, ip the plaintext position it starts at;
           a literal is (ip, 0, 1, 0).  None for a stored stream.
    tests: one margin for every control word but the first that the encoder's main loop starts
           (ip <= dsize - 11) past three quarters of the input (ip > 3 * (dsize >> 2)): the places
           where quicklz.c:218 compares.  margin = (ip - (ip >> 5)) - op, op the core offset of
           that control word (0 = the first byte after the header); the block stays compressed
           while every margin is >= 0 (>= 9 under Go's rule, which counts the header)."""
    s = stream
    hdr = 9 if s[0] & 2 else 3
    csize, dsize = ((int.from_bytes(s[1:5], "little"), int.from_bytes(s[5:9], "little")) if hdr == 9
                    else (s[1], s[2]))
    assert csize == len(s) and (s[0] >> 2) & 3 == 3, "not a whole level-3 stream"
    if not s[0] & 1:
        return dsize, None, []
    items, tests = [], []
    x, ip, cw, first = hdr, 0, 1, True
    while ip < dsize:
        if cw == 1:
            if not first and ip <= dsize - 11 and ip > 3 * (dsize >> 2):
                tests.append((ip - (ip >> 5)) - (x - hdr))
            first = False
            cw = int.from_bytes(s[x:x + 4], "little")
            assert cw >> 31
            x += 4
        if cw & 1:
            b0 = s[x]
            tl = 1 if b0 & 3 == 0 else 2 if b0 & 3 != 3 else 3 if b0 & 127 != 3 else 4
            t = int.from_bytes(s[x:x + tl], "little")
            off, ml = ((t >> 2, 3) if tl == 1 or t & 3 == 1 else (t >> 6, (t >> 2 & 15) + 3) if tl == 2 else
                       (t >> 7, (t >> 2 & 31) + 2) if tl == 3 else (t >> 15, (t >> 7 & 255) + 3))
            items.append((ip, tl, ml, off))
            ip += ml
            x += tl
        else:
            items.append((ip, 0, 1, 0))
            ip += 1
            x += 1
        cw >>= 1
    assert ip == dsize and (x == csize or (x < hdr + 9 and csize == hdr + 9))
    return dsize, items, tests


def replay(stream: bytes, items) -> bytes:
    """The plaintext from a disassembly: literals are read from the stream in item order."""
    hdr = 9 if stream[0] & 2 else 3
    out, x = bytearray(), hdr
    for k, (ip, tl, ml, off) in enumerate(items):
        if k % 31 == 0:
            x += 4
        assert ip == len(out)
        if tl == 0:
            out.append(stream[x])
            x += 1
        else:
            seg = out[ip - off:ip - off + ml]
            out += seg if off >= ml else (seg * (ml // off + 1))[:ml]
            x += tl
    return bytes(out)
