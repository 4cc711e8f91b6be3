"""Plaintexts built to force each decision of the level-3 compressor -- TEST INFRASTRUCTURE ONLY.

The encoder tests elsewhere feed natural data and leave it to chance whether a given decision
of qlz_compress_core (quicklz.c:197-494) occurs.  Every case here plants one: a match at a token
form's edge, a match cut by the end of the block, a hash counter that has wrapped, a tie, an
evicted slot, a bail-out test that passes with nothing to spare.  The cases are deterministic
(their random bytes come from their names), named, and grouped in families;
tests/test_encoder_cases.py shows with the instrumented model (tests/qlz_model.py) and the
disassembler (tests/qlz_asm.py) that each decision really occurs, and
tests/test_gpu_encoder_cases.py sends every case to every encoder.

How things are planted.  The carrier is compressible so the block is not left stored: runs of
zeros (one bucket, matches of 255), and where literals are wanted, filler bytes 0x03..0x7F.
Planted strings use bytes 0x80..0xFF, so their 3-grams occur nowhere else.  A planted source is
preceded by 0x01 and followed by 0x02, its repeat is preceded by zeros (or filler) and followed
by another byte, so the match can neither start earlier nor run on.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import qlz_asm
import qlz_model
from qlz_asm import XorShift64, name_seed
from oracle import oracle as O

# name: unique; family; plain: bytes; tags: what the builder meant to plant (the census checks it)
Case = namedtuple("Case", "name family plain tags")


def size_class(n: int):
    """The encoder size class of a block: the smallest workgroup kernel that takes it, or huge."""
    return 4096 if n <= 4096 else 16384 if n <= 16384 else 65536 if n <= 65536 else "huge"


class Plain:
    def __init__(self, name: str):
        self.name = name
        self.rng = XorShift64(name_seed(name))
        self.b = bytearray()

    def __len__(self):
        return len(self.b)

    def zeros(self, k: int):
        self.b += bytes(max(k, 0))

    def filler(self, k: int):
        """Bytes of 0x03..0x7F: literals, with the odd accidental 3-byte match."""
        self.b += bytes(3 + x % 125 for x in self.rng.bytes(k))

    def rand(self, k: int):
        self.b += self.rng.bytes(k)

    def high(self, k: int) -> bytes:
        """k bytes of 0x80..0xFF with no 3-gram twice (not appended)."""
        while True:
            s = bytes(0x80 | x for x in self.rng.bytes(k))
            if len({s[i:i + 3] for i in range(k - 2)}) == max(k - 2, 0):
                return s

    def put(self, s: bytes):
        self.b += s

    def source(self, s: bytes):
        self.put(b"\x01" + s + b"\x02")

    def done(self, family: str, **tags) -> Case:
        return Case(self.name, family, bytes(self.b), tags)


def text(seed: int, n: int) -> bytes:
    return O.gen_text(seed, n, n)


def items_of(plain: bytes):
    return qlz_asm.disassemble(O.compress(plain))[1]


def _item_index(plain: bytes, ip: int):
    """Index of the item that starts at ip in the oracle's parse (None: stored, or no item there)."""
    items = items_of(plain)
    if items is None:
        return None
    for j, it in enumerate(items):
        if it[0] == ip:
            return j
    return None


# ------------------------------------------------------------------ token_edges ----
def _pair(name, L, off, bit=None, n=None, lead=40, family="token_edges"):
    """One match (L, off) on a zero carrier, its item at bit `bit` of its control word.
    Layout: zeros | pad literals | 01 S 02 | zeros | S 03 | zeros | tail."""
    assert off >= L + 2
    for pad in range(0, 62):
        p = Plain(name)
        s = p.high(L)
        if n:
            _front(p, n, lead + pad + L + 2 + off - L - 1 + L + 1 + 74)
        p.zeros(lead)
        p.filler(pad)
        p.source(s)
        p.zeros(off - L - 1)
        at = len(p)
        p.put(s + b"\x03")
        p.zeros(60)
        p.filler(14)
        j = _item_index(bytes(p.b), at)
        if bit is None or (j is not None and j % 31 == bit):
            return p.done(family, match=(L, off), at=at, bit=bit)
    raise AssertionError(name)


def _repeat300(name, bit=None, n=None, family="token_edges"):
    """A 300-byte repeat 352 back: a match of 255 and one of 45."""
    for pad in range(62):
        p = Plain(name)
        s = p.high(300)
        if n:
            _front(p, n, 40 + pad + 302 + 50 + 301 + 74)
        p.zeros(40)
        p.filler(pad)
        p.source(s)
        p.zeros(50)
        at = len(p)
        p.put(s + b"\x03")
        p.zeros(60)
        p.filler(14)
        j = _item_index(bytes(p.b), at)
        if bit is None or (j is not None and j % 31 == bit):
            return p.done(family, split=(at, 255, 45), at=at, bit=bit)
    raise AssertionError(name)


BITS = (0, 30, 15)   # the item's place in its control word: first, last (31st), in the middle


def token_edges():
    """One planted match per case at the (length, offset) pairs where the token form changes
    (quicklz.c:377-406), each as the first, the last and a middle item of its control word (the
    32nd item of one word is the first of the next)."""
    out = []
    pairs = [(3, 63), (3, 64), (3, 16383), (3, 16384)]
    pairs += [(L, off) for L in range(4, 19) for off in (1023, 1024)]
    pairs += [(18, 40), (19, 40), (33, 50), (34, 50), (33, 2000), (34, 2000), (254, 300), (255, 300)]
    for L, off in pairs:
        for bit in BITS:
            out.append(_pair(f"token_edges/len{L}_off{off}_bit{bit}", L, off, bit))
    for bit in BITS:                                   # a 300-byte repeat: 255 + 45
        out.append(_repeat300(f"token_edges/repeat300_bit{bit}", bit))
    for period in (1, 2, 3):                           # overlapping runs; period 3 is offset 3, the minimum
        for run in (7, 40, 300):
            p = Plain(f"token_edges/period{period}_run{run}")
            unit = p.high(3)[:period]
            p.zeros(40)
            p.filler(5 + period)
            at = len(p)
            p.put((unit * (run // period + 1))[:run] + b"\x03")
            p.zeros(60)
            p.filler(14)
            out.append(p.done("token_edges", period=period, run=run, at=at))
    # the same at the larger classes, the match in the last quarter
    for n in (16384, 65536):
        for L, off in ((3, 64), (18, 1023), (19, 40), (34, 50), (255, 300)):
            out.append(_pair(f"token_edges/n{n}_len{L}_off{off}", L, off, None, n=n))
    return out


# ------------------------------------------------------------------ tail_edges ----
def tail_edges():
    """A repeat that runs to the end of the block: the match taken at ip ends at
    limit = n - 4 - ip (quicklz.c:310) for every limit 7..12 (ip <= n - 11, so 7 is the least:
    the `limit > 7` split of the kernel's first pass is 7 against 8); a repeat that starts at
    n - 10 (not searched) and one inside the last 10 bytes; n = 215, 216, 217 for the header
    switch, sizes of 300 to 700, limits 7 and 8 at the ends of the two larger workgroup classes
    and every limit again at 70001 bytes, for the whole-GPU encoder."""
    out = []
    for n in (215, 216, 217, 300, 431, 700, 16384, 65536, 70001):
        for back in list(range(11, 17)) + [10, 6]:    # the repeat starts at n - back
            if n > 700 and back not in ((11, 12, 10) if n <= 65536 else (11, 12, 13, 14, 15, 16, 10)):
                continue
            p = Plain(f"tail_edges/n{n}_start{back}")
            s = p.high(40)
            p.zeros(60)
            p.source(s)
            p.zeros(n - back - len(p))
            at = len(p)
            p.put(s[:back])
            assert len(p) == n
            out.append(p.done("tail_edges", at=at, limit=back - 4 if back >= 11 else None))
    return out


# ------------------------------------------------------------------ table_edges ----
def collider(g: bytes) -> bytes:
    """Other 3 bytes with the same hash_func value: the hash xors bits 4-7 of byte 0 with bits
    0-3 of byte 2 (quicklz.c:70), so flipping bit 4 of byte 0 and bit 0 of byte 2 cancels."""
    return bytes([g[0] ^ 0x10, g[1], g[2] ^ 0x01])


def _hash(g: bytes) -> int:
    f = g[0] | g[1] << 8 | g[2] << 16
    return ((f >> 12) ^ f) & 4095


def _copies(p: Plain, g: bytes, k: int, start: int = 0):
    """k insertions into g's bucket: g and two bytes that number the copy."""
    for i in range(start, start + k):
        p.put(g + bytes([3 + i % 120, 3 + i // 120]))


def _front(p: Plain, n: int, body: int):
    """Zeros and text in front so that a body of `body` bytes ends a block of n bytes."""
    pad = n - body - len(p)
    if pad > 0:
        t = min(pad - pad // 3, 4000 if n > 65536 else pad)   # over 64 KiB: mostly zeros, to keep the model quick
        p.zeros(pad - t)
        p.put(text(name_seed(p.name) & 0xFFFF, t))


def _wrap(name, r, n=None):
    """The probe g X is an item start at rank r of g's bucket; the copy of rank r - c - 1
    (c = r mod 256), the most recent slot NOT read, holds g X."""
    c = r & 255
    hid = r - c - 1 if c < 16 else r - 16
    body = 40 + 5 * (r - 1) + 15 + 3 + 16 + 74
    for attempt in range(20):                          # until no other 3 bytes fall into g's bucket
        p = Plain(f"{name}#{attempt}")
        g, x = p.high(3), p.high(12)
        if n:
            _front(p, n, body)
        p.zeros(40)
        _copies(p, g, hid)
        p.put(g + x)
        _copies(p, g, r - hid - 1, hid + 1)
        p.put(b"\x7d\x7e\x7f")
        at = len(p)
        p.put(g + x + b"\x03")
        p.zeros(60)
        p.filler(14)
        assert n is None or len(p) == n, (name, len(p))
        if qlz_model.Table(bytes(p.b)).rank[at] == r:
            return p.done("table_edges", wrap_rank=r, at=at)._replace(name=name)
    raise AssertionError(name)


def _two_sources(name, kind, between=0, n=None):
    """Sources of g X and then the probe g X, for a tie, an eviction or a collision; drawn again
    until the probe's rank in g's bucket is the number of insertions planted (no other 3 bytes
    fell into the bucket), so that `between` is exact."""
    for attempt in range(20):
        p = Plain(f"{name}#{attempt}")
        g, x = p.high(3), p.high(10)
        if n:
            _front(p, n, 400)
        start = len(p)
        p.zeros(40)
        if kind == "tie":                              # two sources of the same length: the later wins
            p.source(g + x + b"\x10")
            p.filler(9)
            p.source(g + x + b"\x11")
            rank = 2
        elif kind == "tie3":                           # four of the same length, the oldest running on otherwise
            p.source(g + x + p.high(4))
            for k in range(3):
                p.filler(5)
                p.source(g + x[:6] + bytes([0x10 + k]))
            rank = 4
        elif kind == "evict":                          # `between` insertions after the source
            p.source(g + x)
            _copies(p, g, between)
            rank = between + 1
        elif kind == "collision":
            g2 = collider(g)
            assert g2 != g and _hash(g2) == _hash(g) and min(g2) >= 0x80
            p.source(g2 + x)
            p.filler(7)
            rank = 1
        p.filler(6)
        at = len(p)
        p.put(g + (x[:6] + b"\x13" if kind == "tie3" else x) + b"\x03")
        p.zeros(60)
        p.filler(14)
        if n:
            p.zeros(start + 400 - len(p))
            p.filler(10)
            assert len(p) == n + 10
            del p.b[n:]
        if qlz_model.Table(bytes(p.b)).rank[at] == rank:
            return p.done("table_edges", kind=kind, between=between, at=at)._replace(name=name)
    raise AssertionError(name)


def table_edges():
    """The 16-slot ring and its byte-wide counter: reads after the counter has wrapped (ranks
    256, 257, 271 hide a longer match; 272 hides nothing; 512 + 5), ties, a source evicted by
    exactly 16 later insertions (15: still there; 17), a slot holding other bytes of the same
    hash, and candidates refused by o + 2 >= ip (the runs of token_edges have them too)."""
    out = []
    for r in (256, 257, 271, 272, 517):
        out.append(_wrap(f"table_edges/wrap_rank{r}", r))
    for kind in ("tie", "tie3", "collision"):
        out.append(_two_sources(f"table_edges/{kind}", kind))
    for between in (15, 16, 17):
        out.append(_two_sources(f"table_edges/evict_{between}", "evict", between))
    p = Plain("table_edges/minoffset")
    h = p.high(1)
    p.zeros(40)
    p.filler(8)
    p.put(h * 9 + b"\x03")
    p.zeros(60)
    p.filler(14)
    out.append(p.done("table_edges", kind="minoffset"))
    for n in (16384, 65536):
        out.append(_wrap(f"table_edges/n{n}_wrap_rank257", 257, n))
        out.append(_wrap(f"table_edges/n{n}_wrap_rank256", 256, n))
        for kind in ("tie", "collision"):
            out.append(_two_sources(f"table_edges/n{n}_{kind}", kind, n=n))
        out.append(_two_sources(f"table_edges/n{n}_evict_16", "evict", 16, n=n))
    return out


# ---------------------------------------------------------------- compact_edges ----
BANDS = {"lt20": (0.0, 0.20, range(3, 20)), "35_55": (0.35, 0.55, (45,)), "gt70": (0.70, 1.0, (75,))}


def _compact(name, n, band, counts):
    """Mostly random bytes behind a run of zeros (the repeat share is about the zeros' share of
    the block: the least that keeps the block compressed for the band below 20 %); for every k
    of `counts`, k sources g X[:i] with different i and then the probe g X: k candidates that
    can match, of differing lengths, two of them equal (a tie) -- and the longest are the oldest."""
    lo, hi, pcts = BANDS[band]
    tries = 0
    for zero_pct in [q for q in pcts for _ in range(3)]:   # up to three draws each: a probe whose bucket
        tries += 1                                         # took other bytes in between sees fewer
        p = Plain(f"{name}#{tries}")
        z = n * zero_pct // 100
        p.zeros(z)
        room = (n - z - 20) // len(counts)
        ats = []
        for k in counts:
            end = len(p) + room
            g, x = p.high(3), p.high(k + 8)
            for i in range(k):
                ln = k + 4 - i if i != 1 else k + 4  # the longest first; the second ties with it
                p.put(b"\x01" + g + x[:ln] + b"\x02")
                p.rand(3)
            p.rand(5)
            ats.append(len(p))
            p.put(g + x + b"\x03")
            p.rand(max(0, end - len(p)))
        p.rand(n - len(p))
        assert len(p) == n, (name, len(p))
        plain = bytes(p.b)
        if is_stored(O.compress(plain)) or not lo <= qlz_model.Table(plain).repeat_share < hi:
            continue
        seen = qlz_model.compress(plain)[1].at
        if [seen.get(at, (0, 0))[1] for at in ats] == list(counts):
            return p.done("compact_edges", counts=counts, band=band, ats=ats)._replace(name=name)
    raise AssertionError(name)


def compact_edges():
    """The switch of the kernel's compact candidate loop (kMatchCompactMax = 10 candidates that
    can match, wave-uniform): positions with 9, 10, 11 and 16 such candidates of differing
    lengths, in blocks whose 3-gram repeat share is below 20 %, 35-55 % and above 70 %."""
    out = []
    for n in (4096, 16384, 65536):
        for band in BANDS:
            for counts in ((9,), (10,), (11,), (16,), (9, 10, 11, 16)):
                if (n > 4096) == (len(counts) == 1):   # 4096: one count per block; above: all four
                    continue
                out.append(_compact(f"compact_edges/n{n}_share{band}_k{'_'.join(map(str, counts))}", n, band, counts))
    return out


# ---------------------------------------------------------------- parse_rounds ----
def _run_in_text(name, n, run, at_frac=0.7, seed=77):
    """Text with a run of one high byte of `run` bytes: the walkers that start inside the run
    jump 255 from their own start, the true path from the run's start, and each round corrects
    one more segment."""
    p = Plain(name)
    t = text(seed, n)
    a = (int(n * at_frac) & ~63) + 1
    p.put(t[:a])
    p.put(p.high(1) * run)
    p.put(t[a:n - run])
    return p.done("parse_rounds", run=run)


def _alphabet_in_text(name, n, seed, seg=2048):
    """Text with `seg` random bytes of a two-letter alphabet (0x80, 0x81) in it: many matches of
    middling length whose ends depend on where the walk entered."""
    p = Plain(name)
    t = text(79, n)
    a = (n - seg) // 2 & ~63
    rng = XorShift64(seed)
    p.put(t[:a])
    p.put(bytes(0x80 | x & 1 for x in rng.bytes(seg)))
    p.put(t[a:n - seg])
    return p.done("parse_rounds", seed=seed)


# run lengths (found with qlz_model.walker_rounds, which the census repeats) per target round count
PARSE_RUNS = (258, 267, 384)      # 1 round (the match ends the run), 4 and 5
PARSE_SEEDS = (5, 35)             # 2 and 3 rounds


def parse_rounds():
    """Blocks on which the segment-walker scheme of k_encode_wg (64-position segments, re-walked
    when their entry changes) needs 1, 2, 3, 4 and more than 4 rounds: kParseRounds = 4 sends
    the last two to the serial item walk.  Text needs one; a run of one byte in it adds one round
    per segment whose walker started inside the run, more than 255 bytes from its end."""
    out = []
    for n in (4096, 16384, 65536):
        out.append(Case(f"parse_rounds/n{n}_text", "parse_rounds", text(78, n), {}))
        for run in PARSE_RUNS:
            out.append(_run_in_text(f"parse_rounds/n{n}_run{run}", n, run))
        for seed in PARSE_SEEDS:
            out.append(_alphabet_in_text(f"parse_rounds/n{n}_alphabet{seed}", n, seed))
        out.append(Case(f"parse_rounds/n{n}_zeros", "parse_rounds", bytes(n), {}))
    return out


# ------------------------------------------------------------------ bail_edges ----
def _noise_prefix(t: bytes, noise: bytes, k: int) -> bytes:
    return noise[:k] + t[k:]


def _noise_perm(t: bytes, noise: bytes, perm, k: int) -> bytes:
    b = bytearray(t)
    for i in perm[:k]:
        b[i] = noise[i]
    return bytes(b)


def _permutation(rng: XorShift64, n: int):
    perm = list(range(n))
    for i in range(n - 1, 0, -1):
        j = rng.below(i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def is_stored(stream: bytes) -> bool:
    return not stream[0] & 1


@functools.lru_cache(maxsize=None)
def bail_family(kind: str, n: int, seed: int, go: bool = False):
    """make(k) of a one-parameter family, and its flip: the k (found by bisection with the
    oracle, under Go's rule with `go`) at which make(k) is compressed and make(k + 1) is stored."""
    comp = O.compress_go if go else O.compress
    rng = XorShift64(name_seed(f"bail/{kind}/{n}/{seed}"))
    t = text(1000 + seed, n)
    noise = rng.bytes(n)
    if kind == "prefix":
        def make(k):
            return _noise_prefix(t, noise, k)
    else:
        perm = _permutation(rng, n)

        def make(k):
            return _noise_perm(t, noise, perm, k)
    lo, hi = 0, n
    assert not is_stored(comp(make(lo))) and is_stored(comp(make(hi)))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if is_stored(comp(make(mid))):
            hi = mid
        else:
            lo = mid
    return make, lo


BAIL_SIZES = (300, 4096, 16384, 40000, 65536, 65537, 70000)
# (kind, n): two of the seeds 0..15.  The compressed neighbour of the first passes the bail-out
# test with margin 0 at the first tested control word; that of the second with a margin of 1..8
# ('prefix': compressed by the C rule, stored by Go's) or, for 'perm', with margin 0 at a later word.
BAIL_SEEDS = {("prefix", 300): (0, 4), ("prefix", 4096): (2, 0), ("prefix", 16384): (7, 2),
              ("prefix", 40000): (5, 1), ("prefix", 65536): (2, 4), ("prefix", 65537): (0, 2),
              ("prefix", 70000): (4, 1), ("perm", 300): (1, 14), ("perm", 4096): (6, 0), ("perm", 16384): (2, 7),
              ("perm", 40000): (2, 0), ("perm", 65536): (1, 0), ("perm", 65537): (2, 3), ("perm", 70000): (3, 0)}


# the same under Go's rule: the neighbour Go still compresses passes with margin exactly 9
BAIL_SEEDS_GO = {("prefix", 300): 1, ("prefix", 4096): 4, ("prefix", 16384): 3, ("prefix", 65536): 0,
                 ("prefix", 70000): 7, ("perm", 4096): 0, ("perm", 16384): 2, ("perm", 65536): 0, ("perm", 70000): 0}


def bail_edges():
    """One-parameter families bisected with the oracle to the stored / compressed flip; both
    neighbours are kept.  'prefix': text whose first k bytes are random; 'perm': text with the
    first k positions of a fixed permutation made random (a repeat share near the prefix-first
    pass's threshold).  The compressed neighbour passes quicklz.c:218 narrowly: the seeds are
    chosen so that for every size one passes with margin 0.  The flip under Go's rule
    (quicklz.go:119 counts the 9-byte header) is kept as well, with margin exactly 9."""
    out = []
    for kind in ("prefix", "perm"):
        for n in BAIL_SIZES:
            for seed in BAIL_SEEDS[kind, n]:
                make, k = bail_family(kind, n, seed)
                for d in (0, 1):
                    out.append(Case(f"bail_edges/{kind}_n{n}_seed{seed}_k{k + d}", "bail_edges", make(k + d),
                                    dict(kind=kind, flip=d)))
    for (kind, n), seed in BAIL_SEEDS_GO.items():
        make, k = bail_family(kind, n, seed, True)
        for d in (0, 1):
            out.append(Case(f"bail_edges/go_{kind}_n{n}_seed{seed}_k{k + d}", "bail_edges", make(k + d),
                            dict(kind=kind, go_flip=d)))
    return out


# ------------------------------------------------------------------ huge_edges ----
def _far(name, off, nearer=False):
    """A 12-byte repeat `off` back across zeros; with `nearer`, also a 5-byte one 500 back."""
    p = Plain(name)
    s = p.high(12)
    p.zeros(3000)
    p.put(text(5, 3000))
    p.source(s)
    a = len(p) - 13
    p.zeros(off - 13 - (507 if nearer else 0))
    if nearer:
        p.source(s[:5])
        p.zeros(500)
    at = len(p)
    assert at - a == off, (at - a, off)
    p.put(s + b"\x03")
    p.zeros(3000)
    p.put(text(6, 1000))
    return p.done("huge_edges", far=off, at=at, nearer=nearer)


# every pair at which the token form changes, but of (L, 1023 / 1024) only L = 4 and 18
HUGE_PAIRS = [(3, 63), (3, 64), (3, 16383), (3, 16384), (4, 1023), (4, 1024), (18, 1023), (18, 1024), (18, 40),
              (19, 40), (33, 50), (34, 50), (33, 2000), (34, 2000), (254, 300), (255, 300)]


def huge_edges():
    """Over 64 KiB, for the whole-GPU encoder: repeats 131069..131072 back (131070 is the last
    offset taken, quicklz.c:361), the longest one out of reach while a nearer, shorter one is
    there; 65537 and 65547 bytes, 65545 and 65546, 131081 and 131082 (he_levels steps at 65536 and
    131072 main-loop positions, n - 10); the token-form edges of token_edges and the counter
    ranks 256, 257, 271 and 272 of table_edges planted beyond position 65536.  The bail-out
    families of bail_edges at 65537 and 70000 bytes and the cut limits of tail_edges at 70001
    come here as well."""
    out = []
    for off in (131069, 131070, 131071, 131072):
        out.append(_far(f"huge_edges/far{off}", off))
    for off in (131070, 131071):
        out.append(_far(f"huge_edges/far{off}_nearer", off, nearer=True))
    for n in (65537, 65545, 65546, 65547, 131081, 131082):
        out.append(Case(f"huge_edges/text_n{n}", "huge_edges", text(9, n), {}))
    for L, off in HUGE_PAIRS:                          # the shared token table (match_token), its own emission
        out.append(_pair(f"huge_edges/len{L}_off{off}", L, off, None, n=70000 + L, family="huge_edges"))
    out.append(_repeat300("huge_edges/repeat300", None, n=70300, family="huge_edges"))
    for r in (256, 257, 271, 272):
        out.append(_wrap(f"huge_edges/wrap_rank{r}", r, 70000)._replace(family="huge_edges"))
    for kind in ("tie", "collision"):
        out.append(_two_sources(f"huge_edges/{kind}", kind, n=66000)._replace(family="huge_edges"))
    return out


FAMILIES = {"token_edges": token_edges, "tail_edges": tail_edges, "table_edges": table_edges,
            "compact_edges": compact_edges, "parse_rounds": parse_rounds, "bail_edges": bail_edges,
            "huge_edges": huge_edges}


@functools.lru_cache(maxsize=None)
def collection() -> tuple:
    out = []
    for fn in FAMILIES.values():
        out += fn()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)
