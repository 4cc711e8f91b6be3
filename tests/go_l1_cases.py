"""TEST INFRASTRUCTURE ONLY: hand-assembled Go level-1 streams and plaintexts, one per decoder
branch, panic site or compressor decision of quicklz.go:80-191 and 291-431.

The level-1 stream format, as Decompress reads it:

  header   9 bytes: flags, compressed size (4, never read by Go), decompressed size (4);
           3 bytes when flags & 2 is clear: flags, compressed size, decompressed size.
           flags = 0x40 | level << 2 | 2 (9-byte header) | 1 (compressed)
  cword    4 bytes, little endian; bit k is item k: 1 a match token, 0 a literal byte.  The
           encoder fills 31 items and sets bit 31; the decoder reloads when the word is 1.
  match    short: 2 bytes, bucket << 4 | (len - 2), len 3..17
           long:  3 bytes, bucket << 4 (low nibble 0), then the length byte
           the source of the copy is the position the decoder last hashed into `bucket`
  literal  1 byte; the last 10 bytes of a block are always literals (the tail loop)

`collection()` returns the cases, each with a name and a family:

  panic_sites  pairs of neighbours: one panics at the site, the other gets past it
  odd_tokens   token forms no encoder emits, on streams that decode OK
  headers      header forms, levels, stored bodies, dst_cap
  zero_fill    streams whose result is mostly Go's make([]byte, size) zero-fill
  mutants      every truncation and single-bit flip of the small golden level-1 streams
  encoder      plaintexts, each built to force one decision of Compress(src, 1)

Two of the eleven sites cannot panic, and the collection has no case for them:
  literal       `destination[dst] = source[src]` runs only while dst <= lastMatchStart, and then
                the fetch before it (after the control word, the match or the literal before)
                has already read source[src + 2];
  rehash_first  fastRead(destination, lastHashed+1, 3) reads up to lastHashed + 3 <= dst + 2
                (lastHashed <= dst - 1 always), which the match copy just before it has written.
tests/test_go_l1_cases.py asserts that no case of any family, the 50,724 mutants included,
panics there.  Likewise, of the five byte comparisons of the RLE exception only source[src-3]
and source[src-2] can fail alone: cache == 0 with o == src - 1 already means that
source[src-1 .. src+2] are four equal bytes.

The bail-out pair was found by a search with the model over plaintexts of the shape built by
`_bail_plain`: margin 0 and margin -1 were both reached, so no weaker bar is recorded.
"""
from __future__ import annotations

import functools
import json
import os
import random
from dataclasses import dataclass

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MUTANT_MAX_INPUT = 300          # golden level-1 vectors whose input is at most this long
MUTANT_CAP_PAD = 64             # dst_cap of a mutant: the original size + this


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    stream: bytes | None = None         # decoder cases
    cap: int | None = None              # dst_cap; None: the size the header claims
    plain: bytes | None = None          # encoder cases
    site: str | None = None             # panic_sites: the site of the pair
    panics: bool = False                # panic_sites: this member panics there


# ---- the assembler ------------------------------------------------------------------------

def header(size: int, csize: int = 0, *, hdr: int = 9, level: int = 1, compressed: bool = True) -> bytes:
    flags = 0x40 | (level << 2) | (1 if compressed else 0) | (2 if hdr == 9 else 0)
    if hdr == 9:
        return bytes([flags]) + (csize & 0xFFFFFFFF).to_bytes(4, "little") + size.to_bytes(4, "little")
    return bytes([flags, csize & 0xFF, size])


def bucket(b3: bytes) -> int:
    """The bucket the decoder hashes a position into, from its three bytes."""
    f = b3[0] | (b3[1] << 8) | (b3[2] << 16)
    return ((f >> 12) ^ f) & 4095


def lit(bs: bytes) -> list:
    return [("L", bytes([b])) for b in bs]


def short(bkt: int, n: int) -> tuple:
    assert 3 <= n <= 17 and 0 <= bkt < 4096
    f = (bkt << 4) | (n - 2)
    return ("M", bytes([f & 0xFF, f >> 8]))


def long(bkt: int, n: int) -> tuple:
    assert 0 <= n <= 255 and 0 <= bkt < 4096
    f = bkt << 4
    return ("M", bytes([f & 0xFF, f >> 8, n]))


def body(items: list, cwords: dict | None = None) -> bytes:
    """Items in groups of 31 under one control word each: the item kinds in bits 0..30 and bit
    31 set, as the encoder leaves it.  cwords[k] replaces the k-th word."""
    out = bytearray()
    for k in range(0, max(len(items), 1), 31):
        group = items[k:k + 31]
        cw = 0x80000000 | sum(1 << i for i, (kind, _) in enumerate(group) if kind == "M")
        cw = (cwords or {}).get(k // 31, cw)
        out += cw.to_bytes(4, "little")
        for _, b in group:
            out += b
    return bytes(out)


def stream(size: int, items: list, *, cwords: dict | None = None, csize: int | None = None, **hdr) -> bytes:
    b = body(items, cwords)
    n = len(b) + (9 if hdr.get("hdr", 9) == 9 else 3)
    return header(size, n if csize is None else csize, **hdr) + b


def claimed_size(s: bytes) -> int:
    """SizeDecompressed, 0 where the header is too short to hold it."""
    if len(s) == 0 or len(s) < (9 if s[0] & 2 else 3):
        return 0
    return int.from_bytes(s[5:9], "little") if s[0] & 2 else s[2]


# ---- panic_sites --------------------------------------------------------------------------

ABC = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"


def _panic_sites() -> list:
    out = []

    def pair(site, tag, bad, good, ok=None):
        """`bad` panics at `site`; `good`, one source byte or one in the size field away, does
        not; `ok`, where `good` panics further on, is the whole stream, which decodes."""
        out.append(Case(f"{site}/{tag}/panics", "panic_sites", stream=bad, site=site, panics=True))
        out.append(Case(f"{site}/{tag}/passes", "panic_sites", stream=good, site=site))
        if ok is not None:
            out.append(Case(f"{site}/{tag}/ok", "panic_sites", stream=ok, site=site))

    stored0 = header(0, 9, compressed=False)
    pair("header", "h9_len8", stored0[:8], stored0)
    s3 = header(0, 3, hdr=3, compressed=False)
    pair("header", "h3_len2", s3[:2], s3)

    # the first control word of a size-0 stream, which then ends in the (empty) tail loop
    z = stream(0, [])
    pair("cword", "first", z[:-1], z)
    # the second control word, after 31 literals
    s = stream(42, lit(ABC[:42]))
    cut = 9 + 4 + 31
    pair("cword", "second", s[:cut + 3], s[:cut + 4], s)

    s = stream(20, lit(ABC[:20]))
    pair("fetch_cword", "first", s[:9 + 4 + 2], s[:9 + 4 + 3], s)
    s = stream(42, lit(ABC[:42]))            # dst = 31 = lastMatchStart at the second word
    pair("fetch_cword", "second", s[:cut + 4 + 2], s[:cut + 4 + 3], s)
    # the same bytes with size 41: dst = 31 is past lastMatchStart, no fetch, and the tail loop runs
    pair("fetch_cword", "size", stream(42, lit(ABC[:41]))[:cut + 4 + 2], stream(41, lit(ABC[:41]))[:cut + 4 + 2],
         stream(41, lit(ABC[:41])))

    # size < 11: fetch is never loaded and stays 0, so a match bit takes the long form and reads
    # source[src + 2] with nothing having read that far
    s = stream(5, [long(0, 3)] + lit(b"abc"))
    pair("len_byte", "never_loaded", s[:9 + 4 + 2], s[:9 + 4 + 3], s)

    # the write passes size while the read is in range: 10 literals, then a copy of 11 from 0
    pair("match_copy", "write_past_size",
         stream(20, lit(ABC[:10]) + [short(bucket(b"abc"), 11)] + lit(b"xyz")),
         stream(20, lit(ABC[:10]) + [short(bucket(b"abc"), 10)] + lit(b"xyz")))
    # offset2 + 2 >= size at dst = 0: the third unrolled copy, read and write at the same index
    pair("match_copy", "read_at_dst0", stream(2, [long(0, 0)] + lit(b"abc")), stream(3, [long(0, 0)] + lit(b"abc")))
    pair("match_copy", "long_17_of_16", stream(26, lit(ABC[:10]) + [long(bucket(b"abc"), 17)] + lit(b"xyz")),
         stream(26, lit(ABC[:10]) + [long(bucket(b"abc"), 16)] + lit(b"xyz")))

    # the loop's destination[lastHashed + 3]: after 10 literals and a match of 7, a match of 3
    # that ends at size re-hashes its first position, whose third-next byte is destination[size]
    pre = lit(ABC[:10]) + [short(bucket(b"abc"), 7)]
    bcd = bucket(b"bcd")
    for tag, tok in (("len3_ends_at_size", short(bcd, 3)), ("len0_at_size_minus_3", long(bcd, 0)),
                     ("len1_at_size_minus_3", long(bcd, 1)), ("len2_at_size_minus_3", long(bcd, 2))):
        pair("rehash_loop", tag, stream(20, pre + [tok] + lit(b"wxyz")), stream(21, pre + [tok] + lit(b"wxyz")))
    pair("rehash_loop", "size3_vs_4", stream(3, [long(0, 0)] + lit(b"abcd")), stream(4, [long(0, 0)] + lit(b"abcd")))
    # one source byte apart: the match before it one shorter, so that the match of 3 ends at size - 1
    pair("rehash_loop", "ends_at_size_vs_size_minus_1",
         stream(20, lit(ABC[:10]) + [short(bucket(b"abc"), 7), long(bucket(b"bcd"), 3)] + lit(b"wxyz")),
         stream(20, lit(ABC[:10]) + [short(bucket(b"abc"), 6), long(bucket(b"bcd"), 3)] + lit(b"wxyz")))

    s = stream(20, lit(ABC[:10]) + [short(bucket(b"abc"), 10)] + lit(b"xyz"))
    pair("fetch_match", "after_last_match", s[:-1], s)
    s = stream(20, lit(b"abcd") + [short(bucket(b"abc"), 4)] + lit(b"mnopqrstuvwx"))
    pair("fetch_match", "mid_stream", s[:9 + 4 + 4 + 2 + 2], s[:9 + 4 + 4 + 2 + 3], s)

    s = stream(20, lit(b"a") + [short(0, 3)] + lit(b"xyz"))
    pair("literal_ahead", "first", s[:9 + 4 + 3], s[:9 + 4 + 4])
    s = stream(20, lit(ABC[:20]))            # the look-ahead of the last literal before the tail loop
    pair("literal_ahead", "tenth", s[:9 + 4 + 12], s[:9 + 4 + 13], s)

    s = stream(5, lit(b"abcde"))
    pair("tail", "size5", s[:-1], s)
    s = stream(35, lit(ABC[:35]))            # the control word skipped inside the tail loop
    pair("tail", "after_skip", s[:-1], s)
    out.append(Case("tail/inside_skipped_word/panics", "panic_sites", stream=s[:9 + 4 + 31 + 2], site="tail",
                    panics=True))
    return out


# ---- odd_tokens ---------------------------------------------------------------------------

def _odd_tokens() -> list:
    out = []

    def add(name, s, cap=None):
        out.append(Case("odd/" + name, "odd_tokens", stream=s, cap=cap))

    abc = bucket(b"abc")
    tail10 = lit(b"0123456789")
    # token lengths, short and long form, copied from position 0 of 20 distinct literals
    for n in (3, 17):
        add(f"short_len_{n}", stream(20 + n + 10, lit(ABC[:20]) + [short(abc, n)] + lit(b"xyz") + tail10))
    for n in (3, 17, 18):
        add(f"long_len_{n}", stream(20 + n + 10, lit(ABC[:20]) + [long(abc, n)] + lit(b"xyz") + tail10))
    add("long_len_255", stream(300 + 255 + 10, lit((ABC * 5)[:300]) + [long(abc, 255)] + lit(b"xyz") + tail10))
    # long-form lengths 0, 1 and 2 at dst = 0 through a never-written bucket: the copy reads the
    # zero-filled destination[0..2], position 0 is hashed from those zeros into bucket 0, and
    # with 1 and 2 the zeros stay in the output.  Literals follow, then a match through bucket 0.
    # (With 0 the output is the same whatever the destination held: a never-written bucket reads
    # as position 0 as well.  The self_copy cases below make length 0 depend on the zero-fill.)
    for n in (0, 1, 2):
        add(f"long_len_{n}_dst0", stream(30, [long(77, n)] + lit(b"pqrstuvw") + [short(0, 5)] +
                                         lit(ABC[:30 - n - 8 - 5])))
    # the same lengths mid-stream: the copy leaves 3 - n bytes past dst, the re-hash enters the
    # position under the copied bytes, literals overwrite them, and a later match through that
    # bucket copies what the literals left
    for n in (0, 1, 2):
        add(f"long_len_{n}_stale_bucket", stream(40, lit(b"abcdefg") + [long(abc, n)] + lit(b"PQRSTU") +
                                                 [short(abc, 6)] + lit(ABC[:40 - 7 - n - 6 - 6])))
    # length 0 leaves bucket(abc) = dst; a second token through it copies the block onto itself,
    # so everything past its third byte is zero-fill that no store of the decoder has written
    for n in (5, 9):
        add(f"self_copy_{n}", stream(40, lit(b"abcd") + [long(abc, 0), long(abc, n)] + lit(ABC[:40 - 4 - n])))
    add("self_copy_after_len1", stream(40, lit(b"abcd") + [long(abc, 0), long(abc, 1), long(abc, 0), long(abc, 6)] +
                                       lit(ABC[:40 - 5 - 6])))
    add("self_copy_after_len2", stream(40, lit(b"abcd") + [long(abc, 0), long(abc, 2), long(abc, 0), long(abc, 7)] +
                                       lit(ABC[:40 - 6 - 7])))
    add("overlap_run", stream(40, lit(b"aaaa") + [short(bucket(b"aaa"), 17)] + lit(ABC[:19])))
    add("unwritten_bucket_mid", stream(30, lit(b"abcdef") + [short(1234, 6)] + lit(ABC[:18])))
    # size 0..12, all literals and with a leading match bit (below 11 fetch is never loaded)
    for size in range(13):
        add(f"size{size}_literals", stream(size, lit(ABC[:size])))
        # sizes 0..3 cannot get past the copy and the re-hash of a leading match
        add(f"size{size}_match_first", stream(size, [long(0, min(size, 3))] + lit(ABC[:max(size - 3, 3)])))
    add("size4_match_len0", stream(4, [long(0, 0)] + lit(b"wxyz")))
    add("size11_short_match_first", stream(11, [short(5, 3)] + lit(b"abcdefgh")))
    # a control word of 0: 32 literal bits and never a reload; a control word of 1: one match
    # bit, then 0 for ever
    add("cword_0", stream(20, lit(ABC[:20]), cwords={0: 0}))
    add("cword_0_size40", stream(40, lit(ABC[:40]), cwords={0: 0})[:9 + 4 + 40])
    add("cword_1", stream(20, [short(9, 4)] + lit(ABC[:16]), cwords={0: 1}))
    add("cword_1_small", stream(6, [long(0, 3)] + lit(b"abc"), cwords={0: 1}))
    # 31 items that leave dst past lastMatchStart: the next control word is loaded without a
    # fetch, and its match bit is decoded from the stale one (the word's own first three bytes)
    add("stale_fetch", stream(14, lit(b"abcd") + [long(abc, 0)] * 27 + [("M", b"\x55\xAA")] + lit(b"0123456789XYZ"),
                              cwords={1: 0x80000011}))
    add("tail_cword_skip", stream(35, lit(ABC[:35])))
    add("cword_reload_past_last_match_start", stream(72, lit((ABC * 2)[:72])))
    good = stream(30, lit(ABC[:12]) + [short(abc, 8)] + lit(ABC[20:30]))
    add("trailing_garbage", good + b"\xde\xad\xbe\xef" * 5)
    add("csize_zero", good[:1] + bytes(4) + good[5:])
    add("csize_huge", good[:1] + b"\xff\xff\xff\xff" + good[5:])
    add("csize_short", good[:1] + (12).to_bytes(4, "little") + good[5:])
    add("header3", stream(30, lit(ABC[:12]) + [short(abc, 8)] + lit(ABC[20:30]), hdr=3))
    add("header3_size255", stream(255, lit(ABC[:20]) + [long(abc, 225)] + lit(b"xyz") + tail10, hdr=3))
    add("header3_csize_wrong", stream(12, lit(ABC[:12]), hdr=3, csize=200))
    add("stored_short_body", header(12, 12, compressed=False) + b"abc")
    return out


# ---- headers ------------------------------------------------------------------------------

def _headers() -> list:
    out = []

    def add(name, s, cap=None):
        out.append(Case("hdr/" + name, "headers", stream=s, cap=cap))

    full9 = stream(12, lit(ABC[:12]))
    full3 = stream(12, lit(ABC[:12]), hdr=3)
    for n in range(10):
        add(f"h9_len{n}", full9[:n])
        add(f"h3_len{n}", full3[:n])
        add(f"h9_stored_len{n}", (header(4, 13, compressed=False) + b"wxyz")[:n])
        add(f"h3_stored_len{n}", (header(4, 7, hdr=3, compressed=False) + b"wxyz")[:n])
    for level in (0, 2):
        add(f"level{level}_compressed", stream(12, lit(ABC[:12]), level=level))
        add(f"level{level}_stored", header(4, 13, level=level, compressed=False) + b"wxyz")
        add(f"level{level}_h3", stream(12, lit(ABC[:12]), level=level, hdr=3))
    # a compressed level-3 stream: 12 literals under one control word is valid level 3 as well
    add("level3_compressed", stream(12, lit(ABC[:12]), level=3))
    add("level3_compressed_h3", stream(12, lit(ABC[:12]), level=3, hdr=3))
    for level in (1, 3):
        for size, tag in ((20, "size"), (0, "size0")):
            for blen, btag in ((size - 1, "minus1"), (size, "exact"), (size + 5, "plus5"), (0, "empty")):
                if blen < 0:
                    continue
                add(f"stored_l{level}_{tag}_{btag}", header(size, 9 + blen, level=level, compressed=False) +
                    ABC[:blen])
        add(f"stored_l{level}_h3_minus1", header(20, 22, level=level, hdr=3, compressed=False) + ABC[:19])
    for tag, s in (("compressed", stream(20, lit(ABC[:20]))), ("stored", header(20, 29, compressed=False) + ABC[:20]),
                   ("corrupt", stream(20, lit(ABC[:20]))[:-3])):
        for cap, ctag in ((19, "size_minus1"), (20, "size"), (0, "zero")):
            add(f"dst_cap_{ctag}_{tag}", s, cap=cap)
    add("dst_cap_zero_size0", stream(0, []), cap=0)
    add("dst_cap_huge_size", header(0xFFFFFFFF, 13) + bytes(8), cap=64)
    add("dst_cap_bad_level", stream(20, lit(ABC[:20]), level=2), cap=0)
    return out


# ---- zero_fill ----------------------------------------------------------------------------

ZERO_FILL_SIZES = (1, 15, 16, 17, 31, 33, 4096 + 5)


def _zero_fill() -> list:
    out = []
    for size in ZERO_FILL_SIZES:
        out.append(Case(f"zf/stored_empty_{size}", "zero_fill", stream=header(size, 9, compressed=False)))
        if size > 1:
            out.append(Case(f"zf/stored_one_{size}", "zero_fill", stream=header(size, 10, compressed=False) + b"Q"))
        # a compressed stream that panics on its first control word, after the zero-fill
        out.append(Case(f"zf/corrupt_early_{size}", "zero_fill", stream=header(size, 11) + b"\x00\x00"))
        if size >= 15:
            # a length-1 token at dst = 0 leaves one zero-filled byte in the output; the long
            # self-copies after it hand the zero-fill on, 255 bytes at a time
            n = size - 10 - 1
            reps, last = divmod(n, 255)
            items = [long(9, 1), long(0, 0)] + [long(0, 255)] * reps + ([long(0, last)] if last else [])
            out.append(Case(f"zf/self_copy_{size}", "zero_fill", stream=stream(size, items + lit(b"0123456789"))))
    return out


# ---- mutants ------------------------------------------------------------------------------

def _l1_vectors():
    man = json.load(open(os.path.join(GOLDEN, "golden_l1.json")))
    blob = open(os.path.join(GOLDEN, "qlz_l1_vectors.bin"), "rb").read()
    get = lambda span: blob[span[0]:span[0] + span[1]]  # noqa: E731
    return [(v["name"], get(v["input"]), get(v["ref"])) for v in man["vectors"]]


def _mutants() -> list:
    out = []
    for name, data, ref in _l1_vectors():
        if len(data) > MUTANT_MAX_INPUT:
            continue
        cap = len(data) + MUTANT_CAP_PAD
        for n in range(len(ref)):
            out.append(Case(f"mut/{name}/trunc{n}", "mutants", stream=ref[:n], cap=cap))
        for bit in range(8 * len(ref)):
            b = bytearray(ref)
            b[bit >> 3] ^= 1 << (bit & 7)
            out.append(Case(f"mut/{name}/flip{bit}", "mutants", stream=bytes(b), cap=cap))
    return out


# ---- encoder ------------------------------------------------------------------------------

def _distinct(n: int, seed: int) -> bytes:
    """n bytes with no trigram repeated (so the encoder finds no match inside it)."""
    rng = random.Random(seed)
    out = bytearray()
    seen = set()
    while len(out) < n:
        out.append(rng.randrange(33, 127))
        if len(out) >= 3:
            t = bytes(out[-3:])
            if t in seen:
                out.pop()
                continue
            seen.add(t)
    return bytes(out)


def _bail_plain(n_lit: int, n_rep: int, rep_len: int, n_tail: int, seed: int) -> bytes:
    """n_lit distinct bytes, then n_rep copies of their first rep_len bytes, each followed by
    one fresh byte, then n_tail distinct bytes: literals, then matches, then literals."""
    a = _distinct(n_lit, seed)
    fresh = bytes(range(128, 256))
    mid = b"".join(a[:rep_len] + fresh[k % 128:k % 128 + 1] for k in range(n_rep))
    return a + mid + _distinct(n_tail, seed + 1000)


# name -> (n_lit, n_rep, rep_len, n_tail, seed) of _bail_plain.  What each reaches, the margin
# (src - (src >> 5)) - dst at the control words tested at src - 3*(len>>2), is asserted with the
# model in tests/test_go_l1_cases.py (BAIL_EXPECT there).
BAIL_CASES = {
    "bail_margin_0": (4, 14, 3, 11, 21),                    # margin 0 at its only test: kept
    "bail_margin_minus1": (4, 13, 3, 13, 21),               # margin -1: stored
    # a control word at src == 3*(len>>2): `src >` is false whatever the margin
    "bail_at_threshold_behind_kept": (4, 7, 3, 30, 21),     # margin -7 there, and no later word
    "bail_at_threshold_behind_stored": (22, 24, 3, 70, 21),  # margin -1 there, stored by the next word
    "bail_at_threshold_ahead_kept": (4, 26, 3, 45, 21),     # margin 6 there
    "bail_at_threshold_ahead_stored": (18, 27, 3, 70, 21),  # margin 2 there, stored by the next word
    "bail_threshold_plus1_stored": (4, 6, 3, 30, 21),       # src == 3*(len>>2) + 1, margin < 0
    "bail_threshold_plus1_kept": (4, 25, 3, 45, 21),        # src == 3*(len>>2) + 1, margin >= 0
}


def _encoder() -> list:
    out = []

    def add(name, plain):
        assert 0 < len(plain) <= 4096, name
        out.append(Case("enc/" + name, "encoder", plain=bytes(plain)))

    A = _distinct(320, 11)
    T = _distinct(12, 12)                           # the last literals of a block
    for n in range(1, 13):
        add(f"len{n}", ABC[:n])
    for n in range(1, 13):
        add(f"run{n}", b"a" * n)
    add("counter0_bucket0", bytes(3) + ABC[:20])
    add("counter0_zeros_run", bytes(40))
    add("minoffset_1", b"qzzzz" + ABC[:20])
    add("minoffset_2", b"ababab" + ABC[:20])
    add("minoffset_2_long", b"abababababababababab" + ABC[:20])
    # the RLE exception and its refusals: a run that starts at 0 refuses lits 1, 2, then src == 3,
    # then is taken at 4; a run after a match refuses lits == 2 with everything else true
    add("rle_taken_from_start", b"a" * 30 + ABC[:12])
    add("rle_src3_alone", b"a" * 14)         # lastMatchStart = 3: the loop ends on the refusal
    add("rle_taken_mid", ABC[:9] + b"z" * 30 + ABC[10:22])
    add("rle_lits2_after_match", b"ABCDEz!" + ABC[:8] + b"ABCDEz" + b"z" * 12 + T)
    add("rle_m3_alone", ABC[:9] + b"zzzz" + ABC[10:30])
    add("rle_m2_alone", ABC[:9] + b"zqzzzz" + ABC[10:30])
    add("rle_m2_then_taken", ABC[:9] + b"zqzzzzzzzzzz" + ABC[10:30])
    for n in (3, 4, 5, 6, 7, 16, 17, 18, 19, 254, 255):
        add(f"match_{n}", A[:n + 1] + b"\x80" + A[:n] + b"\x81" + T)
    add("match_256_split", A[:257] + b"\x80" + A[:256] + b"\x81" + T)
    add("match_300_split", A[:301] + b"\x80" + A[:300] + b"\x81" + T)
    add("match_513_split", (A + _distinct(200, 13)) + b"\x80" + (A + _distinct(200, 13))[:513] + b"\x81" + T)
    # a match that would go on, cut by remaining = len - 4 - src
    for ln in (7, 8, 9, 254):
        add(f"cut_remaining_{ln}", A[:ln + 5] + b"\x80" + A[:ln + 4])
    add("remaining_255_not_cut", A[:260] + b"\x80" + A[:259])
    add("cut_remaining_run", ABC[:9] + b"z" * 40)
    for items in (31, 62, 93):
        add(f"last_cword_full_{items}", _distinct(items, 14))
    add("last_cword_full_with_match", A[:20] + b"\x80" + A[:15] + b"\x81" + T[:8])
    add("last_cword_30_items", _distinct(30, 14))
    add("last_cword_32_items", _distinct(32, 14))
    for name, args in BAIL_CASES.items():
        add(name, _bail_plain(*args))
    add("stored_random_4096", random.Random(16).randbytes(4096))
    add("text_4096", (b"the quick brown fox jumps over the lazy dog, " * 100)[:4096])
    add("zeros_4096", bytes(4096))
    return out


@functools.lru_cache(maxsize=None)
def collection() -> tuple:
    cs = _panic_sites() + _odd_tokens() + _headers() + _zero_fill() + _encoder() + _mutants()
    names = [c.name for c in cs]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1][:5]
    return tuple(cs)
