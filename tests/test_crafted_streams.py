"""Hand-assembled level-3 streams (tests/qlz_asm.py) against the CPU oracle, a pure-Python model
decoder and the reference decoder's recorded outputs (tests/golden/streams.json).  No GPU.

The streams hold what no encoder emits: every token form at offsets and lengths its encoder
never picks for it, lengths 256-258, offset 131071, junk bits in the last control word, the
checks C3 and C4 at their exact edges.  The assembler's plaintext is the expected output; the
invalid streams are one edit away from a valid one and must be refused as E_CORRUPT."""
import hashlib
import json
import os
from collections import Counter

import pytest

import qlz_asm
from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streams.json")


def model_decode(s: bytes):
    """(status, output) of a compressed level-3 stream whose header is right: the format and the
    checks C1-C5 written down once more, with nothing taken from oracle/."""
    hdr = 9 if s[0] & 2 else 3
    csize, dsize = (int.from_bytes(s[1:5], "little"), int.from_bytes(s[5:9], "little")) if hdr == 9 else (s[1], s[2])
    assert csize == len(s) and s[0] & 1 and (s[0] >> 2) & 3 == 3
    out, ip, cw, tail = bytearray(), hdr, 1, False
    while len(out) < dsize:
        if cw == 1:
            if ip + 4 > csize or not s[ip + 3] >> 7:
                return O.E_CORRUPT, b""                                  # C1
            cw, ip = int.from_bytes(s[ip:ip + 4], "little"), ip + 4
        if ip >= csize:
            return O.E_CORRUPT, b""                                      # C2
        if not cw & 1:  # the literals up to the next match, the end of the word, of csize or of dsize
            n = min((cw & -cw).bit_length() - 1, csize - ip, dsize - len(out))
            tail = tail or len(out) + n - 1 >= dsize - 11
            out += s[ip:ip + n]
            cw, ip = cw >> n, ip + n
            continue
        tl = 1 if s[ip] & 3 == 0 else 2 if s[ip] & 3 != 3 else 3 if s[ip] & 127 != 3 else 4
        if tail or ip + tl > csize:
            return O.E_CORRUPT, b""                                      # C4, C2
        t = int.from_bytes(s[ip:ip + tl], "little")
        off, ml = ((t >> 2, 3) if tl == 1 or t & 3 == 1 else (t >> 6, (t >> 2 & 15) + 3) if tl == 2 else
                   (t >> 7, (t >> 2 & 31) + 2) if tl == 3 else (t >> 15, (t >> 7 & 255) + 3))
        op = len(out)
        if off < 3 or off > op or op + ml + 4 > dsize:
            return O.E_CORRUPT, b""                                      # C3
        seg = out[op - off:op - off + ml]
        out += seg if off >= ml else (seg * (ml // off + 1))[:ml]
        cw, ip = cw >> 1, ip + tl
    if not (ip == csize or (ip < hdr + 9 and csize == hdr + 9)):
        return O.E_CORRUPT, b""                                          # C5
    return O.OK, bytes(out)


def test_assembler_forms_and_refusals():
    """Token bytes of each form at a known value; field ranges asserted; C3 and C4 refused."""
    assert qlz_asm.encode("A", 63, 3) == bytes([0xFC])
    assert qlz_asm.encode("B", 16383, 3) == bytes([0xFD, 0xFF])
    assert qlz_asm.encode("C", 1023, 18) == bytes([0xFE, 0xFF])
    assert qlz_asm.encode("D", 131071, 33) == bytes([0xFF, 0xFF, 0xFF])
    assert qlz_asm.encode("D", 3, 3) == bytes([0x87, 0x01, 0x00])
    assert qlz_asm.encode("E", 131071, 258) == bytes([0x83, 0xFF, 0xFF, 0xFF])
    for form, off, ml in (("A", 64, 3), ("A", 3, 4), ("B", 16384, 3), ("C", 1024, 3), ("C", 3, 19), ("D", 3, 2),
                          ("D", 3, 34), ("D", 131072, 3), ("E", 3, 259), ("E", 131072, 3)):
        with pytest.raises(AssertionError):
            qlz_asm.encode(form, off, ml)
    a = qlz_asm.Asm("t")
    a.lits(20)
    for off in (2, 21):
        with pytest.raises(ValueError):
            a.match("E", off, 3)                # C3: offset below 3, offset beyond op
    a.match("E", 5, 10)                     # no literal may stand in the 11 bytes before the end
    a.match("E", 5, 3)
    a.finish(a.op + 3)
    with pytest.raises(ValueError):
        a.stream()                              # C3: op + len + 4 > dsize
    a.finish(a.op + 1)
    assert O.decompress(a.stream()) == (O.OK, bytes(a.plain))
    b = qlz_asm.Asm("t")
    b.lits(20)
    b.match("A", 3, 3)
    b.finish(b.op + 8)                          # the literal at op 19 == dsize - 12: not the tail
    assert O.decompress(b.stream()) == (O.OK, bytes(b.plain))
    c = qlz_asm.Asm("t")
    c.lits(20)
    c.match("A", 3, 3)
    c.finish(c.op + 7)                          # now it is at dsize - 11
    with pytest.raises(ValueError):
        c.stream()                              # C4
    # the issue's example: junk over the zero padding of a 9-byte core
    d = qlz_asm.Asm("t")
    for ch in b"abc":
        d.lit(ch)
    assert d.stream(short_header=True, junk=0x7FFFFFFF) == bytes.fromhex("4d0c03f8ffffff6162630000")
    r = qlz_asm.XorShift64(1)
    assert [r.next() for _ in range(2)] == [0x40822041, 0x100041060C011441]


def test_family_sizes():
    """The families hold what they are described to hold (the GPU tests count against these)."""
    fam = Counter(c.family for c in qlz_asm.collection())
    pairs = sum(len(qlz_asm.LEN_EDGES[f]) for f in "ABCDE" for o in qlz_asm.S_OFFSETS if o <= qlz_asm.FORMS[f][1])
    assert fam["forms_S"] == pairs == 143
    assert fam["forms_M"] == 8 + 2 * 11 + 2 * 11        # B: 8 offsets, one length; D, E: 11 offsets, two lengths
    assert fam["forms_L"] == 2 * 2 * 5
    assert fam["chunk_cover"] == 3 * 4 * 4 + 3 * 5 + 3 * 6
    assert fam["lastword"] == 2 * 2 * (3 * (1 + len(qlz_asm.PADS)) + 8)
    assert fam["random"] == qlz_asm.N_RANDOM == 200
    assert set(fam) == set(qlz_asm.FAMILIES)
    for c in qlz_asm.collection():
        if c.family == "forms_S":
            assert len(c.plain) <= 4096
        if c.family == "forms_M":
            assert len(c.plain) == 65536
    sizes = [len(c.plain) for c in qlz_asm.collection() if c.family == "random"]
    for lo, hi in ((1, 300), (301, 4096), (4097, 32768), (65536, 65536), (70 << 10, 140 << 10)):
        assert sum(lo <= n <= hi for n in sizes) == 40
    # what no encoder emits is there: lengths 256-258, offset 131071, the 4-byte form at length 3
    toks = Counter((it.form, it.off, it.ml) for c in qlz_asm.collection() if c.family != "random"
                   for it in c.asm.seq if isinstance(it, qlz_asm.Item))
    for key in (("E", 131071, 258), ("D", 131071, 3), ("E", 3, 3), ("E", 3, 256), ("E", 257, 257), ("B", 3, 3),
                ("C", 3, 3), ("D", 3, 3), ("E", 65535, 258), ("E", 65536, 3)):
        assert toks[key] > 0, key
    inv = Counter(i.kind for i in qlz_asm.invalid_collection())
    assert set(inv) == set(qlz_asm.MUTATIONS) and min(inv.values()) >= 2, inv
    for fam_name in qlz_asm.INVALID_FAMILIES:
        kinds = {i.kind for i in qlz_asm.invalid_collection() if i.family == fam_name}
        assert {"off_op+1", "end+1", "match_in_tail", "trailing_byte", "trailing_word", "word2_no_bit31",
                "cut_last_token", "off0_D", "off1_D", "off2_D"} <= kinds, fam_name


def test_valid_streams_oracle_and_model():
    n = 0
    for c in qlz_asm.collection():
        assert O.decompress(c.stream) == (O.OK, c.plain), c.name
        assert model_decode(c.stream) == (O.OK, c.plain), c.name
        n += 1
    assert n == len(qlz_asm.collection()) >= 600


def test_invalid_streams_oracle_and_model():
    n = 0
    for i in qlz_asm.invalid_collection():
        assert O.decompress(i.stream)[0] == O.E_CORRUPT, i.name
        assert model_decode(i.stream)[0] == O.E_CORRUPT, i.name
        n += 1
    assert n == len(qlz_asm.invalid_collection()) >= 200


def test_reference_fixture():
    """tests/golden/streams.json (make_golden_streams.py): the regenerated stream is the one the
    reference decoder saw, and the assembler's plaintext is what the reference made of it."""
    rows = json.load(open(GOLDEN))["streams"]
    cases = qlz_asm.collection()
    assert [r["name"] for r in rows] == [c.name for c in cases]
    for r, c in zip(rows, cases):
        assert (r["stream_len"], r["stream_sha256"]) == (len(c.stream), hashlib.sha256(c.stream).hexdigest()), c.name
        assert (r["ref_len"], r["ref_sha256"]) == (len(c.plain), hashlib.sha256(c.plain).hexdigest()), c.name


def test_gpu_routes_cover_every_case():
    """The routing table of tests/test_gpu_crafted_streams.py, checked where no GPU is needed:
    every case has exactly one single-call route and one of the batch routes K1 + K2 / huge, and
    the per-family counts of every route are the ones its test states."""
    import test_gpu_crafted_streams as G
    for c in G._cases():
        cs, ds = len(c[2]), c[3]
        assert G.ADMIT["small"](cs, ds) + G.ADMIT["solo"](cs, ds) + G.ADMIT["huge"](cs, ds) == 1, c[0]
        assert G.ADMIT["mixed"](cs, ds) + G.ADMIT["huge"](cs, ds) == 1, c[0]
    for route in G.EXPECT:
        G._route(route)
    for k in G.ALL_VALID:
        assert sum(G.EXPECT[r][0].get(k, 0) for r in ("small", "solo", "huge")) == G.ALL_VALID[k]
    for k in G.ALL_INVALID:
        assert sum(G.EXPECT[r][1].get(k, 0) for r in ("small", "solo", "huge")) == G.ALL_INVALID[k]
    assert sum(G.ALL_VALID.values()) == len(qlz_asm.collection())
    assert sum(G.ALL_INVALID.values()) == len(qlz_asm.invalid_collection())
