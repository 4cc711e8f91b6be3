""".data images built to force each decision of the replay reader -- TEST INFRASTRUCTURE ONLY.

The replay tests elsewhere feed random record files with random byte flips and leave it to
chance whether a given decision of the sequential reader occurs.  Every case here plants one.
The reader is DataStreamReader (store/datafile.go:228-277 Next, :202-226 nextValid, :114-170
readRecordAt) with the size limits of config/mc_config.go:33-39 and, for records flagged
FLAG_COMPRESS, Payload.Decompress (store/item.go:163-176).  What matters for the expectations:

  * Next() at position p: fewer than 24 bytes left -> io.EOF (none left: clean end) or an
    unexpected-EOF error (1..23 left); then the key size, then the value size (either bad ->
    nextValid); then the key and the body are read in full (short -> unexpected-EOF error); then
    the CRC (bad -> nextValid).
  * nextValid() tries readRecordAt at p, p + 256, ... up to the end of the file.  EVERY failure
    there (short header, bad sizes, a record running past the end, a bad CRC) just moves on by
    256, so a slot that ends the stream with an error when Next() lands on it is skipped in
    silence when nextValid walks over it.  Its sizeBroken counts from p -- the end of the
    previous record -- and starts at 0 on every call.
  * readRecordAt checks the key size, then the value size, then reads: a header whose sizes are
    bad and which ALSO runs past the end of the file is a bad size, not a short read.
  * a body that does not decode stays as stored and keeps FLAG_COMPRESS.

A case is a file, the reader's parameters, and the rows the reader must return, written down
from the layout: (offset, sizeBroken, key), for the compressed-body cases also (flag, value)
after Payload.Decompress.  No expectation here comes from oracle/replay.py: tests/
test_datafile_cases.py holds the oracle against these rows, tests/test_gpu_replay_cases.py holds
the GPU against the oracle.  `claims` says what the file is meant to reach; the host test
verifies each claim from the file's own headers, so a pass on the GPU is not vacuous.

Junk and filler bytes are 0x80..0xFF: any four of them read as a key size of at least
0x80808080, so a slot that starts in them never has valid sizes.
"""
from __future__ import annotations

import functools
import struct
import zlib
from collections import namedtuple

import numpy as np

from qlz_asm import name_seed
from oracle import oracle as O
from oracle import replay as R

HDR, SLOT = 24, 256
FLAG_COMPRESS = 0x00010000
MAX_KEY = 250                 # config/mc_config.go:6
BODY_MAX = 50 << 20           # config/mc_config.go:7
EOF_ERR = "unexpected EOF"

# gobeansdb_amd/csrc/qlzx_recfile.h: a CRC span (20 + ksz + vsz) above kRpLong leaves the
# wave-per-record kernel for the segmented one, which cuts it into kRpSeg pieces; the scans work
# in tiles of kScanTile elements, kScanTile tile sums per batch of k_scan_top.
RP_LONG = 128 << 10
RP_SEG = 16 << 10
SCAN_TILE = 1024

# name; family; data: the file; start, max_key, body_max: the reader's parameters; rows: what the
# reader returns; end_error: None or EOF_ERR; claims: what the file is built to reach
Case = namedtuple("Case", "name family data start max_key body_max rows end_error claims")


def pad256(n: int) -> int:
    return (n + 255) & ~255


def record_crc(image: bytes) -> int:
    """The CRC field of a record image (store/datafile.go:66-76: crc32 of header[4:24] ‖ key ‖
    value, the common CRC-32, store/crc32.go)."""
    return zlib.crc32(image[4:]) & 0xFFFFFFFF


class DataFile:
    """A .data image, slot by slot."""

    def __init__(self, name: str):
        self.name = name
        self.rng = np.random.default_rng(name_seed(name))
        self.b = bytearray()

    def __len__(self):
        return len(self.b)

    @property
    def at(self) -> int:
        """The next free slot's offset."""
        assert len(self.b) % SLOT == 0, (self.name, len(self.b))
        return len(self.b)

    def filler(self, n: int) -> bytes:
        """n seeded bytes of 0x80..0xFF (not appended)."""
        return self.rng.integers(0x80, 0x100, n, dtype=np.uint8).tobytes()

    def put(self, off: int, s: bytes):
        """Overwrite (and extend with zeros up to) [off, off + len(s))."""
        if len(self.b) < off + len(s):
            self.b += bytes(off + len(s) - len(self.b))
        self.b[off:off + len(s)] = s

    def record(self, key: bytes, body: bytes, flag: int = 0, ver: int = 0, ts: int = 0) -> int:
        """Append a valid padded record (WriteRecord.append); returns its offset."""
        off = self.at
        self.b += R.make_record(key, body, flag=flag, ver=ver, ts=ts)
        return off

    def compressed(self, key: bytes, plain: bytes, ver: int = 0) -> int:
        return self.record(key, O.compress(plain), flag=FLAG_COMPRESS, ver=ver)

    def header(self, off: int, ksz: int, vsz: int, flag: int = 0, ver: int = 0, ts: int = 0, good_crc=False) -> int:
        """A bare 24-byte header at slot offset `off` (the rest of its slot is left as it is, or
        zeros where the file ended before).  good_crc: the CRC of the bytes the header claims, as
        they stand in the file now (they must all be there); otherwise that CRC, or 0 when the
        claim runs past the end, XOR 0xDEADBEEF."""
        assert off % SLOT == 0
        self.put(off + 4, struct.pack("<IIiII", ts, flag, ver, ksz, vsz))
        end = off + HDR + ksz + vsz
        assert not good_crc or end <= len(self.b), (self.name, off)
        crc = record_crc(bytes(self.b[off:end])) if end <= len(self.b) else 0
        self.put(off, struct.pack("<I", crc if good_crc else crc ^ 0xDEADBEEF))
        if len(self.b) % SLOT:
            self.b += bytes(-len(self.b) % SLOT)
        return off

    def seal(self, off: int):
        """Recompute the CRC field of the record at `off` from the file's bytes as they stand."""
        ksz, vsz = struct.unpack_from("<II", self.b, off + 16)
        self.put(off, struct.pack("<I", record_crc(bytes(self.b[off:off + HDR + ksz + vsz]))))

    def break_crc(self, off: int):
        """Make the record at `off` fail its CRC without touching its sizes, key or body."""
        self.b[off] ^= 0x40

    def flip(self, pos: int, mask: int = 1):
        self.b[pos] ^= mask

    def zeros(self, nslots: int = 1) -> int:
        off = self.at
        self.b += bytes(SLOT * nslots)
        return off

    def junk(self, nslots: int = 1) -> int:
        off = self.at
        self.b += self.filler(SLOT * nslots)
        return off

    def cut(self, n: int):
        assert n <= len(self.b)
        del self.b[n:]

    def body_with(self, ksz: int, vsz: int, items: dict) -> bytes:
        """A body of vsz filler bytes for a record with a key of ksz bytes, with items[j] (bytes)
        laid over it at the record's slot j, i.e. at body index 256 j - 24 - ksz."""
        body = bytearray(self.filler(vsz))
        for j, s in items.items():
            i = SLOT * j - HDR - ksz
            assert 0 <= i and i + len(s) <= vsz, (self.name, j)
            body[i:i + len(s)] = s
        return bytes(body)

    def done(self, family, rows, end_error=None, start=0, max_key=MAX_KEY, body_max=BODY_MAX, **claims) -> Case:
        return Case(self.name, family, bytes(self.b), start, max_key, body_max, rows, end_error, claims)


# ---- what a file holds, read from its own headers (the host test's view of the claims) ----
def slot_kind(data: bytes, off: int, max_key: int = MAX_KEY, body_max: int = BODY_MAX) -> str:
    """readRecordAt's verdict on the slot at `off` (store/datafile.go:123-168, in its order):
    partial | key_size | value_size | trunc | bad_crc | valid."""
    if off + HDR > len(data):
        return "partial"
    ksz, vsz = struct.unpack_from("<II", data, off + 16)
    if ksz == 0 or ksz > max_key:
        return "key_size"
    if vsz > body_max:
        return "value_size"
    end = off + HDR + ksz + vsz
    if end > len(data):
        return "trunc"
    crc, = struct.unpack_from("<I", data, off)
    return "valid" if record_crc(data[off:end]) == crc else "bad_crc"


def scan(data: bytes, max_key: int = MAX_KEY, body_max: int = BODY_MAX):
    """Every candidate slot of the file (valid sizes, fits the file): [(offset, span, valid)]
    with span = 20 + ksz + vsz, the bytes its CRC covers."""
    out = []
    for off in range(0, len(data), SLOT):
        k = slot_kind(data, off, max_key, body_max)
        if k in ("valid", "bad_crc"):
            ksz, vsz = struct.unpack_from("<II", data, off + 16)
            out.append((off, 20 + ksz + vsz, k == "valid"))
    return out


def _first(f: DataFile) -> int:
    return f.record(b"first", b"value of first", ver=1, ts=11)


def _after(f: DataFile) -> int:
    return f.record(b"after", b"value of after", ver=2, ts=22)


# ------------------------------------------------------------------ landing ----
# One planted slot X, once where Next() lands (directly behind a valid record) and once where
# only nextValid walks over it (behind a slot of zeros, which sends Next() into nextValid):
#   landed:  first @0 | X @256 (nx slots) | after        Next() reads X's header itself
#   walked:  first @0 | zeros @256 | X @512 | after      Next() lands on the zeros (ksz == 0),
#                                                        nextValid meets X at 512
# edge = {"ksz": d} / {"vsz": d}: X's header holds max_key + d / body_max + d (the host test reads it).
# X resyncs (or is skipped): `after` comes back with sizeBroken = its offset - 256, the end of
# `first`.  X ends the stream (valid sizes, runs past the end, landed on): only `first`, error.
def _planted(name, plant, kind, *, max_key=MAX_KEY, body_max=BODY_MAX, landed_error=False, edge=None):
    out = []
    for walked in (False, True):
        f = DataFile(f"{name}_{'walked' if walked else 'landed'}")
        _first(f)
        if walked:
            f.zeros()
        x = f.at
        plant(f)
        a = _after(f)
        if landed_error and not walked:
            rows, err = [(0, 0, b"first")], EOF_ERR
        else:
            rows, err = [(0, 0, b"first"), (a, a - 256, b"after")], None
        out.append(f.done("landing", rows, err, max_key=max_key, body_max=body_max,
                          slot=x, kind=kind, landed=not walked, edge=edge))
    return out


def _landing_cases():
    cs = []
    # ksz == 0: IsValidKeySize fails (mc_config.go:34) -> nextValid (datafile.go:239-242)
    cs += _planted("ksz0", lambda f: f.header(f.at, 0, 10, ts=7), "key_size")
    # ksz == max_key + 1, on a record that is valid in every other respect (its CRC included)
    cs += _planted("ksz251", lambda f: f.record(b"k" * 251, b"x" * 8), "key_size", edge={"ksz": 1})
    cs += _planted("ksz9_maxkey8", lambda f: f.record(b"ninebytes", b"x" * 8), "key_size", max_key=8,
                   edge={"ksz": 1})
    # vsz == body_max + 1, again on an otherwise valid record (5 slots, the body is filler)
    cs += _planted("vsz1001_bodymax1000", lambda f: f.record(b"big", f.filler(1001)), "value_size", body_max=1000,
                   edge={"vsz": 1})
    # the default BodyMax: a header that only claims 50 MiB + 1 (datafile.go:244-247)
    cs += _planted("vsz_50MiB_plus1", lambda f: f.header(f.at, 3, BODY_MAX + 1), "value_size", edge={"vsz": 1})
    # valid sizes, wrong CRC (datafile.go:265-271)
    def bad_crc(f):
        f.break_crc(f.record(b"badcrc", b"value of badcrc"))
    cs += _planted("bad_crc", bad_crc, "bad_crc")
    # valid sizes, the body runs past the end of the file: io.ReadFull fails in Next()
    # (datafile.go:250-258, error); readRecordAt fails in nextValid (datafile.go:149-155, skipped)
    cs += _planted("past_eof", lambda f: f.header(f.at, 3, 5000), "trunc", landed_error=True)
    # bad sizes that also run past the end: the size checks come first (datafile.go:129-137,
    # 239-247), so these resync and never report an error
    cs += _planted("ksz0_past_eof", lambda f: f.header(f.at, 0, 5000), "key_size")
    cs += _planted("ksz251_past_eof", lambda f: f.header(f.at, 251, 5000), "key_size", edge={"ksz": 1})
    cs += _planted("vsz_over_past_eof", lambda f: f.header(f.at, 3, 5000), "value_size", body_max=1000)
    return cs


# ------------------------------------------------------------------ bounds ----
def _valid_at_bound(name, key, body, edge=None, **lim):
    """first | X | after with X exactly on a limit: all three come back."""
    f = DataFile(name)
    _first(f)
    x = f.record(key, body, ver=5)
    a = _after(f)
    return f.done("bounds", [(0, 0, b"first"), (x, 0, key), (a, 0, b"after")], slot=x, kind="valid", landed=True,
                  edge=edge, **lim)


def _bounds_cases():
    f = DataFile("x")
    return [
        _valid_at_bound("ksz1", b"k", b"value"),                              # mc_config.go:34, ksz != 0
        _valid_at_bound("ksz250", b"K" * 250, b"value", {"ksz": 0}),          # ksz <= MaxKeyLen
        _valid_at_bound("ksz8_maxkey8", b"8bytes__", b"value", {"ksz": 0}, max_key=8),
        _valid_at_bound("ksz9_default", b"ninebytes", b"x" * 8),              # ksz9_maxkey8's record
        _valid_at_bound("vsz1000_bodymax1000", b"big", f.filler(1000), {"vsz": 0}, body_max=1000),  # mc_config.go:38
        _valid_at_bound("vsz0", b"empty", b""),
        _valid_at_bound("ksz8_vsz1000_both_limits", b"8bytes__", f.filler(1000), {"ksz": 0, "vsz": 0}, max_key=8,
                        body_max=1000),
    ]


# ------------------------------------------------------------------ end of file ----
def _partial(n: int, walked: bool) -> Case:
    """n bytes (1..23) of a header -- a valid one's, ksz = 3 and vsz = 5 as far as it gets -- at
    the end of the file.  Landed on: io.ReadFull's unexpected EOF (datafile.go:230-237).  Behind
    a slot of zeros: nextValid's readRecordAt fails on it (datafile.go:123-127) and the loop runs
    off the end: no record, no error (datafile.go:224-225).  Every n: 16 ends right before
    ksz, 17..19 cut it, 20 holds a whole plausible ksz and no vsz, 21..23 cut vsz."""
    f = DataFile(f"partial{n}_{'walked' if walked else 'landed'}")
    _first(f)
    if walked:
        f.zeros()
    x = f.at
    f.record(b"key", b"value")
    f.cut(x + n)
    return f.done("eof", [(0, 0, b"first")], None if walked else EOF_ERR, slot=x, kind="partial", landed=not walked)


def _eof_cases():
    cs = [_partial(n, w) for n in range(1, 24) for w in (False, True)]
    # the last record's padding is cut off: key and body are read in full, Discard's short
    # count is ignored (datafile.go:259-263), the next Next() is at EOF
    f = DataFile("padding_cut")
    _first(f)
    x = f.record(b"last", b"value of last")
    f.cut(x + HDR + 4 + 13)
    cs.append(f.done("eof", [(0, 0, b"first"), (x, 0, b"last")], slot=x, kind="valid", landed=True))
    # ... and one byte less is a short body
    f = DataFile("body_cut_by_one")
    _first(f)
    x = f.record(b"last", b"value of last")
    f.cut(x + HDR + 4 + 12)
    cs.append(f.done("eof", [(0, 0, b"first")], EOF_ERR, slot=x, kind="trunc", landed=True))
    # the last record ends exactly at size: 24 + 4 + 228 = 256
    f = DataFile("ends_at_size")
    _first(f)
    x = f.record(b"last", f.filler(228))
    assert len(f) == 512
    cs.append(f.done("eof", [(0, 0, b"first"), (x, 0, b"last")], slot=x, kind="valid", landed=True))
    # start == size: io.EOF at once
    f = DataFile("start_at_size")
    _first(f)
    _after(f)
    cs.append(f.done("eof", [], start=512))
    # start at the last slot
    f = DataFile("start_at_last_slot")
    _first(f)
    _after(f)
    x = f.record(b"last", b"value of last")
    cs.append(f.done("eof", [(x, 0, b"last")], start=x, slot=x, kind="valid", landed=True))
    # start inside a record (its second slot): resync to the next one
    f = DataFile("start_inside_record")
    f.record(b"two", f.filler(300))
    a = _after(f)
    cs.append(f.done("eof", [(a, 256, b"after")], start=256, slot=256, kind="key_size", landed=True))
    # one slot of zeros
    f = DataFile("one_zero_slot")
    f.zeros()
    cs.append(f.done("eof", [], slot=0, kind="key_size", landed=True))
    # no valid record after the landing slot: nextValid runs off the end, clean
    f = DataFile("junk_to_the_end")
    _first(f)
    x = f.junk(3)
    cs.append(f.done("eof", [(0, 0, b"first")], slot=x, kind="key_size", landed=True))
    # the same with a last slot that is short: nextValid's last readRecordAt is a short read
    f = DataFile("junk_to_a_ragged_end")
    _first(f)
    x = f.junk(3)
    f.cut(x + 2 * 256 + 100)
    cs.append(f.done("eof", [(0, 0, b"first")], slot=x, kind="key_size", landed=True))
    return cs


# ------------------------------------------------------------------ embedding ----
def _embedding_cases():
    cs = []
    for broken in (False, True):
        # outer: key "outer", 1500 bytes of body (6 slots); at its slot 2 a whole valid record
        # "inner" (one slot), at its slot 4 a header with valid sizes and a wrong CRC
        f = DataFile("embedded_outer_broken" if broken else "embedded_intact")
        inner = R.make_record(b"inner", b"value of inner", ver=9)
        fake = bytearray(R.make_record(b"fake", b"value of fake"))
        fake[1] ^= 0x10
        o = f.record(b"outer", f.body_with(5, 1500, {2: inner, 4: bytes(fake)}))
        a = _after(f)
        assert a == 1536
        if broken:
            # Next() at 0: CRC fails -> nextValid from 0 finds inner at 512 (sizeBroken 512, the
            # distance from outer's start); the next Next() lands at 768 in outer's filler ->
            # nextValid walks 768, 1024 (the fake), 1280 and finds `after` (sizeBroken 768, from
            # inner's end, not from outer's start)
            f.break_crc(o)
            rows = [(512, 512, b"inner"), (a, a - 768, b"after")]
        else:
            rows = [(0, 0, b"outer"), (a, 0, b"after")]
        cs.append(f.done("embedding", rows, slot=512, kind="valid", landed=False, nvalid=2 if broken else 3))
    # two resyncs in a row: each sizeBroken counts from the end of the record before it
    f = DataFile("two_resyncs")
    _first(f)
    f.junk(2)
    m = f.record(b"middle", b"value of middle")
    f.zeros(1)
    f.junk(2)
    a = _after(f)
    assert (m, a) == (768, 1792)
    cs.append(f.done("embedding", [(0, 0, b"first"), (768, 512, b"middle"), (1792, 768, b"after")]))
    return cs


# ------------------------------------------------------------------ long CRC spans ----
LONG_SPANS = {
    "long_minus1": RP_LONG - 1,            # the last but one wave-per-record size
    "long_exact": RP_LONG,                 # the last wave-per-record size
    "long_plus1": RP_LONG + 1,             # the first segmented one: 8 segments and 1 byte
    "long_plus_seg": RP_LONG + RP_SEG,     # a whole number of segments
    "seg9_plus1": 9 * RP_SEG + 1,          # last segment of 1, 2, 3 bytes: wave_crc's len < 4
    "seg9_plus2": 9 * RP_SEG + 2,
    "seg9_plus3": 9 * RP_SEG + 3,
}


def _long_span_case(name: str, span: int) -> Case:
    """long (valid, CRC span `span`) | mid | long2 (the same sizes, its last body byte flipped: a
    false candidate) | after.  The reader returns long and mid, fails long2's CRC and resyncs
    through its filler body to `after`: sizeBroken is long2's whole padded size."""
    f = DataFile(name)
    vsz = span - 20 - 4
    rs = pad256(HDR + 4 + vsz)
    f.record(b"long", f.filler(vsz), ver=3)
    m = f.record(b"mid", b"value of mid")
    x = f.record(b"lon2", f.filler(vsz), ver=4)
    f.flip(x + HDR + 4 + vsz - 1)
    a = _after(f)
    assert (m, x, a) == (rs, rs + 256, 2 * rs + 256)
    return f.done("long_crc", [(0, 0, b"long"), (m, 0, b"mid"), (a, rs, b"after")], spans=[span, span],
                  last_segment=span % RP_SEG or RP_SEG, segmented=span > RP_LONG)


MANY_LONG_FIRST, MANY_LONG_LAST, MANY_LONG_MIXED = 1, 76, 70


def _many_long_case(variant: str) -> Case:
    """More long candidates than one 64-entry step of the list walk takes: an outer raw record of
    160 KiB whose body holds, on its slots 1..76, headers "in_01".."in_76" that each claim a span
    over kRpLong inside the file: 76 overlapping candidates, with outer itself 77 listed ones.
    The list is in push order, which the file does not control, so nothing here depends on which
    entry lands in which step: EVERY planted header is made valid (sealed from slot 76 down to
    slot 1, each CRC covering only later headers; outer's last), and the count of valid records
    that replay.index reports needs a right verdict from every entry of every step.
      intact        78 valid; the reader returns outer and after
      outer_broken  outer's CRC broken, 77 valid: nextValid finds in_01 at 256 (sizeBroken 256),
                    which ends at 132608 in outer's filler; the next resync reaches `after`
      mixed         outer and in_01..in_69 broken (70 false candidates), in_70..in_76 and after
                    valid: nextValid walks 70 slots to in_70, which ends at 150784"""
    f = DataFile(f"many_long_{variant}")
    vsz_outer = 160 << 10
    o = f.record(b"outer", f.filler(vsz_outer))
    a = _after(f)
    assert a == pad256(HDR + 5 + vsz_outer) == 164096
    vsz_of = lambda j: (129 << 10) + 7 * j            # spans 132128 .. 132653, all inside the file
    for j in range(MANY_LONG_FIRST, MANY_LONG_LAST + 1):
        assert 256 * j + HDR + 5 + vsz_of(j) < a
        f.header(256 * j, 5, vsz_of(j), ts=j)
        f.put(256 * j + HDR, b"in_%02d" % j)
    for j in range(MANY_LONG_LAST, MANY_LONG_FIRST - 1, -1):
        f.seal(256 * j)
    f.seal(o)
    assert len(f) == a + 256
    end_of = lambda j: 256 * j + pad256(HDR + 5 + vsz_of(j))
    if variant == "intact":
        rows, nvalid = [(0, 0, b"outer"), (a, 0, b"after")], 78
    elif variant == "outer_broken":
        f.break_crc(o)
        assert end_of(1) == 256 + 132352 == 132608 and a - end_of(1) == 31488
        rows, nvalid = [(256, 256, b"in_01"), (a, 31488, b"after")], 77
    else:
        for j in range(MANY_LONG_MIXED):          # slot 0 is outer
            f.break_crc(256 * j)
        assert end_of(70) == 17920 + 132864 == 150784 and a - end_of(70) == 13312
        rows, nvalid = [(17920, 17920, b"in_70"), (a, 13312, b"after")], 8
    return f.done("long_crc", rows, nlong=77, nvalid=nvalid)


MANY_LONG = ("intact", "outer_broken", "mixed")


def _long_cases():
    return [_long_span_case(n, s) for n, s in LONG_SPANS.items()] + [_many_long_case(v) for v in MANY_LONG]


# ------------------------------------------------------------------ compressed bodies ----
def qlz_header(csize: int, dsize: int, long: bool, compressed: bool = True) -> bytes:
    """A level-3 QuickLZ header (quicklz.go:32-51): 3 bytes, or 9 with the long-header bit."""
    b0 = 0x4C | (2 if long else 0) | (1 if compressed else 0)
    return bytes([b0]) + (struct.pack("<II", csize, dsize) if long else bytes([csize, dsize]))


def _compressed_case() -> Case:
    """Bodies under FLAG_COMPRESS that CDecompressSafe (quicklz/cquicklz.go:84-101) refuses or
    fails on, around one that decodes: Payload.Decompress logs the error and returns
    (store/item.go:167-171), so flag and body stay as stored.  The short ones are shorter than
    the header their first byte announces (3 bytes, 9 with the long-header bit) or end before
    their first control word; the two long-header ones carry the right compressed size, a control
    word and two literals, and claim far more output than that (0xFFFFFFFF; exactly BodyMax)."""
    f = DataFile("compressed_bodies")
    text = O.gen_text(77, 0, 600)
    cw = struct.pack("<I", 0x80000000)       # 31 literals to come
    bodies = [
        (b"len0", b""),
        (b"len1", b"\x4d"),
        (b"len2", b"\x4d\x02"),
        (b"len3", qlz_header(3, 5, long=False)),                    # a whole short header, nothing after
        (b"len3_longbit", b"\x4f\x03\x05"),                         # announces 9 bytes of header
        (b"len8", qlz_header(8, 200, long=False) + cw + b"a"),      # control word and one literal of 200
        (b"len8_longbit", b"\x4f\x08\x00\x00\x00\xc8\x00\x00"),     # one byte short of its header
        (b"text", None),
        (b"len9", qlz_header(9, 100, long=True)),                   # a whole long header, nothing after
        (b"dsize_ffffffff", qlz_header(15, 0xFFFFFFFF, long=True) + cw + b"ab"),
        (b"dsize_bodymax", qlz_header(15, BODY_MAX, long=True) + cw + b"ab"),
        (b"text2", None),
    ]
    rows = []
    for i, (key, body) in enumerate(bodies):
        if body is None:
            off = f.compressed(key, text, ver=i)
            rows.append((off, 0, key, 0x20, text))
            f.b[off + 8] |= 0x20      # another flag bit, kept by `Flag -= FLAG_COMPRESS` (item.go:174)
            f.seal(off)
        else:
            off = f.record(key, body, flag=FLAG_COMPRESS | 0x20, ver=i)
            rows.append((off, 0, key, FLAG_COMPRESS | 0x20, body))
    return f.done("compressed", rows, body_lens=[0, 1, 2, 3, 3, 8, 8, 9, 15, 15], ncomp=12)


# ------------------------------------------------------------------ the collection ----
@functools.lru_cache(maxsize=None)
def collection():
    cs = (_landing_cases() + _bounds_cases() + _eof_cases() + _embedding_cases() + _long_cases()
          + [_compressed_case()])
    assert len({c.name for c in cs}) == len(cs)
    return cs


def by_name(name: str) -> Case:
    return next(c for c in collection() if c.name == name)


def names(*families):
    return [c.name for c in collection() if not families or c.family in families]


# ------------------------------------------------------------------ generated ----
MANY_N = 5000


@functools.lru_cache(maxsize=None)
def many_compressed() -> Case:
    """5000 records, four of five a compressed text of 200..1999 bytes (sizes all over the
    256-byte classes, so the decoder's destination offsets differ), every fifth raw.  4000
    compressed records: k_rp_dstoff's waves 0..14 own 256 of them each and walk four 64-entry
    steps, wave 15 owns the last 160 and walks three; the visited list and the doubling run over
    5000 records.  The rows follow from the layout: record i starts where record i - 1 ended."""
    f = DataFile("many_compressed")
    rows, ncomp = [], 0
    for i in range(MANY_N):
        key = b"key_%05d" % i
        if i % 5 == 4:
            off = f.record(key, f.filler(40 + i % 300), ver=i)
        else:
            off = f.compressed(key, O.gen_text(5, i, 200 + (i * 37) % 1800), ver=i)
            ncomp += 1
        rows.append((off, 0, key))
    return f.done("generated", rows, ncomp=ncomp, nrec=MANY_N)


Million = namedtuple("Million", "data block block_off reps offsets rs nslots nrec")
MILLION_BLOCK, MILLION_REPS, MILLION_TWO_SLOT = 64, 16500, 20


def tiled_expect(offsets, rs, broken_at=None, start=0):
    """(offsets, sizeBroken) the reader returns on a gap-free run of valid records at `offsets`
    with padded sizes `rs`, by arithmetic: with record `broken_at` failing its CRC (it is left
    out and the one behind it gets its padded size as sizeBroken: its later slots hold filler),
    or from `start` (a record's start, or a later slot of a record: the first record at or
    behind `start`, with the distance as its sizeBroken)."""
    first = int(np.searchsorted(offsets, start, "left"))
    off = offsets[first:].copy()
    brk = np.zeros(len(off), np.int64)
    if len(off):
        brk[0] = off[0] - start
    if broken_at is not None:
        i = broken_at - first
        assert 0 <= i < len(off) - 1
        off, brk = np.delete(off, i), np.delete(brk, i)
        brk[i] += rs[broken_at]
    return off, brk


@functools.lru_cache(maxsize=None)
def million_block():
    """The tiled block: 64 distinct raw records, 63 of one slot and one (index 20) of two."""
    f = DataFile("million_slots")
    offs = []
    for j in range(MILLION_BLOCK):
        body = f.filler(300 if j == 20 else 20 + 3 * j)
        offs.append(f.record(b"k%02d" % j, body, ver=j, ts=1000 + j))
    assert len(f) == 65 * 256 and offs[MILLION_TWO_SLOT + 1] - offs[MILLION_TWO_SLOT] == 512
    rs = np.diff(np.asarray(offs + [len(f)], np.int64))
    return bytes(f.b), np.asarray(offs, np.int64), rs


def million_slots(reps: int = MILLION_REPS) -> Million:
    """The block tiled 16,500 times (records do not depend on their position): 1,072,500 slots
    and 1,056,000 records, 262 MiB.  Slots and valid records both exceed 1024 tiles of 1024, so
    k_scan_top runs a second batch in both compactions, and the doubling walks a chain of over a
    million records.  Expected offsets: block offsets + k * len(block).  `reps` below the full
    count gives a prefix (for the pure-Python oracle).  Not cached: 262 MiB, the caller keeps it
    for as long as it needs it."""
    block, boff, brs = million_block()
    data = np.tile(np.frombuffer(block, np.uint8), reps)
    offsets = (np.arange(reps, dtype=np.int64)[:, None] * len(block) + boff[None, :]).ravel()
    return Million(data, block, boff, reps, offsets, np.tile(brs, reps), len(data) // SLOT, MILLION_BLOCK * reps)


def counts(c: Case):
    """(candidates, valid records) in the file, from its headers."""
    s = scan(c.data, c.max_key, c.body_max)
    return len(s), sum(v for _, _, v in s)
