"""The .data images of tests/datafile_cases.py on the host: the sequential restatement of the
reader (oracle/replay.py) returns, on every one of them, the rows written down from the layout --
which pins the oracle against the Go text (store/datafile.go:114-170, 202-277, config/
mc_config.go:33-39, store/item.go:163-176) -- and every file reaches what it claims to reach,
read from its own headers.  The claims are what keeps tests/test_gpu_replay_cases.py from
passing vacuously.  No GPU."""
import struct

import numpy as np
import pytest

import datafile_cases as D
from oracle import oracle as O
from oracle import replay as R


def _oracle(c):
    return R.replay(c.data, c.start, c.max_key, c.body_max)


def _rsize(data, off):
    ksz, vsz = struct.unpack_from("<II", data, off + 16)
    return D.pad256(D.HDR + ksz + vsz)


def test_families_are_all_there():
    fam = {f: len(D.names(f)) for f in ("landing", "bounds", "eof", "embedding", "long_crc", "compressed")}
    assert fam == {"landing": 20, "bounds": 7, "eof": 55, "embedding": 3, "long_crc": 10, "compressed": 1}
    assert len(D.collection()) == sum(fam.values())
    assert max(len(c.data) for c in D.collection()) < 1 << 20


def test_the_builder_s_crc_is_the_record_crc():
    rec = R.make_record(b"key", b"value" * 100, flag=3, ver=-2, ts=99)
    assert D.record_crc(rec[:24 + 3 + 500]) == O.record_crc(rec[4:24], b"key", b"value" * 100) \
        == struct.unpack_from("<I", rec)[0]


@pytest.mark.parametrize("name", D.names())
def test_oracle_returns_the_expected_rows(name):
    c = D.by_name(name)
    rows, err = _oracle(c)
    if c.family == "compressed":
        assert [(r[0], r[1], r[2], r[4], r[5]) for r in rows] == c.rows
    else:
        assert [r[:3] for r in rows] == c.rows
    assert err == c.end_error


@pytest.mark.parametrize("name", D.names("landing", "bounds", "eof", "embedding"))
def test_planted_slot_is_what_it_claims(name):
    """The slot under test gets the verdict the case names, and sits where the case says: at a
    position Next() reads (the start, or the end of a returned record) or only on nextValid's
    way.  The error rule itself, restated: a stream ends in an error exactly when Next() lands
    on a partial header or on valid sizes that run past the end."""
    c = D.by_name(name)
    if "slot" not in c.claims:
        assert name in ("start_at_size", "two_resyncs")
        return
    kind = D.slot_kind(c.data, c.claims["slot"], c.max_key, c.body_max)
    assert kind == c.claims["kind"]
    landings = {c.start} | {off + _rsize(c.data, off) for off, *_ in c.rows}
    assert (c.claims["slot"] in landings) == c.claims["landed"]
    assert (c.end_error is not None) == (c.claims["landed"] and kind in ("trunc", "partial"))
    if "nvalid" in c.claims:
        assert D.counts(c)[1] == c.claims["nvalid"]
    # on a limit, or one past it: read from the planted header, against the reader's parameters
    ksz, vsz = struct.unpack_from("<II", c.data, c.claims["slot"] + 16) if kind != "partial" else (None, None)
    edge = c.claims.get("edge") or {}
    if "ksz" in edge:
        assert ksz - c.max_key == edge["ksz"]
    if "vsz" in edge:
        assert vsz - c.body_max == edge["vsz"]


def test_the_limits_are_met_and_passed_by_one():
    """ksz == max_key and vsz == body_max on valid records, max_key + 1 and body_max + 1 at both
    positions, for the default limits and for max_key 8 / body_max 1000."""
    seen = {(k, d, c.max_key if k == "ksz" else c.body_max)
            for c in D.collection() for k, d in (c.claims.get("edge") or {}).items()}
    assert seen == {(k, d, lim) for k, lims in (("ksz", (250, 8)), ("vsz", (50 << 20, 1000))) for lim in lims
                    for d in (0, 1)} - {("vsz", 0, 50 << 20)}          # a 50 MiB body: not in a small file


def test_both_positions_and_both_limits_are_covered():
    """Every "at both positions" row of the table: the same verdict landed on and walked over;
    the limits as parameters: the default, max_key 8, body_max 1000."""
    by = {}
    for c in D.collection():
        if c.family == "landing":
            by.setdefault(c.name.rsplit("_", 1)[0], set()).add(c.claims["landed"])
    assert len(by) == 10 and all(v == {True, False} for v in by.values())
    lim = {(c.max_key, c.body_max) for c in D.collection()}
    assert lim == {(250, 50 << 20), (8, 50 << 20), (250, 1000), (8, 1000)}
    part = {(len(c.data) - c.claims["slot"], c.claims["landed"])
            for c in D.collection() if c.claims.get("kind") == "partial"}
    assert part == {(n, w) for n in range(1, 24) for w in (True, False)}


@pytest.mark.parametrize("name", list(D.LONG_SPANS))
def test_long_span_is_what_it_claims(name):
    c = D.by_name(name)
    span = D.LONG_SPANS[name]
    big = [(s, v) for _, s, v in D.scan(c.data) if s > 1024]
    assert big == [(span, True), (span, False)]                 # once valid, once a false candidate
    assert c.claims["segmented"] == (span > D.RP_LONG)
    assert c.claims["last_segment"] == (span - 1) % D.RP_SEG + 1
    # the false candidate is one flipped bit, in the last byte of the span, away from valid
    x = [off for off, s, v in D.scan(c.data) if s == span and not v][0]
    img = bytearray(c.data[x: x + 4 + span])
    img[-1] ^= 1
    assert D.record_crc(bytes(img)) == struct.unpack_from("<I", img)[0]


def test_long_spans_cover_the_edges():
    L, S = D.RP_LONG, D.RP_SEG
    assert (L, S) == (128 << 10, 16 << 10)      # gobeansdb_amd/csrc/qlzx_recfile.h kRpLong, kRpSeg
    spans = set(D.LONG_SPANS.values())
    assert {L - 1, L, L + 1, L + S} <= spans
    assert {s % S for s in spans if s > L + S} == {1, 2, 3} and all(s // S > 8 for s in spans if s > L + S)


@pytest.mark.parametrize("variant", D.MANY_LONG)
def test_many_long_candidates(variant):
    """77 candidates over kRpLong, so the list walk of k_rp_crc_long takes a second 64-entry step
    whatever order they were pushed in; and which of them are valid.  In `intact` and
    `outer_broken` every planted header is valid, so the valid count the GPU reports is right
    only if every entry of both steps got its verdict."""
    c = D.by_name(f"many_long_{variant}")
    sc = D.scan(c.data)
    long_ = [(off, s, v) for off, s, v in sc if s > D.RP_LONG]
    assert len(long_) == c.claims["nlong"] == 77 > 64
    # outer and 76 consecutive slots, overlapping claims that all end inside the file
    assert [off for off, _, _ in long_] == [256 * j for j in range(0, 77)]
    assert all(off + 4 + s <= len(c.data) for off, s, _ in long_)
    valid = [off // 256 for off, _, v in long_ if v]
    assert valid == {"intact": list(range(77)), "outer_broken": list(range(1, 77)),
                     "mixed": list(range(70, 77))}[variant]
    assert len(valid) + 1 == sum(v for _, _, v in sc) == c.claims["nvalid"] == D.counts(c)[1]      # + `after`
    assert len(valid) > 64 or variant == "mixed"
    assert len(c.data) < 1 << 20


def test_compressed_bodies_are_what_they_claim():
    c = D.by_name("compressed_bodies")
    kept = [(flag, body) for _, _, _, flag, body in c.rows if flag & D.FLAG_COMPRESS]
    assert [len(b) for _, b in kept] == c.claims["body_lens"]
    assert {0, 1, 2, 3, 8, 9} <= {len(b) for _, b in kept}
    decoded = [body for _, _, _, flag, body in c.rows if not flag & D.FLAG_COMPRESS]
    assert len(decoded) == 2 and len(kept) + len(decoded) == c.claims["ncomp"]
    for off, _, key, flag, body in c.rows:         # every record is stored with FLAG_COMPRESS
        _, _, sflag, _, ksz, vsz = struct.unpack_from("<IIIiII", c.data, off)
        stored = c.data[off + 24 + ksz: off + 24 + ksz + vsz]
        assert sflag == D.FLAG_COMPRESS | 0x20
        if flag & D.FLAG_COMPRESS:
            assert stored == body and O.decompress(body)[0] != O.OK
        else:
            assert O.decompress(stored) == (O.OK, body)     # the one expectation the oracle supplies
    # the two long headers: the right compressed size, dsize 0xFFFFFFFF and exactly BodyMax
    claims = [struct.unpack_from("<BII", b) for _, b in kept if len(b) == 15]
    assert claims == [(0x4F, 15, 0xFFFFFFFF), (0x4F, 15, D.BODY_MAX)]


def test_many_compressed():
    c = D.many_compressed()
    rows, err = _oracle(c)
    assert [r[:3] for r in rows] == c.rows and err is None
    ncomp = sum(1 for off, _, _ in c.rows if struct.unpack_from("<I", c.data, off + 8)[0] & D.FLAG_COMPRESS)
    assert ncomp == c.claims["ncomp"] > 1024 and len(c.rows) == c.claims["nrec"] >= 5000
    assert ((ncomp + 15) // 16 + 63) // 64 >= 2          # every k_rp_dstoff wave: more than one step
    assert sum(1 for r in rows if r[4] & D.FLAG_COMPRESS) == 0      # all of them decode
    dsz = {len(r[5]) for i, r in enumerate(rows) if i % 5 != 4}
    assert len(dsz) > 1024 and min(dsz) == 200 and max(dsz) < 2000 and 2 << 20 < len(c.data) < 8 << 20
    ncand, nvalid = D.counts(c)        # a few slots inside compressed bodies pass the size checks
    assert nvalid == 5000 <= ncand < 5100


def test_million_slots():
    M = D.million_slots()
    assert M.nslots > 1048576 + 2048 and M.nrec > 1048576
    assert M.nslots > D.SCAN_TILE * D.SCAN_TILE and M.nrec > D.SCAN_TILE * D.SCAN_TILE
    blen = len(M.block)
    assert len(M.data) == M.reps * blen == M.nslots * 256
    assert np.array_equal(M.data.reshape(M.reps, blen), np.broadcast_to(np.frombuffer(M.block, np.uint8),
                                                                        (M.reps, blen)))
    # the block: 64 candidates, all valid, none reaching past the block (so tiling adds none)
    sc = D.scan(M.block)
    assert [(off, v) for off, _, v in sc] == [(int(o), True) for o in M.block_off]
    assert all(off + 4 + s <= blen for off, s, _ in sc)
    assert D.scan(M.block + M.block)[64:] == [(off + blen, s, v) for off, s, v in sc]
    assert np.array_equal(M.offsets[:64], M.block_off) and M.offsets[-1] == (M.reps - 1) * blen + M.block_off[-1]
    assert np.array_equal(M.offsets + M.rs, np.append(M.offsets[1:], len(M.data)))      # gap-free


@pytest.mark.parametrize("variant", ["intact", "broken", "start"])
def test_million_slots_prefix_against_the_oracle(variant):
    """The arithmetic expectation (tiled_expect) against the pure-Python oracle on a prefix of 50
    blocks, 3250 slots, for the three variants the GPU test runs on the whole file."""
    P = D.million_slots(50)
    data = bytearray(P.data.tobytes())
    i = 30 * D.MILLION_BLOCK + D.MILLION_TWO_SLOT
    kw = {}
    if variant == "broken":
        data[int(P.offsets[i])] ^= 0x40
        kw = dict(broken_at=i)
    elif variant == "start":
        kw = dict(start=int(P.offsets[i]) + 256)
    off, brk = D.tiled_expect(P.offsets, P.rs, **kw)
    rows, err = R.replay(bytes(data), kw.get("start", 0))
    assert err is None
    assert [r[0] for r in rows] == off.tolist() and [r[1] for r in rows] == brk.tolist()
    assert len(rows) == P.nrec - {"intact": 0, "broken": 1, "start": i + 1}[variant]
    assert sorted(set(brk.tolist())) == {"intact": [0], "broken": [0, 512], "start": [0, 256]}[variant]
