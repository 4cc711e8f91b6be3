"""The rules of tests/wide_records.py, by which tests/test_gpu_wide_records.py derives what the
kernels owe for a 4 GiB buffer from the oracle's answers on small windows, checked here against
the oracle itself on real bytes at a small scale (no GPU)."""
import struct

import numpy as np

import hint_model as H
import wide_records as WR
from oracle import gc as G
from oracle import replay as R


def test_replay_rule_over_zero_gaps():
    """Three windows, each ending in zeros, a 1 MiB run of zeros between the first two and a
    short one before the third; the second window starts with empty slots of its own."""
    a, b, c = WR.chunk(1, 12), WR.chunk(2, 9), WR.chunk(3, 5)
    w0 = a + bytes(768)
    w1 = bytes(512) + b + bytes(1024)
    w2 = c + bytes(256)
    lo1 = len(w0) + (1 << 20)
    lo2 = lo1 + len(w1) + 4096
    whole = w0 + bytes(1 << 20) + w1 + bytes(4096) + w2
    assert len(whole) == lo2 + len(w2) and lo1 % 256 == lo2 % 256 == 0
    win = {0: np.frombuffer(w0, np.uint8), lo1: np.frombuffer(w1, np.uint8), lo2: np.frombuffer(w2, np.uint8)}
    parts = [(lo, WR.replay_rows(win, lo)[0], WR.last_rsize(win, lo)) for lo in (0, lo1, lo2)]
    want, err = R.replay(whole)
    assert err is None and len(want) == 26
    got = WR.join_replays(parts)
    assert got == [tuple(r) for r in want]
    assert [r[1] for r in got if r[1]] == [768 + (1 << 20) + 512, 1024 + 4096]
    # from a later window's start the reader returns that window's rows as they are
    assert [tuple(r) for r in R.replay(whole, start=lo1)[0]] == parts[1][1] + got[21:]


def test_gc_rule_for_a_repeated_record():
    """A 1 KiB record physically three times ahead of a small chunk: the rewrite is its image
    three times, then the small chunk's own rewrite from head 3 * 1 KiB."""
    rec = R.make_record(b"big_one", bytes(range(256)) * 3 + b"tail" * 50, ver=3, ts=1700000000)
    assert len(rec) == 1024
    small = WR.chunk(4, 20)
    keep = [i % 3 != 1 for i in range(20)]
    want = G.gc_rewrite(rec * 3 + small, [True] * 3 + keep, data_file_max=1 << 40)
    tail = G.gc_rewrite(small, keep, data_file_max=1 << 40, dst_head=3 * len(rec))
    assert WR.gc_with_repeats(rec, 3, *tail) == want
    assert want[0][0][:3072] == rec * 3


def test_hint_offset_rule_mod_2_32():
    """hint_model fed offsets reduced mod 2^32 writes the items a reader of the file decodes to
    uint32(rec_off), and its datasize is the header's formula in 32-bit arithmetic -- for records
    that lie across 2^32, one ending exactly there."""
    data = WR.chunk(5, 30)
    rows, _ = R.replay(data)
    recs = R.stream_all(data)[0]
    base = (1 << 32) - recs[14].offset - recs[14].rsize           # record 14 ends exactly at 2^32
    shifted = [(base + row[0],) + tuple(row[1:]) for row in rows]
    model = WR.hint_records(shifted, [(base + r.offset, r) for r in recs])
    assert (model[14][2] + model[14][3]) == 1 << 32 and model[15][2] == 0 and shifted[15][0] == 1 << 32
    sp, = H.build(model, split_cap=64, index_interval=128)
    items = {it.key: it for it in H.read_items(sp.file)}
    assert len(items) == 30 == sp.num_key
    for row in shifted:
        assert items[row[2]].offset == row[0] & WR.M32
    assert sp.datasize == WR.hint_datasize(model) == struct.unpack_from("<qII", sp.file)[2]
    assert sp.datasize == max(m[2] + m[3] for m in model[:14])    # the wrapped ends (0, small) never win
    # the same records below the line: no offset changes, the last record's end is the datasize
    low = WR.hint_records(rows, [(r.offset, r) for r in recs])
    assert H.build(low, split_cap=64, index_interval=128)[0].datasize == len(data)
