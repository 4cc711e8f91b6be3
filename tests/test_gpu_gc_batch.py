"""The device-resident GC rewrite (qlzx_gc_plan / qlzx_gc_rewrite, gc.rewrite_batch)
against the record-by-record restatement of store/gc.go:268-353 in oracle/gc.py and the stream
reader of oracle/replay.py.

Every case compares the destination chunk bytes, the (chunk, offset) positions and the CRCs.  `out`
is pre-filled with 0xAA and is GUARD bytes longer than the expected total: the padding must be
written by the kernel and nothing past the records may be touched."""
import functools
import random

import numpy as np
import pytest

from oracle import gc as G
from oracle import oracle as O
from oracle import replay as R

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0xAA


def _chunk(seed: int, n: int, max_body: int = 3000):
    """test_gc.py's chunk generator, so that its (seed, dfm, head, nxt) rows mean the same data."""
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


@functools.lru_cache(maxsize=None)
def _case(seed: int, n: int = 150, p: float = 0.55):
    """(data, records, keep) shared by the tests that use a seed; never modified."""
    data = _chunk(seed, n)
    recs, _ = R.stream_all(data)
    rnd = random.Random(seed)
    return data, recs, [rnd.random() < p for _ in recs]


def _dev(data: bytes, cuda):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(cuda)


def _out(total: int, cuda):
    import torch
    return torch.full((total + GUARD,), FILL, dtype=torch.uint8, device=cuda)


def _written(res):
    from gobeansdb_amd import _lib
    return (res.status == _lib.GC_WRITTEN).cpu().numpy()


def _check(res, out, want_chunks, want_pos, want_crc):
    """Chunk bytes, positions and CRCs of the written records against the oracle's; the rest of
    `out` untouched."""
    total = sum(len(c) for c in want_chunks)
    got = out.cpu().numpy()
    assert got[:total].tobytes() == b"".join(want_chunks)
    assert (got[total:] == FILL).all()
    nch = len(want_chunks) if total else 0
    assert [c.cpu().numpy().tobytes() for c in res.chunks] == list(want_chunks[:nch])
    w = _written(res)
    pos = list(zip(res.new_chunk.cpu().numpy()[w].tolist(), res.new_off.cpu().numpy()[w].tolist()))
    assert pos == [tuple(p) for p in want_pos]
    assert res.crc.cpu().numpy().view(np.uint32)[w].tolist() == list(want_crc)
    nw = ~w
    assert not res.crc.cpu().numpy()[nw].any() and not res.new_off.cpu().numpy()[nw].any()
    assert not res.new_chunk.cpu().numpy()[nw].any()
    t = res.totals
    assert int(t[2]) == int(w.sum()) and int(t[3]) == nch and int(t[4]) | (int(t[5]) << 32) == total


@pytest.mark.parametrize("seed,dfm,head,nxt", [(5, 1 << 30, 0, ()), (6, 8192, 0, ()), (7, 4096, 2048, ()),
                                              (8, 600, 0, ()), (10, 4096, 1024, (512, 3584)),
                                              (11, 2560, 0, (2048,))])
def test_matches_oracle_and_rewrite(cuda, seed, dfm, head, nxt):
    import torch
    from gobeansdb_amd import _lib, gc, replay
    data, recs, keep = _case(seed)
    want_chunks, want_pos = G.gc_rewrite(data, keep, data_file_max=dfm, dst_head=head, next_heads=nxt)
    d = _dev(data, cuda)
    off = replay.index(d)[0]
    assert off.numel() == len(recs)
    kt = torch.tensor(keep, device=cuda)
    out = _out(sum(map(len, want_chunks)), cuda)
    res = gc.rewrite_batch(d, off, kt, dst_head=head, data_file_max=dfm, next_heads=nxt, out=out)
    torch.cuda.synchronize()
    _check(res, out, want_chunks, want_pos, [r.crc for r, k in zip(recs, keep) if k])
    assert res.status.cpu().tolist() == [_lib.GC_WRITTEN if k else _lib.GC_DROPPED for k in keep]
    t = res.totals
    assert [int(t[0]), int(t[1]), int(t[6]), int(t[7])] == [len(recs), sum(keep), 0, 0]
    # the same answer as the host-planned path, field by field
    old, new = gc.rewrite(d, off, kt, dst_head=head, data_file_max=dfm, next_heads=nxt), res.result()
    torch.cuda.synchronize()
    assert [c.cpu().numpy().tobytes() for c in new.chunks] == [c.cpu().numpy().tobytes() for c in old.chunks]
    assert new.chunk.tolist() == old.chunk.tolist() and new.offset.tolist() == old.offset.tolist()
    assert new.crc.tolist() == old.crc.tolist() and new.crc_mismatch == old.crc_mismatch == 0


@functools.lru_cache(maxsize=None)
def _tails():
    """A 9-byte key with every value length 0..300 (every size % 16 and % 256, exact multiples and
    vsz = 0 included), then keys of 1 and 250 bytes."""
    rnd = random.Random(21)
    recs = [(b"k%08d" % v, rnd.randbytes(v)) for v in range(301)]
    recs += [(b"x", rnd.randbytes(v)) for v in (0, 6, 7, 230, 231, 232)]
    recs += [(bytes([65 + v % 26]) * 250, rnd.randbytes(v)) for v in (0, 1, 237, 238, 239, 500)]
    return b"".join(R.make_record(k, v, ver=i % 7 - 1, ts=1700000000 + i) for i, (k, v) in enumerate(recs))


def test_every_tail_length(cuda):
    import torch
    from gobeansdb_amd import gc, replay
    data = _tails()
    recs, _ = R.stream_all(data)
    assert len(recs) == 313
    want_chunks, want_pos = G.gc_rewrite(data, [True] * len(recs), data_file_max=gc.DATA_FILE_MAX)
    d = _dev(data, cuda)
    off = replay.index(d)[0]
    out = _out(len(data), cuda)
    res = gc.rewrite_batch(d, off, torch.ones(len(recs), dtype=torch.bool, device=cuda), out=out)
    torch.cuda.synchronize()
    _check(res, out, want_chunks, want_pos, [r.crc for r in recs])
    assert want_chunks == [data]


@functools.lru_cache(maxsize=None)
def _longs():
    """Values whose CRC span 20 + ksz + vsz is 131072 (the last wave-per-record size), 131073 and
    well past it, then two segmented ones whose image end E = 24 + ksz + vsz leaves no tail bytes
    (E % 16 == 0) and a last segment of a single 16-byte chunk, between small records."""
    rnd = random.Random(22)
    recs = []
    for i, v in enumerate((131049, 131050, 200000, 131109, 131066)):
        recs.append((b"s%02d" % i, rnd.randbytes(100 + i)))
        recs.append((b"L%02d" % i, rnd.randbytes(v)))
    recs.append((b"end", b"tail"))
    return b"".join(R.make_record(k, v, ts=1700000000 + i) for i, (k, v) in enumerate(recs))


def test_long_records(cuda):
    import torch
    from gobeansdb_amd import gc, replay
    data = _longs()
    recs, _ = R.stream_all(data)
    assert [20 + len(r.key) + len(r.body) for r in recs[1::2]] == [131072, 131073, 200023, 131132, 131089]
    ends = [24 + len(r.key) + len(r.body) for r in recs[7:10:2]]
    assert ends[0] % 16 == 0 and (ends[1] & ~15) % (16 << 10) == 16
    keep = [True, True, False, True, True, True, True, True, True, True, True]
    want_chunks, want_pos = G.gc_rewrite(data, keep, data_file_max=gc.DATA_FILE_MAX)
    d = _dev(data, cuda)
    off = replay.index(d)[0]
    assert off.numel() == 11
    out = _out(len(want_chunks[0]), cuda)
    res = gc.rewrite_batch(d, off, torch.tensor(keep, device=cuda), out=out)
    torch.cuda.synchronize()
    _check(res, out, want_chunks, want_pos, [r.crc for r, k in zip(recs, keep) if k])


def test_chain_without_read_back(cuda):
    """qlzx_replay_index -> qlzx_gc_plan -> qlzx_gc_rewrite on one stream through _lib: `result`
    stays on the device and the host synchronises once, at the end."""
    import torch
    from gobeansdb_amd import _lib
    L = _lib.lib()
    data, recs, keep = _case(6)
    dfm, heads = 32768, [0, 256, 0, 0, 0, 0, 0, 0]
    want_chunks, want_pos = G.gc_rewrite(data, keep, data_file_max=dfm, dst_head=0, next_heads=heads[1:])
    assert 2 < len(want_chunks) <= len(heads)
    total = sum(map(len, want_chunks))
    d = _dev(data, cuda)
    size, cap, mc = len(data), len(data) // 256 + 1, len(heads)
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=cuda)   # noqa: E731
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=cuda)   # noqa: E731
    rec_off, broken, result = i64(cap), i32(cap), torch.zeros(4, dtype=torch.int32, device=cuda)
    kp = torch.zeros(cap, dtype=torch.uint8, device=cuda)
    kp[:len(keep)] = torch.tensor(keep, dtype=torch.uint8)
    hd = torch.tensor(heads, dtype=torch.int64, device=cuda)
    status, new_chunk, new_off, crc = i32(cap), i32(cap), i64(cap), i32(cap)
    base, cbytes, totals = i64(mc), i64(mc), torch.full((8,), 7, dtype=torch.int32, device=cuda)
    out = _out((size + 255) // 256 * 256, cuda)          # pad256(size) always suffices: no read-back
    ws1, ws2 = L.qlzx_replay_workspace_size(size), L.qlzx_gc_workspace_size(cap, mc)
    w1, w2 = torch.empty(ws1, dtype=torch.uint8, device=cuda), torch.empty(ws2, dtype=torch.uint8, device=cuda)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = st.cuda_stream
    _lib.check(L.qlzx_replay_index(d.data_ptr(), size, 0, 250, 50 << 20, rec_off.data_ptr(), broken.data_ptr(),
                                   result.data_ptr(), w1.data_ptr(), ws1, s), "qlzx_replay_index")
    _lib.check(L.qlzx_gc_plan(d.data_ptr(), size, rec_off.data_ptr(), result.data_ptr(), cap, kp.data_ptr(), 250,
                              50 << 20, dfm, hd.data_ptr(), mc, status.data_ptr(), new_chunk.data_ptr(),
                              new_off.data_ptr(), base.data_ptr(), cbytes.data_ptr(), totals.data_ptr(),
                              w2.data_ptr(), ws2, s), "qlzx_gc_plan")
    _lib.check(L.qlzx_gc_rewrite(d.data_ptr(), size, rec_off.data_ptr(), result.data_ptr(), cap, hd.data_ptr(), mc,
                                 new_chunk.data_ptr(), new_off.data_ptr(), base.data_ptr(), out.data_ptr(),
                                 out.numel() - GUARD, status.data_ptr(), crc.data_ptr(), totals.data_ptr(),
                                 w2.data_ptr(), ws2, s), "qlzx_gc_rewrite")
    st.synchronize()
    n = len(recs)
    assert int(result[0]) == n
    t = totals.cpu().numpy().view(np.uint32).tolist()
    assert t == [n, sum(keep), sum(keep), len(want_chunks), total, 0, 0, 0]
    got = out.cpu().numpy()
    assert got[:total].tobytes() == b"".join(want_chunks) and (got[total:] == FILL).all()
    lens = [len(c) for c in want_chunks]
    assert cbytes.cpu().tolist() == lens + [0] * (mc - len(lens))
    assert base.cpu().tolist() == [sum(lens[:c]) for c in range(len(lens))] + [total] * (mc - len(lens))
    w = np.asarray(keep)
    assert list(zip(new_chunk.cpu().numpy()[:n][w].tolist(), new_off.cpu().numpy()[:n][w].tolist())) == want_pos
    assert crc.cpu().numpy().view(np.uint32)[:n][w].tolist() == [r.crc for r, k in zip(recs, keep) if k]


def test_rewritten_chunk_replays_to_the_kept_records(cuda):
    import torch
    from gobeansdb_amd import gc, replay
    data, recs, keep = _case(5)
    d = _dev(data, cuda)
    off = replay.index(d)[0]
    res = gc.rewrite_batch(d, off, torch.tensor(keep, device=cuda))
    assert len(res.chunks) == 1
    new = res.chunks[0].clone()
    noff, _, end_err, _, nvalid = replay.index(new)
    kept = [r for r, k in zip(recs, keep) if k]
    assert not end_err and nvalid == len(kept) == noff.numel()
    assert noff.cpu().tolist() == res.new_off.cpu().numpy()[_written(res)].tolist()
    again, err = R.stream_all(new.cpu().numpy().tobytes())
    assert err is None
    assert [(r.crc, r.ts, r.flag, r.ver, r.key, r.body) for r in again] == \
        [(r.crc, r.ts, r.flag, r.ver, r.key, r.body) for r in kept]


def test_nothing_kept_and_no_records(cuda):
    import torch
    from gobeansdb_amd import _lib, gc, replay
    L = _lib.lib()
    data, recs, _ = _case(5)
    d = _dev(data, cuda)
    off = replay.index(d)[0]
    n = len(recs)
    out = _out(1024, cuda)
    res = gc.rewrite_batch(d, off, torch.zeros(n, dtype=torch.bool, device=cuda), out=out)
    torch.cuda.synchronize()
    assert res.totals.tolist() == [n, 0, 0, 0, 0, 0, 0, 0] and res.chunks == []
    assert (res.status == _lib.GC_DROPPED).all() and not res.crc.any() and (out == FILL).all()
    r0 = res.result()
    assert len(r0.chunk) == 0 and r0.chunks[0].numel() == 0
    # result[0] == 0 on the device, capacity n: zero totals, nothing else written
    result = torch.zeros(4, dtype=torch.int32, device=cuda)
    hd = torch.zeros(2, dtype=torch.int64, device=cuda)
    st, nc, crc = (torch.full((n,), 9, dtype=torch.int32, device=cuda) for _ in range(3))
    no = torch.full((n,), 9, dtype=torch.int64, device=cuda)
    base, cb = torch.full((2,), 9, dtype=torch.int64, device=cuda), torch.full((2,), 9, dtype=torch.int64, device=cuda)
    totals = torch.full((8,), 9, dtype=torch.int32, device=cuda)
    kp = torch.ones(n, dtype=torch.uint8, device=cuda)
    wsb = L.qlzx_gc_workspace_size(n, 2)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(L.qlzx_gc_plan(d.data_ptr(), len(data), off.data_ptr(), result.data_ptr(), n, kp.data_ptr(), 250,
                              50 << 20, 1 << 30, hd.data_ptr(), 2, st.data_ptr(), nc.data_ptr(), no.data_ptr(),
                              base.data_ptr(), cb.data_ptr(), totals.data_ptr(), ws.data_ptr(), wsb, s), "plan")
    assert totals.cpu().tolist() == [0] * 8 and base.cpu().tolist() == [0, 0] and cb.cpu().tolist() == [0, 0]
    totals.fill_(9)
    _lib.check(L.qlzx_gc_rewrite(d.data_ptr(), len(data), off.data_ptr(), result.data_ptr(), n, hd.data_ptr(), 2,
                                 nc.data_ptr(), no.data_ptr(), base.data_ptr(), out.data_ptr(), out.numel(),
                                 st.data_ptr(), crc.data_ptr(), totals.data_ptr(), ws.data_ptr(), wsb, s), "rewrite")
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [0] * 8 and (out == FILL).all()
    assert (st == 9).all() and (crc == 9).all() and (no == 9).all()


def test_bad_entries(cuda):
    """Kept entries that fail readRecordAt's size checks get GC_BAD_RECORD and take no space;
    everything else is the oracle's run without them."""
    import struct
    import torch
    from gobeansdb_amd import _lib, gc, replay
    good, recs, keep = _case(7)
    # two slots the reader skips: a header with ksz = 0, and one whose body runs past EOF
    data = good + bytes(256) + struct.pack("<IIIiII", 1, 2, 0, 0, 5, 1000) + bytes(200)
    assert len(R.stream_all(data)[0]) == len(recs)
    want_chunks, want_pos = G.gc_rewrite(data, keep, data_file_max=4096, dst_head=2048)
    d = _dev(data, cuda)
    off = replay.index(d)[0].cpu().tolist()
    assert off == [r.offset for r in recs]
    bad = {3: off[3] + 8, 40: len(good) + 1024, 41: len(good), 100: len(good) + 256}   # 40: a slot past size
    offs, kp = list(off), list(keep)
    for at in sorted(bad):
        offs.insert(at, bad[at])
        kp.insert(at, True)
    out = _out(sum(map(len, want_chunks)), cuda)
    res = gc.rewrite_batch(d, torch.tensor(offs, dtype=torch.int64, device=cuda), torch.tensor(kp, device=cuda),
                           dst_head=2048, data_file_max=4096, out=out)
    torch.cuda.synchronize()
    _check(res, out, want_chunks, want_pos, [r.crc for r, k in zip(recs, keep) if k])
    st = res.status.cpu().tolist()
    assert [j for j, v in enumerate(st) if v == _lib.GC_BAD_RECORD] == sorted(bad)
    t = res.totals
    assert [int(t[0]), int(t[1]), int(t[2]), int(t[7])] == [len(offs), sum(kp), sum(keep), 4]


def test_max_chunks_exhausted(cuda):
    import torch
    from gobeansdb_amd import _lib, gc, replay
    data, recs, keep = _case(8)
    want_chunks, want_pos = G.gc_rewrite(data, keep, data_file_max=600)
    assert len(want_chunks) > 3
    placed = sum(1 for c, _ in want_pos if c < 3)
    d = _dev(data, cuda)
    off = replay.index(d)[0]
    out = _out(sum(map(len, want_chunks[:3])), cuda)
    res = gc.rewrite_batch(d, off, torch.tensor(keep, device=cuda), data_file_max=600, max_chunks=3, out=out)
    torch.cuda.synchronize()
    _check(res, out, want_chunks[:3], want_pos[:placed], [r.crc for r, k in zip(recs, keep) if k][:placed])
    kept = [j for j, k in enumerate(keep) if k]
    st = res.status.cpu().tolist()
    assert [st[j] for j in kept] == [_lib.GC_WRITTEN] * placed + [_lib.GC_NO_CHUNK] * (len(kept) - placed)
    assert int(res.totals[7]) == len(kept) - placed and int(res.totals[1]) == len(kept)


def test_out_cap_short_by_one_record(cuda):
    import torch
    from gobeansdb_amd import _lib, gc, replay
    data, recs, keep = _case(5)
    want_chunks, want_pos = G.gc_rewrite(data, keep, data_file_max=1 << 30)
    kept = [r for r, k in zip(recs, keep) if k]
    total, last = len(want_chunks[0]), kept[-1].rsize
    d = _dev(data, cuda)
    off = replay.index(d)[0]
    out = _out(total, cuda)
    res = gc.rewrite_batch(d, off, torch.tensor(keep, device=cuda), out=out[:total - 256])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[:total - last].tobytes() == want_chunks[0][:total - last]      # the earlier records, intact
    assert (got[total - last:] == FILL).all()                                 # nothing of the last one
    st = res.status.cpu().tolist()
    jl = max(j for j, k in enumerate(keep) if k)
    assert st[jl] == _lib.GC_NO_SPACE and st.count(_lib.GC_NO_SPACE) == 1 and int(res.crc[jl]) == 0
    w = _written(res)
    assert res.crc.cpu().numpy().view(np.uint32)[w].tolist() == [r.crc for r in kept[:-1]]
    t = res.totals
    assert [int(t[1]), int(t[2]), int(t[4]), int(t[5]), int(t[6]), int(t[7])] == \
        [len(kept), len(kept) - 1, total - last, 0, 0, 1]


def test_crc_mismatch_is_rewritten_and_counted(cuda):
    import torch
    from gobeansdb_amd import gc, replay
    data, recs, keep = _case(5)
    j = next(i for i, (r, k) in enumerate(zip(recs, keep)) if k and len(r.body) > 40)
    r = recs[j]
    at = r.offset + R.HDR + len(r.key) + 17
    d = _dev(data, cuda)
    off = replay.index(d)[0]
    d[at] ^= 0x5A                                         # after indexing: the stored CRC is now stale
    body = bytearray(r.body)
    body[17] ^= 0x5A
    fixed = R.make_record(r.key, bytes(body), flag=r.flag, ver=r.ver, ts=r.ts)
    want_crc = int.from_bytes(fixed[:4], "little")
    assert want_crc != r.crc
    altered = data[:r.offset] + fixed + data[r.offset + r.rsize:]
    want_chunks, want_pos = G.gc_rewrite(altered, keep, data_file_max=1 << 30)
    out = _out(len(want_chunks[0]), cuda)
    res = gc.rewrite_batch(d, off, torch.tensor(keep, device=cuda), out=out)
    torch.cuda.synchronize()
    crcs = [want_crc if i == j else q.crc for i, (q, k) in enumerate(zip(recs, keep)) if k]
    _check(res, out, want_chunks, want_pos, crcs)
    assert int(res.totals[6]) == 1 and res.result().crc_mismatch == 1
    assert int(res.crc[j]) & 0xFFFFFFFF == want_crc != r.crc
