"""GPU batched record writes (record.encode_batch: qlzx_write_plan, qlzx_write_decide, qlzx_write_finish
around two qlzx_compress_batch calls) against the CPU oracle: oracle.compress, oracle/replay.py's
make_record and getvhash, and this file's restatement of Record.TryCompress (store/item.go:120-161).
Every run pre-fills the output with 0xAA and compares the whole buffer."""
import functools
import random

import numpy as np
import pytest
import torch

from gobeansdb_amd import _lib, record
from oracle import oracle as O
from oracle import replay as R

pytestmark = pytest.mark.gpu

FC, FCC = 0x10000, 0x10          # FLAG_COMPRESS, FLAG_CLIENT_COMPRESS
OK, KEY_SIZE, VALUE_SIZE, NO_SPACE = range(4)
FILL = 0xAA


@functools.lru_cache(maxsize=None)
def _compress(v: bytes) -> bytes:
    return O.compress(v)


def _pad256(x: int) -> int:
    return (x + 255) // 256 * 256


def _try_compress(key: bytes, v: bytes, flag: int, ver: int, nc):
    """Record.TryCompress: (stored body, flag, tried)."""
    if ver < 0 or flag & (FCC | FC) or _pad256(24 + len(key) + len(v)) <= 256:
        return v, flag, False
    if not record.need_compress(v[:512], nc):
        return v, flag, False
    t = v[:10240]
    c = _compress(t) if t else b""
    if not t or not (np.float32(len(c)) / np.float32(len(t)) <= np.float32(0.7)):
        return v, flag, True
    if len(v) > len(t):
        c = _compress(v)
    return c, flag + FC, True


def _expect(keys, vals, flags, vers, ts, nc=record.NOT_COMPRESS, max_key=250, body_max=50 << 20, out_cap=None):
    """Per record (status, offset, record bytes, flag, vsz, crc, vhash, tried); the data; the bound."""
    rows, data, bound = [], b"", 0
    for k, v, f, ver, t in zip(keys, vals, flags, vers, ts):
        st = KEY_SIZE if len(k) == 0 or len(k) > max_key else VALUE_SIZE if len(v) > body_max else OK
        if st != OK:
            rows.append((st, 0, b"", 0, 0, 0, 0, False))
            continue
        bound += _pad256(24 + len(k) + len(v) + 9)
        body, fl, tried = _try_compress(k, v, f, ver, nc)
        rec = R.make_record(k, body, flag=fl, ver=ver, ts=t)
        if out_cap is not None and len(data) + len(rec) > out_cap:
            rows.append((NO_SPACE, 0, b"", 0, 0, 0, 0, tried))
            data += b"\0" * len(rec)     # it keeps its place in the layout; nothing of it is written
            continue
        rows.append((OK, len(data), rec, fl, len(body), int.from_bytes(rec[:4], "little"), R.getvhash(v), tried))
        data += rec
    return rows, data, bound


def _pack(blocks, rng, misalign=False):
    """The blocks in one device buffer at uneven offsets (with misalign: never a multiple of 16)."""
    from gobeansdb_amd import batch
    offs, o = [], rng.randrange(1, 16)
    for b in blocks:
        if misalign and o % 16 == 0:
            o += rng.randrange(1, 16)
        offs.append(o)
        o += len(b) + rng.randrange(0, 7)
    host = np.full(o + 64, 0x5C, dtype=np.uint8)
    for p, b in zip(offs, blocks):
        host[p:p + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return batch.BlockBatch(torch.from_numpy(host).cuda(),
                            torch.tensor(offs, dtype=torch.int64).reshape(-1).cuda(),
                            torch.tensor([len(b) for b in blocks], dtype=torch.int32).reshape(-1).cuda())


def _run(keys, vals, flags=None, vers=None, ts=None, nc=record.NOT_COMPRESS, max_key=250, body_max=50 << 20,
         short=None, misalign=False, seed=0):
    """encode_batch into a 0xAA-filled buffer, checked against _expect in full.  short = bytes the
    last record's end lies past out_cap.  Returns (result, rows)."""
    n = len(keys)
    flags = [0] * n if flags is None else flags
    vers = [0] * n if vers is None else vers
    ts = [0] * n if ts is None else ts
    rows, data, bound = _expect(keys, vals, flags, vers, ts, nc, max_key, body_max)
    out_cap = None
    if short is not None:
        out_cap = len(data) - short
        rows, data, bound = _expect(keys, vals, flags, vers, ts, nc, max_key, body_max, out_cap)
    rng = random.Random(seed)
    out = torch.full((bound + 512,), FILL, dtype=torch.uint8, device="cuda")
    res = record.encode_batch(_pack(keys, rng), _pack(vals, rng, misalign), flags=flags, vers=vers, ts=ts,
                              not_compress=nc, max_key=max_key, body_max=body_max, out=out, out_cap=out_cap)
    torch.cuda.synchronize()
    t3 = res.totals.cpu().numpy().view(np.uint32)
    written, nbytes = int(t3[0]), int(t3[1]) | (int(t3[2]) << 32)
    want_bytes = sum(len(r[2]) for r in rows)
    assert (written, nbytes) == (sum(r[0] == OK for r in rows), want_bytes)
    got = out.cpu().numpy()
    # the whole buffer: the records, the hole of a NO_SPACE record and everything past the end untouched
    want = np.full(bound + 512, FILL, dtype=np.uint8)
    for r in rows:
        if r[0] == OK:
            want[r[1]:r[1] + len(r[2])] = np.frombuffer(r[2], dtype=np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (int(bad[0]), int(bad.size))
    if short is None:
        assert got[:nbytes].tobytes() == data and nbytes <= bound
    cols = [res.status.cpu().numpy(), res.offset.cpu().numpy(), res.flag.cpu().numpy().view(np.uint32),
            res.vsz.cpu().numpy().view(np.uint32), res.crc.cpu().numpy().view(np.uint32), res.vhash.cpu().numpy()]
    for i, r in enumerate(rows):
        assert tuple(int(c[i]) for c in cols) == (r[0], r[1], r[3], r[4], r[5], r[6]), i
    assert res.tried.cpu().tolist() == [i for i, r in enumerate(rows) if r[7]]
    assert res.counts[0] == sum(r[0] != KEY_SIZE and r[0] != VALUE_SIZE for r in rows)
    assert res.counts[1] == sum(r[7] for r in rows)
    return res, rows


def _texts():
    return {n: O.gen_text(2, n & 0xff, n) for n in (231, 232, 4096, 10240, 10241, 20000, 70000)}


@pytest.fixture(scope="module")
def texts():
    return _texts()


def test_golden_records(cuda, golden):
    recs = golden.records
    keys = [r["key"].encode() for r in recs]
    vals = [golden.get(r["value"]) for r in recs]
    res, rows = _run(keys, vals, vers=[r["ver"] for r in recs], ts=[r["ts"] for r in recs])
    assert b"".join(r[2] for r in rows) == golden.records_data
    assert [r[1] for r in rows] == [r["offset"] for r in recs]
    assert [r[3] for r in rows] == [r["flag"] for r in recs]
    assert [r[5] for r in rows] == [r["crc"] for r in recs]


def test_policy_edges(cuda, texts):
    rnd400 = np.random.default_rng(1).integers(0, 256, 400, dtype=np.uint8).tobytes()
    img = O.gen_image(5, 0, 30000)
    cases = [  # (value, flag, ver), key b"k": slots of the record, tried, compressed
        (texts[231], 0, 0, 1, False, False),            # one slot: skipped
        (texts[232], 0, 0, 2, True, False),             # tried, ratio above 0.7: raw
        (b"v" * 255, 0, 0, 1, True, True),              # store/data_test.go:41-47: compressed into one slot
        (rnd400, 0, 0, 2, True, False),
        (texts[4096], 0, 0, None, True, True),          # the trial's output is the value
        (texts[10240], 0, 0, None, True, True),
        (texts[10241], 0, 0, None, True, True),         # full recompress
        (texts[20000], 0, 0, None, True, True),
        (img, 0, 0, None, True, False),                 # ratio about 1.0: raw
        (texts[4096], 0, -1, None, False, False),       # ver < 0
        (texts[4096], FCC, 0, None, False, False),      # the client compressed it
        (texts[4096], FC, 0, None, False, False),       # already compressed
        (b"ID3\x03" + texts[4096], 0, 0, None, False, False),   # audio/mpeg
    ]
    vals = [c[0] for c in cases]
    flags = [c[1] for c in cases]
    res, rows = _run([b"k"] * len(cases), vals, flags=flags, vers=[c[2] for c in cases], misalign=True)
    for i, (c, r) in enumerate(zip(cases, rows)):
        assert r[0] == OK
        if c[3] is not None:
            assert len(r[2]) == 256 * c[3], i
        assert r[7] == c[4] and (r[3] == c[1] + FC) == c[5] and (r[3] != c[1]) == c[5], i
    for n in (4096, 10240):     # the trial's ratio, as the issue states it
        assert 0.5 < len(_compress(texts[n])) / n < 0.62
    assert res.counts == (len(cases), 8, 5, 2)


def test_ratio_boundary_in_decide(cuda):
    """qlzx_write_decide alone over made-up trial results: float32(c) / float32(t) <= 0.7f."""
    L = _lib.lib()
    dev = torch.device("cuda")
    t_len = [10240, 10240, 10, 30, 10240, 10240, 5000]
    c_len = [7168, 7169, 7, 21, 100, 7168, 3500]
    stat = [0, 0, 0, 0, 2, 0, 0]
    v_len = [10240, 10240, 10, 30, 10240, 20000, 5000]       # record 5 is longer than its trial
    want = [bool(s == 0 and np.float32(c) / np.float32(t) <= np.float32(0.7)) for t, c, s in zip(t_len, c_len, stat)]
    assert want[:5] == [True, False, True, True, False]
    n = len(t_len)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)     # noqa: E731
    val_off, val_len = torch.arange(n, dtype=torch.int64, device=dev) * 32768, i32(v_len)
    totals = i32([n, n, max(t_len), 0, 0, 0, 0])
    keep = torch.full((n,), 0x55, dtype=torch.uint8, device=dev)
    full_idx, full_len = i32([-1] * n), i32([-1] * n)
    full_off, full_dst = torch.full((n,), -1, dtype=torch.int64, device=dev), torch.full((n,), -1, dtype=torch.int64,
                                                                                        device=dev)
    totals2 = i32([-1] * 5)
    wsb = L.qlzx_write_plan_workspace_size(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    try_idx, try_len, try_csize, try_status = i32(list(range(n))), i32(t_len), i32(c_len), i32(stat)
    _lib.check(L.qlzx_write_decide(val_off.data_ptr(), val_len.data_ptr(), n, totals.data_ptr(),
                                   try_idx.data_ptr(), try_len.data_ptr(),
                                   try_csize.data_ptr(), try_status.data_ptr(), keep.data_ptr(), full_idx.data_ptr(),
                                   full_off.data_ptr(), full_len.data_ptr(), full_dst.data_ptr(), totals2.data_ptr(),
                                   ws.data_ptr(), wsb, None), "qlzx_write_decide")
    torch.cuda.synchronize()
    assert [bool(k) for k in keep.cpu().tolist()] == want
    assert totals2.cpu().tolist() == [sum(want), 1, 20000, _pad256(20000 + 400), 0]
    assert (full_idx[0].item(), full_off[0].item(), full_len[0].item(), full_dst[0].item()) == (5, 5 * 32768, 20000, 0)


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(11).integers(0, 256, 6000, dtype=np.uint8).tobytes()


def test_alignment_sweep(cuda, noise):
    """Plain values (flag 0x10 keeps them raw): every key size moves the value's destination, the
    sources never sit on a 16-B boundary."""
    keys, vals = [], []
    for ksz in list(range(1, 41)) + [249, 250]:
        for j, vlen in enumerate((0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 5000)):
            keys.append(bytes((ksz + j + b) & 0xff or 1 for b in range(ksz)))
            vals.append(noise[(ksz * 7 + j) % 900:][:vlen])
    n = len(keys)
    res, rows = _run(keys, vals, flags=[FCC] * n, vers=list(range(n)), ts=[0x01020304 + i for i in range(n)],
                     misalign=True, seed=4)
    assert res.counts == (n, 0, 0, 0) and all(r[3] == FCC for r in rows)


def test_sniff_on_the_device(cuda):
    from test_record import SNIFF
    vals = [d + bytes(512 - len(d)) for d, _ in SNIFF]
    vals += [pat + bytes(300) for _, pat, _ in record._AV_SIGS]
    short = [pat[:k] for _, pat, _ in record._AV_SIGS for k in (len(pat) - 1, len(pat))]
    short += [b"", b"I", b"RIFF\x01\x02\x03\x04WEBPVP8 ", b"MThd\x00\x00\x00\x07" + bytes(8)]
    vals += short
    keys = [b"k"] * (len(vals) - len(short)) + [b"K" * 240] * len(short)     # short values still pad past one slot
    for nc in (record.NOT_COMPRESS, record.NOT_COMPRESS_SHIPPED, frozenset(), frozenset({None}),
               frozenset({"video/avi", "audio/basic", "application/ogg", "audio/aiff", "audio/midi"})):
        res, rows = _run(keys, vals, nc=nc, seed=len(nc))
        # (the empty value is a candidate too: its trial fails with QLZX_E_EMPTY and it stays raw)
        assert [r[7] for r in rows] == [record.need_compress(v[:512], nc) for v in vals]
    want = [e for _, e in SNIFF]
    assert [record.need_compress(v[:512]) for v in vals[:len(SNIFF)]] == want


def test_statuses(cuda, noise):
    t = O.gen_text(3, 1, 3000)
    keys = [b"a", b"", b"b" * 251, b"c" * 250, b"d", b"e", b"f"]
    vals = [t[:700], t[:300], t[:300], noise[:1000], noise[:1001], t[:900], noise[:333]]
    lim = dict(max_key=250, body_max=1000)
    res, rows = _run(keys, vals, vers=[1] * 7, **lim)
    assert [r[0] for r in rows] == [OK, KEY_SIZE, KEY_SIZE, OK, VALUE_SIZE, OK, OK]
    assert rows[3][1] == len(rows[0][2]) and rows[5][1] == rows[3][1] + len(rows[3][2])   # failed ones take no space
    for short in (1, 255, 256):
        res, rows = _run(keys, vals, vers=[1] * 7, short=short, **lim)
        assert [r[0] for r in rows] == [OK, KEY_SIZE, KEY_SIZE, OK, VALUE_SIZE, OK, NO_SPACE]
    res, rows = _run(keys, vals, vers=[1] * 7, short=513, **lim)      # the last record is 512 bytes
    assert [r[0] for r in rows][-2:] == [NO_SPACE, NO_SPACE]
    res, rows = _run(keys, vals, vers=[1] * 7, short=0, **lim)
    assert [r[0] for r in rows][-2:] == [OK, OK]


def test_long_values(cuda, texts):
    img = O.gen_image(8, 1, 140000)
    big = O.gen_text(4, 9, 400000)
    assert len(_compress(big)) > (128 << 10)             # a compressed value on the segment path
    assert 28000 < len(_compress(texts[70000])) < 36000
    # client-compressed noise is copied as it is, so the image end E = 24 + ksz + vsz is exact: the
    # last wave-per-record size, the first segmented one, no tail bytes, a last segment of one chunk
    noise = np.random.default_rng(3).integers(0, 256, 132000, dtype=np.uint8).tobytes()
    ends = [(128 << 10) + 4, (128 << 10) + 5, (128 << 10) + 64, 8 * (16 << 10) + 16 + 5]
    assert ends[2] % 16 == 0 and (ends[3] & ~15) % (16 << 10) == 16
    keys = [b"img140", b"pre140", b"text70", b"text400"] + [b"edge%d" % i for i in range(4)] + [b"tail"]
    vals = [img, img[::-1], texts[70000], big] + [noise[i:i + e - 29] for i, e in enumerate(ends)] + [b"x" * 40]
    res, rows = _run(keys, vals, flags=[0, FC, 0, 0, FCC, FCC, FCC, FCC, 0], misalign=True, seed=2)
    assert [r[3] for r in rows] == [0, FC, FC, FC, FCC, FCC, FCC, FCC, 0]
    assert [r[4] for r in rows][:2] == [140000, 140000]
    assert [24 + 5 + r[4] for r in rows[4:8]] == ends


def test_stored_block(cuda):
    """The trial passes, the full compress bails out to a stored block: vsz = vlen + 9 and the record
    is one slot longer than the plain one would be (the plan's bound allows for it)."""
    n = 256 * 158 - 25
    v = O.gen_text(2, 0, 10240) + np.random.default_rng(6).integers(0, 256, n - 10240, dtype=np.uint8).tobytes()
    assert len(v) == 40423 and len(_compress(v)) == len(v) + 9
    assert np.float32(len(_compress(v[:10240]))) / np.float32(10240) <= np.float32(0.7)
    res, rows = _run([b"k", b"k2"], [v, b"after"])
    assert rows[0][3] == FC and rows[0][4] == n + 9
    assert len(rows[0][2]) == _pad256(24 + 1 + n) + 256 == rows[1][1]


def _shape_inputs(n):
    rng = random.Random(n)
    text = O.gen_text(7, 3, 1400)
    keys, vals, flags, vers = [], [], [], []
    for i in range(n):
        o, ln = rng.randrange(0, 700), rng.choice((0, 5, 100, 231, 232, 300, 700))
        keys.append(b"key%05d" % i)
        vals.append(text[o:o + ln])
        flags.append(rng.choice((0, 0, 0, FCC, 1)))
        vers.append(rng.randrange(-1, 5))
    return keys, vals, flags, vers


@pytest.mark.parametrize("n", [1, 64, 65, 257, 1100])
def test_batch_shapes(cuda, n):
    keys, vals, flags, vers = _shape_inputs(n)
    res, rows = _run(keys, vals, flags=flags, vers=vers, ts=list(range(n)), seed=n)
    assert all(r[0] == OK for r in rows)


def test_no_candidates_and_no_full_recompress(cuda, texts):
    keys = [b"a", b"b", b"c"]
    res, _ = _run(keys, [texts[4096], texts[231], b""], vers=[-1, 0, 0])
    assert res.counts == (3, 0, 0, 0)
    res, _ = _run(keys, [texts[4096], texts[10240], texts[232]])
    assert res.counts == (3, 3, 2, 0)
    assert record.encode_batch(_pack([], random.Random(0)), _pack([], random.Random(0))).counts == (0, 0, 0, 0)


def test_round_trip_through_the_batched_read(cuda, texts):
    from gobeansdb_amd import replay
    img = O.gen_image(5, 2, 9000)
    vals = [texts[4096], img, texts[20000], b"", b"small", texts[232], O.gen_text(9, 9, 150000)]
    keys = [b"rt%d" % i * (i + 1) for i in range(len(vals))]
    res, rows = _run(keys, vals, vers=list(range(len(vals))), ts=[7] * len(vals), seed=3)
    nbytes = int(res.totals[1])
    rd = replay.read_records(res.data[:nbytes], res.offset, keys=keys)
    torch.cuda.synchronize()
    assert rd.status.cpu().tolist() == [_lib.RD_OK] * len(vals)
    assert rd.key_eq.cpu().tolist() == [1] * len(vals)
    assert [rd.value(i) for i in range(len(vals))] == vals
    assert rd.vhash.cpu().tolist() == [R.getvhash(v) for v in vals] == res.vhash.cpu().tolist()
    assert rd.flag.cpu().tolist() == [0] * len(vals)         # FLAG_COMPRESS came and went


def test_on_a_stream_of_the_callers(cuda, texts):
    from gobeansdb_amd import batch
    rng = random.Random(8)
    vals = [texts[4096], texts[20000], O.gen_image(5, 3, 3000), b"tiny"]
    kb, vb = _pack([b"s%d" % i for i in range(len(vals))], rng), _pack(vals, rng)
    ws = batch.Workspace("cuda")
    ref = record.encode_batch(kb, vb, vers=[3] * len(vals), workspace=ws)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = record.encode_batch(kb, vb, vers=[3] * len(vals), workspace=ws, stream=side)
    side.synchronize()
    nbytes = int(ref.totals[1])
    assert got.counts == ref.counts == (4, 3, 2, 1) and int(got.totals[1]) == nbytes
    assert torch.equal(got.data[:nbytes], ref.data[:nbytes]) and torch.equal(got.crc, ref.crc)
    assert torch.equal(got.offset, ref.offset) and torch.equal(got.vhash, ref.vhash)
