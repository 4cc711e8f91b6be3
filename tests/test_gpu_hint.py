"""Hint split files on the GPU (qlzx_keyhash_batch, qlzx_hint_plan / qlzx_hint_write, hint.build;
SURVEY §8 f1c) against tests/hint_model.py fed from the oracle's replay of the same bytes.

Every case builds a chunk with oracle.replay.make_record (zero padding slots between some records),
replays it with replay.replay and compares hint.build's splits with the model's: the file bytes,
consumed, num_key, datasize, n_index and index_offset."""
import functools
import random

import numpy as np
import pytest

import hint_model as H
from oracle import oracle as O
from oracle import replay as R

pytestmark = pytest.mark.gpu
FILL = 0xAA


def _dev(data: bytes, cuda):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(cuda)


def _i64(values, cuda):
    import torch
    return torch.from_numpy(np.asarray(values, dtype=np.uint64).view(np.int64)).to(cuda)


def _key(rnd, n: int) -> bytes:
    return bytes(rnd.choice((rnd.getrandbits(8), 0x80 | rnd.getrandbits(7))) for _ in range(n))


@functools.lru_cache(maxsize=None)
def _chunk(keys: tuple, seed: int = 1, gaps: bool = True, gap_before: int = -1) -> bytes:
    """One record per entry of `keys`, in order: small bodies, a third of the longer ones compressed,
    versions from -3 on, and a zero slot (which the reader resyncs over) before some records."""
    rnd = random.Random(seed)
    out = bytearray()
    for i, key in enumerate(keys):
        if (gaps and rnd.random() < 0.1) or i == gap_before:
            out += bytes(256 * rnd.randint(1, 2))
        body = O.gen_text(seed, i, rnd.randint(301, 700)) if rnd.random() < 0.3 else _key(rnd, rnd.randint(0, 300))
        flag = 0
        if len(body) > 300:
            body, flag = O.compress(body), R.FLAG_COMPRESS
        out += R.make_record(key, body, flag=flag, ver=rnd.randint(-3, 9), ts=1700000000 + i)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def _records(data: bytes):
    """The model's input from the oracle's replay: (keyhash, key, offset, recsize, ver, vhash)."""
    rows, err = R.replay(data)
    recs, _ = R.stream_all(data)
    assert err is None and len(rows) == len(recs)
    return tuple((H.keyhash(row[2]), row[2], row[0], (24 + len(r.key) + len(r.body) + 255) // 256 * 256, row[3],
                  row[6]) for row, r in zip(rows, recs))


def _with_hash(recs, hashes):
    return [(h,) + r[1:] for r, h in zip(recs, hashes)]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g.consumed, g.num_key, g.datasize, g.n_index, g.index_offset, g.skipped) == \
            (w.consumed, w.num_key, w.datasize, w.n_index, w.index_offset, w.skipped)
        assert g.file.cpu().numpy().tobytes() == w.file


def _build(cuda, data: bytes, hashes=None, **kw):
    """hint.build on the device and the model's splits for the same chunk."""
    from gobeansdb_amd import hint, replay
    res = replay.replay(_dev(data, cuda))
    recs = list(_records(data))
    assert res.n == len(recs)
    if hashes is not None:
        recs = _with_hash(recs, hashes)
    got = hint.build(res, keyhash=None if hashes is None else _i64(hashes, cuda), **kw)
    want = H.build(recs, **kw)
    _same(got, want)
    assert sum(g.consumed for g in got) == len(recs)
    return res, recs, got


@functools.lru_cache(maxsize=None)
def _all_lengths():
    rnd = random.Random(3)
    return tuple(_key(rnd, n % 256) for n in range(257))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_keyhash_every_length_unaligned(cuda, n):
    import torch
    from gobeansdb_amd import batch, hint
    keys = _all_lengths()[-n:] if n else ()          # 257: every length 0..255, so every tail and block count
    buf, off = bytearray(b"\xaa"), []
    for i, k in enumerate(keys):
        buf += bytes((i * 7 + 1) % 5)               # every alignment mod 4
        off.append(len(buf))
        buf += k
    b = batch.BlockBatch(_dev(bytes(buf), cuda), _i64(off, cuda),
                         torch.tensor([len(k) for k in keys], dtype=torch.int32, device=cuda))
    got = hint.keyhash(b).cpu().numpy().view(np.uint64).tolist()
    assert got == [H.keyhash(k) for k in keys]
    assert n < 63 or len({o % 4 for o in off}) == 4


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_record_counts_distinct_keys(cuda, n):
    from gobeansdb_amd import hint, replay
    rnd = random.Random(n)
    lens = [1, 250, 2, 3, 4, 5, 249] + [rnd.randint(5, 250) for _ in range(n)]   # lengths below 5 once each
    keys = tuple(_key(rnd, lens[i]) if lens[i] < 5 else _key(rnd, lens[i] - 4) + b"%04d" % i for i in range(n))
    data = _chunk(keys, seed=n)
    res, recs, got = _build(cuda, data, index_interval=128)
    assert len(got) == (1 if n else 0)
    if n:
        assert got[0].num_key == n and (n < 63 or any(r[4] < 0 for r in recs))
        assert [it.key for it in H.read_items(got[0].file.cpu().numpy().tobytes())] == \
            [r[1] for r in sorted(recs, key=lambda r: (r[0], r[1]))]
    else:
        sp = hint.build_split(res, max_offset=77)
        assert (sp.file.numel(), sp.num_key, sp.consumed, sp.datasize, sp.n_index) == (0, 0, 0, 77, 0)
    if n == 257:    # the compressed records' vhash is of the decoded value
        assert any(r.flag & R.FLAG_COMPRESS for r in R.stream_all(data)[0])


def test_duplicates_keep_the_last_version(cuda):
    rnd = random.Random(9)
    names = [_key(rnd, rnd.randint(1, 60)) for _ in range(7)]
    keys = tuple(rnd.choice(names) for _ in range(300))
    res, recs, got = _build(cuda, _chunk(keys, seed=9))
    assert len(got) == 1 and got[0].num_key == 7
    import torch
    from gobeansdb_amd import hint
    side = torch.cuda.Stream()   # the same call on a stream of the caller's: the same file bytes
    on_side = hint.build(res, stream=side)
    side.synchronize()
    assert len(on_side) == 1 and torch.equal(on_side[0].file, got[0].file)
    last = {r[1]: r for r in recs}
    items = H.read_items(got[0].file.cpu().numpy().tobytes())
    assert sorted((i.key, i.offset, i.ver, i.vhash) for i in items) == \
        sorted((r[1], r[2], r[4], r[5]) for r in last.values())


@functools.lru_cache(maxsize=None)
def _collision_keys():
    rnd = random.Random(21)
    base = [_key(rnd, rnd.randint(2, 120)) for _ in range(150)]
    keys = base + [k[:len(k) // 2] for k in base[:70]] + [k + b"\x00" for k in base[:37]]   # prefixes of one another
    keys = list(dict.fromkeys(keys))[:257]
    assert len(keys) == 257
    rnd.shuffle(keys)
    return tuple(keys)


def test_collisions_one_hash_for_257_distinct_keys(cuda):
    keys = _collision_keys()
    for h in (0x1234567800000000, 0xffffffffffffffff):
        res, recs, got = _build(cuda, _chunk(keys, seed=21), hashes=[h] * 257, index_interval=279)
        assert got[0].num_key == 257
        assert [it.key for it in H.read_items(got[0].file.cpu().numpy().tobytes())] == sorted(keys)


def test_collisions_four_hashes_over_40_keys_with_repeats(cuda):
    rnd = random.Random(22)
    names = [_key(rnd, rnd.randint(1, 30)) for _ in range(34)]
    names += [k[:max(1, len(k) - 1)] for k in names[:6]]
    names = list(dict.fromkeys(names))
    hmap = {k: rnd.randrange(4) for k in names}
    keys = tuple(rnd.choice(names) for _ in range(200))
    res, recs, got = _build(cuda, _chunk(keys, seed=22), hashes=[hmap[k] for k in keys], index_interval=128)
    assert got[0].num_key == len(set(keys))
    _build(cuda, _chunk(keys, seed=22), hashes=[hmap[k] for k in keys], split_cap=5, index_interval=303)


def test_hashes_differing_in_one_half_only(cuda):
    rnd = random.Random(23)
    keys = tuple(_key(rnd, 9) for _ in range(64))
    hi = [((63 - i) << 32) | 5 for i in range(32)]          # only the high 32 bits differ
    lo = [(7 << 32) | (0xffffffff - 3 * i) for i in range(32)]  # only the low 32 bits differ
    res, recs, got = _build(cuda, _chunk(keys, seed=23), hashes=hi + lo, index_interval=128)
    items = H.read_items(got[0].file.cpu().numpy().tobytes())
    assert [i.keyhash for i in items] == sorted(hi + lo)


@pytest.mark.parametrize("split_cap", [1, 2, 64])
def test_cut_at_a_full_buffer(cuda, split_cap):
    rnd = random.Random(split_cap)
    names = [b"k%03d" % i + _key(rnd, rnd.randint(0, 20)) for i in range(2 * split_cap + 3)]
    first = names[:split_cap]
    keys = list(first) + [rnd.choice(first) for _ in range(5)]      # repeats after the buffer is full
    cut = len(keys)                                                 # the first new key: a gap before it
    keys += [names[split_cap]] + [rnd.choice(names) for _ in range(3 * split_cap + 20)]
    data = _chunk(tuple(keys), seed=30 + split_cap, gaps=False, gap_before=cut)
    res, recs, got = _build(cuda, data, split_cap=split_cap, index_interval=128)
    assert got[0].consumed == cut and got[0].num_key == split_cap
    assert got[0].datasize == recs[cut][2] > recs[cut - 1][2] + recs[cut - 1][3]   # the rejected record's offset
    assert len(got) >= 2 and got[1].datasize >= got[0].datasize


@functools.lru_cache(maxsize=None)
def _thousand():
    return _chunk(tuple(b"%c%03d" % (65 + i % 7, i) for i in range(1000)), seed=40)


@pytest.mark.parametrize("interval", [128, 279, 280, 303, 4096])
def test_index_rule(cuda, interval):
    res, recs, got = _build(cuda, _thousand(), index_interval=interval)
    file = got[0].file.cpu().numpy().tobytes()
    index = H.load_index(file)
    assert len(index) == got[0].n_index
    if interval <= 279:
        assert got[0].n_index == 1000            # the threshold is not above 0: every item is an entry
    if interval == 4096:
        assert 3 < got[0].n_index < 20
    for it in H.read_items(file)[::37]:
        assert H.get(file, index, it.keyhash, it.key) == it


def test_several_thousand_records(cuda):
    """More records than one workgroup sorts or scans: 6000 one-slot records over 2500 keys, one
    split and several."""
    rnd = random.Random(60)
    keys = [b"%c%05d" % (97 + i % 11, i) for i in range(2500)]
    data = b"".join(R.make_record(rnd.choice(keys), _key(rnd, rnd.randint(0, 40)), ver=rnd.randint(-3, 9))
                    for _ in range(6000))
    res, recs, got = _build(cuda, data, index_interval=1000)
    assert len(got) == 1 and got[0].num_key == len({r[1] for r in recs}) > 2000
    res, recs, got = _build(cuda, data, split_cap=1024, index_interval=4096)
    assert len(got) >= 3 and got[0].num_key == got[1].num_key == 1024


def test_first_max_offset_and_chunk_id(cuda):
    from gobeansdb_amd import hint, replay
    data = _thousand()
    res = replay.replay(_dev(data, cuda))
    recs = list(_records(data))
    top = recs[-1][2] + recs[-1][3] + 4096
    for first, kw in ((1, {}), (333, dict(split_cap=100)), (999, dict(max_offset=top)), (1000, {}), (5000, {})):
        kw = dict(dict(index_interval=400, chunk_id=0x01020304, max_offset=12345), **kw)
        got = hint.build_split(res, first=first, **kw)
        _same([got], [H.build_split(recs, first, **kw)])
    assert hint.build_split(res, first=999, max_offset=top).datasize == top
    items = H.read_items(hint.build_split(res, first=990, chunk_id=0xfffffffe).file.cpu().numpy().tobytes())
    assert len(items) == 10 and {i.chunk_id for i in items} == {0xfffffffe}


def _raw(cuda, res, hdr=None, out=None, out_cap=None, **kw):
    """qlzx_hint_plan + qlzx_hint_write with the test's own hdr / out; (totals, item arrays)."""
    import torch
    from gobeansdb_amd import _lib, batch
    L = _lib.lib()
    n, size = res.n, int(res.data.numel())
    hdr = res.header.contiguous() if hdr is None else hdr
    vh = res.vhash.to(torch.int16).contiguous()
    result = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=cuda)
    item_rec, index_item = (torch.zeros(n, dtype=torch.int32, device=cuda) for _ in range(2))
    item_hash, item_off = (torch.zeros(n, dtype=torch.int64, device=cuda) for _ in range(2))
    totals = torch.zeros(10, dtype=torch.int32, device=cuda)
    wsb = L.qlzx_hint_workspace_size(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    st = batch._stream()
    _lib.check(L.qlzx_hint_plan(res.data.data_ptr(), size, res.offset.data_ptr(), result.data_ptr(), n,
                                hdr.data_ptr(), None, kw.get("first", 0), kw.get("split_cap", 1 << 20),
                                kw.get("index_interval", 4096), kw.get("max_offset", 0), item_rec.data_ptr(),
                                item_hash.data_ptr(), item_off.data_ptr(), index_item.data_ptr(), totals.data_ptr(),
                                ws.data_ptr(), wsb, st), "qlzx_hint_plan")
    if out is not None:
        _lib.check(L.qlzx_hint_write(res.data.data_ptr(), size, res.offset.data_ptr(), n, hdr.data_ptr(),
                                     vh.data_ptr(), kw.get("chunk_id", 0), item_rec.data_ptr(), item_hash.data_ptr(),
                                     item_off.data_ptr(), index_item.data_ptr(), out.data_ptr(), out_cap,
                                     totals.data_ptr(), ws.data_ptr(), wsb, st), "qlzx_hint_write")
    return totals.cpu().numpy().view(np.uint32)


def test_out_guards(cuda):
    import torch
    from gobeansdb_amd import _lib, replay
    data = _chunk(_collision_keys(), seed=21)
    res = replay.replay(_dev(data, cuda))
    want = H.build_split(list(_records(data)), index_interval=128)
    nb = len(want.file)
    assert nb % 16 != 0 and nb % 4 != 0                     # the last chunk is partial, its last dword too
    # one byte short: nothing is written
    out = torch.full((nb + 64,), FILL, dtype=torch.uint8, device=cuda)
    t = _raw(cuda, res, out=out, out_cap=nb - 1, index_interval=128)
    assert t[_lib.HINT_STATUS] == _lib.HINT_NO_SPACE and (out == FILL).all()
    assert int(t[_lib.HINT_BYTES_LO]) == nb
    # exactly enough, at a 16-B aligned but otherwise odd offset of a larger buffer
    big = torch.full((nb + 4096,), FILL, dtype=torch.uint8, device=cuda)
    at = 16 * 9 + (-big.data_ptr()) % 16
    t = _raw(cuda, res, out=big[at:], out_cap=nb, index_interval=128)
    got = big.cpu().numpy()
    assert t[_lib.HINT_STATUS] == 0
    assert got[at:at + nb].tobytes() == want.file
    assert (got[:at] == FILL).all() and (got[at + nb:] == FILL).all()


def test_forged_headers_are_skipped(cuda):
    import torch
    from gobeansdb_amd import _lib, replay
    keys = tuple(b"key%02d" % (i % 9) for i in range(40))
    rnd = random.Random(50)
    data = b"".join(R.make_record(k, _key(rnd, 20), ver=i) for i, k in enumerate(keys))   # one slot each
    res = replay.replay(_dev(data, cuda))
    recs = list(_records(data))
    hdr = res.header.clone()
    hdr[3, 4] = 0                  # ksz = 0
    hdr[17, 4] = 256               # ksz > 255
    hdr[39, 4] = 255               # the key would run past the chunk's end: 39 * 256 + 24 + 255 > size
    hdr[20, 4] = -1
    for j in (3, 17, 39, 20):
        recs[j] = None
    for kw in (dict(index_interval=128), dict(split_cap=4, index_interval=128), dict(first=3, index_interval=300)):
        want = H.build_split(recs, **kw)
        out = torch.full((len(want.file) + 256,), FILL, dtype=torch.uint8, device=cuda)
        t = _raw(cuda, res, hdr=hdr.contiguous(), out=out, out_cap=len(want.file), **kw)
        assert (int(t[0]), int(t[1]), int(t[2]), int(t[3]), int(t[9])) == \
            (want.consumed, want.num_key, want.n_index, want.datasize, want.skipped)
        got = out.cpu().numpy()
        assert got[:len(want.file)].tobytes() == want.file and (got[len(want.file):] == FILL).all()
    assert H.build_split(recs, index_interval=128).skipped == 4


def test_golden_chunk(cuda, golden):
    res, recs, got = _build(cuda, golden.records_data, index_interval=128)
    assert got and sum(g.num_key for g in got) == len({(r[0], r[1]) for r in recs})
    _build(cuda, golden.records_data)
