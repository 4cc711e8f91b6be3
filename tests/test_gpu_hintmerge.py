"""Hint merge on the GPU (qlzx_hint_merge_plan / qlzx_hint_merge_write, hint.merge)
against tests/hintmerge_model.py.

Sources come from hint_model.write_file (any keyhash) unless stated otherwise; every case compares
the file bytes, num_key, datasize, n_index, index_offset, items_read and the collision list."""
import functools
import random
import struct

import numpy as np
import pytest

import hint_model as H
import hintmerge_model as M

pytestmark = pytest.mark.gpu
FILL = 0xAA


def _dev(data: bytes, cuda):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(cuda)


def _key(rnd, n: int) -> bytes:
    return bytes(rnd.choice((rnd.getrandbits(8), 0x80 | rnd.getrandbits(7))) for _ in range(n))


def _source(items, interval=4096, datasize=0) -> bytes:
    return H.write_file(sorted(items, key=lambda it: (it.keyhash, it.key)), datasize, interval)[0]


def _item(rnd, key, kh=None, offset=None):
    return H.Item(H.keyhash(key) if kh is None else kh, key, 0xDEAD,     # the stored chunk is ignored
                  256 * rnd.randrange(1 << 16) if offset is None else offset, rnd.randint(-3, 9), rnd.getrandbits(16))


def _same(got, want, write=True):
    assert (got.num_key, got.datasize, got.n_index, got.index_offset, got.items_read) == \
        (want.num_key, want.datasize, want.n_index, want.index_offset, want.items_read)
    assert got.collisions == want.collisions
    assert got.file.cpu().numpy().tobytes() == (want.file if write else b"")


def _merge(cuda, files, chunks, index_interval=4096, write=True):
    from gobeansdb_amd import hint
    got = hint.merge([_dev(f, cuda) for f in files], chunks, index_interval=index_interval, write=write)
    want = M.merge(files, chunks, index_interval=index_interval, for_gc=not write)
    _same(got, want, write)
    return got, want


@functools.lru_cache(maxsize=None)
def _pool(n: int, seed: int):
    rnd = random.Random(seed)
    return tuple(dict.fromkeys(_key(rnd, rnd.randint(1, 40)) + b"%d" % i for i in range(n)))


def _sources(nsrc, per, seed, intervals=(128, 300, 4096)):
    """nsrc sorted sources of `per` items each over a pool the sources share (so keys repeat)."""
    rnd = random.Random(seed)
    pool = _pool(max(per * 2, per + 3), seed)
    return [_source([_item(rnd, k) for k in rnd.sample(pool, per)], intervals[i % len(intervals)],
                    rnd.getrandbits(32)) for i in range(nsrc)]


@pytest.mark.parametrize("per", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 65])
def test_source_and_item_counts(cuda, nsrc, per):
    files = _sources(nsrc, per, 1000 * nsrc + per)
    rnd = random.Random(nsrc + per)
    got, want = _merge(cuda, files, [rnd.randrange(4) for _ in range(nsrc)], index_interval=300)
    assert got.items_read == nsrc * per and (nsrc == 1 or per == 1 or got.num_key < got.items_read)


def test_six_thousand_items_over_five_sources(cuda):
    """More items than one workgroup sorts or scans."""
    files = _sources(5, 1200, 77)
    got, want = _merge(cuda, files, [3, 1, 4, 1, 5])
    assert got.items_read == 6000 and 1200 < got.num_key < 6000 and got.n_index > 10


# ---- the winner ----
def _winner_case(cuda, offs_a, offs_b, chunks, expect):
    rnd = random.Random(7)
    keys = [b"k%03d" % i for i in range(len(offs_a))]
    a = _source([_item(rnd, k, offset=o) for k, o in zip(keys, offs_a)])
    b = _source([_item(rnd, k, offset=o) for k, o in zip(keys, offs_b)])
    got, want = _merge(cuda, [a, b], chunks)
    items = {it.key: it for it in H.read_items(want.file)}
    assert [(items[k].chunk_id, items[k].offset) for k in keys] == expect


def test_two_splits_of_one_chunk_the_offset_decides(cuda):
    _winner_case(cuda, [256, 1024, 512], [512, 768, 512], [5, 5], [(5, 512), (5, 1024), (5, 512)])


def test_the_higher_chunk_wins_with_the_smaller_offset(cuda):
    _winner_case(cuda, [4096, 8192], [256, 256], [1, 2], [(2, 256), (2, 256)])
    _winner_case(cuda, [4096, 8192], [256, 256], [2, 1], [(2, 4096), (2, 8192)])


def test_offsets_from_2_31_compare_unsigned(cuda):
    _winner_case(cuda, [0x7FFFFF00, 0xFFFFFF00, 0x80000000], [0x80000000, 0x100, 0x7FFFFF00], [3, 3],
                 [(3, 0x80000000), (3, 0xFFFFFF00), (3, 0x80000000)])


@pytest.mark.parametrize("order", ["descending", "shuffled"])
def test_chunk_ids_in_any_order(cuda, order):
    files = _sources(7, 65, 31)
    chunks = [60, 50, 40, 30, 20, 10, 0] if order == "descending" else [3, 0xFFFFFFFE, 0, 7, 3, 1, 0x80000000]
    got, _ = _merge(cuda, files, chunks, index_interval=279)
    import torch
    from gobeansdb_amd import hint
    on_dev = [_dev(f, cuda) for f in files]
    torch.cuda.synchronize()     # the uploads ran on the default stream
    side = torch.cuda.Stream()   # the same call on a stream of the caller's: the same file bytes
    on_side = hint.merge(on_dev, chunks, index_interval=279, stream=side)
    side.synchronize()
    assert torch.equal(on_side.file, got.file) and on_side.num_key == got.num_key


# ---- keys ----
def test_every_key_length_high_bytes_and_prefixes(cuda):
    rnd = random.Random(3)
    every = [_key(rnd, n) for n in range(256)]                       # every length 0..255 once
    every += [k[:len(k) // 2] for k in every[40:90]] + [k + b"\x00" for k in every[1:30]]    # prefixes of one another
    every += [k + b"\xff" for k in every[1:30]]
    every = list(dict.fromkeys(every))
    assert any(b >= 0x80 for k in every for b in k)
    files = [_source([_item(rnd, k, kh=rnd.randrange(8)) for k in rnd.sample(every, 200)], iv)
             for iv in (128, 4096, 700)]
    files.append(_source([_item(rnd, k) for k in every[:256]], 300))
    got, want = _merge(cuda, files, [0, 1, 2, 1], index_interval=303)
    assert {len(it.key) for it in H.read_items(want.file)} >= set(range(256))


# ---- collisions ----
@functools.lru_cache(maxsize=None)
def _collision_keys():
    rnd = random.Random(21)
    base = [_key(rnd, rnd.randint(2, 120)) for _ in range(150)]
    keys = base + [k[:len(k) // 2] for k in base[:70]] + [k + b"\x00" for k in base[:37]]   # prefixes of one another
    keys = list(dict.fromkeys(keys))[:257]
    assert len(keys) == 257
    return tuple(keys)


@pytest.mark.parametrize("kh", [0x1234567800000000, 0xFFFFFFFFFFFFFFFF])
def test_one_hash_for_257_distinct_keys_over_3_sources(cuda, kh):
    keys, rnd = _collision_keys(), random.Random(22)
    parts = [keys[:120], keys[80:200], keys[150:] + keys[:20]]          # repeats across the sources
    files = [_source([_item(rnd, k, kh=kh) for k in p], iv) for p, iv in zip(parts, (128, 4096, 279))]
    got, want = _merge(cuda, files, [2, 0, 1], index_interval=279)
    assert got.num_key == 257 == len(got.collisions)
    assert [c[1] for c in got.collisions] == sorted(keys)


def test_four_hashes_over_40_keys(cuda):
    rnd = random.Random(23)
    names = [_key(rnd, rnd.randint(1, 30)) for _ in range(34)]
    names = list(dict.fromkeys(names + [k[:max(1, len(k) - 1)] for k in names[:6]]))[:40]
    hmap = {k: rnd.randrange(4) for k in names}
    files = [_source([_item(rnd, k, kh=hmap[k]) for k in rnd.sample(names, 25)], 128) for _ in range(4)]
    got, want = _merge(cuda, files, [0, 0, 1, 1], index_interval=128)
    assert len(got.collisions) == got.num_key


def test_hashes_differing_in_one_half_only(cuda):
    rnd = random.Random(24)
    keys = [_key(rnd, 9) for _ in range(64)]
    hi = [((63 - i) << 32) | 5 for i in range(32)]                   # only the high 32 bits differ
    lo = [(7 << 32) | (0xFFFFFFFF - 3 * i) for i in range(32)]       # only the low 32 bits differ
    its = [_item(rnd, k, kh=h) for k, h in zip(keys, hi + lo)]
    files = [_source(its[::2] + its[1:5:2]), _source(its[1::2] + its[60::2])]
    got, want = _merge(cuda, files, [0, 1], index_interval=128)
    assert [it.keyhash for it in H.read_items(want.file)] == sorted(hi + lo) and got.collisions == []


# ---- the output index, the sources' indexes ----
@functools.lru_cache(maxsize=None)
def _thousand():
    rnd = random.Random(40)
    its = [_item(rnd, b"%c%03d" % (65 + i % 7, i)) for i in range(1000)]
    return (_source(its[:400] + its[900:], 4096, 11), _source(its[300:800], 128, 99), _source(its[700:], 1000, 5))


@pytest.mark.parametrize("interval", [128, 279, 280, 303, 4096])
def test_index_rule(cuda, interval):
    got, want = _merge(cuda, list(_thousand()), [0, 0, 1], index_interval=interval)
    assert got.num_key == 1000 and got.datasize == 99
    if interval <= 279:
        assert got.n_index == 1000            # the threshold is not above 0: every item is an entry
    if interval == 4096:
        assert 3 < got.n_index < 20
    file = got.file.cpu().numpy().tobytes()
    index = H.load_index(file)
    for it in H.read_items(file)[::37]:
        assert H.get(file, index, it.keyhash, it.key) == it


def _without_index(f: bytes) -> bytes:
    io, nk, ds = H.read_head(f)
    return struct.pack("<qII", 0, nk, ds) + f[16:io]


def _with_index(f: bytes, offsets) -> bytes:
    io = H.read_head(f)[0]
    return f[:io] + b"".join(struct.pack("<Qq", 0x5555, o) for o in offsets)


def test_a_source_without_an_index(cuda):
    a, b, c = _thousand()
    got, want = _merge(cuda, [a, _without_index(b), c], [0, 0, 1])
    assert want.file == M.merge([a, b, c], [0, 0, 1]).file


@pytest.mark.parametrize("garbage", ["inside an item", "past the file", "decreasing", "first entry below 16",
                                     "more entries than items", "a stretch short of the next entry"])
def test_a_garbage_index_changes_nothing(cuda, garbage):
    a, b, c = _thousand()
    io = H.read_head(a)[0]
    good = [o for _, o in H.load_index(a)]
    assert len(good) >= 3
    bad = {"inside an item": good[:1] + [good[1] + 5] + good[2:],
           "past the file": good[:-1] + [len(a) + 100],
           "decreasing": good[:1] + [good[2], good[1]] + good[3:],
           "first entry below 16": [-8] + good[1:],
           "more entries than items": [16] * 600,
           "a stretch short of the next entry": good[:1] + [good[1] - 1] + good[2:]}[garbage]
    from gobeansdb_amd import hint
    clean = hint.merge([_dev(f, cuda) for f in (a, b, c)], [0, 0, 1])
    dirty = hint.merge([_dev(f, cuda) for f in (_with_index(a, bad), b, c)], [0, 0, 1])
    want = M.merge([a, b, c], [0, 0, 1])
    _same(clean, want)
    _same(dirty, want)


# ---- the raw calls: statuses, capacities ----
def _raw(cuda, files, chunks, lens=None, cap=None, out=None, out_cap=0, write=True, interval=4096):
    """qlzx_hint_merge_plan (+ write) over the packed files with the test's own lengths, cap and out."""
    import torch
    from gobeansdb_amd import _lib, batch
    L = _lib.lib()
    blob = b"".join(files)
    lens = [len(f) for f in files] if lens is None else lens
    offs = np.cumsum([0] + [len(f) for f in files[:-1]]).astype(np.int64)
    if cap is None:
        cap = max(sum(max(n - 16, 0) for n in lens) // 23, 1)
    hints = _dev(blob, cuda)
    off_d, len_d = torch.from_numpy(offs).to(cuda), torch.tensor(lens, dtype=torch.int64, device=cuda)
    chunk_d = torch.tensor(chunks, dtype=torch.int32, device=cuda)
    item_src, item_off = (torch.zeros(cap, dtype=torch.int64, device=cuda) for _ in range(2))
    item_chunk, index_item, coll_item = (torch.zeros(cap, dtype=torch.int32, device=cuda) for _ in range(3))
    totals = torch.zeros(12, dtype=torch.int32, device=cuda)
    wsb = L.qlzx_hint_merge_workspace_size(len(blob), len(files), cap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    st = batch._stream()
    _lib.check(L.qlzx_hint_merge_plan(hints.data_ptr(), len(blob), off_d.data_ptr(), len_d.data_ptr(),
                                      chunk_d.data_ptr(), len(files), cap, interval, item_src.data_ptr(), item_chunk.data_ptr(),
                                      item_off.data_ptr(), index_item.data_ptr(), coll_item.data_ptr(),
                                      totals.data_ptr(), ws.data_ptr(), wsb, st), "qlzx_hint_merge_plan")
    if write:
        _lib.check(L.qlzx_hint_merge_write(hints.data_ptr(), len(blob), cap, item_src.data_ptr(), item_chunk.data_ptr(),
                                           item_off.data_ptr(), index_item.data_ptr(), out.data_ptr(), out_cap,
                                           totals.data_ptr(), ws.data_ptr(), wsb, st), "qlzx_hint_merge_write")
    return totals.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _three():
    return tuple(_sources(3, 65, 55))


@pytest.mark.parametrize("case", ["file_len 15", "indexOffset past the file", "last item cut short", "only a head"])
@pytest.mark.parametrize("at", [0, 2])
def test_bad_file(cuda, case, at):
    import torch
    from gobeansdb_amd import _lib, hint
    files, lens = list(_three()), None
    f = files[at]
    io = H.read_head(f)[0]
    if case == "file_len 15":
        lens = [len(x) for x in files]
        lens[at] = 15
    elif case == "indexOffset past the file":
        files[at] = struct.pack("<q", len(f) + 1) + f[8:]
    elif case == "last item cut short":
        files[at] = struct.pack("<q", 0) + f[8:io - 1]            # no index: the items run to the (cut) end
    else:
        files[at] = struct.pack("<qII", 16, 0, 0)
    if lens is None:
        with pytest.raises(M.BadFile) as e:
            M.merge(files, [0, 1, 2])
        assert e.value.source == at
        with pytest.raises(_lib.QlzxError, match=f"HM_BAD_FILE, source {at}"):
            hint.merge([_dev(x, cuda) for x in files], [0, 1, 2])
    out = torch.full((1 << 15,), FILL, dtype=torch.uint8, device=cuda)
    t = _raw(cuda, files, [0, 1, 2], lens=lens, out=out, out_cap=1 << 15)
    assert (t[_lib.HM_STATUS], t[_lib.HM_STATUS_SOURCE]) == (_lib.HM_BAD_FILE, at)
    assert [t[k] for k in (_lib.HM_NUM_KEY, _lib.HM_N_INDEX, _lib.HM_BYTES_LO, _lib.HM_BYTES_HI,
                           _lib.HM_N_COLLISION)] == [0] * 5
    assert (out == FILL).all()


def test_the_lowest_bad_source_is_named(cuda):
    from gobeansdb_amd import _lib
    files = list(_three())
    files[1] = files[1][:16]
    files[2] = struct.pack("<q", 0) + files[2][8:40]
    t = _raw(cuda, files, [0, 1, 2], write=False)
    assert (t[_lib.HM_STATUS], t[_lib.HM_STATUS_SOURCE]) == (_lib.HM_BAD_FILE, 1)


@pytest.mark.parametrize("case", ["two adjacent items swapped", "a key twice"])
def test_unsorted(cuda, case):
    import torch
    from gobeansdb_amd import _lib, hint
    files = list(_three())
    its = H.read_items(files[1])
    if case == "two adjacent items swapped":
        its[30], its[31] = its[31], its[30]
    else:
        its.insert(31, its[30])
    files[1] = H.write_file(its, 0, 300)[0]
    with pytest.raises(_lib.QlzxError, match="HM_UNSORTED, source 1"):
        hint.merge([_dev(x, cuda) for x in files], [0, 1, 2])
    out = torch.full((1 << 15,), FILL, dtype=torch.uint8, device=cuda)
    t = _raw(cuda, files, [0, 1, 2], out=out, out_cap=1 << 15)
    assert (t[_lib.HM_STATUS], t[_lib.HM_STATUS_SOURCE], t[_lib.HM_NUM_KEY], t[_lib.HM_BYTES_LO]) == \
        (_lib.HM_UNSORTED, 1, 0, 0)
    assert (out == FILL).all()
    # BAD_FILE comes first
    t = _raw(cuda, files[:2] + [files[2][:16]], [0, 1, 2], write=False)
    assert (t[_lib.HM_STATUS], t[_lib.HM_STATUS_SOURCE]) == (_lib.HM_BAD_FILE, 2)


def test_too_many(cuda):
    import torch
    from gobeansdb_amd import _lib
    files = list(_three())
    out = torch.full((1 << 15,), FILL, dtype=torch.uint8, device=cuda)
    t = _raw(cuda, files, [0, 1, 2], cap=3 * 65 - 1, out=out, out_cap=1 << 15)
    assert t[_lib.HM_STATUS] == _lib.HM_TOO_MANY and t[_lib.HM_NUM_KEY] == 0 and (out == FILL).all()
    t = _raw(cuda, files, [0, 1, 2], cap=3 * 65, out=out, out_cap=1 << 15)
    assert t[_lib.HM_STATUS] == _lib.HM_OK and t[_lib.HM_ITEMS_READ] == 3 * 65
    # TOO_MANY comes before UNSORTED
    its = H.read_items(files[1])
    its[3], its[4] = its[4], its[3]
    t = _raw(cuda, [files[0], H.write_file(its, 0, 300)[0], files[2]], [0, 1, 2], cap=3 * 65 - 1, write=False)
    assert t[_lib.HM_STATUS] == _lib.HM_TOO_MANY
    # index entries for more than cap items in all (each source's own claim fits): nothing is proven,
    # every source is walked from 16, and the verdicts are the same
    dense = _sources(3, 65, 56, intervals=(128,))
    assert all(len(H.load_index(f)) == 65 for f in dense)
    t = _raw(cuda, dense, [0, 1, 2], cap=100, write=False)
    assert (t[_lib.HM_STATUS], t[_lib.HM_ITEMS_READ]) == (_lib.HM_TOO_MANY, 3 * 65)
    t = _raw(cuda, [dense[0], dense[1][:-1 - 16 * 65], dense[2]], [0, 1, 2], cap=100, write=False)
    assert (t[_lib.HM_STATUS], t[_lib.HM_STATUS_SOURCE]) == (_lib.HM_BAD_FILE, 1)


def test_no_space_and_an_exact_fit(cuda):
    import torch
    from gobeansdb_amd import _lib
    interval = 300
    for seed in range(50, 70):                             # a file length that is a multiple of neither 16 nor 4
        files = _sources(3, 65, seed)
        want = M.merge(files, [0, 1, 2], index_interval=interval)
        if len(want.file) % 4:
            break
    nb = len(want.file)
    assert nb % 16 != 0 and nb % 4 != 0
    out = torch.full((nb + 64,), FILL, dtype=torch.uint8, device=cuda)
    t = _raw(cuda, files, [0, 1, 2], out=out, out_cap=nb - 1, interval=interval)
    assert t[_lib.HM_STATUS] == _lib.HM_NO_SPACE and (out == FILL).all()
    assert int(t[_lib.HM_BYTES_LO]) == nb and t[_lib.HM_NUM_KEY] == want.num_key
    big = torch.full((nb + 4096,), FILL, dtype=torch.uint8, device=cuda)
    at = 16 * 9 + (-big.data_ptr()) % 16
    t = _raw(cuda, files, [0, 1, 2], out=big[at:], out_cap=nb, interval=interval)
    got = big.cpu().numpy()
    assert t[_lib.HM_STATUS] == _lib.HM_OK
    assert got[at:at + nb].tobytes() == want.file
    assert (got[:at] == FILL).all() and (got[at + nb:] == FILL).all()


def test_plan_alone_is_merge_for_gc(cuda):
    keys, rnd = _collision_keys(), random.Random(25)
    files = [_source([_item(rnd, k, kh=rnd.randrange(30)) for k in rnd.sample(keys, 150)], 300) for _ in range(3)]
    got, want = _merge(cuda, files, [1, 0, 1], write=False)
    assert got.file.numel() == 0 and len(got.collisions) > 100


# ---- end to end on the device ----
def test_replay_build_merge_on_the_device(cuda):
    from gobeansdb_amd import hint, replay
    from oracle import replay as R
    rnd = random.Random(60)
    keys = [b"%c%04d" % (97 + i % 11, i) for i in range(300)]
    got_files, want_files, chunk_ids, every = [], [], [], set()
    for c in (0, 3):
        data = b"".join(R.make_record(rnd.choice(keys), _key(rnd, rnd.randint(0, 40)), ver=rnd.randint(-3, 9),
                                      ts=1700000000 + i) for i in range(400))
        rows, err = R.replay(data)
        recs, _ = R.stream_all(data)
        assert err is None and len(rows) == len(recs) == 400
        model_recs = [(H.keyhash(row[2]), row[2], row[0], (24 + len(r.key) + len(r.body) + 255) // 256 * 256, row[3],
                       row[6]) for row, r in zip(rows, recs)]
        splits = hint.build(replay.replay(_dev(data, cuda)), split_cap=64, chunk_id=c)
        want_splits = H.build(model_recs, split_cap=64, chunk_id=c)
        assert len(splits) == len(want_splits) > 1
        got_files += [sp.file for sp in splits]                     # device tensors: no host copy in between
        want_files += [sp.file for sp in want_splits]
        chunk_ids += [c] * len(splits)
        every |= {(r[0], r[1]) for r in model_recs}
    got = hint.merge(got_files, chunk_ids)
    want = M.merge(want_files, chunk_ids)
    _same(got, want)
    file = got.file.cpu().numpy().tobytes()
    index = H.load_index(file)
    assert got.num_key == len(every)
    for kh, key in every:
        assert H.get(file, index, kh, key).key == key
