"""Hint lookups on the GPU (qlzx_hint_lookup, hint.lookup) against
tests/hintlookup_model.py.

Every case goes through _check: the raw call with every file at an odd offset of one buffer and
every key at an odd offset of another, outputs pre-filled with 0xAA and eight guard entries behind
the n, in both modes (the reference as it is, QLZX_HL_F_BOUNDED) and both kernels (QLZX_HL_F_WAVE,
QLZX_HL_F_LANE: a wave or a lane per request); all seven outputs and totals are compared with the
model.  test_the_kernel_goes_by_the_request_count covers the library's own choice."""
import functools
import random
import struct

import numpy as np
import pytest

import hint_model as H
import hintlookup_model as M

pytestmark = pytest.mark.gpu
FILL, GUARD = 0xAA, 8
TOP = 2 ** 64 - 1


def _dev(data: bytes, cuda):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(cuda)


def _pack_odd(blocks, fill):
    """One buffer with every block at an odd offset: (bytes, offsets)."""
    blob, offs = bytearray(), []
    for b in blocks:
        blob += bytes([fill]) * (1 if len(blob) % 2 == 0 else 2)
        offs.append(len(blob))
        blob += b
    return bytes(blob) + bytes([fill]) * 3, offs


def _raw(cuda, blob, offs, lens, chunks, merged, keys, hashes, flags, nbytes=None):
    """qlzx_hint_lookup with caller-made buffers: (rows of the seven outputs, totals)."""
    import torch
    from gobeansdb_amd import _lib, batch
    L = _lib.lib()
    n, nf = len(keys), len(offs)
    kblob, koff = _pack_odd(keys, 0x55)
    i64 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.uint64).view(np.int64)).to(cuda)
    i32 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.uint32).view(np.int32)).to(cuda)
    hints, kd = _dev(blob, cuda), _dev(kblob, cuda)
    assert hints.data_ptr() % 16 == 0 and kd.data_ptr() % 16 == 0          # so the odd offsets are odd addresses
    off_d, len_d, chunk_d = i64(offs), i64(lens), i32(chunks)
    flag_d = i32([_lib.HL_FILE_MERGED if i == merged else 0 for i in range(nf)])
    koff_d, klen_d = i64(koff), i32([len(k) for k in keys])
    hash_d = None if hashes is None else i64(hashes)
    outs = [torch.full((n + GUARD,), FILL, dtype=torch.uint8, device=cuda).repeat_interleave(w).view(dt)
            for w, dt in ((4, torch.int32),) * 5 + ((2, torch.int16), (8, torch.int64))]
    totals = torch.full((4 + GUARD,), FILL, dtype=torch.uint8, device=cuda).repeat_interleave(4).view(torch.int32)
    wsb = L.qlzx_hint_lookup_workspace_size(n, nf)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    _lib.check(L.qlzx_hint_lookup(hints.data_ptr(), len(blob) if nbytes is None else nbytes, off_d.data_ptr(),
                                  len_d.data_ptr(), chunk_d.data_ptr(), flag_d.data_ptr(), nf, kd.data_ptr(),
                                  koff_d.data_ptr(), klen_d.data_ptr(), batch._ptr(hash_d), n, flags,
                                  *[o.data_ptr() for o in outs], totals.data_ptr(), ws.data_ptr(), wsb,
                                  batch._stream()), "qlzx_hint_lookup")
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for h in host:                                                         # nothing outside [0, n) changed
        assert (h[n:].view(np.uint8) == FILL).all()
    t = totals.cpu().numpy()
    assert (t[4:].view(np.uint8) == FILL).all()
    cols = [host[0].astype(np.int64), host[1].view(np.uint32), host[2].view(np.uint32), host[3].view(np.uint32),
            host[4].astype(np.int64), host[5].view(np.uint16), host[6].view(np.uint64)]
    return [tuple(int(c[i]) for c in cols) for i in range(n)], [int(x) for x in t[:4].view(np.uint32)]


def _check(cuda, files, chunks, keys, merged=None, hashes=None, lens=None, nbytes=None, modes=(False, True),
           shapes=(2, 4)):
    """The device against the model, per mode and kernel (shapes: QLZX_HL_F_LANE = 2, QLZX_HL_F_WAVE = 4,
    0 = the library's choice by n); returns {bounded: model results}."""
    from gobeansdb_amd import _lib
    assert (_lib.HL_F_LANE, _lib.HL_F_WAVE) == (2, 4)
    blob, offs = _pack_odd(files, 0xEE)
    lens = [len(f) for f in files] if lens is None else lens
    size = len(blob) if nbytes is None else nbytes
    seen = [None if o + n > size else f[:n] for f, o, n in zip(files, offs, lens)]
    model = {}
    for bounded in modes:
        want, totals = M.lookup(seen, offs, chunks, merged, keys, hashes, bounded)
        model[bounded] = want
        for shape in shapes:
            flags = (_lib.HL_F_BOUNDED if bounded else 0) | shape
            got, got_totals = _raw(cuda, blob, offs, lens, chunks, merged, keys, hashes, flags, nbytes)
            bad = [(i, g, w.astuple()) for i, (g, w) in enumerate(zip(got, want)) if g != w.astuple()]
            assert not bad, (bounded, shape, bad[:5])
            assert got_totals == totals, (bounded, shape)
    return model


def _key(rnd, n: int) -> bytes:
    return bytes(rnd.choice((rnd.getrandbits(8), 0x80 | rnd.getrandbits(7))) for _ in range(n))


def _item(rnd, kh, key, chunk=0xBEEF):
    return H.Item(kh, key, chunk, 256 * rnd.randrange(1, 1 << 16), rnd.randint(-3, 9), rnd.getrandbits(16))


def _build(items, entries) -> bytes:
    """A file with index entries for the items `entries` names (a writer's layout, the test's choice
    of entries)."""
    body, offs = bytearray(16), []
    for it in items:
        offs.append(len(body))
        body += struct.pack("<QIIiHB", it.keyhash, it.chunk_id, it.offset, it.ver, it.vhash, len(it.key)) + it.key
    io = len(body)
    for e in entries:
        body += struct.pack("<Qq", items[e].keyhash, offs[e])
    body[:16] = struct.pack("<qII", io, len(items), 0)
    return bytes(body)


def _around(items):
    """Every item by its own key, and absent keys at, below and above every keyhash."""
    hs, ks = [], []
    for it in items:
        for kh, k in ((it.keyhash, it.key), (it.keyhash, it.key + b"?"), (it.keyhash - 1, it.key),
                      (it.keyhash + 1, b"absent")):
            hs.append(kh & TOP)
            ks.append(k)
    return hs + [0, 1, 2 ** 63, TOP], ks + [b"lo", b"", b"mid", b"hi"]


# ---- index edges ----
@pytest.mark.parametrize("entries", [(), (0,), (3,), (0, 5), (2, 7), (0, 4, 8), (1, 5, 11)])
def test_index_edges(cuda, entries):
    """0, 1, 2 and 3 entries; targets below the first, at each, between and above the last: j = 0, 1, 2, len."""
    rnd = random.Random(len(entries))
    items = [_item(rnd, 1000 * (i + 1), _key(rnd, rnd.randint(1, 30))) for i in range(12)]
    f = _build(items, entries)
    assert len(H.load_index(f)) == len(entries)
    hs, ks = _around(items)
    model = _check(cuda, [f], [4], ks, hashes=hs)
    js = {M.go_sort_search(len(entries), lambda i: items[entries[i]].keyhash >= h) for h in hs}
    assert js == set(range(len(entries) + 1))
    for b in (False, True):
        assert [r.status for r in model[b][:4 * 12:4]] == [M.FOUND] * 12     # every item by its own key


@pytest.mark.parametrize("count", [1, 2, 3])
def test_a_writers_file_of_one_to_three_items(cuda, count):
    rnd = random.Random(count)
    items = [_item(rnd, 10 * (i + 1), b"%c" % (97 + i)) for i in range(count)]
    f, io, nidx = H.write_file(items, 0, 128)
    assert nidx == count
    hs, ks = _around(items)
    _check(cuda, [f], [0], ks, hashes=hs)


# ---- equal-hash runs ----
def test_a_run_of_five_keys_with_one_hash(cuda):
    rnd = random.Random(5)
    run = sorted(_key(rnd, rnd.randint(1, 20)) for _ in range(5))
    items = [_item(rnd, 50 + i, b"before%d" % i) for i in range(4)] + [_item(rnd, 700, k) for k in run] + \
            [_item(rnd, 900 + i, b"after%d" % i) for i in range(4)]
    f, io, nidx = H.write_file(items, 0, 128)             # every item has an entry: some sit inside the run
    index = H.load_index(f)
    assert nidx == len(items) and sum(kh == 700 for kh, _ in index) == 5
    absent = _key(rnd, 21)
    model = _check(cuda, [f], [1], run + [absent], hashes=[700] * 6)
    for b in (False, True):
        assert [r.status for r in model[b]] == [M.FOUND] * 5 + [M.MISS]
        assert len({r.item_src for r in model[b][:5]}) == 5


# ---- into the index ----
@functools.lru_cache(maxsize=None)
def _small_hash_file(count):
    rnd = random.Random(100 + count)
    items = [_item(rnd, 10 * (i + 1), _key(rnd, 1 + i % 3)) for i in range(count)]
    f, io, nidx = H.write_file(items, 0, 128)
    assert nidx == count
    return items, f


def test_targets_above_the_last_item_walk_into_the_index(cuda):
    unbounded = []
    for count in (2, 3, 40):
        items, f = _small_hash_file(count)
        above = [items[-1].keyhash + 1, items[-1].keyhash + 7, 0x2801, 2 ** 40, 2 ** 63, TOP]
        keys = [b"above"] * len(above) + [items[-1].key]
        model = _check(cuda, [f], [2], keys, hashes=above + [items[-1].keyhash])
        unbounded += [r.status for r in model[False][:-1]]
        assert [r.status for r in model[True][:-1]] == [M.MISS] * len(above)
        assert model[False][-1].status == model[True][-1].status == M.FOUND      # a present key of the last stretch
    assert M.ERR in unbounded and M.MISS in unbounded and set(unbounded) <= {M.ERR, M.MISS}    # from the model


# ---- keys ----
def test_key_lengths_high_bytes_and_prefixes(cuda):
    rnd = random.Random(9)
    long = _key(rnd, 255)
    stored = [b"", long, b"\x80\xff\xfe", b"prefix", b"prefix-and-more", _key(rnd, 64), _key(rnd, 65), _key(rnd, 128)]
    items = sorted((_item(rnd, H.keyhash(k), k) for k in stored), key=lambda it: (it.keyhash, it.key))
    f = H.write_file(items, 0, 300)[0]
    wanted = stored + [b"prefi", b"prefix-", b"prefix-and-more!", long[:254], long + b"x", long + _key(rnd, 45),
                       stored[5][:63] + b"\x00", stored[6][:64] + bytes([stored[6][64] ^ 0x80])]
    assert {len(k) for k in wanted} >= {0, 255, 256, 300}
    model = _check(cuda, [f], [6], wanted)                                 # the default hash, on the device
    assert [r.status for r in model[True]] == [M.FOUND] * len(stored) + [M.MISS] * 8
    # the same walk under the stored key's hash: the candidate is compared and refused
    hashes = [H.keyhash(k) for k in stored] + [H.keyhash(b"prefix")] * 2 + [H.keyhash(b"prefix-and-more")] + \
             [H.keyhash(long)] * 3 + [H.keyhash(stored[5]), H.keyhash(stored[6])]
    model = _check(cuda, [f], [6], wanted, hashes=hashes)
    assert [r.status for r in model[True]] == [M.FOUND] * len(stored) + [M.MISS] * 8


def test_an_explicit_keyhash_replaces_the_default(cuda):
    rnd = random.Random(10)
    keys = [b"key%d" % i for i in range(40)]
    mine = {k: rnd.getrandbits(64) for k in keys}
    assert all(mine[k] != H.keyhash(k) for k in keys)
    items = sorted((_item(rnd, mine[k], k) for k in keys), key=lambda it: (it.keyhash, it.key))
    f = H.write_file(items, 0, 300)[0]
    model = _check(cuda, [f], [0], keys, hashes=[mine[k] for k in keys], modes=(True,))
    assert all(r.status == M.FOUND for r in model[True])
    model = _check(cuda, [f], [0], keys, modes=(True,))                    # the default hash finds none of them
    assert all(r.status == M.MISS for r in model[True])


# ---- order across files ----
def _order_files():
    rnd = random.Random(11)
    mk = lambda spec, chunk: H.write_file([H.Item(kh, k, chunk, off, 1, 2) for kh, k, off in spec], 0, 4096)[0]
    f0 = mk([(10, b"a", 0x300), (15, b"e", 0xA00)], 70)
    f1 = mk([(10, b"a", 0x200), (20, b"b", 0x500)], 71)
    f2 = mk([(10, b"a", 0x100), (20, b"b", 0x400), (25, b"f", 0xB00)], 72)
    mg = mk([(10, b"a", 0x000), (20, b"b", 0x400), (30, b"c", 0x600)], 5)
    old = mk([(40, b"d", 0x700), (10, b"a", 0x800)][::-1], 73)
    return [f0, f1, f2, mg, old], [9, 9, 8, 0, 1]


def test_the_first_file_in_the_order_wins(cuda):
    files, chunks = _order_files()
    keys, hs = [b"a", b"b", b"f", b"c", b"d", b"e", b"zz"], [10, 20, 25, 30, 40, 15, 10]
    model = _check(cuda, files, chunks, keys, merged=3, hashes=hs)
    for b in (False, True):
        got = [(r.status, r.hit_file, r.chunk, r.offset) for r in model[b]]
        assert got == [(M.FOUND, 0, 9, 0x300), (M.FOUND, 1, 9, 0x500), (M.FOUND, 2, 8, 0xB00),
                       (M.FOUND, 3, 5, 0x600),             # merged: the chunk stored in the item
                       (M.MISS, 3, 0, 0),                  # nothing after the merged file is searched
                       (M.FOUND, 0, 9, 0xA00), (M.MISS, 3, 0, 0)]
    model = _check(cuda, files, chunks, keys, merged=None, hashes=hs)
    assert (model[True][4].status, model[True][4].hit_file, model[True][4].chunk) == (M.FOUND, 4, 1)
    model = _check(cuda, files[3:], chunks[3:], keys, merged=0, hashes=hs)     # the merged file first
    assert [r.status for r in model[True]] == [M.FOUND, M.FOUND, M.MISS, M.FOUND, M.MISS, M.MISS, M.MISS]


def test_an_error_in_file_0_ends_the_search(cuda):
    f0 = H.write_file([H.Item(kh, k, 0, 0, 0, 0) for kh, k in ((10, b"a"), (20, b"b"), (30, b"c"))], 0, 128)[0]
    f1 = H.write_file([H.Item(2 ** 63, b"d", 0, 0x900, 3, 4)], 0, 128)[0]
    model = _check(cuda, [f0, f1], [4, 3], [b"d", b"c"], hashes=[2 ** 63, 30])
    assert model[False][0].astuple() == (M.ERR, 0, 0, 0, 0, 0, 0)
    assert model[True][0].astuple()[:6] == (M.FOUND, 1, 3, 0x900, 3, 4)


# ---- shapes ----
@functools.lru_cache(maxsize=None)
def _spread(nf, per, seed):
    """nf files of `per` items with the default hash, and keys: half stored somewhere, half absent."""
    rnd = random.Random(seed)
    files, stored = [], []
    for i in range(nf):
        ks = list(dict.fromkeys(_key(rnd, rnd.randint(1, 24)) + b"%d" % i for _ in range(per)))
        items = sorted((_item(rnd, H.keyhash(k), k) for k in ks), key=lambda it: (it.keyhash, it.key))
        files.append(H.write_file(items, 0, (128, 600, 4096)[i % 3])[0])
        stored += ks
    return tuple(files), tuple(stored)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("nf", [1, 2, 65])
def test_request_and_file_counts(cuda, n, nf):
    files, stored = _spread(nf, 30, nf)
    rnd = random.Random(n * 100 + nf)
    keys = [rnd.choice(stored) if i % 2 == 0 else _key(rnd, 9) + b"-absent" for i in range(n)]
    model = _check(cuda, list(files), [nf - i for i in range(nf)], keys)
    assert all(r.status == M.FOUND for r in model[True][::2])
    assert all(r.status == M.MISS and r.hit_file == nf - 1 for r in model[True][1::2])


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_the_kernel_goes_by_the_request_count(cuda, delta, monkeypatch):
    """Without QLZX_HL_F_WAVE / QLZX_HL_F_LANE: a wave per request below QLZX_HL_LANE_FROM requests, a
    lane per request from there on.  The requests cycle through 96 distinct ones, so the model runs once
    for each."""
    from gobeansdb_amd import _lib
    files, stored = _spread(2, 30, 77)
    rnd = random.Random(78)
    pool = [rnd.choice(stored) if i % 2 == 0 else _key(rnd, 9) + b"-absent" for i in range(96)]
    n = _lib.HL_LANE_FROM + delta
    keys = [pool[i % 96] for i in range(n)]
    lookup = M.lookup

    def cycled(fs, offs, chunks, merged, ks, hashes=None, bounded=False):
        out, _ = lookup(fs, offs, chunks, merged, ks[:96], hashes, bounded)
        out = [out[i % 96] for i in range(len(ks))]
        return out, [sum(r.status == s for r in out) for s in (M.FOUND, M.MISS, M.ERR, M.BAD_FILE)]

    monkeypatch.setattr(M, "lookup", cycled)
    model = _check(cuda, list(files), [1, 0], keys, shapes=(0,))
    assert sum(r.status == M.FOUND for r in model[True]) >= n // 2


def test_a_file_without_index_entries_is_walked_whole(cuda):
    """3,000 items and no entry: one stretch of the whole file, many LDS windows."""
    rnd = random.Random(12)
    items = [_item(rnd, 1000 + 3 * i, _key(rnd, rnd.randint(1, 60))) for i in range(3000)]
    f, io, nidx = H.write_file(items, 0, 1 << 30)
    assert nidx == 0 and len(f) > 20 * 4096
    pick = [items[0], items[1500], items[2999]]
    model = _check(cuda, [f], [3], [it.key for it in pick] + [b"absent", b"beyond"],
                   hashes=[it.keyhash for it in pick] + [1000 + 3 * 1500 + 1, TOP])
    for b in (False, True):
        assert [r.status for r in model[b]] == [M.FOUND] * 3 + [M.MISS] * 2
    assert model[True][2].item_src > 20 * 4096


# ---- damage: each one edit away from a valid file ----
@functools.lru_cache(maxsize=None)
def _valid():
    rnd = random.Random(13)
    items = [_item(rnd, 100 * (i + 1), b"k%02d" % i + _key(rnd, i % 5)) for i in range(20)]
    f, io, nidx = H.write_file(items, 0, 400)
    assert nidx >= 3
    return items, f, io


def _wanted(items):
    hs, ks = _around(items)
    return hs, ks


def test_a_last_item_cut_short(cuda):
    items, f, io = _valid()
    cut = struct.pack("<q", io - 2) + f[8:io - 2]                  # no index section: the file ends in the item
    hs, ks = _wanted(items)
    model = _check(cuda, [cut], [0], ks, hashes=hs)
    for b in (False, True):
        assert model[b][4 * 19].status == M.ERR                    # the last item by its own key
        assert model[b][4 * 18].status == M.FOUND


def test_a_ksz_that_runs_past_the_file(cuda):
    items, f, io = _valid()
    f2 = H.write_file(items, 0, 1 << 30)[0]                        # the items end the file
    last = len(f2) - 23 - len(items[-1].key)
    g = bytearray(f2)
    g[last + 22] = len(items[-1].key) + 1
    hs, ks = _wanted(items)
    model = _check(cuda, [bytes(g)], [0], ks, hashes=hs)
    for b in (False, True):
        assert model[b][4 * 19].status == M.ERR and model[b][4 * 18].status == M.FOUND


@pytest.mark.parametrize("bad", [0, 15, "len + 1", 2 ** 63, -1])
def test_an_index_entry_with_an_offset_outside_the_file(cuda, bad):
    items, f, io = _valid()
    g = bytearray(f)
    struct.pack_into("<Q", g, io + 16 + 8, (len(f) + 1 if bad == "len + 1" else bad) & TOP)      # entry 1
    hs, ks = _wanted(items)
    model = _check(cuda, [bytes(g)], [0], ks, hashes=hs)
    entry2 = H.load_index(f)[2][0]
    for b in (False, True):
        st = [r.status for r in model[b]]
        assert M.ERR in st and M.FOUND in st
        j2 = [i for i, h in enumerate(hs) if H.load_index(f)[1][0] < h <= entry2]
        assert j2 and all(st[i] == M.ERR for i in j2)              # every target with j == 2 reads entry 1


@pytest.mark.parametrize("case", ["indexOffset 15", "indexOffset len + 1", "15 bytes", "past the buffer",
                                  "entries not whole"])
def test_bad_file(cuda, case):
    items, f, io = _valid()
    other = H.write_file([_item(random.Random(1), items[3].keyhash, items[3].key)], 0, 128)[0]
    hs, ks = [items[3].keyhash, 5], [items[3].key, b"x"]
    kw = {}
    if case == "indexOffset 15":
        bad = struct.pack("<q", 15) + f[8:]
    elif case == "indexOffset len + 1":
        bad = struct.pack("<q", len(f) + 1) + f[8:]
    elif case == "15 bytes":
        bad, kw = f, dict(lens=[15, len(other)])
    elif case == "entries not whole":
        bad = f + b"\0"
    else:
        bad = f
    files = [bad, other]
    if case == "past the buffer":                                   # the last file ends one byte behind `bytes`
        files = [other, bad]
        blob, offs = _pack_odd(files, 0xEE)
        kw = dict(nbytes=offs[1] + len(bad) - 1)
    model = _check(cuda, files, [0, 1], ks, hashes=hs, **kw)
    for b in (False, True):
        if case == "past the buffer":
            assert [(r.status, r.hit_file) for r in model[b]] == [(M.FOUND, 0), (M.BAD_FILE, 1)]
        else:
            assert [(r.status, r.hit_file) for r in model[b]] == [(M.BAD_FILE, 0)] * 2      # file 1 is never asked


def test_a_head_alone_is_a_miss(cuda):
    model = _check(cuda, [struct.pack("<qII", 16, 0, 0)], [0], [b"a", b""], hashes=[1, TOP])
    assert [r.status for r in model[False]] == [M.MISS] * 2


def test_an_unsorted_index(cuda):
    items, f, io = _valid()
    entries = H.load_index(f)
    rnd = random.Random(14)
    hs, ks = _wanted(items)
    for _ in range(3):
        rnd.shuffle(entries)
        g = f[:io] + b"".join(struct.pack("<Qq", kh, o) for kh, o in entries)
        _check(cuda, [g], [0], ks, hashes=hs)                      # equal to the model, whatever that is


# ---- the chain: replay -> hint.build -> hint.merge -> hint.lookup -> replay.read_records ----
def test_from_key_to_value_on_the_device(cuda):
    import torch
    from gobeansdb_amd import _lib, batch, hint, replay
    from oracle import replay as R
    rnd = random.Random(61)
    keys = [b"%c%04d" % (97 + i % 11, i) for i in range(150)]
    written = [rnd.choice(keys) for _ in range(400)]
    bodies = [_key(rnd, rnd.randint(0, 40)) for _ in written]
    data = b"".join(R.make_record(k, v, ver=i % 7, ts=1700000000 + i) for i, (k, v) in enumerate(zip(written, bodies)))
    rows, err = R.replay(data)
    assert err is None and len(rows) == 400
    last = {}
    for row, k, v in zip(rows, written, bodies):
        last[k] = (row[0], v)                                      # the last record of every key
    distinct = sorted(last)
    assert any(written.count(k) >= 3 for k in distinct)
    dd = _dev(data, cuda)
    recs, _ = R.stream_all(data)
    model_recs = [(H.keyhash(row[2]), row[2], row[0], (24 + len(r.key) + len(r.body) + 255) // 256 * 256, row[3],
                   row[6]) for row, r in zip(rows, recs)]
    cap = next(c for c in range(len(distinct), 0, -1) if len(H.build(model_recs, split_cap=c)) == 3)
    splits = hint.build(replay.replay(dd), split_cap=cap, chunk_id=6)
    assert len(splits) == 3
    merged = hint.merge([sp.file for sp in splits], [6] * 3)
    kb = batch.BlockBatch.from_bytes(distinct, device=cuda)
    layouts = [([sp.file for sp in splits[::-1]], [6] * 3, None),   # splits only, newest first
               ([merged.file], [0], 0)]                             # the merged file alone
    side = torch.cuda.Stream()
    for files, chunks, mg in layouts:
        res = hint.lookup(files, chunks, kb, merged=mg, bounded=True)
        assert res.totals == (len(distinct), 0, 0, 0)
        on_side = hint.lookup(files, chunks, kb, merged=mg, bounded=True, stream=side)   # a stream of the caller's
        side.synchronize()
        assert on_side.totals == res.totals and torch.equal(on_side.status, res.status)
        assert torch.equal(on_side.chunk, res.chunk) and torch.equal(on_side.offset, res.offset)
        assert res.status.cpu().tolist() == [_lib.HL_FOUND] * len(distinct)
        assert res.chunk.cpu().tolist() == [6] * len(distinct)
        offsets = res.offset.to(torch.int64) & 0xFFFFFFFF
        assert offsets.cpu().tolist() == [last[k][0] for k in distinct]
        rd = replay.read_records(dd, offsets, keys=distinct)       # the positions never left the device
        torch.cuda.synchronize()
        assert rd.status.cpu().tolist() == [_lib.RD_OK] * len(distinct)
        assert rd.key_eq.cpu().tolist() == [1] * len(distinct)
        assert [rd.value(i) for i in range(len(distinct))] == [last[k][1] for k in distinct]
    # without a file every key is a miss
    none = hint.lookup([], [], kb)
    assert none.totals == (0, len(distinct), 0, 0) and int(none.status.abs().sum()) == 0
