"""GPU: hint merge, hint lookup and the HTree build over hint files packed into one buffer of
4 GiB + 4 MiB (tests/wide.py), through hint.merge_packed, qlzx_hint_lookup and htree.build_packed,
against tests/hintmerge_model.py, tests/hintlookup_model.py and tests/htree_model.py.

Five source files at odd addresses:
  0  wholly below 2^31
  1  begins below 2^31 and ends above it
  2  "straddle": begins below 2^32 with its items, its index section lies above 2^32;
     "starts_at": begins exactly at 2^32
  3  above 2^32
  4  wholly between the two lines, without an index (indexOffset 0): the merge and the HTree walk it,
     the lookup, which searches it last, reports it as a bad file
One arrangement cannot hold both forms of file 2, so the tests run in both.  Under every file
byte at or above 2^32 lies, 2^32 lower, a byte of a decoy file of the same make with other keys.
hint.merge_packed does not return the merge's item_src, so the plan is also called directly and
item_src compared with file_off plus the item's place in its file.  The lookup runs through
hint.lookup_packed (the mirror's own offset handling; it picks the kernel by n) and through
qlzx_hint_lookup itself, which alone can force the lane and the wave kernel."""
import functools
import random
import struct

import numpy as np
import pytest

import hint_model as H
import hintlookup_model as ML
import hintmerge_model as MM
import htree_model as MT
import wide
from wide import B31, B32, BIG_BYTES

pytestmark = pytest.mark.gpu

widebuf = wide.fixture()
w = wide.per_test()

KINDS = ("straddle", "starts_at")
PER = (60, 300, 200, 120, 90)
INTERVALS = (128, 4096, 128, 4096, 128)
CHUNKS = [5, 4, 3, 2, 1]          # search order: newest chunk first
FILL, GUARD = 0xAA, 8
TOP = 2 ** 64 - 1
KEYS_AT = B32 + (1 << 20) + 1     # the lookup keys, packed at odd addresses above 2^32


def _key(rnd, n: int) -> bytes:
    return bytes(rnd.choice((rnd.getrandbits(8), 0x80 | rnd.getrandbits(7))) for _ in range(n))


def _no_index(f: bytes) -> bytes:
    io, n, ds = H.read_head(f)
    return struct.pack("<qII", 0, n, ds) + f[16:io]


@functools.lru_cache(maxsize=None)
def _merge_files(seed: int):
    """Five sorted sources over a shared pool (keys repeat across sources); a quarter of the keys
    have a forced small keyhash, so distinct keys collide.  Returns (files, every key)."""
    rnd = random.Random(seed)
    pool = list(dict.fromkeys(_key(rnd, rnd.randint(1, 40)) + b"%d" % i for i in range(450)))
    forced = {k: rnd.randrange(40) for k in pool[::4]}
    files = []
    for i, (per, iv) in enumerate(zip(PER, INTERVALS)):
        items = [H.Item(forced.get(k, H.keyhash(k)), k, 0xDEAD, 256 * rnd.randrange(1 << 16), rnd.randint(-3, 9),
                        rnd.getrandbits(16)) for k in rnd.sample(pool, per)]
        f = H.write_file(sorted(items, key=lambda it: (it.keyhash, it.key)), rnd.getrandbits(32), iv)[0]
        files.append(_no_index(f) if i == 4 else f)
    return tuple(files), tuple(pool), forced


def _starts(files, kind):
    """Where the five files begin (see the module's text)."""
    io2 = H.read_head(files[2])[0]
    s2 = B32 if kind == "starts_at" else (B32 - io2 + 1) | 1
    starts = [(B31 - 300001), (B31 - len(files[1]) // 2) | 1, s2, B32 + 70001, B32 - 500001]
    spans = sorted((s, s + len(f)) for s, f in zip(starts, files))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert starts[0] + len(files[0]) < B31 and starts[1] < B31 < starts[1] + len(files[1])
    assert B31 < starts[4] and starts[4] + len(files[4]) < B32 and starts[3] > B32
    if kind == "straddle":       # the items (but the last one's tail) below the line, the index section above it
        assert starts[2] + io2 > B32 >= starts[2] + io2 - 2 and len(files[2]) - io2 >= 16
    assert all(s % 2 == 1 for i, s in enumerate(starts) if not (i == 2 and kind == "starts_at"))
    return starts


def _place(wb, files, decoys, kind):
    starts = _starts(files, kind)
    assert wide.census([(s, len(f)) for s, f in zip(starts, files)]) == \
        ({"cross31": 1, "cross32": 1, "above32": 1} if kind == "straddle" else {"cross31": 1, "at32": 1, "above32": 1})
    for s, f, d in zip(starts, files, decoys):
        wb.place_with_decoy(s, f, d)
    return starts


# ---------------------------------------------------------------- merge

def _item_places(f: bytes):
    """{key: offset in the file} of a source's items."""
    io = H.read_head(f)[0] or len(f)
    out, p = {}, 16
    while p < io:
        it, nxt = H.next_item(f, p, io)
        out[it.key] = p
        p = nxt
    return out


def _merged_item_src(files, starts, merged_file: bytes):
    """item_src of every merged item, in the merged file's order: its source is the file of the
    chunk id the merged item carries (CHUNKS are distinct), its place the key's in that file."""
    places = [_item_places(f) for f in files]
    by_chunk = {c: i for i, c in enumerate(CHUNKS)}
    out = []
    for it in H.read_items(merged_file):
        i = by_chunk[it.chunk_id]
        out.append(starts[i] + places[i][it.key])
    return out


def _plan_item_src(wb, offs, lens, chunks, interval, num_key):
    """qlzx_hint_merge_plan over big: item_src of the merged items."""
    import torch
    from gobeansdb_amd import _dev, _lib, batch
    L = _lib.lib()
    dev = wb.device
    cap = sum(max(n - 16, 0) for n in lens) // 23
    off_d, len_d, chunk_d = _dev.u64(offs, dev), _dev.u64(lens, dev), _dev.u32(chunks, dev)
    item_src, item_off = (torch.zeros(cap, dtype=torch.int64, device=dev) for _ in range(2))
    item_chunk, index_item, coll_item = (torch.zeros(cap, dtype=torch.int32, device=dev) for _ in range(3))
    totals = torch.zeros(12, dtype=torch.int32, device=dev)
    wsb = L.qlzx_hint_merge_workspace_size(BIG_BYTES, len(offs), cap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.qlzx_hint_merge_plan(wb.big.data_ptr(), BIG_BYTES, off_d.data_ptr(), len_d.data_ptr(),
                                      chunk_d.data_ptr(), len(offs), cap, interval, item_src.data_ptr(),
                                      item_chunk.data_ptr(), item_off.data_ptr(), index_item.data_ptr(),
                                      coll_item.data_ptr(), totals.data_ptr(), ws.data_ptr(), wsb, batch._stream()),
               "qlzx_hint_merge_plan")
    t = _dev.readback(totals)
    assert int(t[_lib.HM_STATUS]) == _lib.HM_OK and int(t[_lib.HM_NUM_KEY]) == num_key
    return item_src[:num_key].cpu().numpy().view(np.uint64).tolist()


@pytest.mark.parametrize("write", [True, False], ids=["write", "for_gc"])
@pytest.mark.parametrize("kind", KINDS)
def test_merge(w, kind, write):
    """File bytes, totals and collision items are hintmerge_model's."""
    from test_gpu_hintmerge import _same
    from gobeansdb_amd import hint
    files, _, _ = _merge_files(11)
    decoys, _, _ = _merge_files(12)
    want = MM.merge(files, CHUNKS, index_interval=300, for_gc=not write)
    other = MM.merge(decoys, CHUNKS, index_interval=300, for_gc=not write)
    assert want.collisions and want.collisions != other.collisions and want.num_key != other.num_key
    starts = _starts(files, kind)
    want_src = _merged_item_src(files, starts, MM.merge(files, CHUNKS, index_interval=300).file)
    assert len(want_src) == want.num_key and sum(x > B32 for x in want_src) >= 15
    assert sum(B31 < x < B32 for x in want_src) >= 20 and sum(x < B31 for x in want_src) >= 20
    starts = _place(w, files, decoys, kind)
    got = hint.merge_packed(w.big, starts, [len(f) for f in files], CHUNKS, index_interval=300, write=write)
    _same(got, want, write)
    assert _plan_item_src(w, starts, [len(f) for f in files], CHUNKS, 300, want.num_key) == want_src


def test_merge_error_clauses(w):
    """file_off + file_len one past `bytes` with file_off above 2^32, and an indexOffset that
    points past the file that straddles 2^32: HM_BAD_FILE, naming the source."""
    from gobeansdb_amd import _lib, hint
    files, _, _ = _merge_files(11)
    decoys, _, _ = _merge_files(12)
    starts = _place(w, files, decoys, "straddle")
    lens = [len(f) for f in files]
    cut = starts[3] + lens[3] - 1
    assert starts[3] > B32 and cut > max(s + n for s, n in zip(starts, lens) if s != starts[3])
    # (the model reads whole files and has no `bytes`; the clause is include/qlzx.h's own)
    with pytest.raises(_lib.QlzxError, match="HM_BAD_FILE, source 3"):
        hint.merge_packed(w.big[:cut], starts, lens, CHUNKS)
    bad = struct.pack("<q", lens[2] + 1) + files[2][8:]
    with pytest.raises(MM.BadFile):
        MM.merge(list(files[:2]) + [bad] + list(files[3:]), CHUNKS)
    w.place(w.big, starts[2], bad[:8])
    with pytest.raises(_lib.QlzxError, match="HM_BAD_FILE, source 2"):
        hint.merge_packed(w.big, starts, lens, CHUNKS)


# ---------------------------------------------------------------- lookup

def _pack_odd(blocks, fill, base):
    """One blob with every block at an odd address when the blob stands at `base`: (bytes, offsets)."""
    blob, offs = bytearray(), []
    for b in blocks:
        blob += bytes([fill]) * (1 if (base + len(blob)) % 2 == 0 else 2)
        offs.append(base + len(blob))
        blob += b
    return bytes(blob) + bytes([fill]) * 3, offs


def _raw(wb, offs, lens, chunks, merged, koff, klens, hashes, flags, nbytes):
    """qlzx_hint_lookup with hints = keys = big: (rows of the seven outputs, totals)."""
    import torch
    from gobeansdb_amd import _dev, _lib, batch
    L = _lib.lib()
    dev, n, nf = wb.device, len(koff), len(offs)
    off_d, len_d, chunk_d = _dev.u64(offs, dev), _dev.u64(lens, dev), _dev.u32(chunks, dev)
    flag_d = _dev.u32([_lib.HL_FILE_MERGED if i == merged else 0 for i in range(nf)], dev)
    koff_d, klen_d = _dev.u64(koff, dev), _dev.u32(klens, dev)
    hash_d = None if hashes is None else _dev.u64(hashes, dev)
    outs = [torch.full((n + GUARD,), FILL, dtype=torch.uint8, device=dev).repeat_interleave(k).view(dt)
            for k, dt in ((4, torch.int32),) * 5 + ((2, torch.int16), (8, torch.int64))]
    totals = torch.full((4 + GUARD,), FILL, dtype=torch.uint8, device=dev).repeat_interleave(4).view(torch.int32)
    wsb = L.qlzx_hint_lookup_workspace_size(n, nf)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.qlzx_hint_lookup(wb.big.data_ptr(), nbytes, off_d.data_ptr(), len_d.data_ptr(), chunk_d.data_ptr(),
                                  flag_d.data_ptr(), nf, wb.big.data_ptr(), koff_d.data_ptr(), klen_d.data_ptr(),
                                  batch._ptr(hash_d), n, flags, *[o.data_ptr() for o in outs], totals.data_ptr(),
                                  ws.data_ptr(), wsb, batch._stream()), "qlzx_hint_lookup")
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for h in host:
        assert (h[n:].view(np.uint8) == FILL).all()
    t = totals.cpu().numpy()
    assert (t[4:].view(np.uint8) == FILL).all()
    cols = [host[0].astype(np.int64), host[1].view(np.uint32), host[2].view(np.uint32), host[3].view(np.uint32),
            host[4].astype(np.int64), host[5].view(np.uint16), host[6].view(np.uint64)]
    return [tuple(int(c[i]) for c in cols) for i in range(n)], [int(x) for x in t[:4].view(np.uint32)]


def _mirror(wb, offs, lens, chunks, merged, koff, klens, hashes, bounded, nbytes):
    """hint.lookup_packed over big[:nbytes], the keys a BlockBatch over big: (rows, totals)."""
    from gobeansdb_amd import _dev, batch, hint
    dev = wb.device
    keys = batch.BlockBatch(wb.big, _dev.u64(koff, dev), _dev.u32(klens, dev))
    r = hint.lookup_packed(wb.big[:nbytes], offs, lens, chunks, keys, merged=merged, bounded=bounded,
                           keyhash=None if hashes is None else _dev.u64(hashes, dev))
    cols = [r.status.cpu().numpy().astype(np.int64), _dev.readback(r.hit_file), _dev.readback(r.chunk),
            _dev.readback(r.offset), r.ver.cpu().numpy().astype(np.int64), r.vhash.cpu().numpy().view(np.uint16),
            r.item_src.cpu().numpy().view(np.uint64)]
    return [tuple(int(c[i]) for c in cols) for i in range(len(koff))], list(r.totals)


def _lookup_model(files, starts, keys, hashes, merged=None, lens=None, nbytes=BIG_BYTES):
    """{bounded: (results, totals)} of hintlookup_model for files packed into `nbytes` bytes."""
    lens = [len(f) for f in files] if lens is None else lens
    seen = [None if o + n > nbytes else f[:n] for f, o, n in zip(files, starts, lens)]
    return {bounded: ML.lookup(seen, starts, CHUNKS, merged, keys, hashes, bounded) for bounded in (False, True)}


def _lookup_both(wb, files, starts, keys, hashes, merged=None, lens=None, nbytes=BIG_BYTES, model=None):
    """Both modes against the model, through the mirror and through both kernels; the keys stand
    in big above 2^32, other bytes of the same lengths under them in A0."""
    from gobeansdb_amd import _lib
    assert (_lib.HL_F_LANE, _lib.HL_F_WAVE) == (2, 4)
    lens = [len(f) for f in files] if lens is None else lens
    model = model or _lookup_model(files, starts, keys, hashes, merged, lens, nbytes)
    kblob, koff = _pack_odd(keys, 0x55, KEYS_AT)
    assert all(o % 2 == 1 and o > B32 for o in koff)
    wb.place_with_decoy(KEYS_AT, kblob, bytes(b ^ 0x33 for b in kblob))
    out = {}
    for bounded in (False, True):
        want, totals = model[bounded]
        out[bounded] = want
        got, got_totals = _mirror(wb, starts, lens, CHUNKS, merged, koff, [len(k) for k in keys], hashes, bounded,
                                  nbytes)
        bad = [(i, g, x.astuple()) for i, (g, x) in enumerate(zip(got, want)) if g != x.astuple()]
        assert not bad, (bounded, "lookup_packed", len(bad), bad[:5])
        assert got_totals == totals, (bounded, "lookup_packed")
        for shape in (_lib.HL_F_LANE, _lib.HL_F_WAVE):
            flags = (_lib.HL_F_BOUNDED if bounded else 0) | shape
            got, got_totals = _raw(wb, starts, lens, CHUNKS, merged, koff, [len(k) for k in keys], hashes, flags,
                                   nbytes)
            bad = [(i, g, x.astuple()) for i, (g, x) in enumerate(zip(got, want)) if g != x.astuple()]
            assert not bad, (bounded, shape, len(bad), bad[:5])
            assert got_totals == totals, (bounded, shape)
    return out


@pytest.mark.parametrize("explicit", [False, True], ids=["default_hash", "given_hash"])
@pytest.mark.parametrize("kind", KINDS)
def test_lookup(w, kind, explicit):
    """Every key of every file, keys one byte longer, a key only a decoy holds and, with given
    hashes, misses just below and above each file's range: all seven outputs and totals."""
    files, pool, forced = _merge_files(11)
    decoys, dpool, _ = _merge_files(12)
    earlier = {it.key for f in decoys[:3] for it in H.read_items(f)}
    only_decoy = next(it.key for it in H.read_items(decoys[3])        # in the decoy of the file above 2^32 alone
                      if it.key not in earlier and it.key not in set(pool) and it.keyhash == H.keyhash(it.key))
    keys = list(pool) + [k + b"?" for k in pool[::9]] + [only_decoy]
    hashes = None
    if explicit:
        hashes = [forced.get(k, H.keyhash(k)) for k in pool] + [H.keyhash(k) for k in pool[::9]]
        hashes.append(H.keyhash(only_decoy))
        for f in files:
            items = H.read_items(f if H.read_head(f)[0] else struct.pack("<q", len(f)) + f[8:])
            for kh in (items[0].keyhash - 1, items[-1].keyhash + 1, items[-1].keyhash + 7):
                keys.append(b"absent")
                hashes.append(kh & TOP)
    starts = _starts(files, kind)
    model = _lookup_model(files, starts, keys, hashes)              # on the host, before any GPU call
    bounded = model[True][0]
    found = [r for r in bounded if r.status == ML.FOUND]
    assert len(found) >= 250 and sum(r.item_src > B32 for r in found) >= 10
    assert sum(B31 < r.item_src < B32 for r in found) >= 50
    assert {r.hit_file for r in found} == {0, 1, 2, 3}
    assert any(r.status == ML.BAD_FILE and r.hit_file == 4 for r in bounded)
    want_decoy = bounded[keys.index(only_decoy)]
    assert want_decoy.status == ML.BAD_FILE and want_decoy.hit_file == 4      # no file holds it; the last has no index
    # what a reader of the decoy would answer differs
    dfound = ML.lookup(list(decoys), starts, CHUNKS, None, [only_decoy], None, True)[0][0]
    assert dfound.status == ML.FOUND and dfound.hit_file == 3 and dfound.item_src > B32
    assert _place(w, files, decoys, kind) == starts
    _lookup_both(w, files, starts, keys, hashes, model=model)


def test_lookup_error_clauses(w):
    """The two error clauses of test_merge_error_clauses, as the lookup reports them."""
    files, pool, forced = _merge_files(11)
    decoys, _, _ = _merge_files(12)
    starts = _starts(files, "straddle")
    keys = list(pool[:200])
    cut = starts[3] + len(files[3]) - 1
    bad = struct.pack("<q", len(files[2]) + 1) + files[2][8:]
    broken = list(files[:2]) + [bad] + list(files[3:])
    m_cut = _lookup_model(files, starts, keys, None, nbytes=cut)
    m_bad = _lookup_model(broken, starts, keys, None)
    assert any(r.status == ML.BAD_FILE and r.hit_file == 3 for r in m_cut[True][0])
    assert any(r.status != ML.FOUND and r.hit_file == 2 for r in m_bad[True][0])
    _place(w, files, decoys, "straddle")
    _lookup_both(w, files, starts, keys, None, nbytes=cut, model=m_cut)
    w.restore()
    _place(w, files, decoys, "straddle")
    w.place(w.big, starts[2], bad[:8])
    _lookup_both(w, broken, starts, keys, None, model=m_bad)


# ---------------------------------------------------------------- HTree

@pytest.mark.parametrize("depth,height", [(0, 3), (1, 3)])
@pytest.mark.parametrize("kind", KINDS)
def test_htree(w, kind, depth, height):
    """Every level, leaf_first, the totals and the file bytes are htree_model's."""
    import test_gpu_htree as T
    from gobeansdb_amd import htree
    rnd = random.Random(depth)
    pool = T._pool(rnd, 450, depth, height)
    dpool = T._pool(random.Random(99), 450, depth, height)
    files, decoys = [], []
    for i, (per, iv) in enumerate(zip(PER, INTERVALS)):
        for out, p in ((files, pool), (decoys, dpool)):
            items = [T._item(rnd, s, depth) for s in rnd.sample(p, per)]
            if i % 2 == 0:
                items.sort(key=lambda it: (it.keyhash, it.key))
            f = H.write_file(items, rnd.getrandbits(32), iv)[0]
            out.append(_no_index(f) if i == 4 else f)
    chunks = [0, 0, 1, 3, 5]
    tree, dump, nset, nrem = MT.build(files, chunks, depth, height)
    assert MT.build(decoys, chunks, depth, height)[1] != dump
    starts = _place(w, files, decoys, kind)
    got = htree.build_packed(w.big, starts, [len(f) for f in files], chunks, depth, height)
    T._same(got, tree, dump, nset, nrem)
