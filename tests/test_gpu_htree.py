"""The HTree build on the GPU (qlzx_htree_plan / qlzx_htree_write, htree.build)
against tests/htree_model.py.

Sources come from hint_model.write_file; every case compares every level's counts and hashes,
leaf_first, the totals and the file bytes."""
import functools
import random
import struct

import numpy as np
import pytest

import hint_model as H
import htree_model as M
import ws_contract as W

pytestmark = pytest.mark.gpu
FILL = 0xAA
GEOMETRIES = [(0, 1), (0, 2), (1, 3), (2, 3), (2, 5)]      # L = 8, 8, 7, 6, 5; 1 to 65,536 leaves


def _dev(data: bytes, cuda):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(cuda)


def _pool(rnd, n, depth, height, leaves=None):
    """n distinct slots: keyhashes with zero bucket nibbles, spread over `leaves` (default: any)."""
    p = depth + height - 1
    out = set()
    while len(out) < n:
        kh = rnd.getrandbits(64) & (M.M64 >> (4 * depth))
        if leaves is not None and height > 1:
            kh = (kh & (M.M64 >> (4 * p))) | (rnd.choice(leaves) << (64 - 4 * p))
        out.add(kh)
    return sorted(out)


def _item(rnd, slot, depth, ver=None):
    """An op on `slot`: any bucket nibbles (aliases of one slot), a key of any length (never read)."""
    kh = slot | (rnd.getrandbits(4 * depth) << (64 - 4 * depth)) if depth else slot
    return H.Item(kh, bytes(rnd.getrandbits(8) for _ in range(rnd.choice((0, 1, 9, 40)))), 0xDEAD,
                  256 * rnd.randrange(1 << 24), rnd.randint(-3, 9) if ver is None else ver, rnd.getrandbits(16))


def _sources(nsrc, per, seed, depth, height, leaves=None, intervals=(128, 300, 4096), pool=None):
    """nsrc sources of `per` ops each over slots the sources share: set, removed and set again
    across sources, a last op that removes, removes of absent slots.  Every other source is in
    keyhash order as a dumped split is, the rest in any order."""
    rnd = random.Random(seed)
    pool = _pool(rnd, max(per * 3 // 2, per + 3), depth, height, leaves) if pool is None else pool
    files = []
    for i in range(nsrc):
        items = [_item(rnd, s, depth) for s in rnd.sample(pool, per)]
        if i % 2 == 0:
            items.sort(key=lambda it: (it.keyhash, it.key))
        files.append(H.write_file(items, rnd.getrandbits(32), intervals[i % len(intervals)])[0])
    return files


def _levels(tree):
    return [(np.array([n.count for n in lv], np.uint32), np.array([n.hash for n in lv], np.uint16))
            for lv in tree.levels]


def _same(got, tree, dump, nset, nrem, write=True):
    assert (got.n_ops, got.n_set, got.n_remove) == (nset + nrem, nset, nrem)
    first = tree.leaf_first()
    assert got.n_slots == first[-1]
    assert len(got.levels) == len(tree.levels)
    for l, ((count, hash_), (wc, wh)) in enumerate(zip(got.levels, _levels(tree))):
        assert np.array_equal(count.cpu().numpy().view(np.uint32), wc), l
        assert np.array_equal(hash_.cpu().numpy().view(np.uint16), wh), l
    assert got.leaf_first.cpu().numpy().view(np.uint32).tolist() == first
    assert got.file.cpu().numpy().tobytes() == (dump if write else b"")


def _build(cuda, files, chunks, depth, height, write=True):
    from gobeansdb_amd import htree
    got = htree.build([_dev(f, cuda) for f in files], chunks, depth, height, write=write)
    tree, dump, nset, nrem = M.build(files, chunks, depth, height)
    _same(got, tree, dump, nset, nrem, write)
    return got, tree


@pytest.mark.parametrize("per", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 65])
def test_source_and_op_counts(cuda, nsrc, per):
    files = _sources(nsrc, per, 1000 * nsrc + per, 1, 3)
    rnd = random.Random(nsrc + per)
    got, _ = _build(cuda, files, sorted(rnd.randrange(9) for _ in range(nsrc)), 1, 3)
    assert got.n_ops == nsrc * per and (nsrc < 3 or per < 63 or 0 < got.n_slots < got.n_set)


@pytest.mark.parametrize("depth,height", GEOMETRIES)
def test_every_stored_length_and_leaf_count(cuda, depth, height):
    files = _sources(3, 257, 10 * depth + height, depth, height)
    got, tree = _build(cuda, files, [0, 0, 5], depth, height)
    assert tree.khash_len == {(0, 1): 8, (0, 2): 8, (1, 3): 7, (2, 3): 6, (2, 5): 5}[(depth, height)]
    assert got.n_remove > 0 and got.n_slots > 100


def test_six_thousand_ops_over_five_sources(cuda):
    """More ops than one workgroup sorts or scans; the root holds more than 256: hash *= 97."""
    files = _sources(5, 1200, 77, 0, 2)
    got, tree = _build(cuda, files, [1, 3, 3, 4, 5], 0, 2)
    assert got.n_ops == 6000 and tree.levels[0][0].count > 256
    plain = sum(n.hash for n in tree.levels[1]) & 0xFFFF
    assert tree.levels[0][0].hash != plain
    # the listing: node lines at the root, item lines at a leaf and under a longer prefix
    assert got.list_dir("") == tree.list_dir("") and got.list_dir("").count(b"/") == 16
    one = tree.list_dir("c").split(b"\n")[0][:16].decode()
    for path in ("3", "c", "3a", one[:3], one[:9], one):
        assert got.list_dir(path) == tree.list_dir(path), path
    assert got.list_dir(one).count(b"\n") == 1
    assert got.list_dir("3").count(b"\n") == tree.levels[1][3].count > 0


def test_list_dir_under_a_bucket(cuda):
    files = _sources(3, 400, 5, 1, 3)
    got, tree = _build(cuda, files, [0, 1, 2], 1, 3)
    assert 256 <= tree.levels[0][0].count
    assert got.list_dir("7") == tree.list_dir("7") and got.list_dir("7").count(b"/") == 16    # nodes
    some = bytes(tree.list_dir("7a")).split(b"\n")[0][:16].decode()
    for path in ("7a", "7a3", some[:3], some[:4], some, "b" + some[1:3]):
        assert got.list_dir(path) == tree.list_dir(path), path
    assert got.list_dir(some).count(b"\n") == 1
    with pytest.raises(ValueError, match="too short"):
        got.list_dir("")


def test_a_slot_set_removed_and_set_again(cuda):
    """The issue's worked case: the slot removed and set again moves behind the one rewritten in place."""
    A, B = 0x1000000200000001, 0x1000000500000002
    it = lambda kh, ver, vhash=0, off=0: H.Item(kh, b"k", 0, off, ver, vhash)
    files = [H.write_file([it(A, 1, 3, 0x300), it(B, 2, 7, 0x100)], 0, 4096)[0],
             H.write_file([it(A, -1), it(B, 3, 10, 0x200)], 0, 4096)[0],
             H.write_file([it(A, 5, 1, 0x400)], 0, 4096)[0]]
    got, tree = _build(cuda, files, [0, 1, 2], 0, 2)
    file = got.file.cpu().numpy().tobytes()
    assert len(file) == 198 and file[6:12] == bytes.fromhex("020000003400")
    assert file[100:142] == bytes.fromhex("26000000" "0200000005000010" "03000000" "0a00" "020000" "0100"
                                          "0100000002000010" "05000000" "0100" "040000" "0200")
    assert got.list_dir("") == b"1000000500000002 10 3\n1000000200000001 1 5\n"
    assert got.node(0, 0) == (2, 52)


def test_last_op_removes_and_removes_of_absent_slots(cuda):
    rnd = random.Random(8)
    pool = _pool(rnd, 90, 1, 3)
    a = H.write_file([_item(rnd, s, 1, ver=rnd.randint(1, 9)) for s in pool[:60]], 0, 300)[0]
    b = H.write_file([_item(rnd, s, 1, ver=rnd.randint(-3, 0)) for s in pool[30:]], 0, 300)[0]   # 30 present, 30 absent
    c = H.write_file([_item(rnd, s, 1, ver=3) for s in pool[20:40]], 0, 300)[0]
    got, _ = _build(cuda, [a, b, c], [0, 0, 1], 1, 3)
    assert (got.n_set, got.n_remove, got.n_slots) == (80, 60, 40)
    got, _ = _build(cuda, [a, b], [0, 1], 1, 3)
    assert got.n_slots == 30
    got, _ = _build(cuda, [b], [4], 1, 3)                     # nothing but removes: an empty tree
    assert got.n_slots == 0 and got.file.numel() == 2560


def test_aliases_of_one_slot_share_it(cuda):
    low = 0x00B0000700000009
    its = [H.Item(low | (b << 56), b"x", 0, 256 * i, v, 100 + i) for i, (b, v) in
           enumerate([(0x30, 1), (0x5F, 2), (0xC1, -1), (0x77, 4), (0x01, 5)])]
    files = [H.write_file(its[:2], 0, 4096)[0], H.write_file(its[2:], 0, 4096)[0]]
    # depth 2 drops the top byte: one slot, set, set, removed, set, set
    got, tree = _build(cuda, files, [0, 1], 2, 3)
    assert got.n_slots == 1 and bytes(tree.leafs[0xB0])[6:10] == struct.pack("<i", 5)
    # depth 1 drops its first nibble only: slots 0, f, 7 set once, slot 1 removed while absent and then set
    got, tree = _build(cuda, files, [0, 1], 1, 3)
    assert got.n_slots == 4


def test_an_empty_leaf_between_full_ones_and_all_ops_in_one_leaf(cuda):
    files = _sources(3, 257, 12, 1, 3, leaves=[0x00, 0x01, 0x03, 0xFE, 0xFF])
    got, tree = _build(cuda, files, [0, 1, 1], 1, 3)
    first = tree.leaf_first()
    assert first[1] < first[2] == first[3] < first[4]          # leaf 2 is empty, 1 and 3 are not
    files = _sources(3, 400, 13, 0, 2, leaves=[9])
    got, tree = _build(cuda, files, [0, 1, 1], 0, 2)
    assert tree.levels[1][9].count == got.n_slots > 256 and got.list_dir("").count(b"/") == 16


# ---- the sources' heads and indexes ----
def _without_index(f: bytes) -> bytes:
    io, nk, ds = H.read_head(f)
    return struct.pack("<qII", 0, nk, ds) + f[16:io]


def _with_index(f: bytes, offsets) -> bytes:
    io = H.read_head(f)[0]
    return f[:io] + b"".join(struct.pack("<Qq", 0x5555, o) for o in offsets)


@functools.lru_cache(maxsize=None)
def _three():
    return tuple(_sources(3, 300, 55, 1, 3, intervals=(128, 300, 700)))


def test_sources_without_an_index_with_a_garbage_index_and_without_items(cuda):
    a, b, c = _three()
    good = [o for _, o in H.load_index(a)]
    assert len(good) >= 3
    want = M.build([a, b, c], [0, 1, 2], 1, 3)
    empty = [struct.pack("<qII", 16, 0, 0), struct.pack("<qII", 0, 0, 0), struct.pack("<qII", 7, 0, 0) + bytes(20)]
    for files in ([a, _without_index(b), c],
                  [_with_index(a, good[:1] + [good[1] + 5] + good[2:]), b, c],        # inside an item
                  [_with_index(a, good[:1] + [good[2], good[1]] + good[3:]), b, c],   # decreasing
                  [_with_index(a, [16] * 600), b, _with_index(c, [len(c) + 100])]):   # more entries than items
        got, tree = _build(cuda, files, [0, 1, 2], 1, 3)
        assert got.file.cpu().numpy().tobytes() == want[1]
    got, _ = _build(cuda, [empty[0], a, empty[1], b, c, empty[2]], [0, 0, 0, 1, 2, 2], 1, 3)
    assert got.file.cpu().numpy().tobytes() == want[1]
    got, _ = _build(cuda, empty, [0, 1, 2], 1, 3)
    assert (got.n_ops, got.n_slots, got.file.numel()) == (0, 0, 2560)


def test_no_source_is_an_empty_tree(cuda):
    for depth, height in GEOMETRIES:
        got, tree = _build(cuda, [], [], depth, height)
        assert got.n_ops == 0 and got.file.numel() == 10 * 16 ** (height - 1)
        assert not got.file.any() and got.list_dir("0" * depth) == b""


# ---- the raw calls: statuses, capacities ----
def _raw(cuda, files, chunks, depth=1, height=3, lens=None, nbytes=None, cap=None, out=None, out_cap=0, write=True):
    """qlzx_htree_plan (+ write) over the packed files with the test's own lengths, cap and out:
    (totals, node_count, leaf_first)."""
    import torch
    from gobeansdb_amd import _lib, batch
    L = _lib.lib()
    blob = b"".join(files)
    nbytes = len(blob) if nbytes is None else nbytes
    lens = [len(f) for f in files] if lens is None else lens
    offs = np.cumsum([0] + [len(f) for f in files[:-1]]).astype(np.int64)
    if cap is None:
        cap = max(sum(max(n - 16, 0) for n in lens) // 23, 1)
    nleaf, nodes = 16 ** (height - 1), (16 ** height - 1) // 15
    hints = _dev(blob, cuda)
    off_d, len_d = torch.from_numpy(offs).to(cuda), torch.tensor(lens, dtype=torch.int64, device=cuda)
    chunk_d = torch.tensor(chunks, dtype=torch.int32, device=cuda)
    node_count = torch.full((nodes,), 0x5C5C5C5C, dtype=torch.int32, device=cuda)
    node_hash = torch.full((nodes,), 0x5C5C, dtype=torch.int16, device=cuda)
    leaf_first = torch.full((nleaf + 1,), 0x5C5C5C5C, dtype=torch.int32, device=cuda)
    slot_src = torch.zeros(cap, dtype=torch.int64, device=cuda)
    slot_chunk = torch.zeros(cap, dtype=torch.int32, device=cuda)
    totals = torch.full((10,), 0x5C5C5C5C, dtype=torch.int32, device=cuda)
    wsb = L.qlzx_htree_workspace_size(nbytes, len(files), cap, height)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    st = batch._stream()
    _lib.check(L.qlzx_htree_plan(hints.data_ptr(), nbytes, off_d.data_ptr(), len_d.data_ptr(), chunk_d.data_ptr(),
                                 len(files), cap, depth, height, node_count.data_ptr(), node_hash.data_ptr(),
                                 leaf_first.data_ptr(), slot_src.data_ptr(), slot_chunk.data_ptr(), totals.data_ptr(),
                                 ws.data_ptr(), wsb, st), "qlzx_htree_plan")
    if write:
        _lib.check(L.qlzx_htree_write(hints.data_ptr(), nbytes, cap, depth, height, node_count.data_ptr(),
                                      node_hash.data_ptr(), leaf_first.data_ptr(), slot_src.data_ptr(),
                                      slot_chunk.data_ptr(), out.data_ptr(), out_cap, totals.data_ptr(),
                                      ws.data_ptr(), wsb, st), "qlzx_htree_write")
    return (totals.cpu().numpy().view(np.uint32), node_count.cpu().numpy().view(np.uint32),
            leaf_first.cpu().numpy().view(np.uint32))


def _refused(t, node_count, leaf_first, status, source=None):
    from gobeansdb_amd import _lib
    assert t[_lib.HT_STATUS] == status and (source is None or t[_lib.HT_STATUS_SOURCE] == source)
    assert [t[k] for k in (_lib.HT_OPS_READ, _lib.HT_N_SET, _lib.HT_N_REMOVE, _lib.HT_N_SLOTS, _lib.HT_BYTES_LO,
                           _lib.HT_BYTES_HI)] == [0] * 6
    assert t[_lib.HT_N_LEAF] == 256 and t[9] == 0
    assert not node_count.any() and not leaf_first.any()


BAD = ["file_len 15", "the source runs past bytes", "indexOffset negative", "indexOffset past the file",
       "last item cut short"]


@pytest.mark.parametrize("case", BAD)
@pytest.mark.parametrize("at", [0, 2])
def test_bad_file(cuda, case, at):
    import torch
    from gobeansdb_amd import _lib, htree
    files, lens, nbytes = list(_three()), None, None
    f = files[at]
    io = H.read_head(f)[0]
    if case == "file_len 15":
        lens = [len(x) for x in files]
        lens[at] = 15
    elif case == "the source runs past bytes":
        nbytes = sum(len(x) for x in files[:at + 1]) - 1      # source `at` (and what follows) ends past it
    elif case == "indexOffset negative":
        files[at] = struct.pack("<q", -1) + f[8:]
    elif case == "indexOffset past the file":
        files[at] = struct.pack("<q", len(f) + 1) + f[8:]
    else:
        files[at] = struct.pack("<q", 0) + f[8:io - 1]        # no index: the items run to the (cut) end
    if lens is None and nbytes is None:
        with pytest.raises(M.BadHintFile):
            M.build(files, [0, 1, 2], 1, 3)
        with pytest.raises(_lib.QlzxError, match=f"HT_BAD_FILE, source {at}"):
            htree.build([_dev(x, cuda) for x in files], [0, 1, 2], 1, 3)
    out = torch.full((1 << 16,), FILL, dtype=torch.uint8, device=cuda)
    t, nc, lf = _raw(cuda, files, [0, 1, 2], lens=lens, nbytes=nbytes, out=out, out_cap=1 << 16)
    _refused(t, nc, lf, _lib.HT_BAD_FILE, at)
    assert (out == FILL).all()


def test_the_lowest_bad_source_is_named(cuda):
    from gobeansdb_amd import _lib
    files = list(_three())
    files[1] = struct.pack("<q", -5) + files[1][8:]
    files[2] = struct.pack("<q", 0) + files[2][8:40]
    t, nc, lf = _raw(cuda, files, [0, 1, 2], write=False)
    _refused(t, nc, lf, _lib.HT_BAD_FILE, 1)


def test_too_many(cuda):
    import torch
    from gobeansdb_amd import _lib
    files = list(_three())
    out = torch.full((1 << 16,), FILL, dtype=torch.uint8, device=cuda)
    t, nc, lf = _raw(cuda, files, [0, 1, 2], cap=3 * 300 - 1, out=out, out_cap=1 << 16)
    _refused(t, nc, lf, _lib.HT_TOO_MANY)
    assert (out == FILL).all()
    t, nc, lf = _raw(cuda, files, [0, 1, 2], cap=3 * 300, out=out, out_cap=1 << 16)
    assert t[_lib.HT_STATUS] == _lib.HT_OK and t[_lib.HT_OPS_READ] == 3 * 300
    # BAD_FILE comes first
    t, nc, lf = _raw(cuda, files[:2] + [files[2][:15]], [0, 1, 2], cap=100, write=False)
    _refused(t, nc, lf, _lib.HT_BAD_FILE, 2)


def test_no_space_and_an_exact_fit(cuda):
    import torch
    from gobeansdb_amd import _lib
    files = list(_three())
    for _ in range(12):                                     # a file length that is a multiple of neither 16 nor 4
        tree, dump, nset, nrem = M.build(files, [0, 1, 2], 1, 3)
        if len(dump) % 4:
            break
        files[2] = H.write_file(H.read_items(files[2])[:-1], 0, 300)[0]   # 18-byte items: an odd number of slots
    nb = len(dump)
    assert nb % 4 != 0
    out = torch.full((nb + 64,), FILL, dtype=torch.uint8, device=cuda)
    t, nc, lf = _raw(cuda, files, [0, 1, 2], out=out, out_cap=nb - 1)
    assert t[_lib.HT_STATUS] == _lib.HT_NO_SPACE and (out == FILL).all()
    assert int(t[_lib.HT_BYTES_LO]) == nb and t[_lib.HT_N_SLOTS] == tree.leaf_first()[-1]
    big = torch.full((nb + 4096,), FILL, dtype=torch.uint8, device=cuda)
    at = 16 * 9 + (-big.data_ptr()) % 16
    t, nc, lf = _raw(cuda, files, [0, 1, 2], out=big[at:], out_cap=nb)
    got = big.cpu().numpy()
    assert t[_lib.HT_STATUS] == _lib.HT_OK
    assert got[at:at + nb].tobytes() == dump
    assert (got[:at] == FILL).all() and (got[at + nb:] == FILL).all()


def test_plan_alone(cuda):
    files = list(_three())
    got, _ = _build(cuda, files, [0, 1, 2], 1, 3, write=False)
    assert got.file.numel() == 0 and got.n_slots > 0
    assert got.list_dir("4") != b""                        # the listing needs no file


def test_on_a_stream_of_the_callers(cuda):
    import torch
    from gobeansdb_amd import htree
    files = list(_three())
    on_dev = [_dev(f, cuda) for f in files]
    got = htree.build(on_dev, [0, 1, 2], 1, 3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    on_side = htree.build(on_dev, [0, 1, 2], 1, 3, stream=side)
    side.synchronize()
    assert torch.equal(on_side.file, got.file) and on_side.n_slots == got.n_slots


# ---- the workspace contract ----
HT_ENTRY_POINTS = ("qlzx_htree_plan", "qlzx_htree_write")


class HtProxy(W.Proxy):
    """ws_contract.Proxy for the two entry points of include/qlzx_htree.h."""

    def __getattr__(self, name):
        if name in HT_ENTRY_POINTS:
            return functools.partial(self._call, name, getattr(self._real, name))
        return super().__getattr__(name)


@pytest.mark.parametrize("poison", ["ff", "5a", "random"])
def test_workspace_contract(cuda, monkeypatch, poison):
    from gobeansdb_amd import _lib
    proxy = HtProxy(_lib.lib(), poison)
    monkeypatch.setattr(_lib, "_lib", proxy)
    a, b, c = _three()
    good = [o for _, o in H.load_index(a)]
    _build(cuda, [_with_index(a, good[:1] + [good[1] + 5] + good[2:]), _without_index(b), c,
                  struct.pack("<qII", 16, 0, 0)], [0, 1, 2, 2], 1, 3)
    _build(cuda, _sources(2, 65, 3, 2, 5), [0, 1], 2, 5)
    _build(cuda, [], [], 0, 2)
    proxy.require(HT_ENTRY_POINTS)
    assert proxy.calls["qlzx_htree_plan"] == proxy.calls["qlzx_htree_write"] == 3
    t, nc, lf = _raw(cuda, [a, b[:15], c], [0, 1, 2], write=False)
    _refused(t, nc, lf, _lib.HT_BAD_FILE, 1)


# ---- end to end on the device ----
def test_replay_build_htree_on_the_device(cuda):
    from gobeansdb_amd import hint, htree, replay
    from oracle import replay as R
    rnd = random.Random(61)
    keys = [b"%c%04d" % (97 + i % 11, i) for i in range(300)]
    got_files, want_files, chunk_ids = [], [], []
    for c in (0, 3):
        data = b"".join(R.make_record(rnd.choice(keys), bytes(rnd.getrandbits(8) for _ in range(rnd.randint(0, 40))),
                                      ver=rnd.randint(-3, 9), ts=1700000000 + i) for i in range(400))
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
    for depth, height in ((0, 3), (1, 3)):
        got = htree.build(got_files, chunk_ids, depth, height)
        tree, dump, nset, nrem = M.build(want_files, chunk_ids, depth, height)
        _same(got, tree, dump, nset, nrem)
        assert got.n_slots > 100 and got.list_dir("0" * depth) == tree.list_dir("0" * depth)
