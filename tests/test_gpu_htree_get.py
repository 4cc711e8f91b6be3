"""The HTree queries on the GPU (qlzx_htree_index / qlzx_htree_get / qlzx_gc_liveness /
qlzx_htree_move; htree.load_image / get / move, gc.liveness) against tests/htree_get_model.py.

Trees come from htree_model.build over hint_model.write_file sources (their dump uploaded and
indexed) and from htree.build on the device (its image taken as it is)."""
import functools
import random
import struct

import numpy as np
import pytest

import hint_model as H
import htree_get_model as G
import htree_model as M
import ws_contract as W
from gobeansdb_amd import _lib

pytestmark = pytest.mark.gpu
GEOMETRIES = [(0, 1), (0, 2), (1, 3), (2, 3), (2, 5)]      # L = 8, 8, 7, 6, 5; 1 to 65,536 leaves
SIZES = [0, 1, 63, 64, 65, 128, 129, 257]                  # items per leaf: around one, two and four steps of 64
POISON = 0x5C


def _dev(data: bytes, cuda):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(cuda)


def _u(t):
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize])


def _in_leaf(rnd, leaf, depth, height):
    """A keyhash of `leaf` with zero bucket nibbles."""
    p = depth + height - 1
    kh = rnd.getrandbits(64) & (M.M64 >> (4 * depth))
    if height > 1:
        kh = (kh & (M.M64 >> (4 * p))) | (leaf << (64 - 4 * p))
    return kh


def _alias(rnd, kh, depth):
    return kh | (rnd.getrandbits(4 * depth) << (64 - 4 * depth)) if depth else kh


def _leaves(depth, height, sizes, seed):
    """One source whose items fill leaf 2 i + 1 with sizes[i] distinct slots (leaf 0 of a tree
    with one leaf): (file, per size the keyhashes in leaf order)."""
    rnd = random.Random(seed)
    items, per = [], []
    for i, n in enumerate(sizes):
        seen = set()
        while len(seen) < n:
            seen.add(_in_leaf(rnd, 2 * i + 1 if height > 1 else 0, depth, height))
        khs = list(seen)
        rnd.shuffle(khs)
        per.append(khs)
        items += [H.Item(_alias(rnd, kh, depth), b"k", 0, 256 * rnd.randrange(1 << 24), rnd.randint(1, 9),
                         rnd.getrandbits(16)) for kh in khs]
    return H.write_file(items, 0, 300)[0], per


def _check_get(got, tree, khs):
    """Every output of htree.get equals the model's, the totals included."""
    first = tree.leaf_first()
    want = [G.get(tree, kh, first) for kh in khs]
    cols = [_u(x).tolist() for x in (got.status, got.chunk, got.offset, got.ver, got.vhash, got.slot)]
    cols[3] = got.ver.cpu().numpy().tolist()                           # signed
    assert [tuple(c[i] for c in cols) for i in range(len(khs))] == want
    nfound = sum(w[0] for w in want)
    assert got.totals == (nfound, len(khs) - nfound)
    return want


def _offs(offs, cuda):
    import torch
    return torch.tensor(list(offs), dtype=torch.int64, device=cuda)


def _khs(khs, cuda):
    import torch
    return torch.from_numpy(np.array(khs, np.uint64).view(np.int64)).to(cuda)


# ---- get ----
@pytest.mark.parametrize("depth,height", GEOMETRIES)
def test_get_leaf_sizes_on_every_geometry(cuda, depth, height):
    """Leaves of every size around the 64-item step, the hit at index 0, 63, 64 and last; every L,
    and (items of L + 11 bytes behind 4-byte length words) every item alignment modulo 4."""
    from gobeansdb_amd import htree
    rnd = random.Random(depth * 10 + height)
    groups = [SIZES] if height > 1 else [[n] for n in SIZES]            # one leaf: a tree per size
    for sizes in groups:
        file, per = _leaves(depth, height, sizes, 7 * depth + height + sizes[0])
        tree, dump, _, _ = M.build([file], [5], depth, height)
        khs = []
        for leaf in per:
            hits = [leaf[k] for k in sorted({0, 63, 64, len(leaf) - 1}) if 0 <= k < len(leaf)]
            khs += [_alias(rnd, kh, depth) for kh in hits]
            khs += [kh ^ 1 for kh in hits[:2]]                         # the lowest stored bit differs
        khs.append(_in_leaf(rnd, 0, depth, height))                    # an empty leaf (or a miss in the only one)
        image = htree.load_image(_dev(dump, cuda), depth, height)
        assert _u(image.leaf_first).tolist() == tree.leaf_first() and image.n_items == sum(sizes)
        want = _check_get(htree.get(image, keyhash=_khs(khs, cuda)), tree, khs)
        assert sum(w[0] for w in want) == sum(len({0, 63, 64, n - 1} & set(range(n))) for n in sizes)
        built = htree.build([_dev(file, cuda)], [5], depth, height)    # the device's own tree, no index call
        assert built.file.cpu().numpy().tobytes() == dump
        for shape in ("wave", "lane"):
            _check_get(htree.get(built.image(), keyhash=_khs(khs, cuda), _shape=shape), tree, khs)
    # the items start at every residue modulo 4 that their length reaches: all four for 19 and 17 bytes
    starts = {(6 * len(tree.leafs) + 4 + tree.item_len * k) % 4 for k in range(tree.leaf_first()[-1])}
    assert len(starts) == {19: 4, 18: 2, 17: 4, 16: 1}[tree.item_len]


@pytest.mark.parametrize("depth,height", [(0, 2), (1, 3), (2, 3), (2, 5)])
def test_get_near_misses_and_aliases(cuda, depth, height):
    from gobeansdb_amd import htree
    rnd = random.Random(99 + depth + height)
    file, per = _leaves(depth, height, [70, 3], 31)
    tree, dump, _, _ = M.build([file], [2], depth, height)
    L = tree.khash_len
    kh = per[0][66]
    khs = [kh, kh ^ (1 << (8 * (L - 1)))]                              # byte L - 1 differs: the same leaf, a miss
    assert G.leaf_of(tree, khs[1]) == G.leaf_of(tree, kh)
    if 8 * L < 64 - 4 * depth:                                         # the low L bytes of an item of another leaf
        khs.append(kh ^ (1 << (8 * L)))
        assert G.leaf_of(tree, khs[-1]) != G.leaf_of(tree, kh)
    if depth:                                                          # only the bucket nibbles differ: the same slot
        khs += [kh | (b << (64 - 4 * depth)) for b in (1, (1 << (4 * depth)) - 1)]
    image = htree.load_image(_dev(dump, cuda), depth, height)
    for shape in ("wave", "lane"):
        want = _check_get(htree.get(image, keyhash=_khs(khs, cuda), _shape=shape), tree, khs)
        assert [w[0] for w in want] == [1, 0] + [0] * (8 * L < 64 - 4 * depth) + [1, 1] * bool(depth)


def test_get_a_negative_version_and_the_lower_of_two_equal_items(cuda):
    """An uploaded image may hold what no build makes: a ver < 0 item (HTree.set stores it), and
    (hand-made) two items with equal stored bytes in one leaf."""
    from gobeansdb_amd import htree
    rnd = random.Random(4)
    tree = M.HTree(1, 3)
    khs = [_in_leaf(rnd, 0x21, 1, 3) for _ in range(70)]
    for i, kh in enumerate(khs):
        tree.set(kh, -3 if i in (0, 65) else i + 1, 100 + i, 4, 256 * i)
    dup = struct.pack("<Q", khs[65])[:7] + M.item_to_bytes(77, 7, 0x7700, 9)
    tree.leafs[0x21] += dup                                            # behind the item it repeats
    tree.leafs[0x21][0:0] = struct.pack("<Q", khs[68])[:7] + M.item_to_bytes(88, 8, 0x8800, 9)   # before it
    image = htree.load_image(_dev(tree.dump(), cuda), 1, 3)
    assert image.n_items == 72
    for shape in ("wave", "lane"):
        want = _check_get(htree.get(image, keyhash=_khs(khs, cuda), _shape=shape), tree, khs)
        assert want[0][3] == want[65][3] == -3 and want[65][5] == 66 and want[68] == (1, 9, 0x8800, 88, 8, 0)


@functools.lru_cache(maxsize=None)
def _keyed_tree():
    """600 keys at depth 1, height 3, hashed by the model: (keys, tree, dump)."""
    keys = [b"key:%05d" % i + b"x" * (i % 7) for i in range(600)]
    items = [H.Item(H.keyhash(k), k, 0, 256 * (i + 1), 1 + i % 5, (i * 7) & 0xFFFF) for i, k in enumerate(keys)]
    file = H.write_file(sorted(items, key=lambda it: (it.keyhash, it.key)), 0, 128)[0]
    tree, dump, _, _ = M.build([file], [6], 1, 3)
    return keys, tree, dump


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, _lib.HTG_LANE_FROM - 1, _lib.HTG_LANE_FROM])
def test_get_batch_sizes_both_shapes_keys_and_hashes(cuda, n):
    """Batches around a block of four waves and of 256 lanes, and on each side of the switch from a
    wave to a lane per key (the tree's leaves hold two or three items: below QLZX_HTG_LANE_LEAF);
    keys hashed on the device and hashes given; both shapes and the default one give the same
    entries; slot indexes the image."""
    import torch
    from gobeansdb_amd import batch, htree
    keys, tree, dump = _keyed_tree()
    rnd = random.Random(n)
    ask = [rnd.choice(keys) if rnd.random() < 0.7 else b"absent:%d" % i for i in range(n)]
    khs = [H.keyhash(k) for k in ask]
    image = htree.load_image(_dev(dump, cuda), 1, 3)
    blocks = batch.BlockBatch.from_bytes(ask, device=cuda)
    results = [htree.get(image, blocks, _shape=s) for s in (None, "wave", "lane")]
    results += [htree.get(image, keyhash=_khs(khs, cuda), _shape=s) for s in (None, "wave", "lane")]
    results.append(htree.get(image, blocks, keyhash=_khs(khs, cuda)))
    want = _check_get(results[0], tree, khs)
    for r in results[1:]:
        assert r.totals == results[0].totals
        for a, b in zip(tuple(r)[:6], tuple(results[0])[:6]):
            assert torch.equal(a, b)
    # re-reading the item at `slot` gives the same fields
    first = np.array(tree.leaf_first())
    for (found, chunk, offset, ver, vhash, slot), kh in zip(want, khs):
        if found:
            leaf = int(np.searchsorted(first, slot, side="right")) - 1
            at = 6 * 256 + 4 * (leaf + 1) + 18 * slot
            assert dump[at:at + 7] == struct.pack("<Q", kh & (M.M64 >> 4))[:7]
            assert M.bytes_to_item(dump[at + 7:at + 18]) == (ver, vhash, offset, chunk)


def test_get_past_the_grid_caps_of_both_shapes(cuda):
    """The get's two kernels stride over what 2,048 blocks do not hold: more than 8,192 keys for
    the wave shape, more than 524,288 for the lane shape.  4,096 keys checked against the model,
    then asked for 129 times over and five more: every entry is its base entry's, the totals sum."""
    import torch
    from gobeansdb_amd import htree
    keys, tree, dump = _keyed_tree()
    rnd = random.Random(77)
    base = [H.keyhash(rnd.choice(keys) if rnd.random() < 0.7 else b"absent:%d" % i) for i in range(4096)]
    image = htree.load_image(_dev(dump, cuda), 1, 3)
    base_d = _khs(base, cuda)
    first = htree.get(image, keyhash=base_d)
    want = _check_get(first, tree, base)
    n = 4096 * 129 + 5
    assert n > 256 * 2048 and n > 4 * 2048
    tiled = base_d.repeat(130)[:n]
    nfound = sum(w[0] for w in want) * 129 + sum(w[0] for w in want[:5])
    for shape in ("wave", "lane", None):
        got = htree.get(image, keyhash=tiled, _shape=shape)
        assert got.totals == (nfound, n - nfound)
        for a, b in zip(tuple(got)[:6], tuple(first)[:6]):
            assert torch.equal(a, b.repeat(130)[:n])


# ---- index ----
@pytest.mark.parametrize("depth,height", GEOMETRIES)
def test_index_of_the_write_equals_the_plans_leaf_first(cuda, depth, height):
    import torch
    from gobeansdb_amd import htree
    file, _ = _leaves(depth, height, [5, 0, 70, 1] if height > 1 else [76], 3)
    built = htree.build([_dev(file, cuda)], [1], depth, height)
    image = htree.load_image(built.file, depth, height)
    assert torch.equal(image.leaf_first, built.leaf_first) and image.n_items == built.n_slots == 76
    assert image.file.data_ptr() == built.file.data_ptr()              # indexed in place, not copied


@pytest.mark.parametrize("where", ["first", "last", "every 16th"])
@pytest.mark.parametrize("depth,height", [(0, 1), (1, 3), (2, 5)])
def test_index_where_the_counts_do_not_give_the_places(cuda, depth, height, where):
    """ver < 0 items are in the leaf and not in its count: the guess fails from that leaf on."""
    from gobeansdb_amd import htree
    rnd = random.Random(5)
    tree = M.HTree(depth, height)
    nleaf = len(tree.leafs)
    odd = {"first": [0], "last": [nleaf - 1], "every 16th": list(range(0, nleaf, 16))}[where]
    for leaf in sorted(set(odd + [rnd.randrange(nleaf) for _ in range(200)])):
        for k in range(rnd.randint(1, 3)):
            neg = leaf in odd and k == 0
            tree.set(_in_leaf(rnd, leaf, depth, height), -2 if neg else 3, rnd.getrandbits(16), 1, 256 * k)
    tree.update_nodes(0, 0)
    dump = tree.dump()
    image = htree.load_image(_dev(dump, cuda), depth, height)
    assert _u(image.leaf_first).tolist() == tree.leaf_first()
    assert image.n_items == tree.leaf_first()[-1] > sum(n.count for n in tree.levels[-1])
    assert G.load(dump, depth, height).leaf_first() == tree.leaf_first()


def _raw_index(cuda, image: bytes, depth, height, nbytes=None):
    import torch
    from gobeansdb_amd import _lib, batch
    L = _lib.lib()
    nleaf = 16 ** (height - 1)
    dev = _dev(image + bytes(64), cuda)                                # room behind a cut: `bytes` is the limit
    leaf_first = torch.full((nleaf + 1,), 0x5C5C5C5C, dtype=torch.int32, device=cuda)
    totals = torch.full((4,), 0x5C5C5C5C, dtype=torch.int32, device=cuda)
    wsb = L.qlzx_htree_index_workspace_size(height)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    _lib.check(L.qlzx_htree_index(dev.data_ptr(), len(image) if nbytes is None else nbytes, depth, height,
                                  leaf_first.data_ptr(), totals.data_ptr(), ws.data_ptr(), wsb, batch._stream()),
               "qlzx_htree_index")
    return _u(totals).tolist(), _u(leaf_first)


def test_index_bad_and_odd_images(cuda):
    from gobeansdb_amd import _lib, htree
    file, _ = _leaves(1, 3, [5, 0, 70, 1], 3)                          # leaves 1, 5 and 7 hold items
    tree, dump, _, _ = M.build([file], [1], 1, 3)
    first = tree.leaf_first()
    at5 = 1536 + 4 * 5 + 18 * first[5]                                 # leaf 5's length word
    cases = [(dump[:1000], "the node table"), (dump[:at5 + 2], "a length word"), (dump[:at5 + 4 + 18 * 70 - 1], "a leaf"),
             (dump[:at5] + struct.pack("<I", 18 * 70 + 1) + dump[at5 + 4:] + b"\0", "item_len + 1"),
             (dump[:-1], "the last leaf's last byte"), (b"", "no byte at all")]
    for image, what in cases:
        with pytest.raises(G.BadImage) as e:
            G.load(image, 1, 3)
        t, lf = _raw_index(cuda, image, 1, 3)
        assert t == [0, 256, _lib.HTG_BAD_FILE, e.value.leaf] and not lf.any(), what
        if image:
            with pytest.raises(_lib.QlzxError, match=f"HTG_BAD_FILE, leaf {e.value.leaf}$"):
                htree.load_image(_dev(image, cuda), 1, 3)
    # two bad leaves: the lowest is named
    two = bytearray(dump)
    two[1536 + 4:1536 + 8] = struct.pack("<I", 18 * 5 + 1)
    t, lf = _raw_index(cuda, bytes(two), 1, 3)
    assert t == [0, 256, _lib.HTG_BAD_FILE, 1] and not lf.any()
    # trailing bytes are ignored; `bytes` is the limit, not the buffer
    t, lf = _raw_index(cuda, dump + b"\xff" * 37, 1, 3)
    assert t == [76, 256, _lib.HTG_OK, 0] and lf.tolist() == first
    t, lf = _raw_index(cuda, dump + b"\xff" * 37, 1, 3, nbytes=len(dump) - 1)
    assert t[2:] == [_lib.HTG_BAD_FILE, 255]
    # no item at all
    for depth, height in GEOMETRIES:
        t, lf = _raw_index(cuda, M.HTree(depth, height).dump(), depth, height)
        assert t == [0, 16 ** (height - 1), _lib.HTG_OK, 0] and not lf.any()


# ---- liveness and move ----
SRC = 3


def _gc_case(count, seed=0):
    """A chunk of `count` rec_off entries (one of them no record when count > 1) and the tree of
    its bucket: (data, rec_off, records for the model, keys, tree).
    The tree comes from hints that name, per key in turn: this chunk at the key's last record
    (NEWEST there, OTHER_POS at its older versions), this chunk at another offset, another chunk at
    the same offset (both OTHER_POS), nothing (NOT_IN_TREE); then a ver < 0 item elsewhere is set
    on the model tree, as HTree.set stores it."""
    from oracle import replay as R
    rnd = random.Random(1000 * count + seed)
    nrec = count - 1 if count > 1 else 1
    keys = [b"gc:%04d" % i for i in range(max(nrec * 2 // 3, 1))]
    data, offs, recs = b"", [], []
    for i in range(nrec):
        key = keys[i] if i < len(keys) else rnd.choice(keys)            # every key, then more versions of some
        ver = (-2, 1, 2, 7)[i % 4] if i < len(keys) else rnd.choice((-2, 1, 2, 7))   # key 8, never in the tree: a delete
        body = bytes(rnd.getrandbits(8) for _ in range(rnd.choice((0, 10, 300))))
        offs.append(len(data))
        recs.append((len(data), H.keyhash(key), ver, key))
        data += R.make_record(key, body, ver=ver, ts=1700000000 + i)
    if count > 1:                                                       # 256 zero bytes: a header with ksz = 0
        at = count // 2
        offs.insert(at, len(data))
        recs.insert(at, (len(data), None, 0, None))
        data += bytes(256)
    last = {}
    for off, kh, ver, key in recs:
        if key is not None:
            last[key] = (off, kh)
    items, neg = [], []
    for i, key in enumerate(keys):
        off, kh = last[key]
        how = i % 5
        if how == 0 or how == 4:
            items.append(H.Item(kh, key, 0, off, 5, 40 + i))            # chunk SRC (the file's), this offset
        elif how == 1:
            items.append(H.Item(kh, key, 0, off + 256, 5, 40 + i))      # chunk SRC, another offset
        elif how == 2:
            neg.append((kh, off, i))                                   # set below with ver < 0
    other = [H.Item(last[k][1], k, 0, last[k][0], 6, 90 + i) for i, k in enumerate(keys) if i % 5 == 3 and i % 10 != 8]
    tree = M.build([H.write_file(items, 0, 128)[0], H.write_file(other, 0, 128)[0]], [SRC, SRC + 1], 1, 3)[0]
    for kh, off, i in neg:
        tree.set(kh, -9, 60 + i, SRC + 2, off)
    tree.update_nodes(0, 0)
    return data, offs, [r[:3] for r in recs], keys, tree


def _raw_liveness(cuda, data_d, offs, image, flags, extra=7, keyhash=None):
    """qlzx_gc_liveness with arrays of len(offs) + extra entries poisoned first: every output as a
    numpy array (whole), ask_idx and totals."""
    import torch
    from gobeansdb_amd import _lib, batch
    from gobeansdb_amd.record import BODY_MAX, MAX_KEY_LEN
    L = _lib.lib()
    n, cap = len(offs), len(offs) + extra
    rec_off = torch.tensor(list(offs) + [0] * extra, dtype=torch.int64, device=cuda)
    result = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=cuda)
    keep = torch.full((cap,), POISON, dtype=torch.uint8, device=cuda)
    verdict, tree_ver, slot, ask = (torch.full((cap,), 0x5C5C5C5C, dtype=torch.int32, device=cuda) for _ in range(4))
    vhash = torch.full((cap,), 0x5C5C, dtype=torch.int16, device=cuda)
    totals = torch.full((8,), 0x5C5C5C5C, dtype=torch.int32, device=cuda)
    wsb = L.qlzx_gc_liveness_workspace_size(cap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    kh = None if keyhash is None else _khs(list(keyhash) + [0] * extra, cuda)
    _lib.check(L.qlzx_gc_liveness(data_d.data_ptr(), int(data_d.numel()), rec_off.data_ptr(), result.data_ptr(), cap,
                                  MAX_KEY_LEN, BODY_MAX, SRC, image.file.data_ptr(), int(image.file.numel()),
                                  image.leaf_first.data_ptr(), image.depth, image.height,
                                  None if kh is None else kh.data_ptr(), flags, keep.data_ptr(), verdict.data_ptr(),
                                  vhash.data_ptr(), tree_ver.data_ptr(), slot.data_ptr(), ask.data_ptr(),
                                  totals.data_ptr(), ws.data_ptr(), wsb, batch._stream()), "qlzx_gc_liveness")
    return (_u(keep), verdict.cpu().numpy(), _u(vhash), tree_ver.cpu().numpy(), _u(slot)), _u(ask), _u(totals).tolist()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_liveness_against_the_model(cuda, count):
    from gobeansdb_amd import gc, htree
    data, offs, recs, keys, tree = _gc_case(count)
    data_d = _dev(data, cuda)
    image = htree.load_image(_dev(tree.dump(), cuda), 1, 3)
    for begin in (False, True):
        rows, ask, t = G.gc_liveness(tree, recs, SRC, begin)
        for hashes in (None, [kh or 0 for _, kh, _ in recs]):
            cols, got_ask, got_t = _raw_liveness(cuda, data_d, offs, image, int(begin), keyhash=hashes)
            assert got_t == t
            assert [tuple(int(c[j]) for c in cols) for j in range(count)] == rows
            assert got_ask[:len(ask)].tolist() == ask == sorted(ask)
            assert (got_ask[len(ask):] == 0x5C5C5C5C).all()            # the list holds OTHER_POS records only
            for c, fill in zip(cols, (POISON, 0x5C5C5C5C, 0x5C5C, 0x5C5C5C5C, 0x5C5C5C5C)):
                assert (c[count:] == fill).all()                       # entries past result[0] are not written
        live = gc.liveness(data_d, _offs(offs, cuda), image, SRC, begin_gt_0=begin)
        assert live.totals.tolist() == t and _u(live.ask_idx).tolist() == ask
        assert [tuple(int(x) for x in r) for r in zip(_u(live.keep), live.verdict.cpu().numpy(), _u(live.vhash),
                                                      live.tree_ver.cpu().numpy(), _u(live.slot))] == rows
    if count >= 63:                                                     # the case holds every verdict
        assert all(t[k] > 0 for k in range(8))


def _moved_model(tree, recs, live, gcb, ids):
    from gobeansdb_amd import _lib
    verdict, status = live.verdict.cpu().numpy(), gcb.status.cpu().numpy()
    chunk, off = gcb.new_chunk.cpu().numpy(), _u(gcb.new_off)
    moved = 0
    for j, (_, kh, _) in enumerate(recs):
        if verdict[j] == _lib.GL_NEWEST and status[j] == _lib.GC_WRITTEN:
            assert G.update_pos(tree, kh, ids[int(chunk[j])], int(off[j]))
            moved += 1
    return moved


def test_move_after_liveness_and_rewrite_with_a_rotation(cuda):
    from gobeansdb_amd import _lib, gc, htree
    data, offs, recs, keys, tree = _gc_case(257, seed=1)
    before = tree.dump()
    data_d = _dev(data, cuda)
    image = htree.load_image(_dev(before, cuda), 1, 3)
    offs_d = _offs(offs, cuda)
    live = gc.liveness(data_d, offs_d, image, SRC)
    gcb = gc.rewrite_batch(data_d, offs_d, live.keep, dst_head=512, data_file_max=40 * 256, max_chunks=64)
    assert len(gcb.chunks) > 2 and int(gcb.totals[2]) == int(live.totals[_lib.GL_N_KEEP]) > 20
    ids = [7 + 3 * c for c in range(64)]
    moved, skipped = htree.move(image, live, gcb, ids)
    want_moved = _moved_model(tree, recs, live, gcb, ids)
    assert (moved, skipped) == (want_moved, 0) and moved == int(gcb.totals[2])
    after = image.file.cpu().numpy().tobytes()
    assert after == tree.dump() and after != before
    assert after[:1536] == before[:1536]                                # the node table: counts and hashes stay
    assert len(after) == len(before)


def test_move_skips_and_counts_what_it_cannot_store(cuda):
    import torch
    from gobeansdb_amd import _lib, batch, htree
    file, per = _leaves(1, 3, [5, 70], 8)
    tree, dump, _, _ = M.build([file], [1], 1, 3)
    image = htree.load_image(_dev(dump, cuda), 1, 3)
    L = _lib.lib()
    N, W_, D = _lib.GL_NEWEST, _lib.GC_WRITTEN, _lib.GC_DROPPED
    #        verdict            gc_status slot        chunk off
    rows = [(N, W_, 0, 0, 0x100),                                       # moved
            (N, W_, 74, 1, 0xFFFFFF00),                                 # moved: the last item, the largest offset
            (N, W_, 1, 0, 1 << 32),                                     # new_off >= 2^32
            (N, W_, 2, 0, 0x180),                                       # no multiple of 256
            (N, W_, 3, 2, 0x100),                                       # chunk id 65536
            (N, W_, 4, 3, 0x100),                                       # new_chunk >= max_chunks
            (N, W_, 75, 0, 0x100),                                      # behind the last item
            (N, W_, 0xFFFFFFFF, 0, 0x100),                              # no slot
            (N, D, 5, 0, 0x100), (_lib.GL_OTHER_POS, W_, 6, 0, 0x100),  # not acted on, not counted
            (N, W_, 7, 0, 0x100)]                                       # past result[0]
    t32 = lambda k: torch.from_numpy(np.array([r[k] for r in rows], np.uint32).view(np.int32)).to(cuda)
    new_off = torch.from_numpy(np.array([r[4] for r in rows], np.uint64).view(np.int64)).to(cuda)
    ids = torch.tensor([9, 65535, 65536], dtype=torch.int32, device=cuda)
    result = torch.tensor([len(rows) - 1, 0, 0, 0], dtype=torch.int32, device=cuda)
    totals = torch.full((2,), 0x5C5C5C5C, dtype=torch.int32, device=cuda)
    wsb = L.qlzx_htree_move_workspace_size(len(rows))
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    cols = [t32(k) for k in range(4)]
    _lib.check(L.qlzx_htree_move(image.file.data_ptr(), len(dump), image.leaf_first.data_ptr(), 1, 3, result.data_ptr(),
                                 len(rows), cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(),
                                 cols[3].data_ptr(), new_off.data_ptr(), ids.data_ptr(), 3, totals.data_ptr(),
                                 ws.data_ptr(), wsb, batch._stream()), "qlzx_htree_move")
    assert _u(totals).tolist() == [2, 6]
    first = tree.leaf_first()
    want = bytearray(dump)
    for slot, pos in ((0, bytes.fromhex("010000" "0900")), (74, bytes.fromhex("ffffff" "ffff"))):
        leaf = int(np.searchsorted(np.array(first), slot, side="right")) - 1
        at = 1536 + 4 * (leaf + 1) + 18 * slot + 7 + 6
        want[at:at + 5] = pos
    assert image.file.cpu().numpy().tobytes() == bytes(want)


# ---- the workspace contract, the caller's stream ----
HTG_ENTRY_POINTS = ("qlzx_htree_index", "qlzx_htree_get", "qlzx_gc_liveness", "qlzx_htree_move")


class HtgProxy(W.Proxy):
    """ws_contract.Proxy for the four entry points of include/qlzx_htree_get.h."""

    def __getattr__(self, name):
        if name in HTG_ENTRY_POINTS:
            return functools.partial(self._call, name, getattr(self._real, name))
        return super().__getattr__(name)


@pytest.mark.parametrize("poison", ["ff", "5a", "random"])
def test_workspace_contract(cuda, monkeypatch, poison):
    from gobeansdb_amd import _lib, batch, gc, htree
    proxy = HtgProxy(_lib.lib(), poison)
    monkeypatch.setattr(_lib, "_lib", proxy)
    data, offs, recs, keys, tree = _gc_case(65, seed=2)
    before = tree.dump()
    data_d = _dev(data, cuda)
    image = htree.load_image(_dev(before, cuda), 1, 3)                  # ver < 0 items: the walk
    assert _u(image.leaf_first).tolist() == tree.leaf_first()
    ask = keys[:40] + [b"nowhere"]
    khs = [H.keyhash(k) for k in ask]
    for shape in ("wave", "lane"):
        _check_get(htree.get(image, batch.BlockBatch.from_bytes(ask, device=cuda), _shape=shape), tree, khs)
    offs_d = _offs(offs, cuda)
    live = gc.liveness(data_d, offs_d, image, SRC, begin_gt_0=True)
    rows, want_ask, t = G.gc_liveness(tree, recs, SRC, True)
    assert live.totals.tolist() == t and _u(live.ask_idx).tolist() == want_ask
    gcb = gc.rewrite_batch(data_d, offs_d, live.keep)
    ids = [11]
    assert htree.move(image, live, gcb, ids) == (_moved_model(tree, recs, live, gcb, ids), 0)
    assert image.file.cpu().numpy().tobytes() == tree.dump()
    t0, lf = _raw_index(cuda, before[:2000], 1, 3)                      # a refused image, through the proxy too
    assert t0[2] == _lib.HTG_BAD_FILE and not lf.any()
    proxy.require(HTG_ENTRY_POINTS)
    assert proxy.calls["qlzx_htree_get"] == 2 and proxy.calls["qlzx_htree_index"] == 2


def test_on_a_stream_of_the_callers(cuda):
    import torch
    from gobeansdb_amd import gc, htree
    data, offs, recs, keys, tree = _gc_case(65, seed=3)
    data_d, dump_d, offs_d = _dev(data, cuda), _dev(tree.dump(), cuda), _offs(offs, cuda)
    khs = _khs([H.keyhash(k) for k in keys], cuda)

    def run(stream):
        image = htree.load_image(dump_d.clone(), 1, 3, stream=stream)
        got = htree.get(image, keyhash=khs, stream=stream)
        live = gc.liveness(data_d, offs_d, image, SRC, stream=stream)
        gcb = gc.rewrite_batch(data_d, offs_d, live.keep, stream=stream)
        moved = htree.move(image, live, gcb, [8], stream=stream)
        return image, got, live, moved

    base = run(None)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    on_side = run(side)
    side.synchronize()
    assert torch.equal(on_side[0].file, base[0].file) and torch.equal(on_side[0].leaf_first, base[0].leaf_first)
    assert torch.equal(on_side[1].slot, base[1].slot) and on_side[1].totals == base[1].totals
    assert torch.equal(on_side[2].keep, base[2].keep) and on_side[3] == base[3] and base[3][0] > 0


# ---- end to end on the device ----
def test_open_get_gc_get_on_the_device(cuda):
    """Records -> replay -> hint.build -> htree.build -> htree.get -> read_records; then
    gc.liveness -> gc.rewrite_batch -> htree.move -> htree.get -> read_records in the rewritten
    chunk.  Between the steps only totals are read back."""
    import torch
    from gobeansdb_amd import _lib, batch, gc, hint, htree, replay
    from oracle import replay as R
    rnd = random.Random(17)
    keys = [b"%c%04d" % (97 + i % 11, i) for i in range(150)]
    data = b"".join(R.make_record(rnd.choice(keys), bytes(rnd.getrandbits(8) for _ in range(rnd.randint(0, 600))),
                                  ver=rnd.choice((-1, 1, 2, 3, 4)), ts=1700000000 + i) for i in range(400))
    rows, err = R.replay(data)
    assert err is None and len(rows) == 400
    by_off = {row[0]: row for row in rows}
    data_d = _dev(data, cuda)
    res = replay.replay(data_d)
    splits = hint.build(res, split_cap=64, chunk_id=SRC)
    built = htree.build([sp.file for sp in splits], [SRC] * len(splits), 1, 3)
    image = built.image()
    ask = keys + [b"never:%d" % i for i in range(9)]
    blocks = batch.BlockBatch.from_bytes(ask, device=cuda)
    # the last request asks with another key's hash: it shares that key's slot
    khs = hint.keyhash(blocks)
    got0 = htree.get(image, blocks)
    shared = int(torch.nonzero(got0.status == _lib.HTG_FOUND)[0])
    khs[-1] = khs[shared]
    got = htree.get(image, blocks, keyhash=khs)
    # the model's tree over the same files
    tree = M.build([sp.file.cpu().numpy().tobytes() for sp in splits], [SRC] * len(splits), 1, 3)[0]
    want = _check_get(got, tree, [H.keyhash(k) for k in ask[:-1]] + [H.keyhash(ask[shared])])
    found = torch.nonzero(got.status == _lib.HTG_FOUND).flatten()
    idx = found.cpu().numpy().tolist()
    assert idx[-1] == len(ask) - 1 and 50 < len(idx) < len(keys)
    assert all(want[i][1] == SRC for i in idx)
    rd = replay.read_records(data_d, (got.offset[found].to(torch.int64) & 0xFFFFFFFF), keys=[ask[i] for i in idx])
    assert (rd.status == _lib.RD_OK).all()
    assert rd.key_eq.cpu().numpy().tolist() == [1] * (len(idx) - 1) + [0]
    values = {}
    for k, i in enumerate(idx[:-1]):
        row = by_off[want[i][2]]
        assert row[2] == ask[i] and rd.value(k) == row[5] and want[i][3] == row[3] and want[i][4] == row[6]
        values[ask[i]] = row[5]
    # GC of the chunk against its own tree, and the tree after it
    live = gc.liveness(data_d, res.offset, image, SRC)
    assert int(live.totals[_lib.GL_N_NEWEST]) == len(idx) - 1 == int(live.totals[_lib.GL_N_KEEP])
    assert int(live.totals[_lib.GL_N_OTHER_POS]) + int(live.totals[_lib.GL_N_NOT_IN_TREE]) == 400 - (len(idx) - 1)
    gcb = gc.rewrite_batch(data_d, res.offset, live.keep)
    assert int(gcb.totals[2]) == len(idx) - 1 and int(gcb.totals[6]) == 0 and len(gcb.chunks) == 1
    assert htree.move(image, live, gcb, [SRC + 2]) == (len(idx) - 1, 0)
    kept = [ask[i] for i in idx[:-1]]
    got2 = htree.get(image, batch.BlockBatch.from_bytes(kept, device=cuda))
    assert got2.totals == (len(kept), 0) and (got2.chunk == SRC + 2).all()
    # every kept record's new position is where the rewrite put it
    newest = torch.nonzero(live.verdict == _lib.GL_NEWEST).flatten()
    assert sorted(_u(gcb.new_off[newest]).tolist()) == sorted(_u(got2.offset).tolist())
    rd2 = replay.read_records(gcb.chunks[0], got2.offset.to(torch.int64) & 0xFFFFFFFF, keys=kept)
    assert (rd2.status == _lib.RD_OK).all() and rd2.key_eq.all()
    assert [rd2.value(k) for k in range(len(kept))] == [values[k] for k in kept]
