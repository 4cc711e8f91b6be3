"""The hint-file batch calls past their grid caps ("Counts beyond the grid caps"):
hint.build and hint.keyhash over 1,056,000 records, hint.merge of 1,200,000 items, hint.lookup of
1,056,000 requests, htree.build over 1,072,500 ops.  Inputs and expectations are tests/scale.py's, whose rules and vectorised
restatements tests/test_scale_rules.py holds against the models; every comparison is exact."""
import numpy as np
import pytest
import torch

import htree_model as HT
import scale as S

pytestmark = pytest.mark.gpu
NDUP = 4096
EARLY = 200          # keys that the HTree's source 0 alone holds


def _t(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ------------------------------------------------------------------ hint build, keyhash ----
@pytest.fixture(scope="module")
def records(cuda):
    """N one-slot records as a replay of their chunk would hand them over: the chunk holds every
    record's key behind its header (hint.build reads nothing else of it), written with torch."""
    from gobeansdb_amd import batch, replay
    r = S.hint_records(S.N, NDUP)
    n = S.N
    data = torch.zeros(n, 256, dtype=torch.uint8, device=cuda)
    data[:, 24:24 + S.KEY_LEN] = _t(r.keys, cuda)
    header = np.zeros((n, 6), np.int32)
    header[:, 3], header[:, 4], header[:, 5] = r.ver, S.KEY_LEN, r.vsz
    data[:, :24] = _t(header.view(np.uint8).reshape(n, 24), cuda)
    z32 = torch.zeros(n, dtype=torch.int32, device=cuda)
    none = batch.BlockBatch(torch.zeros(1, dtype=torch.uint8, device=cuda), torch.zeros(0, dtype=torch.int64, device=cuda),
                            torch.zeros(0, dtype=torch.int32, device=cuda))
    res = replay.ReplayResult(_t(r.off, cuda), z32, _t(header, cuda), z32, _t(r.vsz, cuda),
                              _t(r.vhash.astype(np.int32), cuda),
                              none, False, n, n, torch.zeros(n, dtype=torch.uint8, device=cuda),
                              _t(r.off + 24 + S.KEY_LEN, cuda), data.reshape(-1))
    torch.cuda.synchronize()
    yield r, res
    del res, data
    torch.cuda.empty_cache()


@pytest.mark.parametrize("interval", [4096, 128])
def test_scale_hint_build(records, interval):
    """The default split_cap of 2^20 cuts for real: 1,051,904 distinct keys, 4,096 of them written
    twice (the later record wins, datasize counts both), so the first split takes 1,052,672 records
    and the second the rest.  Second trips of every plan kernel, of the index kernels and of
    k_hint_file; rocPRIM's sort and scans at their large-input sizes.  At interval 128 every item
    is an index entry (the threshold 128 - 23 - 256 is negative)."""
    from gobeansdb_amd import hint
    r, res = records
    for k in ("k_hint_hash", "k_hint_compact", "k_hint_runs", "k_hint_first", "k_hint_cut", "k_hint_items", "k_hint_emit",
              "k_hint_file"):
        assert res.n == S.N > S.over("qlzx_hint.hip", k)
    want = S.hint_build_fixed(r, hint.SPLIT_CAP, interval, chunk_id=7)
    assert hint.SPLIT_CAP == S.TWO20 and [w.num_key for w in want] == [S.TWO20, S.N - NDUP - S.TWO20]
    assert want[0].consumed == S.TWO20 + NDUP and want[0].num_key > S.over("qlzx_hint_fmt.h", "k_hint_index")
    assert interval != 128 or want[0].n_index == want[0].num_key
    got = hint.build(res, index_interval=interval, chunk_id=7)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert (g.consumed, g.num_key, g.datasize, g.n_index, g.index_offset, g.skipped) == \
            (w.consumed, w.num_key, w.datasize, w.n_index, w.index_offset, w.skipped)
        wf = _t(w.file, g.file.device)
        assert g.file.numel() == wf.numel()
        bad = torch.nonzero(g.file != wf)
        assert bad.numel() == 0, (int(bad[0]), int(bad.numel()))


def test_scale_keyhash(records):
    """hint.keyhash over the same N keys, packed 13 bytes apart behind one odd byte: the keys'
    addresses take every residue mod 4, so three of four go through the byte-assembling loads."""
    from gobeansdb_amd import batch, hint
    r, res = records
    assert S.N > S.over("qlzx_api.hip", "k_keyhash")
    dev = res.data.device
    rows = torch.full((S.N, 13), 0x5C, dtype=torch.uint8, device=dev)
    rows[:, :S.KEY_LEN] = _t(r.keys, dev)
    buf = torch.cat([torch.full((1,), 0x5C, dtype=torch.uint8, device=dev), rows.reshape(-1)])
    off = 1 + 13 * torch.arange(S.N, dtype=torch.int64, device=dev)
    at = (buf.data_ptr() + off) % 4                     # the addresses, not the offsets
    assert buf.data_ptr() % 16 == 0 and torch.bincount(at, minlength=4).min().item() >= S.N // 4
    assert int((at[S.over("qlzx_api.hip", "k_keyhash"):] != 0).sum()) > 300000      # unaligned ones in the second trip
    keys = batch.BlockBatch(buf, off, torch.full((S.N,), S.KEY_LEN, dtype=torch.int32, device=dev))
    got = hint.keyhash(keys)
    torch.cuda.synchronize()
    bad = torch.nonzero(got != _t(r.kh.view(np.int64), dev))
    assert bad.numel() == 0, (int(bad[0]), int(bad.numel()))


# ------------------------------------------------------------------ lookup ----
@pytest.fixture(scope="module")
def lookups(cuda):
    b = S.lookup_base()
    files = [_t(f, cuda) for f in b.files]
    # the keys behind one byte: odd addresses
    keys = torch.cat([torch.full((1,), 0x55, dtype=torch.uint8, device=cuda), _t(b.keys, cuda).reshape(-1)])
    model = {bounded: S.lookup_model(bounded)[0] for bounded in (False, True)}
    torch.cuda.synchronize()
    yield b, files, keys, model
    del files, keys
    torch.cuda.empty_cache()


def _lookup(lookups, n, bounded, with_hash):
    """hint.lookup of n requests tiled from the base set against the model's rows, tiled."""
    from gobeansdb_amd import batch, hint
    b, files, keys, model = lookups
    dev = keys.device
    idx = S.tile_index(n, S.LOOKUP_BASE, torch).to(dev)
    kb = batch.BlockBatch(keys, 1 + S.KEY_LEN * idx, torch.full((n,), S.KEY_LEN, dtype=torch.int32, device=dev))
    kh = _t(S.keyhash_fixed(b.keys).view(np.int64), dev)[idx] if with_hash else None
    got = hint.lookup(files, S.LOOKUP_CHUNKS, kb, merged=S.LOOKUP_MERGED, bounded=bounded, keyhash=kh)
    torch.cuda.synchronize()
    rows = model[bounded]
    want = _t(rows, dev)[idx]
    cols = [got.status.to(torch.int64), got.hit_file.to(torch.int64), got.chunk.to(torch.int64) & 0xFFFFFFFF,
            got.offset.to(torch.int64) & 0xFFFFFFFF, got.ver.to(torch.int64), got.vhash.to(torch.int64) & 0xFFFF,
            got.item_src]
    for c, name in enumerate(("status", "hit_file", "chunk", "offset", "ver", "vhash", "item_src")):
        bad = torch.nonzero(cols[c] != want[:, c])
        assert bad.numel() == 0, (name, int(bad[0]), int(bad.numel()))
    assert list(got.totals) == S.lookup_totals(rows, idx.cpu().numpy())


@pytest.mark.parametrize("with_hash", [False, True])
@pytest.mark.parametrize("bounded", [False, True])
def test_scale_lookup(lookups, bounded, with_hash):
    """1,056,000 requests over eight split files and their merged file: the second trip of
    k_hl_lane and, without a keyhash array, of the lookup's k_keyhash."""
    assert S.N > S.over("qlzx_hintlookup.hip", "k_hl_lane") and S.N > S.over("qlzx_hintlookup.hip", "k_keyhash")
    _lookup(lookups, S.N, bounded, with_hash)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_scale_lookup_kernel_switch(lookups, delta):
    """Around QLZX_HL_LANE_FROM, the count at which the library hands over from a wave to a lane
    per request (qlzx_hintlookup.hip), by its own choice."""
    from gobeansdb_amd import _lib
    assert _lib.HL_LANE_FROM == S.HL_LANE_FROM == S.lane_from()
    n = S.HL_LANE_FROM + delta
    assert (n >= S.HL_LANE_FROM) == (delta >= 0) and n < S.over("qlzx_hintlookup.hip", "k_hl_wave")
    _lookup(lookups, n, False, False)
    _lookup(lookups, n, True, True)


# ------------------------------------------------------------------ merge ----
@pytest.fixture(scope="module")
def merges(cuda):
    src = S.merge_sources(S.MERGE_PER)
    e = S.merge_expect(src)
    files = [_t(f, cuda) for f in src.files]
    want = _t(e.file, cuda)
    torch.cuda.synchronize()
    yield src, e, files, want
    del files, want
    torch.cuda.empty_cache()


@pytest.mark.parametrize("for_gc", [False, True])
def test_scale_merge(merges, for_gc):
    """Three sources of 400,000 items at interval 128, every item an index entry: 1,200,000 items
    and as many stretches, past the second trip of the item discovery (k_hm_count / settle / fill),
    of every plan kernel of the merge and of its k_hint_file.  The key sets overlap pairwise;
    CmpKey decides against the source order; 300 keys share one keyhash near the top of the order
    (k_hint_fix at positions beyond 700,000); source 1's index has two entries swapped, so
    k_hm_settle walks its 400,000 items with one lane, within the budget of a test.  for_gc: the
    plan alone."""
    import time
    from gobeansdb_amd import hint
    src, e, files, want = merges
    for f, k in [("qlzx_hint_walk.h", k) for k in ("k_hm_count", "k_hm_settle", "k_hm_fill")] + \
            [("qlzx_hintmerge.hip", k) for k in ("k_hm_sorted", "k_hm_cmpkey", "k_hm_hashkey", "k_hint_runs", "k_hm_cflag",
                                                 "k_hm_winners", "k_hm_emit", "k_hint_file")]:
        assert S.MERGE_ITEMS > S.over(f, k)
    assert e.items_read == S.MERGE_ITEMS > S.TWO20 and e.n_index == e.num_key > S.over("qlzx_hint_fmt.h", "k_hint_index")
    assert len(e.collisions) == 300 and (e.index_offset - 16) // S.ITEM - 300 > 700000
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = hint.merge(files, S.MERGE_CHUNKS, index_interval=128, write=not for_gc)
    torch.cuda.synchronize()
    took = time.perf_counter() - t0
    print(f"merge of {S.MERGE_ITEMS} items, one source walked by one lane: {took:.3f} s")
    assert took < 5.0, took
    assert (got.num_key, got.datasize, got.index_offset, got.n_index, got.items_read) == \
        (e.num_key, e.datasize, e.index_offset, e.n_index, e.items_read)
    assert got.collisions == e.collisions
    if for_gc:
        assert got.file.numel() == 0
    else:
        assert got.file.numel() == want.numel()
        bad = torch.nonzero(got.file != want)
        assert bad.numel() == 0, (int(bad[0]), int(bad.numel()))


# ------------------------------------------------------------------ htree ----
def _same_tree(got, files, chunks, depth, height, n_ops, n_set):
    tree, dump, _, _ = HT.build([f.tobytes() for f in files], chunks, depth, height)
    assert (got.n_ops, got.n_set, got.n_remove) == (n_ops, n_set, n_ops - n_set)
    first = tree.leaf_first()
    assert got.n_slots == first[-1] and len(got.levels) == len(tree.levels) == height
    for l, ((count, hash_), lv) in enumerate(zip(got.levels, tree.levels)):
        assert np.array_equal(count.cpu().numpy().view(np.uint32), np.array([n.count for n in lv], np.uint32)), l
        assert np.array_equal(hash_.cpu().numpy().view(np.uint16), np.array([n.hash for n in lv], np.uint16)), l
    assert got.leaf_first.cpu().numpy().view(np.uint32).tolist() == first
    assert got.file.cpu().numpy().tobytes() == dump
    return tree


@pytest.fixture(scope="module")
def sources(cuda):
    plain = S.htree_sources(S.HTREE_SOURCES, S.HTREE_KEYS)
    removes = S.htree_sources(S.HTREE_SOURCES, S.HTREE_KEYS, remove_at=40, removed=1000, set_again=500)
    early = S.htree_sources(S.HTREE_SOURCES, S.HTREE_KEYS, early=EARLY)
    host = {"plain": plain, "removes": removes, "early": early}
    dev = {k: [_t(f, cuda) for f in v] for k, v in host.items()}
    torch.cuda.synchronize()
    yield host, dev
    del dev
    torch.cuda.empty_cache()


@pytest.mark.parametrize("depth,height", [(0, 2), (1, 3)])
@pytest.mark.parametrize("variant", ["plain", "removes", "early"])
def test_scale_htree(sources, variant, depth, height):
    """65 sources of 16,500 items over the same keys, 1,072,500 ops: the second trip of k_ht_key /
    runs / slots and of k_ht_file, at L = 8 (16 leaves) and L = 7 (256 leaves).  plain: the tree of
    the last source alone.  removes: source 40 removes 1,000 keys, the later ones set 500 of them
    again: the tree of sources 39, 40 and 64.  early: source 0 alone holds 200 more keys, so ops of
    the first grid trip decide slots of the answer: the tree of sources 0 and 64."""
    from gobeansdb_amd import htree
    host, dev = sources
    assert htree.geometry(depth, height)[0] == {(0, 2): 8, (1, 3): 7}[(depth, height)]
    for k in ("k_ht_key", "k_ht_runs", "k_ht_slots", "k_ht_file"):
        assert S.HTREE_OPS > S.over("qlzx_htree.hip", k)
    remove_at = 40 if variant == "removes" else None
    m = S.htree_that_matter(S.HTREE_SOURCES, remove_at, early=variant == "early")
    n_remove = 1000 + 24 * 500 if variant == "removes" else 0
    n_ops = S.HTREE_OPS + (EARLY if variant == "early" else 0)
    got = htree.build(dev[variant], list(range(S.HTREE_SOURCES)), depth, height)
    torch.cuda.synchronize()
    tree = _same_tree(got, [host[variant][i] for i in m], m, depth, height, n_ops, n_ops - n_remove)
    assert got.n_slots == S.HTREE_KEYS + {"plain": 0, "removes": -500, "early": EARLY}[variant]
    if variant == "removes":      # not the answer without removes
        assert got.file.cpu().numpy().tobytes() != HT.build([host["plain"][-1].tobytes()], [64], depth, height)[1]
