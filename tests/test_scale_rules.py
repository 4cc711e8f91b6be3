"""The rules of tests/scale.py, by which tests/test_gpu_scale_records.py and test_gpu_scale_hints.py
derive what the kernels owe for a million items from the models' answers on small base sets,
checked here against the models themselves at a small count (no GPU); and the census of the
capped launches."""
import re
from pathlib import Path

import numpy as np

import hint_model as H
import htree_model as HT
import scale as S

TESTS = Path(__file__).resolve().parent


# ------------------------------------------------------------------ the census ----
def test_census_every_capped_launch_stands_in_the_table():
    """Every launch of csrc whose grid is a grid_for( call or a fixed dim3(2048) / dim3(1024) is a
    key of scale.LAUNCHES with its items per workgroup and its cap as they stand in the source, so
    a changed cap cannot leave its loop's second trip untested in silence; the table names nothing
    that the sources no longer launch."""
    found = S.launches()
    assert len(found) > 50 and len(set(found)) == len(found)
    missing = [tuple(l) for l in found if l not in S.LAUNCHES]
    assert not missing, missing
    stale = [tuple(l) for l in S.LAUNCHES if l not in found]
    assert not stale, stale
    files = {l.file for l in found}
    assert files >= {"qlzx_write.hip", "qlzx_read.hip", "qlzx_gc.hip", "qlzx_replay.hip", "qlzx_hint.hip",
                     "qlzx_hintmerge.hip", "qlzx_hintlookup.hip", "qlzx_htree.hip", "qlzx_hint_fmt.h", "qlzx_hint_walk.h"}
    assert S.scan_tile() ** 2 == S.SCAN_TOP.over
    assert S.lane_from() == S.HL_LANE_FROM < S.over("qlzx_hintlookup.hip", "k_hl_wave")
    assert S.DSTOFF.count > S.DSTOFF.over


def test_census_rows_name_a_test_and_a_count_above_the_cap():
    """A covered row's count exceeds what it takes for a second trip, which is at least a full
    grid of items (a grid item may stand for several of the call's), and its test exists."""
    for l, row in S.LAUNCHES.items():
        if row.test is S.NOT_COVERED:
            continue
        module, name = row.test.split("::")
        assert re.search(rf"^def {name}\(", (TESTS / module).read_text(), re.M), row.test
        assert row.count > row.over, (tuple(l), row)
        if l.per and row.unit in ("record", "request", "key", "item", "op"):
            assert row.over == l.per * l.most, (tuple(l), row)
    assert S.SCAN_TOP.count > S.SCAN_TOP.over
    # what no scale test crosses, by name (DESIGN.md §6 gives the reasons): the list cannot grow unseen
    open_rows = sorted((l.file, l.kernel) for l, row in S.LAUNCHES.items() if row.test is S.NOT_COVERED)
    assert open_rows == sorted(
        [("qlzx_hint.hip", "k_hint_fix"), ("qlzx_hintmerge.hip", "k_hint_fix"), ("qlzx_hintlookup.hip", "k_hl_head"),
         ("qlzx_hintlookup.hip", "k_hl_wave"), ("qlzx_hint_walk.h", "k_hm_head"), ("qlzx_htree.hip", "k_ht_leaves"),
         ("qlzx_htree.hip", "k_ht_level")])


def test_census_parser_reads_every_launch_form(tmp_path):
    """The forms the sources use: a direct call, a variable, a dim3 constructed from a call, several
    bindings on a line, std::max around the call, a fixed grid, a parenthesised template kernel."""
    (tmp_path / "a.hip").write_text("""
        inline uint32_t grid_for(uint64_t n, uint32_t per = 256, uint32_t most = 4096) { return 0; }
        const uint32_t grid = grid_for(cap);   // grid_for(n, 1, 1) in a comment
        hipLaunchKernelGGL(k_one, dim3(grid), dim3(256), 0, s, a);
        const dim3 B(256), GF(grid_for(nf, 256, 2048)), GS(grid_for((uint64_t)c + nf, 128, 512));
        hipLaunchKernelGGL(k_two<P>, GF, B, 0, s, a);
        hipLaunchKernelGGL((k_three<F, G>), GS, B, 0, s, a,
                           b);
        hipLaunchKernelGGL(k_four, dim3(std::max(grid_for(x / 16 + 1, 256, 2048), 1u)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_five<W>, dim3(2048), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_six, dim3(1), dim3(1024), 0, s, a);
        hipLaunchKernelGGL(qlzx::k_seven, dim3(qlzx::grid_for(n, 4, 8192)), dim3(256), 0, s, a);
    """)
    (tmp_path / "qlzx_recfile.h").write_text("constexpr uint32_t kScanTile = 512;\n")
    assert [tuple(l)[1:] for l in S.launches(tmp_path)] == [
        ("k_one", 256, 4096), ("k_two", 256, 2048), ("k_three", 128, 512), ("k_four", 256, 2048), ("k_five", 0, 2048),
        ("k_seven", 4, 8192)]
    assert S.scan_tile(tmp_path) == 512


# ------------------------------------------------------------------ tiling ----
def test_tile_index_is_a_rotation_per_repetition():
    idx = S.tile_index(3 * 50 + 7, 50)
    for r in range(3):
        assert sorted(idx[50 * r:50 * r + 50].tolist()) == list(range(50))
    assert idx[:3].tolist() == [0, 1, 2] and idx[50:53].tolist() == [31, 32, 33] and idx[150] == (31 * 3) % 50
    import torch
    assert torch.equal(S.tile_index(157, 50, torch), torch.from_numpy(idx))


# ------------------------------------------------------------------ writes ----
def test_write_block_holds_what_it_claims():
    rows, bound = S.write_block_rows()
    keys, vals, flags, vers, ts = S.write_block()
    slots = [len(r[1]) // 256 for r in rows]
    kept = [j for j, r in enumerate(rows) if r[6] and r[2] & S.FC]
    refused = [j for j, r in enumerate(rows) if r[6] and not r[2] & S.FC]
    assert len(kept) == 8 and all(232 <= len(vals[j]) <= 300 and slots[j] == 1 for j in kept)
    assert {len(vals[j]) for j in kept} >= {232, 300}
    assert len(refused) == 4 and all(slots[j] == 2 for j in refused)
    assert sum(r[0] == 1 for r in rows) == 1 and sum(slots) == 73
    untried_two_slot = [j for j, r in enumerate(rows) if not r[6] and slots[j] == 2]
    assert sum(vers[j] < 0 for j in untried_two_slot) == 2 and sum(flags[j] == S.FCC for j in untried_two_slot) == 3
    assert sum(vals[j].startswith(b"ID3") for j in untried_two_slot) == 1 and len(untried_two_slot) == 6
    assert any(len(v) == 0 for v in vals)
    assert 290e6 < 73 * 256 * (S.N // 64) < 320e6


def test_write_rule_against_the_full_expectation():
    """Three repetitions of the block through test_gpu_write_batch._expect, the write tests' own
    restatement of the set path over the whole input."""
    from test_gpu_write_batch import _expect
    keys, vals, flags, vers, ts = (x * 3 for x in S.write_block())
    rows, data, bound = _expect(keys, vals, flags, vers, ts)
    e = S.write_expect(3)
    assert e.block * 3 == data and e.nbytes == len(data) and e.bound == bound
    assert e.status.tolist() == [r[0] for r in rows] and e.offset.tolist() == [r[1] for r in rows]
    assert e.flag.tolist() == [r[3] for r in rows] and e.vsz.tolist() == [r[4] for r in rows]
    assert e.crc.tolist() == [r[5] for r in rows] and e.vhash.tolist() == [r[6] for r in rows]
    assert e.tried.tolist() == [i for i, r in enumerate(rows) if r[7]]
    assert e.written == sum(r[0] == 0 for r in rows)
    assert e.counts == (e.written, len(e.tried), sum(r[7] and bool(r[3] & S.FC) for r in rows), 0)


# ------------------------------------------------------------------ reads ----
def _read_rows():
    from test_gpu_read_batch import _expect
    b = S.read_base()
    return [_expect(b.data, int(o)) for o in b.offsets]


def test_read_base_holds_what_it_claims():
    b, rows = S.read_base(), _read_rows()
    assert {r[0] for r in rows} == set(range(7))
    for st in range(1, 7):
        # EOF_HEADER twice: inside the last 24 bytes, and past the end
        assert sum(r[0] == st for r in rows) == (2 if st == S.RD_EOF_HEADER else 1)
    ok = [r for r in rows if r[0] == S.RD_OK]
    assert any(r[1][2] & S.FC and r[5] for r in ok) and any(not r[1][2] & S.FC for r in ok)
    assert sum(not r[5] for r in ok) == 1 and any(r[3] == b"" for r in ok)
    assert len(b.data) < (1 << 16)


def test_read_rule_against_the_oracle_over_the_tiled_requests():
    """Three repetitions and a ragged tail: every column of every request is what the oracle says of
    that request; the planned requests' destinations are the running sum of their rounded sizes."""
    from test_gpu_read_batch import _expect
    b, rows = S.read_base(), _read_rows()
    n = 3 * S.READ_BASE + 77
    e = S.read_expect(n, rows, with_keys=True)
    idx = S.tile_index(n, S.READ_BASE)
    dst, nok, ncomp, mx = 0, 0, 0, 0
    for i in range(n):
        off = int(b.offsets[idx[i]])
        st, hdr, flag, val, vh, dec_ok = _expect(b.data, off)
        assert (e.status[i], tuple(e.header[i]), e.flag[i], e.vhash[i], bool(e.dec_ok[i])) == (st, hdr, flag, vh, dec_ok), i
        assert e.value_len[i] == (len(val) if val is not None else 0)
        assert e.key_eq[i] == (st == S.RD_OK and b.wanted[idx[i]] == b.data[off + 24:off + 24 + hdr[4]])
        nok += st == S.RD_OK
        if st == S.RD_OK and hdr[2] & S.FC:
            body = b.data[off + 24 + hdr[4]:off + 24 + hdr[4] + hdr[5]]
            d = S.qlz_dsize(body)
            assert not dec_ok or d == len(val)
            assert (e.in_out[i], e.val_off[i]) == ((1, dst) if dec_ok else (0, off + 24 + hdr[4]))
            dst, ncomp, mx = dst + S.pad256(d), ncomp + 1, max(mx, d)
        else:
            assert (e.in_out[i], e.val_off[i]) == (0, off + 24 + hdr[4] if st == S.RD_OK else 0)
    assert e.totals == (nok, ncomp, mx, dst)
    assert S.read_expect(n, rows, with_keys=False).key_eq is None


# ------------------------------------------------------------------ gc ----
def test_gc_restatement_against_the_oracle():
    """30 blocks (1,920 records, 487 KiB), data_file_max 64 KiB: five rotations, six destination chunks.
    The chunks' bytes and every kept record's position against oracle/gc.py; then max_chunks and
    out_cap, which the oracle does not have, against the ABI's words: the placed records are a
    prefix of the unbounded answer, the rest NO_CHUNK; a record past out_cap keeps its planned
    position and nothing else changes."""
    import datafile_cases as D
    from oracle import gc as G
    M = D.million_slots(30)
    data = M.data.tobytes()
    dfm = 64 << 10
    shape = S.gc_shape(M, dfm)
    assert shape.keep[:64].all() and shape.keep[-64:].sum() == 1 and shape.keep[64 * shape.named[1]:][:64].sum() == 1
    crc_block = np.array([int.from_bytes(M.block[o:o + 4], "little") for o in M.block_off.tolist()], np.uint32)
    chunks, pos = G.gc_rewrite(data, shape.keep.tolist(), dfm, shape.dst_head, shape.next_heads)
    e = S.gc_expect(M, crc_block, shape, dfm)
    assert len(chunks) == len(e.chunk_bytes) == 6 and len(e.rotations) == len(chunks) - 1
    assert [len(c) for c in chunks] == e.chunk_bytes.tolist()
    w = e.status == S.GC_WRITTEN
    assert (w == shape.keep).all() and list(zip(e.new_chunk[w].tolist(), e.new_off[w].tolist())) == [tuple(p) for p in pos]
    out = np.full((int(e.chunk_bytes.sum()) // 256 + 1, 256), 0xEE, np.uint8)
    out[e.dst_slot] = M.data.reshape(-1, 256)[e.src_slot]
    assert out[:-1].tobytes() == b"".join(chunks) and (out[-1] == 0xEE).all()
    assert e.totals == [M.nrec, int(shape.keep.sum()), len(pos), len(chunks), len(b"".join(chunks)), 0, 0, 0]
    assert e.crc[w].tolist() == [int.from_bytes(data[o:o + 4], "little") for o in M.offsets[w].tolist()]
    # max_chunks 3: everything from the third rotation on is NO_CHUNK
    m = S.gc_expect(M, crc_block, shape, dfm, max_chunks=3)
    cut = e.rotations[2]
    assert (m.status[:cut] == e.status[:cut]).all() and set(m.status[cut:].tolist()) == {S.GC_DROPPED, S.GC_NO_CHUNK}
    assert (m.new_off[:cut] == e.new_off[:cut]).all() and not m.new_off[cut:].any() and not m.crc[cut:].any()
    assert m.chunk_bytes.tolist() == e.chunk_bytes[:3].tolist() and m.totals[2:4] == [int((m.status == 0).sum()), 3]
    assert m.totals[7] == int((m.status == S.GC_NO_CHUNK).sum()) > 0
    # out_cap one record short
    total = int(e.chunk_bytes.sum())
    o = S.gc_expect(M, crc_block, shape, dfm, out_cap=total - 256)
    last = int(np.nonzero(shape.keep)[0][-1])
    assert o.status[last] == S.GC_NO_SPACE and (np.delete(o.status, last) == np.delete(e.status, last)).all()
    assert (o.new_off == e.new_off).all() and (o.new_chunk == e.new_chunk).all() and o.crc[last] == 0
    assert o.chunk_bytes.tolist() == e.chunk_bytes.tolist() and o.totals == [M.nrec, e.totals[1], e.totals[2] - 1,
                                                                             e.totals[3], total - 256, 0, 0, 1]
    assert len(o.dst_slot) == len(e.dst_slot) - 1


def test_gc_shape_at_the_full_count_rotates_behind_record_2_20():
    import datafile_cases as D
    _, boff, brs = D.million_block()
    reps = D.MILLION_REPS
    M = D.Million(None, None, boff, reps, (np.arange(reps, dtype=np.int64)[:, None] * 65 * 256 + boff[None, :]).ravel(),
                  np.tile(brs, reps), 65 * reps, 64 * reps)
    shape = S.gc_shape(M)
    e = S.gc_expect(M, np.zeros(64, np.uint32), shape)
    assert len(e.rotations) >= 5 and e.rotations[-1] > S.TWO20 and 64 * shape.named[1] > S.TWO20
    assert e.rotations[len(e.rotations) // 2] > S.N // 4


# ------------------------------------------------------------------ hint build ----
def test_vector_hashes_against_the_model():
    k = S.fixed_keys(np.arange(0, 3000, 7))
    assert (k >= 0x80).any(axis=1).sum() == len(k[::3])
    assert S.keyhash_fixed(k).tolist() == [H.keyhash(r.tobytes()) for r in k]
    for L in (1, 4, 7, 8):     # every tail length of murmur3
        assert S.murmur3_fixed(k[:, :L]).tolist() == [H.murmur3_32(r[:L].tobytes()) for r in k]


def _same_splits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g.consumed, g.num_key, g.datasize, g.n_index, g.index_offset, g.skipped) == \
            (w.consumed, w.num_key, w.datasize, w.n_index, w.index_offset, w.skipped)
        assert g.file.tobytes() == w.file


def test_hint_build_restatement_against_the_model():
    """20,000 records, split_cap 1,000 (twenty cuts), 300 keys written twice, some of them across a
    cut; at the default interval, at 128 (every item an index entry) and at one between."""
    r = S.hint_records(20000, 300, period=16, back=5)
    recs = S.model_records(r)
    assert len({x[1] for x in recs}) == 20000 - 300
    for interval in (4096, 128, 700):
        want = H.build(recs, split_cap=1000, index_interval=interval, chunk_id=3, max_offset=77)
        assert len(want) == 20 and sum(w.consumed for w in want) == 20000
        _same_splits(S.hint_build_fixed(r, 1000, interval, chunk_id=3, max_offset=77), want)
        assert (interval != 128) or all(w.n_index == w.num_key for w in want)
    assert sum(w.consumed > 1000 for w in want) >= 4           # a split took both records of some key
    tied = r._replace(kh=r.kh // np.uint64(1 << 40))             # a caller's keyhashes, many keys on each
    want = H.build(S.model_records(tied), split_cap=1000, index_interval=128)
    _same_splits(S.hint_build_fixed(tied, 1000, 128), want)


# ------------------------------------------------------------------ merge ----
def test_merge_restatement_against_the_model():
    """Three sources of 4,000 items at interval 128 and at the default, through hintmerge_model's
    heap loop: the file, the totals and the collision items; the for_gc plan gives the same figures
    and no file.  The sources hold what they claim."""
    import hintmerge_model as HM
    src = S.merge_sources(4000)
    raw = [f.tobytes() for f in src.files]
    assert all(HM.is_strictly_ascending(f) for f in raw)
    a, b, c = (set(x.tolist()) for x in src.ids)
    assert len(a & b) == 1500 and len(b & c) == 1000 and len(c & a) == 500 and not a & b & c
    index = H.load_index(raw[1])
    assert [o for _, o in index] != sorted(o for _, o in index) and len(index) == 4000       # the swapped entries
    assert [o for _, o in H.load_index(raw[0])] == sorted(o for _, o in H.load_index(raw[0]))
    for interval in (128, 4096):
        e = S.merge_expect(src, interval)
        for for_gc in (False, True):
            m = HM.merge(raw, S.MERGE_CHUNKS, interval, for_gc=for_gc)
            assert (m.num_key, m.datasize, m.index_offset, m.n_index, m.items_read) == \
                (e.num_key, e.datasize, e.index_offset, e.n_index, e.items_read)
            assert m.collisions == e.collisions and m.file == (b"" if for_gc else e.file.tobytes())
    assert e.num_key == len(a | b | c) == 9000 and e.items_read == 12000
    assert len(e.collisions) == 300 and {x[0] for x in e.collisions} == {S.MERGE_SHARED_HASH}
    assert {x[2] for x in e.collisions} == {5, 9}
    # CmpKey decides, not the source order: source 1 (chunk 9) wins over source 2; between 0 and 2 the offset
    items = {it.key: it for it in H.read_items(e.file.tobytes())}
    won = [items[S.fixed_keys(np.array([i]))[0].tobytes()].chunk_id for i in sorted(b & c)]
    assert set(won) == {9}
    i0, i2 = src.items[0], src.items[2]
    off0 = dict(zip(i0["ids"].tolist(), i0["off"].tolist()))
    off2 = dict(zip(i2["ids"].tolist(), i2["off"].tolist()))
    both = sorted(c & a)
    assert 50 < sum(off0[i] > off2[i] for i in both) < len(both) - 50
    for i in both:
        assert items[S.fixed_keys(np.array([i]))[0].tobytes()].offset == max(off0[i], off2[i])


# ------------------------------------------------------------------ lookup ----
def test_lookup_base_and_tiling_against_the_model():
    """The base set holds what it claims; three repetitions and a ragged tail through the model
    over the whole tiled request list give the base rows tiled (the reference as it is)."""
    import hintlookup_model as HL
    b = S.lookup_base()
    rows, totals = S.lookup_model(False)
    assert set(rows[rows[:, 0] == HL.FOUND, 1].tolist()) == set(range(9))          # hits in every file
    assert totals[2] >= 5 and totals[1] >= 250 and totals[3] == 0                   # the reader's error; misses
    brows, btotals = S.lookup_model(True)
    assert btotals[2] == 0 and btotals[0] > totals[0]                              # bounded: on to the next file
    for f, file in enumerate(b.files):      # every index entry's item is asked for
        named = {file[o:o + S.ITEM].tobytes()[23:] for _, o in H.load_index(file.tobytes())}
        assert named <= {k.tobytes() for k in b.keys}
    n = 3 * S.LOOKUP_BASE + 5
    idx = S.tile_index(n, S.LOOKUP_BASE)
    lens = [len(f) for f in b.files]
    offs = [sum(lens[:i]) for i in range(9)]
    want, wtotals = HL.lookup([f.tobytes() for f in b.files], offs, S.LOOKUP_CHUNKS, S.LOOKUP_MERGED,
                              [b.keys[i].tobytes() for i in idx], None, False)
    assert [r.astuple() for r in want] == [tuple(r) for r in rows[idx].tolist()]
    assert wtotals == S.lookup_totals(rows, idx)


# ------------------------------------------------------------------ htree ----
def _tree_answer(files, chunks, depth, height):
    tree, dump, nset, nrem = HT.build([f.tobytes() for f in files], chunks, depth, height)
    return [[(n.count, n.hash) for n in lv] for lv in tree.levels], tree.leaf_first(), dump


def test_htree_rule_the_last_source_alone():
    files = S.htree_sources(5, 3000)
    assert [it.key for it in H.read_items(files[0].tobytes())] == [it.key for it in H.read_items(files[4].tobytes())]
    assert files[0].tobytes() != files[4].tobytes()
    for depth, height in ((0, 2), (1, 3)):
        m = S.htree_that_matter(5)
        assert _tree_answer(files, list(range(5)), depth, height) == _tree_answer([files[i] for i in m], m, depth, height)


def test_htree_rule_with_removes():
    """Source 2 of 6 removes 400 keys, the later ones set 150 of them again: the tree of all six is
    the tree of sources 1, 2 and 5, and not the tree without removes."""
    files = S.htree_sources(6, 3000, remove_at=2, removed=400, set_again=150)
    vers = lambda f: [it.ver for it in H.read_items(f.tobytes())]     # noqa: E731
    assert [sum(v < 0 for v in vers(f)) for f in files] == [0, 0, 400, 250, 250, 250]
    for depth, height in ((0, 2), (1, 3)):
        m = S.htree_that_matter(6, remove_at=2)
        assert m == [1, 2, 5]
        full = _tree_answer(files, list(range(6)), depth, height)
        assert full == _tree_answer([files[i] for i in m], m, depth, height)
        plain = S.htree_sources(6, 3000)
        assert full != _tree_answer(plain[5:], [5], depth, height)
        assert full[1][-1] == 3000 - 250


def test_htree_rule_with_keys_of_the_first_source_alone():
    """Source 0 of 5 holds 200 keys that no later source has: the tree of all five is the tree of
    sources 0 and 4, holds those keys as source 0 set them, and is not the last source's alone."""
    files = S.htree_sources(5, 3000, early=200)
    assert [len(H.read_items(f.tobytes())) for f in files] == [3200, 3000, 3000, 3000, 3000]
    for depth, height in ((0, 2), (1, 3)):
        m = S.htree_that_matter(5, early=True)
        assert m == [0, 4]
        full = _tree_answer(files, list(range(5)), depth, height)
        assert full == _tree_answer([files[i] for i in m], m, depth, height)
        assert full != _tree_answer(files[4:], [4], depth, height) and full[1][-1] == 3200
