"""tests/hintmerge_model.py pinned without the compiled reference (no GPU): the reference's own
merge test as a property, one worked merge against hand-written bytes, the sorted-sources rule the
library implements, and checkIndex's property over the merged file."""
import random
import struct

import pytest

import hint_model as H
import hintmerge_model as M


def _sorted_items(n: int):
    """genSortedHintItems (store/hint_test.go:91-107)."""
    return [H.Item(i, b"key_%05d" % i, 0, 3 * i * 256, 3 * i + 1, (3 * i + 2) & 0xFFFF) for i in range(n)]


@pytest.mark.parametrize("nsrc", [2, 3])
@pytest.mark.parametrize("seed", range(8))
def test_reference_merge_test_as_a_property(nsrc, seed):
    """testMerge (store/hint_test.go:109-155): each item goes to one source as a copy with Offset - 1
    followed by the item.  Item 0's copy wraps to 0xffffffff, a larger CmpKey, and the item read
    after it still wins: mergeWriter overwrites a run of equal keys in the order they pop."""
    rnd = random.Random(100 * nsrc + seed)
    items = _sorted_items(10)
    where = [rnd.randrange(nsrc) for _ in items]
    where[:nsrc] = range(nsrc)                   # no source stays empty (the reference would dereference nil)
    src = [[] for _ in range(nsrc)]
    for it, w in zip(items, where):
        src[w].append(H.Item(it.keyhash, it.key, 0, (it.offset - 1) & 0xFFFFFFFF, it.ver, it.vhash))
        src[w].append(it)
    assert src[0][0].offset == 0xFFFFFFFF
    files = [H.write_file(s, 0, 4096)[0] for s in src]
    got = M.merge(files, [0] * nsrc)
    assert H.read_items(got.file) == items       # readHintAndCheck
    assert got.collisions == [] and got.num_key == 10 and got.items_read == 20
    assert not any(M.is_strictly_ascending(f) for f in files)


def test_worked_merge_byte_for_byte():
    """Two sources, three keys, one of them in both; index_interval 128 makes every item an entry."""
    a = [H.Item(1, b"a", 9, 0x100, 1, 0x1111), H.Item(2, b"bb", 9, 0x200, -2, 0x2222)]
    b = [H.Item(2, b"bb", 9, 0x100, 3, 0x3333), H.Item(2, b"c", 9, 0x300, 4, 0x4444)]
    fa, fb = H.write_file(a, 0x500, 4096)[0], H.write_file(b, 0x700, 4096)[0]
    got = M.merge([fa, fb], [0, 1], index_interval=128)       # chunk 1 beats chunk 0 for "bb"

    def item(kh, chunk, off, ver, vhash, key):
        return struct.pack("<QIIiHB", kh, chunk, off, ver, vhash, len(key)) + key

    body = item(1, 0, 0x100, 1, 0x1111, b"a") + item(2, 1, 0x100, 3, 0x3333, b"bb") + item(2, 1, 0x300, 4, 0x4444, b"c")
    assert len(body) == 24 + 25 + 24
    index = struct.pack("<Qq", 1, 16) + struct.pack("<Qq", 2, 40) + struct.pack("<Qq", 2, 65)
    want = struct.pack("<qII", 16 + 73, 3, 0x700) + body + index
    assert got.file == want
    assert (got.num_key, got.datasize, got.index_offset, got.n_index, got.items_read) == (3, 0x700, 89, 3, 4)
    assert got.collisions == [(2, b"bb", 1, 0x100, 3, 0x3333), (2, b"c", 1, 0x300, 4, 0x4444)]
    assert set(got.table.items) == {2} and set(got.table.items[2]) == {b"bb", b"c"}
    # forGC: the same collisions, no file
    gc = M.merge([fa, fb], [0, 1], index_interval=128, for_gc=True)
    assert gc.file == b"" and gc.collisions == got.collisions
    # the lower chunk loses whatever its offset
    assert M.merge([fa, fb], [1, 0]).collisions[0] == (2, b"bb", 1, 0x200, -2, 0x2222)


def _random_sources(rnd, nsrc, forced):
    names = [bytes(rnd.getrandbits(8) for _ in range(rnd.randint(0, 12))) for _ in range(40)]
    names = list(dict.fromkeys(names + [k[:len(k) // 2] for k in names[:10]]))
    hashes = {k: (rnd.randrange(4) if forced else H.keyhash(k)) for k in names}
    files = []
    for _ in range(nsrc):
        mine = rnd.sample(names, rnd.randint(1, len(names)))
        items = sorted((H.Item(hashes[k], k, 7, rnd.choice((0, 256, 1 << 31, 0xFFFFFF00)), rnd.randint(-3, 9),
                               rnd.getrandbits(16)) for k in mine), key=lambda it: (it.keyhash, it.key))
        files.append(H.write_file(items, rnd.getrandbits(32), rnd.choice((128, 300, 4096)))[0])
    return files


@pytest.mark.parametrize("forced", [False, True])
def test_sorted_sources_equal_sort_and_keep_last(forced):
    rnd = random.Random(5 + forced)
    for _ in range(40):
        nsrc = rnd.randint(1, 6)
        files = _random_sources(rnd, nsrc, forced)
        chunks = [rnd.randrange(3) for _ in range(nsrc)]
        assert all(M.is_strictly_ascending(f) for f in files)
        got = M.merge(files, chunks, index_interval=rnd.choice((128, 303, 4096)))
        want = M.merged_by_sort(files, chunks)
        assert H.read_items(got.file) == want
        assert got.datasize == max(H.read_head(f)[2] for f in files)
        by_hash = {}
        for it in want:
            by_hash.setdefault(it.keyhash, []).append(it)
        assert got.collisions == [M.as_tuple(it) for it in want if len(by_hash[it.keyhash]) > 1]
        assert got.collisions or not forced


def test_every_source_key_is_found_through_the_merged_index():
    """checkIndex (store/hint_test.go:79-89)."""
    rnd = random.Random(11)
    files = _random_sources(rnd, 4, False) + _random_sources(rnd, 2, True)
    chunks = [0, 1, 2, 3, 4, 5]
    got = M.merge(files, chunks, index_interval=300)
    index = H.load_index(got.file)
    assert len(index) == got.n_index > 1
    newest = {(it.keyhash, it.key): it for it in M.merged_by_sort(files, chunks)}
    for f in files:
        for it in H.read_items(f):
            assert H.get(got.file, index, it.keyhash, it.key) == newest[(it.keyhash, it.key)]


def test_bad_sources():
    good = H.write_file(_sorted_items(3), 0, 4096)[0]
    for bad in (good[:15], struct.pack("<qII", len(good) + 1, 3, 0) + good[16:], good[:16],
                struct.pack("<qII", 0, 3, 0) + good[16:60]):
        with pytest.raises(M.BadFile) as e:
            M.merge([good, bad], [0, 1])
        assert e.value.source == 1
    # indexOffset 0: the items run to the file's end
    io = H.read_head(good)[0]
    noindex = struct.pack("<qII", 0, 3, 0) + good[16:io]
    assert M.merge([noindex], [0]).file == M.merge([good], [0]).file
