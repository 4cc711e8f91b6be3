"""tests/hintlookup_model.py pinned by answers worked by hand from the Go text
(store/hintindex.go:28-69, store/hintfile.go:57-124, store/hint.go:270-296 and :570-596), and
checked against hint_model.get where the two must agree (no GPU)."""
import random
import struct

import pytest

import hint_model as H
import hintlookup_model as M


def _items(spec, chunk=0):
    return [H.Item(kh, key, chunk, 0, 0, 0) for kh, key in spec]


# ---- the worked example: three items, interval 128 = every item has an index entry ----
FILE3, IO3, NIDX3 = H.write_file(_items([(10, b"a"), (20, b"b"), (30, b"c")]), 0, 128)


def test_worked_example_layout():
    assert (len(FILE3), IO3, NIDX3) == (136, 88, 3)
    assert H.load_index(FILE3) == [(10, 16), (20, 40), (30, 64)]


def test_found_from_the_second_entry():
    # sort.Search = 2, j > 1: the scan starts at entry 1's offset 40, the item at 64 is the second read
    assert M.get(FILE3, 30, b"c")[:2] == (M.FOUND, 64)
    assert M.get(FILE3, 30, b"c", bounded=True)[:2] == (M.FOUND, 64)


def test_j_equal_1_starts_at_the_head():
    # sort.Search = 1: not > 1, the scan starts at 16 and passes the item at 16 first
    assert M.get(FILE3, 20, b"b")[:2] == (M.FOUND, 40)
    # the same key under hash 10 is reached only because j == 0 starts at the head too
    assert M.get(FILE3, 10, b"a")[:2] == (M.FOUND, 16)


def test_walk_into_the_index_miss():
    # j = 3, start 64.  Item at 64 (24 bytes, consumed 24).  At 88 the index entry (10, 16) reads as
    # an item: keyhash 10, chunk 16, offset 0, ver 20 (the low half of entry 1's keyhash), vhash 0,
    # ksz = byte 110 = 0: 23 bytes, consumed 47.  At 111: byte 111 is the top byte of entry 1's
    # keyhash (0), bytes 112..118 the low 7 bytes of its offset 40 = 0x28: keyhash 0x2800 > 40.
    assert struct.unpack_from("<Q", FILE3, 111)[0] == 0x2800
    assert M.get(FILE3, 40, b"d") == (M.MISS, 0, None)
    assert M.get(FILE3, 40, b"d", bounded=True) == (M.MISS, 0, None)


def test_walk_into_the_index_error():
    # as above, but 0x2800 < 2**63: the garbage item at 111 has ksz = byte 133 = 0 and is passed
    # (consumed 70, 16 + 70 < 88); at 134 two bytes are left for a 23-byte head
    assert FILE3[133] == 0
    assert M.get(FILE3, 2 ** 63, b"d") == (M.ERR, 0, None)
    assert M.get(FILE3, 2 ** 63, b"d", bounded=True) == (M.MISS, 0, None)


def test_consumed_bytes_bound_is_a_miss():
    # Two items (10, a) at 16 and (1 << 48, b) at 40, indexOffset 64, entries (10, 16) and
    # (1 << 48, 40): 96 bytes.  Wanted 2**63: j = 2, start 40.  The item at 40: consumed 24, and
    # 16 + 24 < 64.  At 64 entry 0 reads as an item: keyhash 10, ksz = byte 86 = byte 6 of entry
    # 1's keyhash = 1, so 24 bytes, which the file still has: consumed 48, 16 + 48 >= 64 ends the
    # scan at position 88 as a MISS.  By position the 8 bytes left there would have been the error.
    f, io, nidx = H.write_file(_items([(10, b"a"), (1 << 48, b"b")]), 0, 128)
    assert (io, nidx, len(f), f[86]) == (64, 2, 96, 1)
    assert M.get(f, 2 ** 63, b"z") == (M.MISS, 0, None)
    # with byte 6 of that keyhash 0 the garbage item is 23 bytes: consumed 47 at 87, and the next
    # head needs 23 of the 9 bytes left
    f, io, nidx = H.write_file(_items([(10, b"a"), (1 << 40, b"b")]), 0, 128)
    assert (io, nidx, len(f), f[86]) == (64, 2, 96, 0)
    assert M.get(f, 2 ** 63, b"z") == (M.ERR, 0, None)
    # a first item of 223 bytes: items at 16, 239, 263, 287, indexOffset 311, four entries, 375 bytes
    f, io, nidx = H.write_file(_items([(1, b"k" * 200)] + [(2 + i, b"x") for i in range(3)]), 0, 128)
    assert (io, nidx, len(f)) == (311, 4, 375)
    # wanted 2**63: j = 4, start = entry 3's offset 287.  consumed 24 at 311; two 23-byte garbage
    # items (ksz = bytes 333 and 356 = 0) reach 357, consumed 70; the third needs 23 of the 18 bytes left
    assert (f[333], f[356]) == (0, 0)
    assert M.get(f, 2 ** 63, b"z") == (M.ERR, 0, None)
    # wanted 3: j = 2, start = entry 1's offset 239; the item there is 2 < 3; at 263 keyhash 3 with
    # another key: go on; at 287 keyhash 4 > 3
    assert M.get(f, 3, b"y") == (M.MISS, 0, None)
    # one item: indexOffset 40; wanted 9: j = 1, the head; the item is 5 < 9, consumed 24, 16 + 24 >= 40
    small, io, _ = H.write_file(_items([(5, b"q")]), 0, 128)
    assert io == 40 and M.get(small, 9, b"q") == (M.MISS, 0, None)


def test_error_is_decided_before_the_compare():
    # cut the file inside the last item's key: its keyhash equals the wanted one and its head is whole,
    # but ReadFull of the key fails first
    items = _items([(10, b"a"), (20, b"bbbb")])
    f, io, _ = H.write_file(items, 0, 1 << 30)
    assert io == len(f) == 16 + 24 + 27
    cut = f[:len(f) - 2]
    cut = struct.pack("<q", len(cut)) + cut[8:]          # indexOffset = the new length: the head stays valid
    assert M.get(cut, 20, b"bb")[0] == M.ERR
    assert M.get(cut, 20, b"bb", bounded=True)[0] == M.ERR
    assert M.get(cut, 10, b"a")[:2] == (M.FOUND, 16)      # met before the damage
    assert M.get(cut, 15, b"a")[0] == M.ERR               # the item above the target is never whole


def test_go_sort_search():
    arr = [1, 3, 3, 7]
    for x, want in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 3), (7, 3), (8, 4)):
        assert M.go_sort_search(len(arr), lambda i: arr[i] >= x) == want
    # unsorted: the loop's own answer (h = 2: 1 >= 5 no, i = 3; h = 3: 9 >= 5, j = 3)
    arr = [9, 8, 1, 9]
    assert M.go_sort_search(4, lambda i: arr[i] >= 5) == 3


def test_bad_file_conditions():
    assert M.get(b"\0" * 15, 1, b"a")[0] == M.BAD_FILE
    assert M.get(None, 1, b"a")[0] == M.BAD_FILE
    for io in (15, len(FILE3) + 1, 0, -1):
        assert M.get(struct.pack("<q", io) + FILE3[8:], 10, b"a")[0] == M.BAD_FILE
    assert M.get(FILE3 + b"\0", 10, b"a")[0] == M.BAD_FILE             # (len - indexOffset) % 16
    assert M.get(struct.pack("<qII", 16, 0, 0), 10, b"a") == (M.MISS, 0, None)


def test_index_offset_outside_the_file_is_err():
    for bad in (0, len(FILE3) + 1, -1, -(2 ** 63)):
        f = bytearray(FILE3)
        struct.pack_into("<q", f, 88 + 16 + 8, bad)     # entry 1's offset: used by j == 2
        assert M.get(bytes(f), 30, b"c")[0] == M.ERR
        assert M.get(bytes(f), 30, b"c", bounded=True)[0] == M.ERR
        assert M.get(bytes(f), 20, b"b")[0] == M.FOUND  # j == 1 never reads it


def test_key_over_255_bytes_is_never_equal():
    items = _items([(10, b"k" * 255)])
    f, _, _ = H.write_file(items, 0, 4096)
    assert M.get(f, 10, b"k" * 255)[0] == M.FOUND
    assert M.get(f, 10, b"k" * 256)[0] == M.MISS
    assert M.get(f, 10, b"k" * 300, bounded=True)[0] == M.MISS


# ---- against hint_model.get, and every item by its own key ----
def _random_file(seed, n, interval):
    rng = random.Random(seed)
    hashes = sorted(rng.sample(range(1, 1 << 40), n))
    items = [H.Item(kh, bytes(rng.randrange(256) for _ in range(rng.randrange(1, 40))), 3, 256 * i, i - 5, i & 0xFFFF)
             for i, kh in enumerate(hashes)]
    # some equal-hash runs
    for i in range(5, n, 17):
        items[i].keyhash = items[i - 1].keyhash
    items.sort(key=lambda it: (it.keyhash, it.key))
    return items, H.write_file(items, 0, interval)[0]


@pytest.mark.parametrize("interval", [128, 300, 4096])
def test_bounded_equals_hint_model_get(interval):
    items, f = _random_file(interval, 400, interval)
    index = H.load_index(f)
    rng = random.Random(1)
    wanted = [(it.keyhash, it.key) for it in items]
    wanted += [(it.keyhash, it.key + b"x") for it in items[::7]]
    wanted += [(rng.randrange(1 << 41), b"absent") for _ in range(200)] + [(0, b""), (2 ** 64 - 1, b"z")]
    for kh, key in wanted:
        ref = H.get(f, index, kh, key)
        st, at, it = M.get(f, kh, key, bounded=True)
        assert (st == M.FOUND) == (ref is not None)
        assert st in (M.FOUND, M.MISS)
        if ref is not None:
            assert it == ref and f[at + 23:at + 23 + len(key)] == key


@pytest.mark.parametrize("interval", [128, 300, 4096])
@pytest.mark.parametrize("bounded", [False, True])
def test_every_item_is_found_by_its_own_key(interval, bounded):
    """store/hint_test.go:81: every item written is returned by get."""
    items, f = _random_file(7 + interval, 300, interval)
    for it in items:
        st, at, got = M.get(f, it.keyhash, it.key, bounded)
        assert st == M.FOUND and got == it


# ---- hintMgr.getItem's order ----
def _file(spec, chunk, interval=4096):
    return H.write_file([H.Item(kh, key, chunk, off, 1, 2) for kh, key, off in spec], 0, interval)[0]


def test_get_item_order_and_chunk_ids():
    f0 = _file([(10, b"a", 0x300)], 7)
    f1 = _file([(10, b"a", 0x200), (20, b"b", 0x500)], 7)
    mg = _file([(10, b"a", 0x100), (20, b"b", 0x400), (30, b"c", 0x600)], 5)    # items store chunk 5
    old = _file([(40, b"d", 0x700)], 1)
    files, offs, chunks = [f0, f1, mg, old], [0, 1000, 2000, 3000], [9, 8, 0, 1]
    r = M.get_item(files, offs, chunks, 2, 10, b"a")
    assert r.astuple() == (M.FOUND, 0, 9, 0x300, 1, 2, 16)                       # the first file wins
    r = M.get_item(files, offs, chunks, 2, 20, b"b")
    assert r.astuple() == (M.FOUND, 1, 8, 0x500, 1, 2, 1000 + 40)                # a split: file_chunk
    r = M.get_item(files, offs, chunks, 2, 30, b"c")
    assert r.astuple() == (M.FOUND, 2, 5, 0x600, 1, 2, 2000 + 64)                # merged: the stored chunk
    r = M.get_item(files, offs, chunks, 2, 40, b"d")
    assert r.astuple() == (M.MISS, 2, 0, 0, 0, 0, 0)                             # nothing after the merged file
    assert M.get_item(files, offs, chunks, None, 40, b"d").astuple()[:3] == (M.FOUND, 3, 1)
    assert M.get_item([], [], [], None, 40, b"d").astuple() == (M.MISS, 0, 0, 0, 0, 0, 0)


def test_an_error_ends_the_search():
    f0 = FILE3                                                  # 2**63 ends in ERR here
    f1 = _file([(2 ** 63, b"d", 0x900)], 0)
    r = M.get_item([f0, f1], [0, 136], [4, 3], None, 2 ** 63, b"d")
    assert r.astuple() == (M.ERR, 0, 0, 0, 0, 0, 0)
    r = M.get_item([f0, f1], [0, 136], [4, 3], None, 2 ** 63, b"d", bounded=True)
    assert r.astuple() == (M.FOUND, 1, 3, 0x900, 1, 2, 136 + 16)
    out, totals = M.lookup([f0, f1], [0, 136], [4, 3], None, [b"d", b"c"], [2 ** 63, 30])
    assert [o.status for o in out] == [M.ERR, M.FOUND] and totals == [1, 0, 1, 0]
