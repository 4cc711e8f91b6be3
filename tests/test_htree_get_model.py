"""tests/htree_get_model.py pinned by hand-worked answers (no GPU)."""
import struct

import pytest

import hint_model as H
import htree_get_model as G
import htree_model as M

A, B = 0x1000000200000001, 0x1000000500000002


def _three_sources():
    """The worked case of test_a_slot_set_removed_and_set_again: B rewritten in place, A removed
    and set again behind it.  Depth 0, height 2: L = 8, items of 19 bytes, 16 leaves."""
    it = lambda kh, ver, vhash=0, off=0: H.Item(kh, b"k", 0, off, ver, vhash)
    files = [H.write_file([it(A, 1, 3, 0x300), it(B, 2, 7, 0x100)], 0, 4096)[0],
             H.write_file([it(A, -1), it(B, 3, 10, 0x200)], 0, 4096)[0],
             H.write_file([it(A, 5, 1, 0x400)], 0, 4096)[0]]
    return M.build(files, [0, 1, 2], 0, 2)[1]


def test_get_of_a_and_b_from_the_198_byte_file():
    file = _three_sources()
    assert len(file) == 198
    tree = G.load(file, 0, 2)
    assert tree.dump() == file
    assert tree.leaf_first() == [0, 0] + [2] * 15                     # both in leaf 1
    assert (tree.levels[1][1].count, tree.levels[1][1].hash) == (2, 52)
    #                    found    chunk offset ver vhash slot
    assert G.get(tree, B) == (G.FOUND, 1, 0x200, 3, 10, 0)
    assert G.get(tree, A) == (G.FOUND, 2, 0x400, 5, 1, 1)
    assert G.get(tree, A ^ 1) == (G.MISS, 0, 0, 0, 0, G.NO_SLOT)       # another low byte
    assert G.get(tree, A ^ (1 << 56)) == (G.MISS, 0, 0, 0, 0, G.NO_SLOT)   # L = 8: byte 7 is compared
    assert G.get(tree, B ^ (3 << 60)) == (G.MISS, 0, 0, 0, 0, G.NO_SLOT)   # another (empty) leaf


def test_the_file_after_moving_b():
    file = _three_sources()
    tree = G.load(file, 0, 2)
    assert G.update_pos(tree, B, 7, 0x12345600)
    assert not G.update_pos(tree, B ^ 2, 7, 0x100)
    after = tree.dump()
    # B's item starts at 96 + 4 * 2 = 104: eight key bytes, ver, vhash, then the five position bytes
    assert after[:118] == file[:118] and after[123:] == file[123:]
    assert after[118:123] == bytes.fromhex("563412" "0700")
    assert after[6:12] == bytes.fromhex("020000003400")               # the leaf node: count 2, hash 52
    assert G.get(tree, B) == (G.FOUND, 7, 0x12345600, 3, 10, 0)
    assert G.get(tree, A) == (G.FOUND, 2, 0x400, 5, 1, 1)


def test_the_bucket_nibbles_take_no_part():
    # depth 1, height 3: L = 7, the leaf is nibbles 1 and 2, the stored bytes the low seven
    tree = M.HTree(1, 3)
    kh = 0x0AB0000700000009
    tree.set(kh, 4, 9, 3, 0x500)
    assert G.leaf_of(tree, kh) == 0xAB
    for alias in (kh, kh | (0x7 << 60), kh | (0xF << 60)):
        assert G.get(tree, alias) == (G.FOUND, 3, 0x500, 4, 9, 0)
    assert G.get(tree, kh ^ (1 << 48))[0] == G.MISS                    # byte L - 1 = 6 differs
    assert G.get(tree, kh ^ (1 << 52))[0] == G.MISS                    # leaf 0xAA
    other = 0x0CB0000700000009                                         # the same low seven bytes in leaf 0xCB
    assert G.leaf_of(tree, other) == 0xCB and G.get(tree, other)[0] == G.MISS


def test_a_negative_version_is_found_and_the_lower_of_two_equal_items_wins():
    tree = M.HTree(0, 1)
    tree.set(5, -2, 8, 1, 0x100)                                       # HTree.set stores it, uncounted
    assert tree.levels[0][0].count == 0
    assert G.get(tree, 5) == (G.FOUND, 1, 0x100, -2, 8, 0)
    tree.leafs[0] += struct.pack("<Q", 5) + M.item_to_bytes(3, 1, 0x200, 2)   # a hand-made second item
    assert G.get(tree, 5) == (G.FOUND, 1, 0x100, -2, 8, 0)


def test_load_fails_where_read_full_fails():
    file = _three_sources()
    for cut, leaf in ((0, 0), (95, 0), (96, 0), (99, 0), (100, 1), (103, 1), (104, 1), (141, 1), (142, 2),
                      (197, 15)):
        with pytest.raises(G.BadImage) as e:
            G.load(file[:cut], 0, 2)
        assert e.value.leaf == leaf, cut
    assert G.load(file + b"trailing", 0, 2).dump() == file
    odd = file[:100] + struct.pack("<I", 20) + file[104:] + b"\0" * 8
    with pytest.raises(G.BadImage) as e:
        G.load(odd, 0, 2)
    assert e.value.leaf == 1
    empty = M.HTree(2, 3).dump()
    assert len(empty) == 2560 and G.load(empty, 2, 3).leaf_first() == [0] * 257


def test_gc_liveness_by_hand():
    tree = G.load(_three_sources(), 0, 2)
    C = 0x2000000000000003
    tree.set(C, -4, 6, 1, 0x700)
    records = [(0x200, B, 3),       # chunk 1, offset 0x200: where the tree has B
               (0x100, B, 2),       # an older B
               (0x400, A, 5),       # A is at this offset, but in chunk 2
               (0x300, None, 0),    # no record
               (0x500, 0x3000000000000004, -1),   # never in the tree, a delete
               (0x600, 0x3000000000000005, 2),    # never in the tree, a set
               (0x800, C, -4)]      # found elsewhere, the tree's version negative
    rows, ask, t = G.gc_liveness(tree, records, 1, False)
    assert rows == [(1, G.GL_NEWEST, 10, 3, 0), (0, G.GL_OTHER_POS, 10, 3, 0), (0, G.GL_OTHER_POS, 1, 5, 1),
                    (0, G.GL_BAD, 0, 0, G.NO_SLOT), (0, G.GL_NOT_IN_TREE, 0, 0, G.NO_SLOT),
                    (0, G.GL_NOT_IN_TREE, 0, 0, G.NO_SLOT), (0, G.GL_OTHER_POS, 6, -4, 2)]
    assert ask == [1, 2, 6]
    assert t == [7, 1, 3, 1, 2, 0, 1, 1]
    rows, ask, t = G.gc_liveness(tree, records, 1, True)
    assert [r[0] for r in rows] == [1, 0, 0, 0, 1, 0, 0] and t == [7, 1, 3, 1, 2, 1, 1, 2]
    rows, ask, t = G.gc_liveness(tree, records, 2, True)
    assert [r[1] for r in rows][:3] == [G.GL_OTHER_POS, G.GL_OTHER_POS, G.GL_NEWEST] and ask == [0, 1, 6]
