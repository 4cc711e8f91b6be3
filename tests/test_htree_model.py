"""tests/htree_model.py pinned without the compiled reference (no GPU): answers worked by hand from
store/htree.go and store/leaf.go."""
import struct

import pytest

import hint_model
import htree_model as M
from hint_model import Item

A = 0x1000000200000001
B = 0x1000000500000002


def _file(items, index_interval=4096):
    return hint_model.write_file(items, 0, index_interval)[0]


def _it(kh, ver, vhash=0, offset=0, key=b"k"):
    return Item(kh, key, 0, offset, ver, vhash)


def test_set_remove_set_again_orders_the_leaf_by_incarnation():
    files = [_file([_it(A, 1, 3, 0x300), _it(B, 2, 7, 0x100)]),
             _file([_it(A, -1), _it(B, 3, 10, 0x200)]),
             _file([_it(A, 5, 1, 0x400)])]
    tree, dump, nset, nrem = M.build(files, [0, 1, 2], depth=0, height=2)
    leaf_b = bytes.fromhex("0200000005000010" "03000000" "0a00" "020000" "0100")
    leaf_a = bytes.fromhex("0100000002000010" "05000000" "0100" "040000" "0200")
    assert bytes(tree.leafs[1]) == leaf_b + leaf_a
    assert all(len(leaf) == 0 for i, leaf in enumerate(tree.leafs) if i != 1)
    assert (tree.levels[1][1].count, tree.levels[1][1].hash) == (2, 52)     # 10 * 5 + 1 * 2
    assert (tree.levels[0][0].count, tree.levels[0][0].hash) == (2, 52)
    assert (nset, nrem) == (4, 1)
    assert len(dump) == 198
    assert dump[6:12] == bytes.fromhex("020000003400")
    assert dump[:6] == bytes(6) and dump[12:96] == bytes(84)
    assert dump[96:100] == bytes(4)                                         # leaf 0: no bytes
    assert dump[100:104] == bytes.fromhex("26000000")
    assert dump[104:142] == leaf_b + leaf_a
    assert dump[142:] == bytes(56)
    assert tree.leaf_first() == [0, 0] + [2] * 15
    assert tree.list_dir("") == b"1000000500000002 10 3\n1000000200000001 1 5\n"
    assert tree.list_dir("1") == tree.list_dir("")
    assert tree.list_dir("10000005") == b"1000000500000002 10 3\n"
    assert tree.list_dir("2") == b""


def test_remove_of_an_absent_key_and_a_last_remove():
    C = 0x2000000300000007
    files = [_file([_it(A, -2), _it(C, 4, 9, 0x500)]), _file([_it(C, 0)])]   # ver 0 removes too
    tree, dump, nset, nrem = M.build(files, [3, 4], depth=0, height=2)
    assert (nset, nrem) == (1, 2)
    assert dump == bytes(10 * 16)
    assert (tree.levels[0][0].count, tree.levels[0][0].hash) == (0, 0)


def _spread(n_leaf0):
    """n_leaf0 items in leaf 0 and one in leaf 1, every hash term 1 (vhash 1, keyhash bits 32..47 = 1)."""
    items = [_it((1 << 32) | i, 1, 1, 256 * i) for i in range(n_leaf0)]
    return items + [_it((1 << 60) | (1 << 32), 1, 1, 0)]


def test_the_times_97_rule_starts_above_256():
    tree, _, _, _ = M.build([_file(_spread(255))], [0], depth=0, height=2)
    root = tree.levels[0][0]
    assert (root.count, root.hash) == (256, 256)                            # not above: a plain sum
    tree, _, _, _ = M.build([_file(_spread(255) + [_it((2 << 60) | (1 << 32), 1, 1, 0)])], [0], depth=0, height=2)
    root = tree.levels[0][0]
    # ((255 * 97 + 1) * 97 + 1) * 97^13: the children's hashes 255, 1, 1, 0, ... folded with *97 before each
    assert (root.count, root.hash) == (257, (255 * 97 ** 15 + 97 ** 14 + 97 ** 13) % 65536)
    assert root.hash == 9601


def test_list_dir_answers_node_lines_from_256_items_on():
    tree, _, _, _ = M.build([_file(_spread(255))], [0], depth=0, height=2)
    assert tree.list_dir("") == b"0/ 255 255\n1/ 1 1\n" + b"".join(b"%x/ 0 0\n" % i for i in range(2, 16))
    assert tree.list_dir("1") == b"1000000100000000 1 1\n"                  # the leaf level lists items
    assert tree.list_dir("0").count(b"\n") == 255
    tree, _, _, _ = M.build([_file(_spread(254))], [0], depth=0, height=2)
    assert tree.list_dir("").count(b"\n") == 255 and b"/" not in tree.list_dir("")


def test_seven_stored_bytes_and_an_alias_across_buckets():
    K1, K2 = 0x3AB0000700000009, 0x5AB0000700000009      # they differ in the bucket nibble only
    files = [_file([_it(K1, 1, 2, 0x100)]), _file([_it(K2, 2, 5, 0x300)])]
    tree, dump, _, _ = M.build(files, [0, 0], depth=1, height=3)
    assert (tree.khash_len, tree.item_len, len(tree.leafs)) == (7, 18, 256)
    item = bytes.fromhex("090000000700b0" "02000000" "0500" "030000" "0000")
    assert bytes(tree.leafs[0xAB]) == item                                  # one slot, rewritten in place
    assert (tree.levels[2][0xAB].count, tree.levels[2][0xAB].hash) == (1, 35)
    assert (tree.levels[1][0xA].count, tree.levels[1][0xA].hash) == (1, 35)
    assert (tree.levels[0][0].count, tree.levels[0][0].hash) == (1, 35)
    assert len(dump) == 2560 + 18
    assert dump[6 * 0xAB:6 * 0xAB + 6] == bytes.fromhex("010000002300")
    at = 6 * 256 + 4 * 0xAB
    assert dump[at:at + 4 + 18] == struct.pack("<I", 18) + item
    # Iter takes the nibbles above the stored bytes from the path it was asked with
    assert tree.list_dir("3") == b"3ab0000700000009 5 2\n"
    assert tree.list_dir("5ab") == b"5ab0000700000009 5 2\n"
    assert tree.list_dir("3ab00007") == b"3ab0000700000009 5 2\n"
    assert tree.list_dir("3ac") == b""
    with pytest.raises(ValueError, match="too short"):
        tree.list_dir("")


def test_one_level_and_the_deepest_geometry():
    tree, dump, _, _ = M.build([_file([_it(A, 1, 3, 0x300)])], [7], depth=0, height=1)
    assert dump == struct.pack("<IH", 1, 6) + struct.pack("<I", 19) + bytes(tree.leafs[0])
    assert bytes(tree.leafs[0]) == struct.pack("<Q", A) + bytes.fromhex("01000000" "0300" "030000" "0700")
    tree = M.HTree(2, 5)
    assert (tree.khash_len, len(tree.leafs), sum(len(lv) for lv in tree.levels)) == (5, 65536, 69905)


def test_the_reader_fails_where_the_reference_fails():
    good = _file([_it(A, 1, 3, 0x300, b"key")])
    assert [it.keyhash for it in M.read_file(good)] == [A]
    assert M.read_file(struct.pack("<qII", 16, 0, 0)) == []                 # no item: the loop just ends
    assert M.read_file(struct.pack("<qII", 0, 0, 0)) == []
    for bad in (good[:15], good[:16 + 22], good[:16 + 25],                  # head, item head, key cut
                struct.pack("<qII", -1, 0, 0), struct.pack("<qII", 17, 0, 0)):
        with pytest.raises(M.BadHintFile):
            M.read_file(bad)
    no_index = struct.pack("<qII", 0, 1, 0) + good[16:16 + 26]
    assert [it.key for it in M.read_file(no_index)] == [b"key"]
