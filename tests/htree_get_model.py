"""Plain-Python model of the queries over a built HTree (no GPU), the checker of
tests/test_gpu_htree_get.py.  It builds on htree_model.HTree with literal restatements of the
reference: HTree.load (store/htree.go:107-144), HTree.get (:313-330: getLeaf, SliceHeader.Get,
findInBytes, bytesToItem, store/leaf.go:53-59,81-102,155-164), the verdicts of GCMgr.gc
(store/gc.go:280-312) with an empty collision state, and UpdateHtreePos (:85-94).  It is pinned by
hand-worked answers in tests/test_htree_get_model.py.
"""
from __future__ import annotations

import struct

import htree_model as M

MISS, FOUND = 0, 1
GL_BAD, GL_NEWEST, GL_OTHER_POS, GL_NOT_IN_TREE = range(4)
NO_SLOT = 0xFFFFFFFF


class BadImage(Exception):
    """io.ReadFull failed in HTree.load, or (the ABI's own rule) a leaf's length is no whole
    number of items: .leaf is the leaf being read (0 inside the node table)."""

    def __init__(self, leaf: int, what: str):
        super().__init__(f"leaf {leaf}: {what}")
        self.leaf = leaf


def load(file: bytes, depth: int, height: int) -> M.HTree:
    """HTree.load: the leaf nodes' (count, hash), then every leaf's bytes.  What follows the last
    leaf is never read.  The upper nodes stay as newHTree left them (not up to date)."""
    tree = M.HTree(depth, height)
    leafnodes = tree.levels[height - 1]
    at = 0
    for n in leafnodes:
        if len(file) - at < 6:
            raise BadImage(0, "node table cut")
        n.count, n.hash = struct.unpack_from("<IH", file, at)
        at += 6
    for i in range(len(leafnodes)):
        if len(file) - at < 4:
            raise BadImage(i, "length word cut")
        (l,) = struct.unpack_from("<I", file, at)
        at += 4
        if l % tree.item_len:
            raise BadImage(i, "length is no multiple of the item's")     # not the reference's: findInBytes runs off
        if len(file) - at < l:
            raise BadImage(i, "leaf cut")
        tree.leafs[i] = bytearray(file[at:at + l])
        at += l
    return tree


def leaf_of(tree: M.HTree, keyhash: int) -> int:
    """getLeaf: the path's nibbles below the bucket's."""
    path = M.parse_path_uint64(keyhash)[tree.depth:]
    offset = 0
    for level in range(1, tree.height):
        offset = offset * 16 + path[level - 1]
    return offset


def get(tree: M.HTree, keyhash: int, first=None):
    """HTree.get: (found, chunk, offset, ver, vhash, slot); slot = the item's index among all
    items of the dump (first: tree.leaf_first(), for a caller that asks many times).  The
    bucket's nibbles take no part: khashToBytes keeps them only where the stored length reaches
    them, and there both sides drop them (qlzx_htree.h's slot rule)."""
    keyhash &= M.M64 >> (4 * tree.depth)
    off = leaf_of(tree, keyhash)
    leaf = tree.leafs[off]
    kb = struct.pack("<Q", keyhash)[:tree.khash_len]
    mask = struct.pack("<Q", M.M64 >> (4 * tree.depth))[:tree.khash_len]
    idx = -1
    for i in range(0, len(leaf), tree.item_len):                       # findInBytes
        if bytes(a & m for a, m in zip(leaf[i:i + tree.khash_len], mask)) == kb:
            idx = i
            break
    if idx < 0:
        return MISS, 0, 0, 0, 0, NO_SLOT
    ver, vhash, offset, chunk = M.bytes_to_item(bytes(leaf[idx + tree.khash_len:idx + tree.item_len]))
    return FOUND, chunk, offset, ver, vhash, (first or tree.leaf_first())[off] + idx // tree.item_len


def gc_liveness(tree: M.HTree, records, src_chunk: int, begin_gt_0: bool):
    """store/gc.go:280-312 per record with an empty collision state (getCollisionGC answers
    "not covered").  records: (offset, keyhash, ver) per record, keyhash None for a record the
    size checks refuse.  Returns (rows, ask_idx, totals): rows of (keep, verdict, vhash, tree_ver,
    slot), totals[8] as qlzx_gc_liveness's."""
    rows, ask, first = [], [], tree.leaf_first()
    t = [0] * 8
    t[0] = len(records)
    for j, (off, keyhash, ver) in enumerate(records):
        if keyhash is None:
            rows.append((0, GL_BAD, 0, 0, NO_SLOT))
            t[6] += 1
            continue
        found, chunk, offset, tver, tvhash, slot = get(tree, keyhash, first)
        if found:
            if (src_chunk, off) == (chunk, offset):       # oldPos == treePos
                rows.append((1, GL_NEWEST, tvhash, tver, slot))
                t[1] += 1
            else:
                rows.append((0, GL_OTHER_POS, tvhash, tver, slot))
                ask.append(j)
                t[2] += 1
                t[3] += tver < 0                          # isDeleted
        else:
            keep = int(begin_gt_0 and ver < 0)
            rows.append((keep, GL_NOT_IN_TREE, 0, 0, NO_SLOT))
            t[4] += 1
            t[5] += keep
    t[7] = sum(r[0] for r in rows)
    return rows, ask, t


def update_pos(tree: M.HTree, keyhash: int, chunk: int, offset: int) -> bool:
    """UpdateHtreePos: get, then set with the got meta at the new position.  False: not found."""
    found, _, _, ver, vhash, slot = get(tree, keyhash)
    if not found:
        return False
    # the bucket's own nibbles, as the item stores them (one bucket's keys all share them)
    off = leaf_of(tree, keyhash & (M.M64 >> (4 * tree.depth)))
    at = (slot - tree.leaf_first()[off]) * tree.item_len
    stored = int.from_bytes(bytes(tree.leafs[off][at:at + tree.khash_len]), "little")
    tree.set((keyhash & ~tree.khash_mask & M.M64) | stored, ver, vhash, chunk, offset)
    return True
