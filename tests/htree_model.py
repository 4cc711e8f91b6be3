"""Plain-Python model of the HTree (no GPU), the checker of tests/test_gpu_htree.py.

A literal restatement of the reference, item by item, with byte arrays and a linear find:
newHTree, setToLeaf / remvoeFromLeaf, getLeafAndInvalidNodes, getNode, updateNodes, collectItems,
listDir / ListDir and dump (store/htree.go), SliceHeader.Set / Remove / Iter, findInBytes,
itemToBytes / bytesToItem and getNodeKhash (store/leaf.go), InitTree (store/config.go:82-96),
KeyInfo.Prepare (store/key.go:83-142) and updateHtreeFromHint (store/bucket.go:119-151) over
hint_model's reader.  It is pinned by hand-worked answers in tests/test_htree_model.py.
"""
from __future__ import annotations

import struct

import hint_model

M16, M32, M64 = 0xFFFF, 0xFFFFFFFF, (1 << 64) - 1
KHASH_LENS = [8, 8, 7, 7, 6, 6, 5, 5]
TREE_ITEM_HEAD_SIZE = 11
THRESHOLD_LIST_KEY = 64 * 4
THRESHOLD_BIG_HASH = 64 * 4
MAX_DEPTH = 8


class BadHintFile(Exception):
    """hintFileReader.open / next returned an error: bucket open fails."""


class Node:
    def __init__(self):
        self.count = 0
        self.hash = 0
        self.is_hash_updated = False


def parse_path_uint64(khash: int) -> list[int]:
    return [(khash >> (4 * (15 - i))) & 0xF for i in range(16)]


def get_node_khash(path: list[int]) -> int:
    khash = 0
    for i, off in enumerate(path):
        khash = (khash + (((off & 0xF) << (4 * (7 - i))) & M32)) & M32
    return khash


def item_to_bytes(ver: int, vhash: int, offset: int, chunk_id: int) -> bytes:
    v = chunk_id & M32
    return struct.pack("<IH", ver & M32, vhash) + bytes([(offset >> 8) & 0xFF, (offset >> 16) & 0xFF,
                                                         (offset >> 24) & 0xFF, v & 0xFF, (v >> 8) & 0xFF])


def bytes_to_item(b: bytes) -> tuple[int, int, int, int]:
    """(ver, vhash, offset, chunk)."""
    ver, vhash = struct.unpack_from("<iH", b, 0)
    return ver, vhash, (b[6] << 8) | (b[7] << 16) | (b[8] << 24), b[9] | (b[10] << 8)


class HTree:
    def __init__(self, depth: int, height: int):
        if depth + height > MAX_DEPTH:
            raise ValueError("HTree too high")
        self.depth, self.height = depth, height
        # InitTree
        self.khash_len = KHASH_LENS[depth + height - 1]
        shift = 64 - self.khash_len * 8
        self.khash_mask = ((M64 << shift) & M64) >> shift
        self.item_len = self.khash_len + TREE_ITEM_HEAD_SIZE
        # newHTree
        self.levels = [[Node() for _ in range(16 ** i)] for i in range(height)]
        for n in self.levels[height - 1]:
            n.is_hash_updated = True
        self.leafs = [bytearray() for _ in range(16 ** (height - 1))]

    # ---- store/leaf.go ----
    def _find(self, leaf: bytearray, keyhash: int) -> int:
        kb = struct.pack("<Q", keyhash)[:self.khash_len]
        for i in range(0, len(leaf), self.item_len):
            if leaf[i:i + self.khash_len] == kb:
                return i
        return -1

    def _leaf_set(self, leaf: bytearray, keyhash: int, item: bytes):
        """SliceHeader.Set: (old item or None)."""
        idx = self._find(leaf, keyhash)
        old = None
        new = struct.pack("<Q", keyhash)[:self.khash_len] + item
        if idx >= 0:
            old = bytes_to_item(bytes(leaf[idx + self.khash_len:idx + self.item_len]))
            leaf[idx:idx + self.item_len] = new
        else:
            leaf += new
        return old

    def _leaf_remove(self, leaf: bytearray, keyhash: int, old_chunk: int, old_offset: int):
        """SliceHeader.Remove: the removed item or None."""
        idx = self._find(leaf, keyhash)
        if idx >= 0:
            old = bytes_to_item(bytes(leaf[idx + self.khash_len:idx + self.item_len]))
            if old_chunk == -1 or old[2] == old_offset:
                del leaf[idx:idx + self.item_len]      # copy the tail down, Len -= itemLen
                return old
        return None

    # ---- store/htree.go ----
    def _leaf_and_invalid_nodes(self, keyhash: int) -> int:
        if self.height == 1:
            # getLeafAndInvalidNodes indexes path[-1] here (no configuration runs a tree of one
            # level); the ABI defines it: the root is the one leaf, always up to date
            return 0
        path = parse_path_uint64(keyhash)[self.depth:]
        level_n = self.height - 1
        offset = 0
        self.levels[0][0].is_hash_updated = False
        for level in range(1, self.height - 1):
            offset = offset * 16 + path[level - 1]
            self.levels[level][offset].is_hash_updated = False
        return offset * 16 + path[level_n - 1]

    def set(self, keyhash: int, ver: int, vhash: int, chunk_id: int, offset: int) -> None:
        off = self._leaf_and_invalid_nodes(keyhash)
        node = self.levels[self.height - 1][off]
        old = self._leaf_set(self.leafs[off], keyhash, item_to_bytes(ver, vhash, offset, chunk_id))
        v = 0
        if ver > 0:
            v = (v + vhash) & M16
            node.count = (node.count + 1) & M32
        if old is not None and old[0] > 0:
            v = (v - old[1]) & M16
            node.count = (node.count - 1) & M32
        node.hash = (node.hash + v * ((keyhash >> 32) & M16)) & M16

    def remove(self, keyhash: int, old_chunk: int, old_offset: int) -> None:
        off = self._leaf_and_invalid_nodes(keyhash)
        node = self.levels[self.height - 1][off]
        old = self._leaf_remove(self.leafs[off], keyhash, old_chunk, old_offset)
        if old is not None and old[0] > 0:
            node.hash = (node.hash - old[1] * ((keyhash >> 32) & M16)) & M16
            node.count = (node.count - 1) & M32

    def update_nodes(self, level: int = 0, offset: int = 0) -> Node:
        node = self.levels[level][offset]
        if node.is_hash_updated:
            return node
        node.count = 0
        hashs = []
        for i in range(16):
            c = self.update_nodes(level + 1, offset * 16 + i)
            node.count = (node.count + c.count) & M32
            hashs.append(c.hash)
        node.hash = 0
        for i in range(16):
            if node.count > THRESHOLD_BIG_HASH:
                node.hash = (node.hash * 97) & M16
            node.hash = (node.hash + hashs[i]) & M16
        node.is_hash_updated = True
        return node

    def _iter(self, leaf_off: int, path: list[int]):
        """SliceHeader.Iter: (keyhash, ver, vhash) per item."""
        leaf = self.leafs[leaf_off]
        node_khash = (get_node_khash(path) << 32) & ~self.khash_mask & M64
        for i in range(0, len(leaf), self.item_len):
            ver, vhash, _, _ = bytes_to_item(bytes(leaf[i + self.khash_len:i + self.item_len]))
            khash = struct.unpack_from("<Q", bytes(leaf[i:i + 8]))[0]
            yield (khash & self.khash_mask) | node_khash, ver, vhash

    def _collect(self, level: int, offset: int, path: list[int], items: list, want: int, mask: int) -> None:
        if level >= self.height - 1:
            for h, ver, vhash in self._iter(offset, path):
                if mask & h == want:
                    items.append((h, ver, vhash))
        else:
            for i in range(16):
                self._collect(level + 1, offset * 16 + i, path + [i], items, want, mask)

    def list_dir(self, path_str: str) -> bytes:
        """ListDir for ki = {StringKey: path_str, KeyIsPath: true}, Prepare()d."""
        if len(path_str) < self.depth:
            raise ValueError("bad dir path to list: too short")
        key_path = [int(c, 16) for c in path_str]           # ParsePathString
        key_hash = 0
        for i, v in enumerate(key_path):                    # setKeyHashByPath
            key_hash |= v << (60 - 4 * i)
        # listDir
        if len(key_path) == self.depth:
            level, offset, path = 0, 0, key_path
        else:                                                # getNode
            reach = min(self.depth + self.height - 1, len(key_path))
            offset = 0
            for h in range(self.depth, reach):
                offset = offset * 16 + key_path[h]
            level = reach - self.depth
            path = key_path[:self.depth + level]
        node = self.levels[level][offset]
        self.update_nodes(level, offset)
        if level >= self.height - 1 or node.count < THRESHOLD_LIST_KEY:
            shift = 64 - len(path_str) * 4
            mask = 0 if shift >= 64 else ((M64 >> shift) << shift) & M64
            items: list = []
            self._collect(level, offset, list(path), items, key_hash, mask)
            return b"".join(b"%016x %d %d\n" % (h, vhash, ver) for h, ver, vhash in items)
        nodes = [self.levels[level + 1][offset * 16 + i] for i in range(16)]
        return b"".join(b"%x/ %d %d\n" % (i, n.hash, n.count) for i, n in enumerate(nodes))

    def dump(self) -> bytes:
        out = bytearray()
        for n in self.levels[self.height - 1]:
            out += struct.pack("<IH", n.count, n.hash)
        for leaf in self.leafs:
            out += struct.pack("<I", len(leaf))
            out += leaf
        return bytes(out)

    def leaf_first(self) -> list[int]:
        """The exclusive scan of the items per leaf, nleaf + 1 entries."""
        out = [0]
        for leaf in self.leafs:
            out.append(out[-1] + len(leaf) // self.item_len)
        return out


def read_file(file: bytes):
    """hintFileReader.open and next until nil, failing as they fail: the items."""
    if len(file) < hint_model.HEAD:
        raise BadHintFile("head")
    index_offset = hint_model.read_head(file)[0]
    if index_offset == 0:
        index_offset = len(file)                    # "has no index"
    # past the file the reader runs into EOF, an error; a negative one is refused as
    # qlzx_hint_merge_plan's reading refuses it (the reference would read no item)
    if index_offset < 0 or index_offset > len(file):
        raise BadHintFile("indexOffset")
    offset, out = hint_model.HEAD, []
    while offset < index_offset:
        if len(file) - offset < hint_model.ITEM_HEAD:
            raise BadHintFile("item head")
        ksz = file[offset + 22]
        if len(file) - offset - hint_model.ITEM_HEAD < ksz:
            raise BadHintFile("item key")
        it, offset = hint_model.next_item(file, offset, index_offset)
        out.append(it)
    return out


def update_from_hint(tree: HTree, chunk_id: int, file: bytes) -> tuple[int, int]:
    """updateHtreeFromHint: (sets, removes) applied."""
    nset = nrem = 0
    for it in read_file(file):
        if it.ver > 0:
            tree.set(it.keyhash, it.ver, it.vhash, chunk_id, it.offset)
            nset += 1
        else:
            tree.remove(it.keyhash, -1, it.offset)
            nrem += 1
    return nset, nrem


def build(files, chunk_ids, depth: int, height: int = 3):
    """Bucket open's loop over the split files, Update and dump: (tree, file bytes, sets, removes)."""
    tree = HTree(depth, height)
    nset = nrem = 0
    for f, c in zip(files, chunk_ids):
        s, r = update_from_hint(tree, c, f)
        nset, nrem = nset + s, nrem + r
    tree.update_nodes(0, 0)
    return tree, tree.dump(), nset, nrem
