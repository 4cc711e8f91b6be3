"""Plain-Python model of the hint split file (no GPU), the checker of tests/test_gpu_hint.py.

A fresh restatement of the reference's hint build and of the reader that consumes its files:
getKeyHashDefalut (store/key.go:41-59), HintBuffer.Set / Dump (store/hint.go:121-208),
hintFileWriter.writeItem / close (store/hintfile.go:163-212), hintFileIndexBuffer.append
(store/hintindex.go:140-150), and on the reading side hintFileReader.next (store/hintfile.go:89-124),
loadHintIndex and hintFileIndex.get (store/hintindex.go:28-119, its `j > 1` included).
MurmurHash3_x86_32 is not in the reference tree (an imported module): it is pinned by the
published known answers in tests/test_hint_model.py.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

M32 = 0xFFFFFFFF
HEAD, ITEM_HEAD = 16, 23


def fnv1a(key: bytes) -> int:
    """store/key.go:47-55: h ^= uint32(int8(b))."""
    h = 0x811C9DC5
    for b in key:
        h ^= (b - 256 if b >= 128 else b) & M32
        h = (h * 0x01000193) & M32
    return h


def _rotl(x: int, r: int) -> int:
    return ((x << r) | (x >> (32 - r))) & M32


def murmur3_32(key: bytes, seed: int = 0) -> int:
    """MurmurHash3_x86_32."""
    h = seed
    nb = len(key) // 4
    for i in range(nb):
        k = struct.unpack_from("<I", key, 4 * i)[0]
        k = (k * 0xCC9E2D51) & M32
        k = _rotl(k, 15)
        k = (k * 0x1B873593) & M32
        h ^= k
        h = _rotl(h, 13)
        h = (h * 5 + 0xE6546B64) & M32
    tail = key[4 * nb:]
    if tail:
        k = int.from_bytes(tail, "little")
        k = (k * 0xCC9E2D51) & M32
        k = _rotl(k, 15)
        k = (k * 0x1B873593) & M32
        h ^= k
    h ^= len(key)
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def keyhash(key: bytes) -> int:
    """getKeyHashDefalut (store/key.go:57-59)."""
    return (fnv1a(key) << 32) | murmur3_32(key)


@dataclass
class Item:
    keyhash: int
    key: bytes
    chunk_id: int
    offset: int
    ver: int
    vhash: int


class HintBuffer:
    """store/hint.go:93-208."""

    def __init__(self, split_cap: int, max_offset: int = 0):
        self.split_cap = split_cap
        self.maxoffset = max_offset
        self.index: dict[int, int] = {}
        self.collisions: dict[int, dict[bytes, int]] = {}
        self.items: list[Item | None] = []
        self.num = 0

    def set(self, it: Item, rec_size: int) -> bool:
        if not self.index:
            self.items = [None] * self.split_cap
        idx = self.index.get(it.keyhash)
        found = idx is not None
        iscollision = False
        if found and it.key != self.items[idx].key:
            iscollision = True
            keys = self.collisions.get(it.keyhash)
            found = keys is not None
            if found:
                idx = keys.get(it.key)
                found = idx is not None
            else:
                self.collisions[it.keyhash] = {self.items[idx].key: idx}
        if not found:
            idx = self.num
            if idx >= len(self.items):
                if it.offset > self.maxoffset:
                    self.maxoffset = it.offset
                return False
            self.num += 1
        self.items[idx] = it
        self.index[it.keyhash] = idx
        if iscollision:
            self.collisions[it.keyhash][it.key] = idx
        end = (it.offset + rec_size) & M32
        if end > self.maxoffset:
            self.maxoffset = end
        return True

    def dump(self, index_interval: int) -> tuple[bytes, int, int]:
        """(file bytes, indexOffset, index entries)."""
        arr = sorted(self.items[:self.num], key=lambda it: (it.keyhash, it.key))
        return write_file(arr, self.maxoffset, index_interval)


def write_file(items: list[Item], datasize: int, index_interval: int) -> tuple[bytes, int, int]:
    """newHintFileWriter, writeItem per item, close (store/hintfile.go:142-212)."""
    body = bytearray(HEAD)
    offset, lastoffset = HEAD, 0
    index = []
    for it in items:
        body += struct.pack("<QIIiHB", it.keyhash, it.chunk_id & M32, it.offset, it.ver, it.vhash, len(it.key) & 0xFF)
        body += it.key
        if offset - lastoffset > index_interval - ITEM_HEAD - 256:
            index.append((it.keyhash, offset))
            lastoffset = offset
        offset += ITEM_HEAD + len(it.key)
    index_offset = offset
    for kh, o in index:
        body += struct.pack("<Qq", kh, o)
    body[:HEAD] = struct.pack("<qII", index_offset, len(items), datasize)
    return bytes(body), index_offset, len(index)


@dataclass
class Split:
    file: bytes
    consumed: int
    num_key: int
    datasize: int
    n_index: int
    index_offset: int
    skipped: int


def build_split(records, first: int = 0, split_cap: int = 1 << 20, index_interval: int = 4096, chunk_id: int = 0,
                max_offset: int = 0) -> Split:
    """One split from records[first:], each (keyhash, key, offset, recsize, ver, vhash) in append
    order, or None for a record the device guards skip: HintBuffer.Set until it returns false."""
    buf = HintBuffer(split_cap, max_offset)
    j, skipped = first, 0
    while j < len(records):
        r = records[j]
        if r is None:
            skipped += 1
        elif not buf.set(Item(r[0], r[1], chunk_id, r[2], r[4], r[5]), r[3]):
            break
        j += 1
    consumed = max(j - first, 0)
    if buf.num == 0:
        return Split(b"", consumed, 0, buf.maxoffset, 0, HEAD, skipped)
    file, index_offset, n_index = buf.dump(index_interval)
    return Split(file, consumed, buf.num, buf.maxoffset, n_index, index_offset, skipped)


def build(records, split_cap: int = 1 << 20, index_interval: int = 4096, chunk_id: int = 0, max_offset: int = 0):
    """hintChunk.setItem -> rotate (store/hint.go:241-252): splits until the records are used up."""
    out, first = [], 0
    while first < len(records):
        sp = build_split(records, first, split_cap, index_interval, chunk_id, max_offset)
        out.append(sp)
        first += sp.consumed
        max_offset = sp.datasize
    return out


# ---- the reader side ----
def read_head(file: bytes) -> tuple[int, int, int]:
    """hintFileMeta.Loads: (indexOffset, numKey, datasize)."""
    return struct.unpack_from("<qII", file, 0)


def next_item(file: bytes, offset: int, index_offset: int):
    """hintFileReader.next (store/hintfile.go:89-124): (item, next offset), item None at the index."""
    if offset >= index_offset:
        return None, offset
    kh, chunk, off, ver, vhash, ksz = struct.unpack_from("<QIIiHB", file, offset)
    key = file[offset + ITEM_HEAD:offset + ITEM_HEAD + ksz]
    return Item(kh, key, chunk, off, ver, vhash), offset + ITEM_HEAD + ksz


def read_items(file: bytes) -> list[Item]:
    index_offset = read_head(file)[0]
    out, offset = [], HEAD
    while True:
        it, offset = next_item(file, offset, index_offset)
        if it is None:
            return out
        out.append(it)


def load_index(file: bytes) -> list[tuple[int, int]]:
    """loadHintIndex (store/hintindex.go:71-119)."""
    start = read_head(file)[0]
    raw = file[start:]
    return [struct.unpack_from("<Qq", raw, o) for o in range(0, len(raw) - len(raw) % 16, 16)]


def get(file: bytes, index: list[tuple[int, int]], kh: int, key: bytes):
    """hintFileIndex.get (store/hintindex.go:28-69)."""
    j = next((i for i, e in enumerate(index) if e[0] >= kh), len(index))   # sort.Search: first >=
    offset = HEAD
    if j > 1:
        offset = index[j - 1][1]
    index_offset = read_head(file)[0]
    while True:
        it, offset = next_item(file, offset, index_offset)
        if it is None:
            return None
        if it.keyhash < kh:
            continue
        if it.keyhash > kh:
            return None
        if it.key == key:
            return it
