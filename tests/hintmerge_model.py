"""Plain-Python model of the hint merge (no GPU), the checker of tests/test_gpu_hintmerge.py.

A fresh restatement of the reference's sequential merge: hintFileReader.open / next
(store/hintfile.go:57-124), mergeHeap.Less, mergeWriter.write / flush and merge
(store/hintmerge.go:30-159), CollisionTable.compareAndSet (store/collision.go:36-52) and
Position.CmpKey (store/item.go:196).  The file is hint_model.write_file's (hintFileWriter).
Go is not available to the tests, so no golden file comes from the compiled reference: the model
is pinned by tests/test_hintmerge_model.py.

Where the reference leaves the outcome open, the model takes the library's rule: two heap entries
with equal (keyhash, key, CmpKey) pop in source order (the later source is written last and wins).
"""
from __future__ import annotations

import heapq
from dataclasses import dataclass, field

from hint_model import HEAD, ITEM_HEAD, Item, next_item, read_head, write_file


class BadFile(Exception):
    """A reader's error, or the nil first item of a source without one; .source names it."""

    def __init__(self, source: int, what: str):
        super().__init__(f"source {source}: {what}")
        self.source = source


def cmp_key(it: Item) -> int:
    """Position.CmpKey: chunk << 32 | offset, the offset unsigned."""
    return (it.chunk_id << 32) | (it.offset & 0xFFFFFFFF)


class Reader:
    """hintFileReader: the items of one source, each at position (chunk_id, stored offset)."""

    def __init__(self, file: bytes, chunk_id: int, source: int):
        self.file, self.chunk_id, self.source = file, chunk_id, source
        if len(file) < HEAD:
            raise BadFile(source, "short head")
        self.index_offset, _, self.datasize = read_head(file)
        if self.index_offset == 0:             # "has no index"
            self.index_offset = len(file)
        if self.index_offset > len(file) or self.index_offset < 0:
            raise BadFile(source, "indexOffset outside the file")
        self.offset = HEAD

    def next(self) -> Item | None:
        if self.offset >= self.index_offset:
            return None
        if self.offset + ITEM_HEAD > len(self.file):
            raise BadFile(self.source, "item head cut short")
        ksz = self.file[self.offset + ITEM_HEAD - 1]
        if self.offset + ITEM_HEAD + ksz > len(self.file):
            raise BadFile(self.source, "key cut short")
        it, self.offset = next_item(self.file, self.offset, self.index_offset)
        it.chunk_id = self.chunk_id            # hintmerge.go:108,142
        return it


class CollisionTable:
    """store/collision.go: keyhash -> key -> item."""

    def __init__(self):
        self.items: dict[int, dict[bytes, Item]] = {}

    def compare_and_set(self, it: Item) -> None:
        items = self.items.get(it.keyhash)
        if items is None:
            self.items[it.keyhash] = {it.key: it}
            return
        old = items.get(it.key)
        if old is None or cmp_key(it) >= cmp_key(old):
            items[it.key] = it


class MergeWriter:
    """mergeWriter: buf holds the items of one keyhash, one per run of equal keys."""

    def __init__(self, table: CollisionTable):
        self.table = table
        self.buf: list[Item] = []
        self.written: list[Item] = []
        self.collisions: list[Item] = []

    def write(self, it: Item) -> None:
        if not self.buf:
            self.buf = [it]
            return
        last = self.buf[-1]
        if last.keyhash != it.keyhash:
            self.flush()
            self.buf = [it]
        elif last.key != it.key:
            self.buf.append(it)
        else:
            self.buf[-1] = it

    def flush(self) -> None:
        if len(self.buf) > 1:
            for it in self.buf:
                self.table.compare_and_set(it)
                self.collisions.append(it)
        self.written += self.buf       # mw.w.writeItem; forGC has no writer, merge() drops the file


@dataclass
class Merged:
    file: bytes                 # b"" for_gc
    num_key: int
    datasize: int
    index_offset: int
    n_index: int
    items_read: int
    collisions: list            # (keyhash, key, chunk_id, offset, ver, vhash) in flush order
    table: CollisionTable = field(default_factory=CollisionTable)


def as_tuple(it: Item):
    return (it.keyhash, it.key, it.chunk_id, it.offset, it.ver, it.vhash)


def merge(files, chunk_ids, index_interval: int = 4096, for_gc: bool = False,
          table: CollisionTable | None = None) -> Merged:
    """merge(src, dst, ct, hintState, forGC): the heap loop, then flush and close."""
    table = table or CollisionTable()
    datasize, heap, read = 0, [], 0
    for i, (f, c) in enumerate(zip(files, chunk_ids)):
        r = Reader(bytes(f), c, i)
        it = r.next()
        if it is None:
            raise BadFile(i, "no item")        # hp[i].curr.Pos: a nil dereference
        datasize = max(datasize, r.datasize)
        heap.append((it.keyhash, it.key, cmp_key(it), i, it, r))
    heapq.heapify(heap)
    mw = MergeWriter(table)
    while heap:
        _, _, _, i, it, r = heapq.heappop(heap)
        mw.write(it)
        read += 1
        nxt = r.next()
        if nxt is not None:
            heapq.heappush(heap, (nxt.keyhash, nxt.key, cmp_key(nxt), i, nxt, r))
    mw.flush()
    coll = [as_tuple(it) for it in mw.collisions]
    items = mw.written
    # Merge(forGC = true) opens no writer; the figures of the file it would be are still the plan's
    file, index_offset, n_index = write_file(items, datasize, index_interval)
    return Merged(b"" if for_gc else file, len(items), datasize, index_offset, n_index, read, coll, table)


def merged_by_sort(files, chunk_ids) -> list[Item]:
    """For strictly ascending sources: sort by (keyhash, key, CmpKey, source), keep each key's last."""
    every = []
    for i, (f, c) in enumerate(zip(files, chunk_ids)):
        r = Reader(bytes(f), c, i)
        while (it := r.next()) is not None:
            every.append((it.keyhash, it.key, cmp_key(it), i, len(every), it))
    every.sort(key=lambda e: e[:5])
    out: list[Item] = []
    for e in every:
        if out and (out[-1].keyhash, out[-1].key) == (e[0], e[1]):
            out[-1] = e[5]
        else:
            out.append(e[5])
    return out


def is_strictly_ascending(file: bytes) -> bool:
    r = Reader(bytes(file), 0, 0)
    prev = None
    while (it := r.next()) is not None:
        if prev is not None and (prev.keyhash, prev.key) >= (it.keyhash, it.key):
            return False
        prev = it
    return True
