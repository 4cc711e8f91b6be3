"""Plain-Python model of key lookups through hint files (no GPU), the checker of
tests/test_gpu_hintlookup.py.

A line-by-line restatement of hintFileIndex.get (store/hintindex.go:28-69) over
hintFileReader.open / next (store/hintfile.go:57-124) and of the order in which hintMgr.getItem
(store/hint.go:570-596) and hintChunk.get (:270-296) ask a bucket's files, with the verdicts of
qlzx_hint_lookup (include/qlzx.h).  Two things in get decide results and are kept as they are:

  - `j > 1`: the scan starts at index entry j - 1's offset only from the third answer of
    sort.Search on; j == 0 and j == 1 start at the head.  sort.Search is restated with Go's own
    loop (sort/search.go: i, j = 0, n; h = int(uint(i+j) >> 1); !f(h) moves i = h + 1), so that j
    is defined on an unsorted index too.
  - after fd.Seek(offset) the reader's own `offset` field is still 16 (hintfile.go:80) and next()
    tests that field against indexOffset (:90): the scan ends after indexOffset - 16 bytes
    consumed, wherever it started.  From a start above 16 it reads on into the index section.  A
    short io.ReadFull of the 23-byte head or of the key is the error, before the item is compared.

bounded=True is QLZX_HL_F_BOUNDED: the scan ends at indexOffset by position (hint_model.get).
hint_model.py supplies write_file, read_head and load_index; its get is the bounded variant only.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

from hint_model import HEAD, ITEM_HEAD, Item, keyhash, load_index, read_head, write_file  # noqa: F401

MISS, FOUND, ERR, BAD_FILE = range(4)   # enum qlzx_hl_status


def go_sort_search(n: int, f) -> int:
    """sort.Search (sort/search.go)."""
    i, j = 0, n
    while i < j:
        h = (i + j) >> 1
        if not f(h):
            i = h + 1
        else:
            j = h
    return i


def file_ok(file: bytes) -> bool:
    """What loadHintIndex (store/hintindex.go:71-119) needs to return an index: a whole head, an
    indexOffset inside the file, whole entries behind it (QLZX_HL_BAD_FILE otherwise)."""
    if len(file) < HEAD:
        return False
    index_offset = read_head(file)[0]
    return HEAD <= index_offset <= len(file) and (len(file) - index_offset) % 16 == 0


def get(file: bytes, kh: int, key: bytes, bounded: bool = False):
    """hintFileIndex.get: (status, item offset in the file or 0, Item or None).  file = None stands
    for a file that runs past the buffer it is said to lie in."""
    if file is None or not file_ok(file):
        return BAD_FILE, 0, None
    arr = load_index(file)
    index_offset = read_head(file)[0]
    j = go_sort_search(len(arr), lambda i: arr[i][0] >= kh)
    offset = HEAD
    if j > 1:
        offset = arr[j - 1][1]
        if not HEAD <= offset <= len(file):
            # a negative Seek fails and leaves the descriptor where bufio's first read put it; no
            # writer produces such an entry: the library answers ERR for every offset outside the file
            return ERR, 0, None
    pos = offset          # the descriptor's position (fd.Seek, rbuf.Reset)
    reader_offset = HEAD  # hintFileReader.offset, set by open() and not by the Seek
    while True:
        # next(): `if reader.offset >= reader.indexOffset { return nil, nil }`
        if (pos if bounded else reader_offset) >= index_offset:
            return MISS, 0, None
        h = file[pos:pos + ITEM_HEAD]                  # io.ReadFull(reader.rbuf, h)
        if len(h) < ITEM_HEAD:
            return ERR, 0, None
        ikh, chunk, off, ver, vhash, ksz = struct.unpack("<QIIiHB", h)
        k = file[pos + ITEM_HEAD:pos + ITEM_HEAD + ksz]  # io.ReadFull(reader.rbuf, key)
        if len(k) < ksz:
            return ERR, 0, None
        at = pos
        pos += ITEM_HEAD + ksz
        reader_offset += ITEM_HEAD + ksz
        if ikh < kh:
            continue
        if ikh > kh:
            return MISS, 0, None
        if k == key:
            return FOUND, at, Item(ikh, k, chunk, off, ver, vhash)


@dataclass
class Result:
    status: int = MISS
    hit_file: int = 0
    chunk: int = 0
    offset: int = 0
    ver: int = 0
    vhash: int = 0
    item_src: int = 0

    def astuple(self):
        return (self.status, self.hit_file, self.chunk, self.offset, self.ver, self.vhash, self.item_src)


def get_item(files, file_off, file_chunk, merged, kh: int, key: bytes, bounded: bool = False) -> Result:
    """hintMgr.getItem over `files` listed in its search order (newest chunk first, a chunk's splits
    last to first, the merged file where `i <= collisions.Chunk` first holds): the first hit wins,
    an error ends the search, and the merged file's answer is final.  A split hit reports its
    file's chunk id (chunkID = i), a merged hit the chunk stored in the item."""
    r = Result()
    for i, file in enumerate(files):
        r.hit_file = i
        r.status, at, it = get(file, kh, key, bounded)
        if r.status == FOUND:
            r.chunk = it.chunk_id if i == merged else file_chunk[i]
            r.offset, r.ver, r.vhash, r.item_src = it.offset, it.ver, it.vhash, file_off[i] + at
        if r.status != MISS or i == merged:
            break
    return r


def lookup(files, file_off, file_chunk, merged, keys, hashes=None, bounded: bool = False):
    """Every request's Result and totals = [found, miss, err, bad_file]."""
    out = [get_item(files, file_off, file_chunk, merged, keyhash(k) if hashes is None else hashes[i], k, bounded)
           for i, k in enumerate(keys)]
    totals = [sum(r.status == s for r in out) for s in (FOUND, MISS, ERR, BAD_FILE)]
    return out, totals
