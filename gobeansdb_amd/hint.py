"""Hint split files of a replayed chunk, their merge, and key lookups through them, on the GPU
(SURVEY §8 f1c, f1d, f1e).

What buildHintFromData (store/bucket.go:89-117) does with the records of a replay:
getKeyHash of each key (store/key.go:41-59), HintBuffer.Set in append order (store/hint.go:
121-161: one item per (keyhash, key), the last version wins, a new key is refused once
SplitCap items exist and opens the next split), HintBuffer.Dump's sort by (keyhash, key) and
hintFileWriter's file: head, items and the sparse index (store/hintfile.go:142-212).  Every
per-record step runs in libqlzx.so (qlzx_keyhash_batch, qlzx_hint_plan, qlzx_hint_write,
csrc/qlzx_hint.hip); the host reads back totals[10] once per split.

What hintMgr.Merge (store/hint.go:455-508) does with those files: merge (store/hintmerge.go:96-159)
over every split of a bucket gives the one merged file that lookups search first and the items
whose keyhash two or more keys share (the collision table GC's isNewest needs).  merge() takes the
files as device tensors, straight from build(); every per-item step runs in libqlzx.so
(qlzx_hint_merge_plan, qlzx_hint_merge_write, csrc/qlzx_hintmerge.hip); the host reads back
totals[12] once, and the collision items when there are any.

What hintMgr.getItem (store/hint.go:570-596) answers over those files: lookup() takes the files in
the order getItem reaches them and a batch of keys, and returns per key where its record is
(hintFileIndex.get, store/hintindex.go:28-69, as it is, or bounded=True: the scan ends at the
index).  Every step runs in libqlzx.so (qlzx_hint_lookup, csrc/qlzx_hintlookup.hip); the results
stay on the device (they feed replay.read_records / qlzx_read_plan), the host reads back totals[4].

The HTree built from those files is htree.py's.  CollisionTable.compareAndSet against an existing
table and the in-memory HintBuffer.Get stay out of scope; the caller owns the files' bytes.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _dev, _lib, batch, replay
from ._dev import on_stream, ptr, wide

SPLIT_CAP = _lib.HINT_SPLIT_CAP
INDEX_INTERVAL = _lib.HINT_INDEX_INTERVAL


@dataclass
class HintSplit:
    file: torch.Tensor   # uint8 (device): exactly the split file's bytes; empty when num_key == 0
    num_key: int
    datasize: int        # the buffer's maxoffset: the next split's max_offset
    index_offset: int
    n_index: int
    consumed: int        # records taken from `first` on; the next split starts at first + consumed
    skipped: int         # consumed records that failed the key guards (never a replay's own records)


def _pack(files):
    """The files as one device buffer: (buffer, offsets, lengths).  On the device: the files never leave it."""
    lens = [int(f.numel()) for f in files]
    offs = [sum(lens[:i]) for i in range(len(files))]
    hints = torch.cat([f.reshape(-1) for f in files]) if files else torch.empty(0, dtype=torch.uint8)
    return hints, offs, lens


def _files(what: str, file_off, file_len, chunk_ids, dev):
    """The per-file arguments of merge and lookup, checked and uploaded: (lengths on the host,
    offsets, lengths and chunk ids on the device)."""
    lens = [int(x) for x in file_len]
    if not (len(file_off) == len(chunk_ids) == len(lens)):
        raise ValueError(f"{what}: one offset, length and chunk id per file")
    if not lens:
        return lens, None, None, None
    return (lens, _dev.u64([int(x) for x in file_off], dev), _dev.u64(lens, dev),
            _dev.u32([int(c) & 0xFFFFFFFF for c in chunk_ids], dev))


@on_stream
def keyhash(keys: batch.BlockBatch, stream=None) -> torch.Tensor:
    """getKeyHashDefalut of every block: int64 [n] (the u64's bits)."""
    L = _lib.lib()
    out = torch.empty(keys.n, dtype=torch.int64, device=keys.data.device)
    _lib.check(L.qlzx_keyhash_batch(keys.data.data_ptr(), keys.off.data_ptr(), keys.length.data_ptr(), keys.n,
                                    out.data_ptr(), batch._stream()), "qlzx_keyhash_batch")
    return out


@on_stream
def build_split(res: replay.ReplayResult, first: int = 0, split_cap: int = SPLIT_CAP,
                index_interval: int = INDEX_INTERVAL, chunk_id: int = 0, max_offset: int = 0,
                keyhash: torch.Tensor | None = None, workspace: batch.Workspace | None = None,
                stream=None) -> HintSplit:
    """One split file from the records res[first:]: as many as HintBuffer.Set takes with SplitCap =
    split_cap.  keyhash (int64 [n], optional) replaces the default key hash, as the reference's
    getKeyHash variable can.  One read-back: totals."""
    L = _lib.lib()
    data = res.data
    dev = data.device
    size, n = int(data.numel()), res.n
    st_ = batch._stream()
    cap = max(n, 1)
    result = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev)
    rec_off, hdr = _dev.u64(res.offset, dev), _dev.i32(res.header, dev)
    vh16 = res.vhash.to(device=dev, dtype=torch.int16).contiguous()
    if keyhash is not None:
        if keyhash.numel() != n:
            raise ValueError("keyhash: one per record")
        keyhash = _dev.u64(keyhash, dev)
    item_rec = torch.empty(cap, dtype=torch.int32, device=dev)
    index_item = torch.empty(cap, dtype=torch.int32, device=dev)
    item_hash = torch.empty(cap, dtype=torch.int64, device=dev)
    item_off = torch.empty(cap, dtype=torch.int64, device=dev)
    totals = torch.zeros(10, dtype=torch.int32, device=dev)
    out_cap = 16 + 289 * max(n - first, 0)         # always enough: no read-back before the write
    out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    ws_bytes = L.qlzx_hint_workspace_size(cap)
    ws = (workspace or batch.Workspace(dev)).get(ws_bytes)
    if n:
        _lib.check(L.qlzx_hint_plan(ptr(data), size, rec_off.data_ptr(), result.data_ptr(),
                                    cap, hdr.data_ptr(), ptr(keyhash), first, split_cap, index_interval,
                                    max_offset, item_rec.data_ptr(), item_hash.data_ptr(), item_off.data_ptr(),
                                    index_item.data_ptr(), totals.data_ptr(), ws.data_ptr(), ws_bytes, st_),
                   "qlzx_hint_plan")
        _lib.check(L.qlzx_hint_write(ptr(data), size, rec_off.data_ptr(), cap,
                                     hdr.data_ptr(), vh16.data_ptr(), chunk_id, item_rec.data_ptr(),
                                     item_hash.data_ptr(), item_off.data_ptr(), index_item.data_ptr(),
                                     out.data_ptr(), out_cap, totals.data_ptr(), ws.data_ptr(), ws_bytes, st_),
                   "qlzx_hint_write")
        t = _dev.readback(totals)                  # the read-back
    else:
        t = np.zeros(10, np.uint32)
        t[_lib.HINT_DATASIZE], t[_lib.HINT_INDEX_OFF_LO] = max_offset, 16
    if t[_lib.HINT_STATUS] != 0:
        raise _lib.QlzxError("qlzx_hint_write: the file does not fit its buffer")
    nbytes = wide(t, _lib.HINT_BYTES_LO)
    return HintSplit(out[:nbytes], int(t[_lib.HINT_NUM_KEY]), int(t[_lib.HINT_DATASIZE]),
                     wide(t, _lib.HINT_INDEX_OFF_LO),
                     int(t[_lib.HINT_N_INDEX]), int(t[_lib.HINT_CONSUMED]), int(t[_lib.HINT_SKIPPED]))


@on_stream
def build(res: replay.ReplayResult, split_cap: int = SPLIT_CAP, index_interval: int = INDEX_INTERVAL,
          chunk_id: int = 0, max_offset: int = 0, keyhash: torch.Tensor | None = None,
          workspace: batch.Workspace | None = None, stream=None) -> list[HintSplit]:
    """Every split of the chunk, as hintChunk.setItem -> rotate produces them (store/hint.go:
    241-252): the next split starts at the record the full buffer refused, with the previous
    split's datasize as its maxoffset."""
    ws = workspace or batch.Workspace(res.data.device)
    out, first = [], 0
    while first < res.n:
        sp = build_split(res, first, split_cap, index_interval, chunk_id, max_offset, keyhash, ws)
        if sp.consumed == 0:
            raise _lib.QlzxError("qlzx_hint_plan consumed no record")
        out.append(sp)
        first += sp.consumed
        max_offset = sp.datasize
    return out


@dataclass
class HintMerged:
    file: torch.Tensor   # uint8 (device): the merged file's bytes; empty when write=False
    num_key: int
    datasize: int        # the largest of the sources' heads'
    index_offset: int
    n_index: int
    items_read: int      # the items of all sources
    collisions: list     # (keyhash, key, chunk_id, offset, ver, vhash) of every merged item whose keyhash
    #                      is shared by two or more keys, in merged order


@on_stream
def merge_packed(hints: torch.Tensor, file_off, file_len, chunk_ids, index_interval: int = INDEX_INTERVAL,
                 write: bool = True, cap: int | None = None, workspace: batch.Workspace | None = None,
                 stream=None) -> HintMerged:
    """merge() for a caller that holds every source in one device buffer: source i is
    hints[file_off[i] : file_off[i] + file_len[i]] with the reader's chunk id chunk_ids[i].
    cap (the most items the sources may hold) defaults to what their lengths allow."""
    L = _lib.lib()
    dev = hints.device
    lens, off_d, len_d, chunk_d = _files("merge", file_off, file_len, chunk_ids, dev)
    n_files, nbytes = len(lens), int(hints.numel())
    room = sum(max(x - 16, 0) for x in lens)
    if cap is None:
        cap = room // 23
    empty = torch.empty(0, dtype=torch.uint8, device=dev)
    if n_files == 0:
        return HintMerged(empty, 0, 0, 16, 0, 0, [])
    cap = max(cap, 1)                               # a source without room for an item is the device's verdict
    out_cap = 16 + room + 16 * cap if write else 0  # always enough: no read-back before the write
    st_ = batch._stream()
    item_src, item_off = (torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(2))
    item_chunk, index_item, coll_item = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
    totals = torch.zeros(12, dtype=torch.int32, device=dev)
    out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    ws_bytes = L.qlzx_hint_merge_workspace_size(nbytes, n_files, cap)
    ws = (workspace or batch.Workspace(dev)).get(ws_bytes)
    hp = ptr(hints)
    _lib.check(L.qlzx_hint_merge_plan(hp, nbytes, off_d.data_ptr(), len_d.data_ptr(), chunk_d.data_ptr(), n_files, cap,
                                      index_interval, item_src.data_ptr(), item_chunk.data_ptr(), item_off.data_ptr(),
                                      index_item.data_ptr(), coll_item.data_ptr(), totals.data_ptr(), ws.data_ptr(),
                                      ws_bytes, st_), "qlzx_hint_merge_plan")
    if write:
        _lib.check(L.qlzx_hint_merge_write(hp, nbytes, cap, item_src.data_ptr(), item_chunk.data_ptr(),
                                           item_off.data_ptr(), index_item.data_ptr(), out.data_ptr(), out_cap,
                                           totals.data_ptr(), ws.data_ptr(), ws_bytes, st_), "qlzx_hint_merge_write")
    t = _dev.readback(totals)                       # the read-back
    status = int(t[_lib.HM_STATUS])
    if status != _lib.HM_OK:
        name = _lib.HM_NAMES[status] if status < len(_lib.HM_NAMES) else str(status)
        raise _lib.QlzxError(f"qlzx_hint_merge: {name}, source {int(t[_lib.HM_STATUS_SOURCE])}")
    collisions = []
    ncoll = int(t[_lib.HM_N_COLLISION])
    if ncoll:
        # the collision items' 23 + 255 source bytes, gathered on the device: one more read-back
        ci = coll_item[:ncoll].long()
        src = item_src[ci]
        span = (src[:, None] + torch.arange(23 + 255, device=dev)[None, :]).clamp_(max=nbytes - 1)
        raw = hints[span].cpu().numpy()
        chunks = _dev.readback(item_chunk[ci])
        for row, c in zip(raw, chunks):
            b = row.tobytes()
            ksz = b[22]
            collisions.append((int.from_bytes(b[0:8], "little"), b[23:23 + ksz], int(c),
                               int.from_bytes(b[12:16], "little"), int.from_bytes(b[16:20], "little", signed=True),
                               int.from_bytes(b[20:22], "little")))
    nb = wide(t, _lib.HM_BYTES_LO)
    return HintMerged(out[:nb] if write else empty, int(t[_lib.HM_NUM_KEY]), int(t[_lib.HM_DATASIZE]),
                      wide(t, _lib.HM_INDEX_OFF_LO), int(t[_lib.HM_N_INDEX]),
                      int(t[_lib.HM_ITEMS_READ]), collisions)


@on_stream
def merge(files, chunk_ids, index_interval: int = INDEX_INTERVAL, write: bool = True,
          workspace: batch.Workspace | None = None, stream=None) -> HintMerged:
    """hintMgr.Merge over split files in device memory (HintSplit.file straight from build());
    chunk_ids[i] is the chunk file i belongs to.  write=False is Merge(forGC = true): the collision
    items and no file.  Raises QlzxError naming the status and the source for a file the reference's
    readers would fail on (HM_BAD_FILE), or one that does not ascend strictly (HM_UNSORTED)."""
    files = list(files)
    if not files:
        return merge_packed(torch.empty(0, dtype=torch.uint8), [], [], [], index_interval, write)
    hints, offs, lens = _pack(files)
    return merge_packed(hints, offs, lens, chunk_ids, index_interval, write, None, workspace)


@dataclass
class HintLookup:
    status: torch.Tensor     # int32 [n] (device): _lib.HL_MISS / HL_FOUND / HL_ERR / HL_BAD_FILE
    hit_file: torch.Tensor   # int32 [n]: the file where the search ended
    chunk: torch.Tensor      # int32 [n] (u32 bits): a split hit's chunk id, a merged hit's stored chunk
    offset: torch.Tensor     # int32 [n] (u32 bits): the record's offset in its chunk
    ver: torch.Tensor        # int32 [n]
    vhash: torch.Tensor      # int16 [n] (u16 bits)
    item_src: torch.Tensor   # int64 [n]: the item's byte offset in the packed files
    totals: tuple            # (found, miss, err, bad_file), read back once


@on_stream
def lookup_packed(hints: torch.Tensor, file_off, file_len, chunk_ids, keys: batch.BlockBatch,
                  merged: int | None = None, bounded: bool = False, keyhash: torch.Tensor | None = None,
                  workspace: batch.Workspace | None = None, stream=None) -> HintLookup:
    """lookup() for a caller that holds every file in one device buffer: file i is
    hints[file_off[i] : file_off[i] + file_len[i]] with the chunk id chunk_ids[i], in search order."""
    L = _lib.lib()
    dev = keys.data.device
    lens, off_d, len_d, chunk_d = _files("lookup", file_off, file_len, chunk_ids, dev)
    n_files, nbytes, n = len(lens), int(hints.numel()), keys.n
    if merged is not None and not 0 <= merged < n_files:
        raise ValueError("lookup: merged is the index of a file")
    if keyhash is not None:
        if keyhash.numel() != n:
            raise ValueError("keyhash: one per key")
        keyhash = _dev.u64(keyhash, dev)
    status, hit_file, chunk, offset, ver = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(5))
    vhash = torch.zeros(n, dtype=torch.int16, device=dev)
    item_src = torch.zeros(n, dtype=torch.int64, device=dev)
    if n == 0 or n_files == 0:                      # no file: every key is a miss
        return HintLookup(status, hit_file, chunk, offset, ver, vhash, item_src, (0, n, 0, 0))
    flag_d = _dev.u32([_lib.HL_FILE_MERGED if i == merged else 0 for i in range(n_files)], dev)
    totals = torch.zeros(4, dtype=torch.int32, device=dev)
    ws_bytes = L.qlzx_hint_lookup_workspace_size(n, n_files)
    ws = (workspace or batch.Workspace(dev)).get(ws_bytes)
    flags = _lib.HL_F_BOUNDED if bounded else 0     # the kernel (a wave or a lane per request) goes by n
    _lib.check(L.qlzx_hint_lookup(ptr(hints), nbytes, off_d.data_ptr(), len_d.data_ptr(),
                                  chunk_d.data_ptr(), flag_d.data_ptr(), n_files, keys.data.data_ptr(),
                                  keys.off.data_ptr(), keys.length.data_ptr(), ptr(keyhash), n, flags,
                                  status.data_ptr(), hit_file.data_ptr(), chunk.data_ptr(), offset.data_ptr(),
                                  ver.data_ptr(), vhash.data_ptr(), item_src.data_ptr(), totals.data_ptr(),
                                  ws.data_ptr(), ws_bytes, batch._stream()), "qlzx_hint_lookup")
    t = _dev.readback(totals)                       # the read-back
    return HintLookup(status, hit_file, chunk, offset, ver, vhash, item_src, tuple(int(x) for x in t))


@on_stream
def lookup(files, chunk_ids, keys: batch.BlockBatch, merged: int | None = None, bounded: bool = False,
           keyhash: torch.Tensor | None = None, workspace: batch.Workspace | None = None,
           stream=None) -> HintLookup:
    """hintMgr.getItem of every key over hint files in device memory (HintSplit.file / HintMerged.file
    straight from build() / merge()).  THE ORDER OF `files` IS THE SEARCH ORDER: newest chunk first,
    a chunk's splits last to first, the merged file where getItem reaches it; chunk_ids[i] is the
    chunk of file i, merged the index of the merged file (its hits report the chunk stored in the
    item, and nothing after it is searched) or None.  bounded=False is the reference as it is: a
    key above a file's last item usually ends in HL_ERR, which ends the search; bounded=True ends
    the scan at the index and goes on to the next file (what a multi-GET or a GC liveness pass
    wants).  keyhash (int64 [n]) replaces the default key hash.  The results stay on the device; totals is read back once."""
    hints, offs, lens = _pack(list(files))
    return lookup_packed(hints, offs, lens, chunk_ids, keys, merged, bounded, keyhash, workspace)
