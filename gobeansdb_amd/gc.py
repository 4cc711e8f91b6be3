"""GC rewrite of a .data chunk on the GPU.

Host mirror of the data movement of GCMgr.gc (store/gc.go:268-353) for one source
chunk resident in device memory: the records the stream reader returns (their offsets
come from qlzx_replay_index, gobeansdb_amd/replay.py) are filtered by a liveness mask
-- liveness() below makes it on the device from the bucket's HTree image
(store/gc.go:280-312, qlzx_gc_liveness); the collision table and the in-memory hint
buffers that getCollisionGC consults stay the caller's, for the records liveness()
lists in ask_idx -- and every kept record is appended to the destination in order, as
dataChunk.AppendRecordGC -> WriteRecord.append (store/datachunk.go:56-79,
store/datafile.go:307-330) does: header re-encoded with its CRC recomputed over
header[4:24] ‖ key ‖ value (store/datafile.go:66-88), zero padding to 256 B, and a new
destination chunk whenever recsize + writingHead > DataFileMax (store/gc.go:320-332).

The destination offsets are an exclusive scan of the kept records' padded sizes with
those rotations (host, one pass over the sizes); the copies (qlzx_copy_batch) and the
CRCs (qlzx_crc32_batch over the copied records) run in libqlzx.so.  The rewritten
CRC must equal the stored one (the reader verified it); `crc_mismatch` counts the
records where it does not, which would mean a corrupted copy.

rewrite_batch is the same rewrite with every per-record step on the device (SURVEY §8 f4b,
qlzx_gc_plan / qlzx_gc_rewrite, csrc/qlzx_gc.hip): the planning included, each record read once
and written once with its CRC computed on the way, and only totals[8] and the chunk sizes read back.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _dev, _lib, batch
from ._dev import on_stream, ptr
from .record import BODY_MAX, HDR, MAX_KEY_LEN

DATA_FILE_MAX = 4000 << 20   # store/config_default.go:39


@dataclass
class GCResult:
    chunks: list[torch.Tensor]   # destination chunk bytes (device), each from its starting head on
    chunk: np.ndarray            # int32 [kept] destination chunk index of each kept record
    offset: np.ndarray           # uint64 [kept] offset in that chunk (absolute, from the chunk's start)
    crc: np.ndarray              # uint32 [kept] recomputed record CRCs
    crc_mismatch: int            # kept records whose recomputed CRC differs from the stored one


def chunk_head(c: int, dst_head: int, next_heads) -> int:
    """Starting writingHead of destination chunk c: dst_head for the first, next_heads[c - 1]
    for later ones (0 past the list).  beginGCWriting starts a destination at its current size
    unless it is the source chunk being rewritten (store/datachunk.go:185-193)."""
    if c == 0:
        return int(dst_head)
    return int(next_heads[c - 1]) if c - 1 < len(next_heads) else 0


def plan(recsize: np.ndarray, dst_head: int = 0, data_file_max: int = DATA_FILE_MAX, next_heads=()):
    """Destination (chunk, offset) of records of padded size `recsize` appended in order from
    dst_head, rotating when recsize + head > data_file_max (store/gc.go:320); destination
    chunk c >= 1 starts at chunk_head(c)."""
    n = len(recsize)
    chunk = np.zeros(n, np.int32)
    off = np.zeros(n, np.uint64)
    i, c, head = 0, 0, int(dst_head)
    rs = recsize.astype(np.int64)
    while i < n:
        # the longest run from i that fits without rotating, by a cumulative sum
        cs = np.cumsum(rs[i:]) + head
        fit = int(np.searchsorted(cs, data_file_max, side="right"))
        if fit == 0:          # this record starts a new chunk
            c += 1
            head = chunk_head(c, dst_head, next_heads)
            cs = np.cumsum(rs[i:]) + head
            fit = max(1, int(np.searchsorted(cs, data_file_max, side="right")))
        chunk[i:i + fit] = c
        off[i:i + fit] = (cs[:fit] - rs[i:i + fit]).astype(np.uint64)
        head = int(cs[fit - 1])
        i += fit
    return chunk, off


@dataclass
class GCBatch:
    """rewrite_batch's result; the per-record tensors live on the device, one entry per record of
    rec_off (kept or not)."""
    status: torch.Tensor         # int32 enum qlzx_gc_status
    new_chunk: torch.Tensor      # int32 destination chunk index (0 for a record not placed)
    new_off: torch.Tensor        # int64 offset in that chunk, from the chunk's start (0 if not placed)
    crc: torch.Tensor            # int32 recomputed record CRCs (0 for a record not written)
    chunks: list[torch.Tensor]   # views into `out`: destination chunk c's bytes from its head on
    out: torch.Tensor            # uint8 destination buffer, the chunks packed back to back
    totals: np.ndarray           # uint32 [8], as qlzx_gc_plan / qlzx_gc_rewrite leave them
    chunk_bytes: np.ndarray      # uint64 [chunks used]

    def result(self) -> GCResult:
        """The fields gc.rewrite returns, over the records written (this reads the tensors back)."""
        w = (self.status == _lib.GC_WRITTEN).cpu().numpy()
        chunks = self.chunks or [self.out[:0]]
        return GCResult(chunks, self.new_chunk.cpu().numpy()[w].astype(np.int32),
                        self.new_off.cpu().numpy().view(np.uint64)[w], _dev.readback(self.crc)[w],
                        int(self.totals[6]))


@on_stream
def rewrite_batch(data: torch.Tensor, rec_off: torch.Tensor, keep: torch.Tensor, dst_head: int = 0,
                  data_file_max: int = DATA_FILE_MAX, next_heads=(), max_chunks: int | None = None,
                  out: torch.Tensor | None = None, stream=None) -> GCBatch:
    """gc.rewrite with every per-record step on the device (qlzx_gc_plan, qlzx_gc_rewrite): sizes,
    destinations, statuses and CRCs stay there, the records are read once and written once with the
    CRC computed on the way.  The host reads back totals[8] and the chunk sizes, nothing else.
    Destination chunk c starts at chunk_head(c, dst_head, next_heads); at most max_chunks
    (default: as many as the library takes) are used, later survivors get GC_NO_CHUNK.  `out`
    (optional, 16-B aligned, not overlapping data) receives the chunks packed back to back;
    pad256(len(data)) bytes always suffice for record offsets that came from replay.index."""
    L = _lib.lib()
    dev = data.device
    size, n = int(data.numel()), int(rec_off.numel())
    if keep.numel() != n:
        raise ValueError("keep: one per record")
    if max_chunks is None:
        max_chunks = _lib.MAX_NUM_CHUNK
    st_ = batch._stream()
    cap = max(n, 1)
    heads = np.zeros(max_chunks, np.uint64)                # chunk_head(c) for every c: 0 past next_heads
    known = [int(dst_head), *map(int, next_heads)][:max_chunks]
    heads[:len(known)] = known
    heads = _dev.u64(heads, dev)
    result = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev)
    keep8 = keep.to(device=dev, dtype=torch.uint8).contiguous()
    rec_off = _dev.u64(rec_off, dev)
    status = torch.empty(cap, dtype=torch.int32, device=dev)
    new_chunk, crc = torch.empty_like(status), torch.empty_like(status)
    new_off = torch.empty(cap, dtype=torch.int64, device=dev)
    chunk_base = torch.zeros(max_chunks, dtype=torch.int64, device=dev)
    chunk_bytes = torch.zeros(max_chunks, dtype=torch.int64, device=dev)
    totals = torch.zeros(8, dtype=torch.int32, device=dev)
    if out is None:
        out = torch.empty(max((size + 255) // 256 * 256, 16), dtype=torch.uint8, device=dev)
    ws_bytes = L.qlzx_gc_workspace_size(cap, max_chunks)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    if n:
        _lib.check(L.qlzx_gc_plan(ptr(data), size, rec_off.data_ptr(), result.data_ptr(),
                                  cap, keep8.data_ptr(), MAX_KEY_LEN, BODY_MAX, data_file_max, heads.data_ptr(),
                                  max_chunks, status.data_ptr(), new_chunk.data_ptr(), new_off.data_ptr(),
                                  chunk_base.data_ptr(), chunk_bytes.data_ptr(), totals.data_ptr(), ws.data_ptr(),
                                  ws_bytes, st_), "qlzx_gc_plan")
        _lib.check(L.qlzx_gc_rewrite(ptr(data), size, rec_off.data_ptr(),
                                     result.data_ptr(), cap, heads.data_ptr(), max_chunks, new_chunk.data_ptr(),
                                     new_off.data_ptr(), chunk_base.data_ptr(), out.data_ptr(), int(out.numel()),
                                     status.data_ptr(), crc.data_ptr(), totals.data_ptr(), ws.data_ptr(), ws_bytes,
                                     st_), "qlzx_gc_rewrite")
    t = _dev.readback(totals)                              # the read-backs: totals and the chunk sizes
    cb = chunk_bytes[:max(int(t[3]), 1)].cpu().numpy().view(np.uint64)[:int(t[3])]
    base = np.concatenate([[0], np.cumsum(cb.astype(np.int64))])
    chunks = [out[int(base[c]):int(base[c + 1])] for c in range(len(cb))]
    return GCBatch(status[:n], new_chunk[:n], new_off[:n], crc[:n], chunks, out, t, cb)


@on_stream
def rewrite(data: torch.Tensor, rec_off: torch.Tensor, keep: torch.Tensor, dst_head: int = 0,
            data_file_max: int = DATA_FILE_MAX, stream=None, next_heads=()) -> GCResult:
    """Rewrite the kept records of the chunk `data` (record offsets `rec_off` in reader order,
    bool mask `keep`) into destination chunks: the first starts at dst_head, chunk c >= 1 at
    next_heads[c - 1] (0 past the list).  chunks[c] holds the bytes written from that head on."""
    dev = data.device
    ko = rec_off[keep].to(torch.int64)
    n = int(ko.numel())
    if n == 0:
        return GCResult([torch.zeros(0, dtype=torch.uint8, device=dev)], np.zeros(0, np.int32),
                        np.zeros(0, np.uint64), np.zeros(0, np.uint32), 0)
    hidx = ko.unsqueeze(1) + torch.arange(HDR, device=dev).unsqueeze(0)
    hdr = data[hidx.reshape(-1)].reshape(n, HDR).contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    stored_crc, ksz, vsz = hdr[:, 0], hdr[:, 4].astype(np.int64), hdr[:, 5].astype(np.int64)
    size = HDR + ksz + vsz                                    # Record.Sizes (store/item.go:219-222)
    recsize = (size + 255) // 256 * 256
    chunk, off = plan(recsize, dst_head, data_file_max, next_heads)
    src_off = ko.cpu().numpy().view(np.uint64)
    chunks = []
    for c in range(int(chunk[-1]) + 1):
        sel = np.nonzero(chunk == c)[0]
        base = chunk_head(c, dst_head, next_heads)
        end = int(off[sel[-1]] + recsize[sel[-1]]) if len(sel) else base
        buf = torch.zeros(max(end - base, 1), dtype=torch.uint8, device=dev)[: end - base]
        if len(sel):   # record bytes; the zero padding is the fresh buffer's (datafile.go:322-327)
            batch.copy_blocks(data, src_off[sel], size[sel], buf, off[sel] - np.uint64(base))
        chunks.append(buf)
    # encodeHeader/getCRC over each rewritten record, written into its header
    crc = np.zeros(n, np.uint32)
    for c, buf in enumerate(chunks):
        sel = np.nonzero(chunk == c)[0]
        if not len(sel):
            continue
        local = off[sel] - np.uint64(chunk_head(c, dst_head, next_heads))
        got = batch.crc32(batch.BlockBatch(buf, _dev.u64(local + np.uint64(4), dev), _dev.u32(size[sel] - 4, dev)))
        buf.view(torch.int32)[_dev.u64(local // 4, dev)] = got
        crc[sel] = _dev.readback(got)
    return GCResult(chunks, chunk, off, crc, int((crc != stored_crc).sum()))


@dataclass
class GCLiveness:
    """liveness()'s result: one entry per record of rec_off, on the device; only totals is read back."""
    keep: torch.Tensor       # uint8: 1 for a record GC rewrites; goes straight into rewrite_batch
    verdict: torch.Tensor    # int32: _lib.GL_BAD / GL_NEWEST / GL_OTHER_POS / GL_NOT_IN_TREE
    vhash: torch.Tensor      # int16 (u16 bits): the tree's value hash of a found key
    tree_ver: torch.Tensor   # int32: the tree's version of a found key (isDeleted = tree_ver < 0)
    slot: torch.Tensor       # int32 (u32 bits): the key's item in the image, HTG_NO_SLOT when not found
    ask_idx: torch.Tensor    # int32 [totals[GL_N_OTHER_POS]]: the OTHER_POS records, ascending
    totals: np.ndarray       # uint32 [8]: records, NEWEST, OTHER_POS, of those deleted, NOT_IN_TREE, of those kept, BAD, keep


@on_stream
def liveness(data: torch.Tensor, rec_off: torch.Tensor, tree, src_chunk: int, begin_gt_0: bool = False,
             keyhash: torch.Tensor | None = None, stream=None) -> GCLiveness:
    """GC's verdict per record of the chunk `data` (store/gc.go:280-312, qlzx_gc_liveness) against
    `tree` (an htree.HTreeImage): a record is kept when the tree finds its key at
    (src_chunk, its offset), or when the key is not in the tree, begin_gt_0 (gc.Begin > 0) and the
    record is a delete.  Records whose key the tree finds elsewhere are listed in ask_idx, for a
    caller with a collision table to resolve; without one their keep = 0 stands.  keyhash
    (int64, one per record) replaces the default hash of the records' keys."""
    L = _lib.lib()
    dev = data.device
    size, n = int(data.numel()), int(rec_off.numel())
    cap = max(n, 1)
    rec_off = _dev.u64(rec_off, dev)
    if keyhash is not None:
        if keyhash.numel() != n:
            raise ValueError("keyhash: one per record")
        keyhash = _dev.u64(keyhash, dev)
    result = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev)
    keep = torch.zeros(cap, dtype=torch.uint8, device=dev)
    verdict, tree_ver, slot, ask_idx = (torch.zeros(cap, dtype=torch.int32, device=dev) for _ in range(4))
    vhash = torch.zeros(cap, dtype=torch.int16, device=dev)
    totals = torch.zeros(8, dtype=torch.int32, device=dev)
    if n:
        ws_bytes = L.qlzx_gc_liveness_workspace_size(cap)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(L.qlzx_gc_liveness(ptr(data), size, rec_off.data_ptr(), result.data_ptr(), cap, MAX_KEY_LEN,
                                      BODY_MAX, src_chunk, ptr(tree.file), int(tree.file.numel()),
                                      tree.leaf_first.data_ptr(), tree.depth, tree.height, ptr(keyhash),
                                      _lib.GL_F_BEGIN_GT_0 if begin_gt_0 else 0, keep.data_ptr(),
                                      verdict.data_ptr(), vhash.data_ptr(), tree_ver.data_ptr(), slot.data_ptr(),
                                      ask_idx.data_ptr(), totals.data_ptr(), ws.data_ptr(), ws_bytes,
                                      batch._stream()), "qlzx_gc_liveness")
    t = _dev.readback(totals)                              # the read-back
    return GCLiveness(keep[:n], verdict[:n], vhash[:n], tree_ver[:n], slot[:n],
                      ask_idx[:int(t[_lib.GL_N_OTHER_POS])], t)
