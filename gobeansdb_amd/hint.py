"""Hint split files of a replayed chunk on the GPU.

What buildHintFromData (store/bucket.go:89-117) does with the records of a replay:
getKeyHash of each key (store/key.go:41-59), HintBuffer.Set in append order (store/hint.go:
121-161: one item per (keyhash, key), the last version wins, a new key is refused once
SplitCap items exist and opens the next split), HintBuffer.Dump's sort by (keyhash, key) and
hintFileWriter's file: head, items and the sparse index (store/hintfile.go:142-212).  Every
per-record step runs in libqlzx.so (qlzx_keyhash_batch, qlzx_hint_plan, qlzx_hint_write,
csrc/qlzx_hint.hip); the host reads back totals[10] once per split.  The HTree, the hint lookup
structures and hint merge stay out of scope; the caller owns the files' bytes.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, batch, replay

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


def keyhash(keys: batch.BlockBatch, stream=None) -> torch.Tensor:
    """getKeyHashDefalut of every block: int64 [n] (the u64's bits)."""
    L = _lib.lib()
    out = torch.empty(keys.n, dtype=torch.int64, device=keys.data.device)
    _lib.check(L.qlzx_keyhash_batch(keys.data.data_ptr(), keys.off.data_ptr(), keys.length.data_ptr(), keys.n,
                                    out.data_ptr(), batch._stream(stream)), "qlzx_keyhash_batch")
    return out


def build_split(res: replay.ReplayResult, first: int = 0, split_cap: int = SPLIT_CAP,
                index_interval: int = INDEX_INTERVAL, chunk_id: int = 0, max_offset: int = 0,
                keyhash: torch.Tensor | None = None, workspace: batch.Workspace | None = None,
                stream=None) -> HintSplit:
    """One split file from the records res[first:]: as many as HintBuffer.Set takes with SplitCap =
    split_cap.  keyhash (int64 [n], optional) replaces the default key hash, as the reference's
    getKeyHash variable can.  One read-back: totals."""
    if stream is not None:
        with torch.cuda.stream(stream):
            return build_split(res, first, split_cap, index_interval, chunk_id, max_offset, keyhash, workspace, None)
    L = _lib.lib()
    data = res.data
    dev = data.device
    size, n = int(data.numel()), res.n
    st_ = batch._stream()
    cap = max(n, 1)
    result = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev)
    rec_off = res.offset.to(device=dev, dtype=torch.int64).contiguous()
    hdr = res.header.to(device=dev, dtype=torch.int32).contiguous()
    vh16 = res.vhash.to(device=dev, dtype=torch.int16).contiguous()
    if keyhash is not None:
        if keyhash.numel() != n:
            raise ValueError("keyhash: one per record")
        keyhash = keyhash.to(device=dev, dtype=torch.int64).contiguous()
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
        _lib.check(L.qlzx_hint_plan(batch._ptr(data) if size else None, size, rec_off.data_ptr(), result.data_ptr(),
                                    cap, hdr.data_ptr(), batch._ptr(keyhash), first, split_cap, index_interval,
                                    max_offset, item_rec.data_ptr(), item_hash.data_ptr(), item_off.data_ptr(),
                                    index_item.data_ptr(), totals.data_ptr(), ws.data_ptr(), ws_bytes, st_),
                   "qlzx_hint_plan")
        _lib.check(L.qlzx_hint_write(batch._ptr(data) if size else None, size, rec_off.data_ptr(), cap,
                                     hdr.data_ptr(), vh16.data_ptr(), chunk_id, item_rec.data_ptr(),
                                     item_hash.data_ptr(), item_off.data_ptr(), index_item.data_ptr(),
                                     out.data_ptr(), out_cap, totals.data_ptr(), ws.data_ptr(), ws_bytes, st_),
                   "qlzx_hint_write")
        t = totals.cpu().numpy().view(np.uint32)   # the read-back
    else:
        t = np.zeros(10, np.uint32)
        t[_lib.HINT_DATASIZE], t[_lib.HINT_INDEX_OFF_LO] = max_offset, 16
    if t[_lib.HINT_STATUS] != 0:
        raise _lib.QlzxError("qlzx_hint_write: the file does not fit its buffer")
    nbytes = int(t[_lib.HINT_BYTES_LO]) | (int(t[_lib.HINT_BYTES_HI]) << 32)
    return HintSplit(out[:nbytes], int(t[_lib.HINT_NUM_KEY]), int(t[_lib.HINT_DATASIZE]),
                     int(t[_lib.HINT_INDEX_OFF_LO]) | (int(t[_lib.HINT_INDEX_OFF_HI]) << 32),
                     int(t[_lib.HINT_N_INDEX]), int(t[_lib.HINT_CONSUMED]), int(t[_lib.HINT_SKIPPED]))


def build(res: replay.ReplayResult, split_cap: int = SPLIT_CAP, index_interval: int = INDEX_INTERVAL,
          chunk_id: int = 0, max_offset: int = 0, keyhash: torch.Tensor | None = None,
          workspace: batch.Workspace | None = None, stream=None) -> list[HintSplit]:
    """Every split of the chunk, as hintChunk.setItem -> rotate produces them (store/hint.go:
    241-252): the next split starts at the record the full buffer refused, with the previous
    split's datasize as its maxoffset."""
    ws = workspace or batch.Workspace(res.data.device)
    out, first = [], 0
    while first < res.n:
        sp = build_split(res, first, split_cap, index_interval, chunk_id, max_offset, keyhash, ws, stream)
        if sp.consumed == 0:
            raise _lib.QlzxError("qlzx_hint_plan consumed no record")
        out.append(sp)
        first += sp.consumed
        max_offset = sp.datasize
    return out
