"""A bucket's HTree and its .hash dump from hint files in device memory, on the GPU.

What bucket open does once the split files exist: updateHtreeFromHint over every file
(store/bucket.go:119-151, :207-230: HTree.set for an item with ver > 0, HTree.remove otherwise),
HTree.Update (store/htree.go:332-359) and HTree.dump (:146-203).  build() takes the files as
device tensors, straight from hint.build(), in the order bucket open applies them (chunk
ascending, then split ascending); every per-item step runs in libqlzx.so (qlzx_htree_plan,
qlzx_htree_write, include/qlzx_htree.h, csrc/qlzx_htree.hip); the host reads back totals[10] once.

HTreeBuilt.list_dir answers the @path listing (HTree.ListDir, store/htree.go:361-436) on the host,
over the few nodes or the leaf range it reads back.

The built tree is queried as its .hash image plus leaf_first (HTreeImage; include/qlzx_htree_get.h,
csrc/qlzx_htree_get.hip): load_image() is HTree.load of an uploaded file, HTreeBuilt.image() the
same of a tree just built, get() a batched HTree.get (store/htree.go:313-330) and move()
UpdateHtreePos (store/gc.go:85-94) for the records gc.liveness() -> gc.rewrite_batch() moved.

HTree.set / remove of new writes on a live image (they grow leaves) and the store-level tree over
the bucket roots stay out of scope; the caller owns the files' bytes.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _dev, _lib, batch, hint
from ._dev import on_stream, ptr, wide

M64 = (1 << 64) - 1


def geometry(depth: int, height: int) -> tuple[int, int]:
    """(L, nleaf): Conf.TreeKeyHashLen (store/config.go:91) and the leaves of one bucket's tree."""
    if not (0 <= depth <= _lib.HT_MAX_DEPTH and 1 <= height <= _lib.HT_MAX_HEIGHT):
        raise ValueError("htree: depth is 0..2 and height 1..6")
    return _lib.HT_KHASH_LENS[depth + height - 1], 16 ** (height - 1)


def level_base(level: int) -> int:
    """Where level `level` starts in the level-major node arrays."""
    return (16 ** level - 1) // 15


@dataclass
class HTreeBuilt:
    levels: list             # per level (count int32 [16^l], hash int16 [16^l] (u16 bits)), on the device
    leaf_first: torch.Tensor  # int32 [nleaf + 1] (device): the exclusive scan of the slots per leaf
    file: torch.Tensor       # uint8 (device): the .hash file's bytes; empty when write=False
    n_ops: int
    n_set: int
    n_remove: int
    n_slots: int
    depth: int = 0
    height: int = 3
    # the slots in file order: where each one's item lies in `hints`, and its chunk (device)
    slot_src: torch.Tensor | None = field(default=None, repr=False)
    slot_chunk: torch.Tensor | None = field(default=None, repr=False)
    hints: torch.Tensor | None = field(default=None, repr=False)

    def image(self) -> "HTreeImage":
        """The tree as get() / gc.liveness() / move() take it: the build already has leaf_first."""
        if self.file.numel() == 0:
            raise ValueError("htree: image() needs the file (build with write=True)")
        return HTreeImage(self.file, self.leaf_first, self.n_slots, self.depth, self.height)

    def node(self, level: int, offset: int) -> tuple[int, int]:
        """(count, hash) of one node: a read-back."""
        count, hash_ = self.levels[level]
        return int(count[offset]), int(hash_[offset]) & 0xFFFF

    def list_dir(self, path: str) -> bytes:
        """HTree.ListDir for a hex path of `depth` digits or more: the sixteen child lines
        "%x/ %d %d\\n" (hash, count) of a node above the leaves that holds 256 items or more,
        otherwise the item lines "%016x %d %d\\n" (keyhash, vhash, ver) under the path."""
        if len(path) < self.depth:
            raise ValueError("bad dir path to list: too short")
        if len(path) > 16:
            raise ValueError("bad dir path to list: more than 16 digits")
        nib = [int(c, 16) for c in path]                 # ParsePathString
        want = sum(v << (60 - 4 * i) for i, v in enumerate(nib))   # setKeyHashByPath
        # getNode: the path's node, clamped to the leaf level
        reach = min(self.depth + self.height - 1, len(nib))
        level, offset = reach - self.depth, 0
        for v in nib[self.depth:reach]:
            offset = offset * 16 + v
        count, _ = self.node(level, offset)
        if level < self.height - 1 and count >= _lib.HT_LIST_THRESHOLD:
            counts, hashes = self.levels[level + 1]
            c = _dev.readback(counts[16 * offset:16 * offset + 16])
            h = hashes[16 * offset:16 * offset + 16].cpu().numpy().view(np.uint16)
            return b"".join(b"%x/ %d %d\n" % (i, int(h[i]), int(c[i])) for i in range(16))
        # collectItems: the leaves under the node in order, each leaf's items in order
        shift = 64 - 4 * len(path)
        mask = 0 if shift >= 64 else ((M64 >> shift) << shift) & M64   # Go: a shift of 64 or more gives 0
        L, _ = geometry(self.depth, self.height)
        low = (1 << (8 * L)) - 1
        span = 16 ** (self.height - 1 - level)
        first = _dev.readback(self.leaf_first[offset * span:(offset + 1) * span + 1]).astype(np.int64)
        a, b = int(first[0]), int(first[-1])
        if a == b:
            return b""
        src = self.slot_src[a:b]
        rows = self.hints[src[:, None] + torch.arange(23, device=src.device)[None, :]].cpu().numpy()
        out = []
        for j in range(span):
            leaf = offset * span + j
            # Iter: the node's nibbles above the stored low bytes (getNodeKhash << 32 & ^mask)
            digits = nib[:self.depth] + [(leaf >> (4 * (self.height - 2 - i))) & 15 for i in range(self.height - 1)]
            top = sum(v << (60 - 4 * i) for i, v in enumerate(digits)) & ~low & M64
            for k in range(int(first[j]) - a, int(first[j + 1]) - a):
                raw = rows[k].tobytes()
                kh = (int.from_bytes(raw[0:8], "little") & low) | top
                if kh & mask == want:
                    out.append(b"%016x %d %d\n" % (kh, int.from_bytes(raw[20:22], "little"),
                                                   int.from_bytes(raw[16:20], "little", signed=True)))
        return b"".join(out)


@on_stream
def build_packed(hints: torch.Tensor, file_off, file_len, chunk_ids, depth: int, height: int = 3,
                 write: bool = True, cap: int | None = None, workspace: batch.Workspace | None = None,
                 stream=None) -> HTreeBuilt:
    """build() for a caller that holds every source in one device buffer: source i is
    hints[file_off[i] : file_off[i] + file_len[i]] with the chunk id chunk_ids[i].  cap (the most
    items the sources may hold) defaults to what their lengths allow."""
    L = _lib.lib()
    klen, nleaf = geometry(depth, height)
    dev = hints.device
    lens, off_d, len_d, chunk_d = hint._files("htree", file_off, file_len, chunk_ids, dev)
    n_files, nbytes = len(lens), int(hints.numel())
    if cap is None:
        cap = sum(max(x - 16, 0) for x in lens) // 23
    cap = max(cap, 1)
    out_cap = 10 * nleaf + (klen + 11) * cap if write else 0   # always enough: no read-back before the write
    st_ = batch._stream()
    n_nodes = level_base(height)
    node_count = torch.empty(n_nodes, dtype=torch.int32, device=dev)
    node_hash = torch.empty(n_nodes, dtype=torch.int16, device=dev)
    leaf_first = torch.empty(nleaf + 1, dtype=torch.int32, device=dev)
    slot_src = torch.empty(cap, dtype=torch.int64, device=dev)
    slot_chunk = torch.empty(cap, dtype=torch.int32, device=dev)
    totals = torch.zeros(10, dtype=torch.int32, device=dev)
    out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    ws_bytes = L.qlzx_htree_workspace_size(nbytes, n_files, cap, height)
    ws = (workspace or batch.Workspace(dev)).get(ws_bytes)
    hp = ptr(hints)
    _lib.check(L.qlzx_htree_plan(hp, nbytes, ptr(off_d), ptr(len_d), ptr(chunk_d), n_files, cap, depth, height,
                                 node_count.data_ptr(), node_hash.data_ptr(), leaf_first.data_ptr(),
                                 slot_src.data_ptr(), slot_chunk.data_ptr(), totals.data_ptr(), ws.data_ptr(),
                                 ws_bytes, st_), "qlzx_htree_plan")
    if write:
        _lib.check(L.qlzx_htree_write(hp, nbytes, cap, depth, height, node_count.data_ptr(), node_hash.data_ptr(),
                                      leaf_first.data_ptr(), slot_src.data_ptr(), slot_chunk.data_ptr(),
                                      out.data_ptr(), out_cap, totals.data_ptr(), ws.data_ptr(), ws_bytes, st_),
                   "qlzx_htree_write")
    t = _dev.readback(totals)                       # the read-back
    status = int(t[_lib.HT_STATUS])
    if status != _lib.HT_OK:
        name = _lib.HT_NAMES[status] if status < len(_lib.HT_NAMES) else str(status)
        raise _lib.QlzxError(f"qlzx_htree: {name}, source {int(t[_lib.HT_STATUS_SOURCE])}")
    levels = [(node_count[level_base(l):level_base(l + 1)], node_hash[level_base(l):level_base(l + 1)])
              for l in range(height)]
    n_slots = int(t[_lib.HT_N_SLOTS])
    nb = wide(t, _lib.HT_BYTES_LO)
    return HTreeBuilt(levels, leaf_first, out[:nb] if write else out[:0], int(t[_lib.HT_OPS_READ]),
                      int(t[_lib.HT_N_SET]), int(t[_lib.HT_N_REMOVE]), n_slots, depth, height,
                      slot_src[:n_slots], slot_chunk[:n_slots], hints)


@on_stream
def build(files, chunk_ids, depth: int, height: int = 3, write: bool = True,
          workspace: batch.Workspace | None = None, stream=None) -> HTreeBuilt:
    """The HTree of a bucket from its hint split files in device memory (HintSplit.file straight
    from hint.build()), in the order bucket open applies them; chunk_ids[i] is the chunk file i
    belongs to.  depth is Conf.TreeDepth (0 / 1 / 2 for 1 / 16 / 256 buckets), height
    Conf.TreeHeight.  write=False gives the nodes and the slots' order and no file.  Raises
    QlzxError naming the status and the source for a file the reference's reader would fail on
    (HT_BAD_FILE)."""
    files = list(files)
    if not files:
        dev = "cuda" if torch.cuda.is_available() else "cpu"
        return build_packed(torch.empty(0, dtype=torch.uint8, device=dev), [], [], [], depth, height, write)
    hints, offs, lens = hint._pack(files)
    return build_packed(hints, offs, lens, chunk_ids, depth, height, write, None, workspace)


# ---- queries over a built tree (include/qlzx_htree_get.h) ----
@dataclass
class HTreeImage:
    """A tree as the query calls take it: the .hash image and the exclusive scan of its leaves'
    item counts, both on the device."""
    file: torch.Tensor        # uint8 (device): the .hash file's bytes; move() rewrites positions in place
    leaf_first: torch.Tensor  # int32 [nleaf + 1] (device)
    n_items: int
    depth: int
    height: int


@dataclass
class HTreeGet:
    status: torch.Tensor     # int32 [n] (device): _lib.HTG_MISS / HTG_FOUND
    chunk: torch.Tensor      # int32 [n] (u32 bits): the chunk stored in the item
    offset: torch.Tensor     # int32 [n] (u32 bits): the record's offset in its chunk
    ver: torch.Tensor        # int32 [n]: negative for an item that records a delete
    vhash: torch.Tensor      # int16 [n] (u16 bits)
    slot: torch.Tensor       # int32 [n] (u32 bits): the item's index in the image, HTG_NO_SLOT for a miss
    totals: tuple            # (found, miss), read back once

    def __iter__(self):
        return iter((self.status, self.chunk, self.offset, self.ver, self.vhash, self.slot, self.totals))


@on_stream
def load_image(file: torch.Tensor, depth: int, height: int = 3, workspace: batch.Workspace | None = None,
               stream=None) -> HTreeImage:
    """HTree.load (store/htree.go:107-144) of a .hash file in device memory: its leaf_first
    (qlzx_htree_index).  Raises QlzxError naming the leaf where the reference's reader fails, or
    whose length is no whole number of items (HTG_BAD_FILE).  totals[4] is read back."""
    L = _lib.lib()
    _, nleaf = geometry(depth, height)
    dev = file.device
    if file.data_ptr() % 16 or not file.is_contiguous():     # the calls load aligned dwords from the image
        file = file.clone(memory_format=torch.contiguous_format)
    leaf_first = torch.empty(nleaf + 1, dtype=torch.int32, device=dev)
    totals = torch.zeros(4, dtype=torch.int32, device=dev)
    ws_bytes = L.qlzx_htree_index_workspace_size(height)
    ws = (workspace or batch.Workspace(dev)).get(ws_bytes)
    _lib.check(L.qlzx_htree_index(ptr(file), int(file.numel()), depth, height, leaf_first.data_ptr(),
                                  totals.data_ptr(), ws.data_ptr(), ws_bytes, batch._stream()), "qlzx_htree_index")
    t = _dev.readback(totals)                       # the read-back
    if int(t[_lib.HTG_STATUS]) != _lib.HTG_OK:
        raise _lib.QlzxError(f"qlzx_htree_index: HTG_BAD_FILE, leaf {int(t[_lib.HTG_STATUS_LEAF])}")
    return HTreeImage(file, leaf_first, int(t[_lib.HTG_ITEMS]), depth, height)


@on_stream
def get(tree: HTreeImage, keys: batch.BlockBatch | None = None, keyhash: torch.Tensor | None = None,
        workspace: batch.Workspace | None = None, stream=None, _shape: str | None = None) -> HTreeGet:
    """HTree.get of every key (qlzx_htree_get): the lowest item of the key's leaf whose stored low
    bytes equal the keyhash's.  keyhash (int64 [n]) replaces the default hash of `keys`, which may
    then be None.  The results stay on the device; the two totals are read back.  `offset` widened
    to int64 is what replay.read_records takes.  _shape ("lane" / "wave") names the kernel, for
    tests and sweeps: the outputs do not depend on it."""
    L = _lib.lib()
    dev = tree.file.device
    if keyhash is not None:
        keyhash = _dev.u64(keyhash, dev)
        n = int(keyhash.numel())
        if keys is not None and keys.n != n:
            raise ValueError("keyhash: one per key")
    elif keys is None:
        raise ValueError("htree.get: keys or keyhash")
    else:
        n = keys.n
    status, chunk, offset, ver, slot = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(5))
    vhash = torch.zeros(n, dtype=torch.int16, device=dev)
    if n == 0:
        return HTreeGet(status, chunk, offset, ver, vhash, slot, (0, 0))
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    ws_bytes = L.qlzx_htree_get_workspace_size(n)
    ws = (workspace or batch.Workspace(dev)).get(ws_bytes)
    flags = {None: 0, "lane": _lib.HTG_F_LANE, "wave": _lib.HTG_F_WAVE}[_shape]
    kd, ko, kl = (ptr(keys.data), ptr(keys.off), ptr(keys.length)) if keys is not None else (None, None, None)
    _lib.check(L.qlzx_htree_get(ptr(tree.file), int(tree.file.numel()), tree.leaf_first.data_ptr(), tree.depth,
                                tree.height, kd, ko, kl, ptr(keyhash), n, flags, status.data_ptr(),
                                chunk.data_ptr(), offset.data_ptr(), ver.data_ptr(), vhash.data_ptr(),
                                slot.data_ptr(), totals.data_ptr(), ws.data_ptr(), ws_bytes, batch._stream()),
               "qlzx_htree_get")
    t = _dev.readback(totals)                       # the read-back
    return HTreeGet(status, chunk, offset, ver, vhash, slot, (int(t[0]), int(t[1])))


@on_stream
def move(tree: HTreeImage, liveness, gc_batch, dst_chunk_ids, stream=None) -> tuple[int, int]:
    """UpdateHtreePos for a whole chunk (qlzx_htree_move): every record that gc.liveness() called
    NEWEST and gc.rewrite_batch() wrote gets its new position into its item of tree.file, in
    place.  dst_chunk_ids[c] is the real chunk id of gc_batch's destination chunk c.  Returns
    (moved, skipped), read back."""
    L = _lib.lib()
    dev = tree.file.device
    n = int(liveness.verdict.numel())
    if int(gc_batch.status.numel()) != n:
        raise ValueError("move: liveness and gc_batch are of the same records")
    ids = _dev.u32(list(dst_chunk_ids), dev)
    if n == 0 or ids.numel() == 0:
        return 0, 0
    result = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    ws_bytes = L.qlzx_htree_move_workspace_size(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(L.qlzx_htree_move(ptr(tree.file), int(tree.file.numel()), tree.leaf_first.data_ptr(), tree.depth,
                                 tree.height, result.data_ptr(), n, liveness.verdict.data_ptr(),
                                 gc_batch.status.data_ptr(), liveness.slot.data_ptr(), gc_batch.new_chunk.data_ptr(),
                                 gc_batch.new_off.data_ptr(), ids.data_ptr(), int(ids.numel()), totals.data_ptr(),
                                 ws.data_ptr(), ws_bytes, batch._stream()), "qlzx_htree_move")
    t = _dev.readback(totals)                       # the read-back
    return int(t[_lib.HTM_MOVED]), int(t[_lib.HTM_SKIPPED])
