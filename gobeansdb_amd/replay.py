"""Batched replay of a .data chunk on the GPU (SURVEY §8 f1 + f2).

Host mirror of buildHintFromData (store/bucket.go:89-117) over a chunk file
resident in device memory: record discovery with DataStreamReader's nextValid
resync and CRC verify (store/datafile.go:114-277, qlzx_replay_index), value
decompress of FLAG_COMPRESS records (Payload.Decompress, store/item.go:163-176,
errors swallowed as in the reference: the body stays compressed) and the value
hash Getvhash (store/item.go:89-100, qlzx_vhash_batch).  torch tensors are the
device memory; every byte of work runs in libqlzx.so.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _dev, _lib, batch
from ._dev import on_stream, ptr
from .record import BODY_MAX, FLAG_COMPRESS, HDR, MAX_KEY_LEN


def _value(r, j: int) -> bytes:
    """Entry j's value after Payload.Decompress (store/item.go:163-176), of a ReplayResult or a
    ReadResult: the decoded bytes, or the raw body where the record is not compressed or its
    decode failed."""
    o, n = int(r.val_off[j]), int(r.value_len[j])
    src = r.values.data if int(r.in_out[j]) else r.data
    return src[o:o + n].cpu().numpy().tobytes()


@dataclass
class ReplayResult:
    offset: torch.Tensor       # int64 [n] record offsets in the chunk
    size_broken: torch.Tensor  # int32 [n] bytes skipped by the nextValid resync before each record
    header: torch.Tensor       # int32 [n, 6]: crc, ts, flag, ver, ksz, vsz (as stored)
    flag: torch.Tensor         # int32 [n] flag after Payload.Decompress
    value_len: torch.Tensor    # int32 [n] value length after decompress
    vhash: torch.Tensor        # int32 [n] Getvhash of the value (uint16)
    # The FLAG_COMPRESS records only, in record order: their decoder outputs in one packed buffer
    # (lengths = the QuickLZ header dsize, meaningless for a record whose decode failed).  Read a
    # record's value through in_out / val_off (or value(j)), not by position in here.
    values: batch.BlockBatch
    end_error: bool            # the reader stopped on an unexpected EOF after these records
    n_candidates: int
    n_valid: int
    in_out: torch.Tensor       # uint8 [n]: 1 = value in values.data at val_off, 0 = in the chunk at val_off
    val_off: torch.Tensor      # int64 [n] value offset (decoded buffer or chunk, per in_out)
    data: torch.Tensor         # the chunk replayed (val_off's base where in_out is 0)

    @property
    def n(self) -> int:
        return int(self.offset.numel())

    value = _value

    @on_stream
    def value_crcs(self, stream=None) -> torch.Tensor:
        """crc32 (store/crc32.go get) of every record's value after Payload.Decompress, on the
        device (int32 [n]); an XOR of them is the parity digest of a replay."""
        out = torch.zeros(self.n, dtype=torch.int32, device=self.offset.device)
        for where, src in ((1, self.values.data), (0, self.data)):
            m = torch.nonzero(self.in_out == where).flatten()
            if m.numel():
                out[m] = batch.crc32(batch.BlockBatch(src, self.val_off[m], self.value_len[m]))
        return out


def _ptrs(tensors) -> list[int]:
    return [t.data_ptr() for t in tensors]


@dataclass
class _Plan:
    """What qlzx_replay_plan / qlzx_read_plan fill: the stored headers, and per FLAG_COMPRESS
    record its entry, its body in the chunk, the dsize of its QuickLZ header and its place in the
    decoder output; totals = (entries, compressed ones, largest dsize, output bytes lo, hi)."""
    hdr: torch.Tensor
    comp_idx: torch.Tensor
    comp_off: torch.Tensor
    comp_len: torch.Tensor
    comp_dsize: torch.Tensor
    comp_dst: torch.Tensor
    totals: torch.Tensor

    @classmethod
    def alloc(cls, cap: int, dev) -> "_Plan":
        def empty(dtype, k=cap):
            return torch.empty(k, dtype=dtype, device=dev)
        return cls(empty(torch.int32, cap * 6), empty(torch.int32), empty(torch.int64), empty(torch.int32),
                   empty(torch.int32), empty(torch.int64), torch.zeros(5, dtype=torch.int32, device=dev))

    def ptrs(self) -> list[int]:
        """The addresses of the seven arrays, in the order both plan calls take them."""
        return _ptrs((self.hdr, self.comp_idx, self.comp_off, self.comp_len, self.comp_dsize, self.comp_dst,
                      self.totals))


def _decode_planned(data: torch.Tensor, p: _Plan, cap: int, ws: batch.Workspace):
    """The middle of replay() and read_records(), after the plan call: the one read-back (it sizes
    the output buffer and the decoder launch) and the decode of the planned records.  Returns
    (entries, compressed ones, largest dsize, output bytes), the decoder's output, what a finish
    call reads of it (comp_idx, status, dsize, comp_dst, output: the order both take them in) and
    the five arrays it fills (flag, value_len, in_out, val_off, vh16)."""
    dev = data.device
    t = _dev.readback(p.totals)
    ncomp, maxd, out_bytes = int(t[1]), int(t[2]), _dev.wide(t, 3)
    out = torch.empty(out_bytes + 64, dtype=torch.uint8, device=dev)
    cst = torch.zeros(max(ncomp, 1), dtype=torch.int32, device=dev)
    cds = torch.zeros(max(ncomp, 1), dtype=torch.int32, device=dev)
    values = batch.BlockBatch(out, p.comp_dst[:ncomp], p.comp_dsize[:ncomp])
    if ncomp:
        csrc = batch.BlockBatch(data, p.comp_off[:ncomp], p.comp_len[:ncomp])
        cds, cst, _ = batch.decompress(csrc, values, dst_cap=p.comp_dsize[:ncomp], max_dsize=maxd, workspace=ws)
    decoded = [p.comp_idx, cst, cds, p.comp_dst, out]
    fin = [torch.empty(cap, dtype=dt, device=dev)
           for dt in (torch.int32, torch.int32, torch.uint8, torch.int64, torch.int16)]
    return (int(t[0]), ncomp, maxd, out_bytes), values, decoded, fin


def _index_device(data: torch.Tensor, start: int, max_key: int, body_max: int, ws: batch.Workspace):
    """qlzx_replay_index launched on the current stream: (rec_off, rec_broken, result), all on the
    device, with room for size // 256 + 1 records; result = (n, end_error, ncand, nvalid)."""
    L = _lib.lib()
    dev = data.device
    size = int(data.numel())
    cap = size // 256 + 1
    rec_off = torch.empty(cap, dtype=torch.int64, device=dev)
    rec_broken = torch.empty(cap, dtype=torch.int32, device=dev)
    result = torch.zeros(4, dtype=torch.int32, device=dev)
    ws_bytes = L.qlzx_replay_workspace_size(size)
    _lib.check(L.qlzx_replay_index(ptr(data), size, start, max_key, body_max, rec_off.data_ptr(),
                                   rec_broken.data_ptr(), result.data_ptr(), ws.get(ws_bytes).data_ptr(), ws_bytes,
                                   batch._stream()), "qlzx_replay_index")
    return rec_off, rec_broken, result


@on_stream
def index(data: torch.Tensor, start: int = 0, max_key: int = MAX_KEY_LEN, body_max: int = BODY_MAX,
          workspace: batch.Workspace | None = None, stream=None):
    """Records DataStreamReader.Next would return from `start`: (offsets, sizeBroken, end_error, ncand, nvalid)."""
    rec_off, rec_broken, result = _index_device(data, start, max_key, body_max,
                                                workspace or batch.Workspace(data.device))
    r = result.cpu().numpy()
    n = int(r[0])
    return rec_off[:n], rec_broken[:n], bool(r[1]), int(r[2]), int(r[3])


@on_stream
def replay(data: torch.Tensor, start: int = 0, max_key: int = MAX_KEY_LEN, body_max: int = BODY_MAX,
           workspace: batch.Workspace | None = None, stream=None) -> ReplayResult:
    """Index, plan, decompress, finish: every per-record step runs on the device
    (qlzx_replay_index / qlzx_replay_plan / qlzx_decompress_batch / qlzx_replay_finish); the
    host reads back five numbers once (record and compressed counts, the largest dsize and the
    output size), which size the output buffer and the decoder launch."""
    L = _lib.lib()
    dev = data.device
    ws = workspace or batch.Workspace(dev)
    st_ = batch._stream()
    rec_off, rec_broken, result = _index_device(data, start, max_key, body_max, ws)
    cap = int(rec_off.numel())
    p = _Plan.alloc(cap, dev)
    pws = torch.empty(L.qlzx_replay_plan_workspace_size(cap), dtype=torch.uint8, device=dev)
    _lib.check(L.qlzx_replay_plan(ptr(data), rec_off.data_ptr(), result.data_ptr(), cap, *p.ptrs(), pws.data_ptr(),
                                  pws.numel(), st_), "qlzx_replay_plan")
    r = result.cpu().numpy()
    (n, *_), values, decoded, fin = _decode_planned(data, p, cap, ws)
    _lib.check(L.qlzx_replay_finish(ptr(data), rec_off.data_ptr(), result.data_ptr(), p.totals.data_ptr(),
                                    *_ptrs(decoded), cap, *_ptrs(fin), st_), "qlzx_replay_finish")
    flag, value_len, in_out, val_off, vh16 = (x[:n] for x in fin)
    return ReplayResult(rec_off[:n], rec_broken[:n], p.hdr[: 6 * n].view(n, 6), flag, value_len,
                        vh16.to(torch.int32) & 0xFFFF, values, bool(r[1]), int(r[2]), int(r[3]), in_out, val_off, data)


@dataclass
class HostReplayPart:
    """What the pipelined replay of one part leaves in host (pinned) memory.

    want="values": the per-record fields a reader of the values needs (offset, stored header,
    flag and length after Payload.Decompress, in_out / val_off, vhash) and the decoder's output
    buffer; a value with in_out 0 is the part's own bytes at val_off (the host already holds them).
    want="hints": buildHintFromData's fields only (store/bucket.go:89-117: the decompressed body
    only feeds Getvhash and is freed): offset, stored header, vhash."""
    n: int
    end_error: bool
    offset: torch.Tensor
    header: torch.Tensor
    vhash: torch.Tensor
    flag: torch.Tensor | None = None
    value_len: torch.Tensor | None = None
    in_out: torch.Tensor | None = None
    val_off: torch.Tensor | None = None
    values: torch.Tensor | None = None

    def value(self, part: torch.Tensor | np.ndarray, j: int) -> memoryview:
        """Record j's value after Payload.Decompress, from host memory (the decoder output copied
        back, or the part itself)."""
        o, n = int(self.val_off[j]), int(self.value_len[j])
        src = self.values if int(self.in_out[j]) else part
        a = src.numpy() if isinstance(src, torch.Tensor) else src
        return memoryview(a)[o:o + n]


class ReplayPipeline:
    """Replay of .data streams held in pinned host memory (chunk files read from disk),
    pipelined over three streams: pinned H2D of part i+1 || replay of part i || pinned D2H of
    part i-1's results (PCIe is full duplex), two device slots for the parts.  The streams, slots
    and host buffers are made once, here, for parts of at most `part_cap` bytes; run() then moves
    no allocation into the copy/replay loop (a host buffer only grows when a part needs more).

    want="values": the decompressed values and their per-record fields go back into two pinned
    host slots (`values_cap` bytes of decoder output each to start with), reused every other part.
    want="hints": buildHintFromData's fields only, into `nparts` per-part pinned buffers."""

    def __init__(self, part_cap: int, want: str = "values", device=None, workspace: batch.Workspace | None = None,
                 values_cap: int = 0, nparts: int = 0):
        if want not in ("values", "hints"):
            raise ValueError("want is 'values' or 'hints'")
        self.want = want
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.ws = workspace or batch.Workspace(self.dev)
        self.part_cap = max(int(part_cap), 1)
        self.s_h2d, self.s_cmp, self.s_d2h = (torch.cuda.Stream(self.dev) for _ in range(3))
        self.dslot = [torch.empty(self.part_cap, dtype=torch.uint8, device=self.dev) for _ in range(2)]
        self.ev_in = [torch.cuda.Event(), torch.cuda.Event()]      # part landed in its device slot
        self.ev_used = [torch.cuda.Event(), torch.cuda.Event()]    # replay done with the device slot
        self.ev_out = [torch.cuda.Event(), torch.cuda.Event()]     # D2H into the host slot done
        rec_cap = self.part_cap // 256 + 1                         # records are 256-B aligned
        if want == "values":
            self.host = [self._values_slot(rec_cap, values_cap) for _ in range(2)]
        else:
            self.host = [self._hint_slot(rec_cap) for _ in range(max(nparts, 0))]

    @staticmethod
    def _pinned(n, dtype, shape=None):
        return torch.empty(shape if shape is not None else max(n, 1), dtype=dtype).pin_memory()

    def _values_slot(self, recs, nbytes):
        p = self._pinned
        return dict(cap=recs, values=p(nbytes, torch.uint8), off=p(recs, torch.int64),
                    hdr=p(0, torch.int32, (recs, 6)), vh=p(recs, torch.int32), flag=p(recs, torch.int32),
                    vlen=p(recs, torch.int32), io=p(recs, torch.uint8), voff=p(recs, torch.int64))

    def _hint_slot(self, recs):
        p = self._pinned
        return dict(cap=recs, off=p(recs, torch.int64), hdr=p(0, torch.int32, (recs, 6)), vh=p(recs, torch.int32))

    def run(self, parts: list[torch.Tensor], sink=None) -> list["HostReplayPart | None"]:
        """Replay every part (each a whole .data stream cut at record starts, in pinned memory).
        want="values": `sink(i, HostReplayPart)` (optional) runs once part i's copy has landed and
        before its host slot is reused (the host waits for it: a checking pass); without a sink
        nothing waits, and only the last two parts' results are left valid in the returned list
        (the others are None).  want="hints": every part's result is returned (and passed to
        `sink` at the end if given)."""
        np_ = len(parts)
        out: list[HostReplayPart | None] = [None] * np_
        if np_ == 0:
            return out
        if any(int(q.numel()) > self.part_cap for q in parts):
            raise ValueError("a part is larger than the pipeline's part_cap")
        if self.want == "hints":
            while len(self.host) < np_:
                self.host.append(self._hint_slot(self.part_cap // 256 + 1))
        s_h2d, s_cmp, s_d2h = self.s_h2d, self.s_cmp, self.s_d2h
        dslot, ev_in, ev_used, ev_out = self.dslot, self.ev_in, self.ev_used, self.ev_out
        pend: list[int | None] = [None, None]   # part whose results a host slot holds (sink not run yet)

        def h2d(i):
            dslot[i & 1][: parts[i].numel()].copy_(parts[i], non_blocking=True)
            ev_in[i & 1].record(s_h2d)

        def flush(j):
            i = pend[j]
            if i is not None:
                ev_out[j].synchronize()
                sink(i, out[i])
                pend[j] = None

        with torch.cuda.stream(s_h2d):
            h2d(0)
        for i in range(np_):
            j = i & 1
            if i + 1 < np_:   # prefetch the next part while this one replays
                with torch.cuda.stream(s_h2d):
                    if i >= 1:
                        s_h2d.wait_event(ev_used[j ^ 1])
                    h2d(i + 1)
            with torch.cuda.stream(s_cmp):
                s_cmp.wait_event(ev_in[j])
                r = replay(dslot[j][: parts[i].numel()], workspace=self.ws, stream=s_cmp)
                ev_used[j].record(s_cmp)
            n = r.n
            if self.want == "hints":
                h = self.host[i]
                hp = HostReplayPart(n, r.end_error, h["off"][:n], h["hdr"][:n], h["vh"][:n])
            else:
                if sink is not None:
                    flush(j)
                nb = int(r.values.data.numel())
                h = self.host[j]
                if h["cap"] < n or h["values"].numel() < nb:   # grow (a copy may still target the old one)
                    ev_out[j].synchronize()
                    h = self.host[j] = self._values_slot(max(n, h["cap"]), max(nb, h["values"].numel()))
                hp = HostReplayPart(n, r.end_error, h["off"][:n], h["hdr"][:n], h["vh"][:n], h["flag"][:n],
                                    h["vlen"][:n], h["io"][:n], h["voff"][:n], h["values"][:nb])
                if i >= 2 and sink is None:
                    out[i - 2] = None   # its host slot is reused now
            with torch.cuda.stream(s_d2h):
                s_d2h.wait_event(ev_used[j])
                if i >= 2:
                    s_d2h.wait_event(ev_out[j])
                srcs = [(hp.offset, r.offset), (hp.header, r.header), (hp.vhash, r.vhash)]
                if self.want == "values":
                    srcs += [(hp.flag, r.flag), (hp.value_len, r.value_len), (hp.in_out, r.in_out),
                             (hp.val_off, r.val_off), (hp.values, r.values.data)]
                for dst, src in srcs:
                    if src.numel():
                        dst.copy_(src, non_blocking=True)
                        src.record_stream(s_d2h)
                ev_out[j].record(s_d2h)
            out[i] = hp
            if self.want == "values" and sink is not None:
                pend[j] = i
        if self.want == "values" and sink is not None:
            for j in (((np_ - 2) & 1, (np_ - 1) & 1) if np_ >= 2 else (0,)):
                flush(j)
        for e in ev_out:
            e.synchronize()
        if self.want == "hints" and sink is not None:
            for i, hp in enumerate(out):
                sink(i, hp)
        return out


def replay_pipelined(parts: list[torch.Tensor], want: str = "values", device=None,
                     workspace: batch.Workspace | None = None, sink=None) -> list["HostReplayPart | None"]:
    """One-shot ReplayPipeline(max part size, want).run(parts, sink)."""
    cap = max([int(q.numel()) for q in parts], default=1)
    return ReplayPipeline(cap, want, device, workspace, nparts=len(parts)).run(parts, sink)


def host_value_digest(hp: HostReplayPart, part, key_base: int = 0, file_id: int = 0, threads: int = 16) -> int:
    """XOR over the part's records of crc32 (zlib's = store/crc32.go's) of each value as it sits
    in HOST memory after the pipelined replay, keyed by the record's place like the device-only
    digest: crc ^ ((key_base + offset) * 0x85EBCA77 + (file_id + 1) * 0x9E3779B1) mod 2^32."""
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    n = hp.n
    if n == 0:
        return 0
    off = hp.offset.numpy()
    voff = hp.val_off.numpy()
    vlen = hp.value_len.numpy()
    io = hp.in_out.numpy()
    pa = part.numpy() if isinstance(part, torch.Tensor) else np.asarray(part)
    vals = memoryview(hp.values.numpy())
    raw = memoryview(pa)
    keys = ((key_base + off.astype(np.int64)) * 0x85EBCA77 + (file_id + 1) * 0x9E3779B1) & 0xFFFFFFFF

    def run(lo, hi):
        d = 0
        for j in range(lo, hi):
            o = int(voff[j])
            src = vals if io[j] else raw
            d ^= zlib.crc32(src[o:o + int(vlen[j])]) ^ int(keys[j])
        return d

    t = max(1, min(threads, n // 256 + 1))
    cuts = [n * k // t for k in range(t + 1)]
    with ThreadPoolExecutor(t) as ex:
        parts_ = list(ex.map(lambda k: run(cuts[k], cuts[k + 1]), range(t)))
    d = 0
    for x in parts_:
        d ^= x
    return d


def hint_digest(offset, header, vhash, key_base: int = 0, file_id: int = 0) -> int:
    """XOR over records of a keyed mix of the hint fields (offset, stored header, vhash): the
    parity digest of buildHintFromData's output; torch tensors (host or device) or arrays."""
    def a(x):
        return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    off = a(offset).astype(np.int64) + key_base
    hdr = a(header).astype(np.int64).reshape(-1, 6) & 0xFFFFFFFF
    vh = a(vhash).astype(np.int64) & 0xFFFF
    if off.size == 0:
        return 0
    m = (off * 0x85EBCA77 + (file_id + 1) * 0x9E3779B1) & 0xFFFFFFFF
    for c in range(6):
        m = (m * 0x01000193 ^ hdr[:, c]) & 0xFFFFFFFF
    m = (m * 0x01000193 ^ vh) & 0xFFFFFFFF
    return int(np.bitwise_xor.reduce(m))


@dataclass
class ReadResult:
    """read_records' answer, one entry per request (in request order)."""
    status: torch.Tensor       # int32 [n] _lib.RD_*: readRecordAt's verdict
    key_eq: torch.Tensor | None  # uint8 [n] 1 = OK and the record's key is the wanted one; None without keys
    header: torch.Tensor       # int32 [n, 6]: crc, ts, flag, ver, ksz, vsz as stored (zeros: ALIGN, EOF_HEADER)
    flag: torch.Tensor         # int32 [n] flag after Payload.Decompress (0 for a failed request)
    value_len: torch.Tensor    # int32 [n] value length after decompress
    vhash: torch.Tensor        # int32 [n] Getvhash of the value as delivered (uint16)
    dec_status: torch.Tensor   # int32 [n] the decoder's status of a compressed record (_lib.OK otherwise)
    in_out: torch.Tensor       # uint8 [n]: 1 = value in values.data at val_off, 0 = in the chunk at val_off
    val_off: torch.Tensor      # int64 [n]
    # the decoder outputs of the OK requests with FLAG_COMPRESS, in request order (as ReplayResult.values)
    values: batch.BlockBatch
    data: torch.Tensor         # the chunk read (val_off's base where in_out is 0)
    # the plan's read-back: (requests with status OK, compressed ones among them, their largest
    # dsize, bytes of decoder output) -- what sized values.data and the decoder launch
    totals: tuple[int, int, int, int] = (0, 0, 0, 0)

    @property
    def n(self) -> int:
        return int(self.status.numel())

    def value(self, i: int) -> bytes:
        """Request i's value after Payload.Decompress (the decoded bytes, or the raw body where the
        record is not compressed or its decode failed); ValueError for a request that failed."""
        st = int(self.status[i])
        if st != _lib.RD_OK:
            raise ValueError(f"request {i} failed: {_lib.RD_NAMES[st]}")
        return _value(self, i)


@on_stream
def read_records(data: torch.Tensor, offsets, keys: list[bytes] | None = None, max_key: int = MAX_KEY_LEN,
                 body_max: int = BODY_MAX, workspace: batch.Workspace | None = None, stream=None) -> ReadResult:
    """Many records at positions the caller knows, in one pass (a multi-key GET, GC's collision
    lookups, a hint file's positions): dataChunk.GetRecordByOffset (store/datachunk.go:150-169) for
    every offset of `offsets` (a sequence, an ndarray or an int64 device tensor) over the chunk
    `data` in device memory.  qlzx_read_plan checks each request as readRecordAt does (sizes, then
    the record CRC) and plans the decode of those that passed; the host reads five numbers back
    once, as replay() does; qlzx_decompress_batch decodes the compressed ones (no CRC arguments:
    the record CRC was verified before any QuickLZ header was believed); qlzx_read_finish reports
    per request.  `keys` (optional, one per offset) are compared on the device: key_eq[i] == 0 on
    an OK request is the caller's hash collision (store/bucket.go:452-498), not an error."""
    L = _lib.lib()
    dev = data.device
    ws = workspace or batch.Workspace(dev)
    st_ = batch._stream()
    size = int(data.numel())
    off = _dev.u64(offsets, dev).reshape(-1)
    n = int(off.numel())
    cap = max(n, 1)
    wk = wk_off = wk_len = key_eq = None
    if keys is not None:
        if len(keys) != n:
            raise ValueError("keys: one per offset")
        klen = np.fromiter(map(len, keys), np.int32, count=n)
        koff, _ = batch.pack_offsets(klen, align=1)
        wk = torch.from_numpy(np.frombuffer(b"".join(keys) + b"\0", dtype=np.uint8).copy()).to(dev)
        wk_off, wk_len = _dev.u64(koff, dev), _dev.i32(klen, dev)     # (null pointers when n == 0: not read)
        key_eq = torch.empty(cap, dtype=torch.uint8, device=dev)
    if n == 0:
        off = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.empty(cap, dtype=torch.int32, device=dev)
    p = _Plan.alloc(cap, dev)
    ws_bytes = L.qlzx_read_plan_workspace_size(n)
    _lib.check(L.qlzx_read_plan(ptr(data), size, off.data_ptr(), n, max_key, body_max, ptr(wk), ptr(wk_off),
                                ptr(wk_len), status.data_ptr(), ptr(key_eq), *p.ptrs(), ws.get(ws_bytes).data_ptr(),
                                ws_bytes, st_), "qlzx_read_plan")
    t, values, decoded, fin = _decode_planned(data, p, cap, ws)
    dec = torch.empty(cap, dtype=torch.int32, device=dev)
    _lib.check(L.qlzx_read_finish(ptr(data), off.data_ptr(), n, status.data_ptr(), p.totals.data_ptr(),
                                  *_ptrs(decoded), *_ptrs(fin), dec.data_ptr(), st_), "qlzx_read_finish")
    flag, value_len, in_out, val_off, vh16 = (x[:n] for x in fin)
    return ReadResult(status[:n], None if key_eq is None else key_eq[:n], p.hdr[: 6 * n].view(n, 6), flag, value_len,
                      vh16.to(torch.int32) & 0xFFFF, dec[:n], in_out, val_off, values, data, t)


def read_record(rec: bytes) -> tuple[int, bytes] | None:
    """One record as a GET reads it: readRecordAt's CRC check (store/datafile.go:161-168) and
    Payload.Decompress (store/item.go:163-176) -- header[4:24] and the key through crc32_write
    (the library folds such short slices on the host), then the value's CRC and its decode in ONE
    request (qlzx_read_record1).  Returns (flag after Payload.Decompress, value), or None when the
    record CRC does not match (readRecordAt's error).  As in the reference, a value that fails to
    decode stays compressed with its flag unchanged."""
    import struct
    L = _lib.lib()
    crc, _ts, flag, _ver, ksz, vsz = struct.unpack_from("<IIIiII", rec, 0)
    key = rec[HDR:HDR + ksz]
    val = bytes(rec[HDR + ksz:HDR + ksz + vsz])
    st = L.crc32_write(0xFFFFFFFF, bytes(rec[4:HDR]), 20)
    if ksz:
        st = L.crc32_write(st, bytes(key), ksz)
    comp = bool(flag & FLAG_COMPRESS)
    cap = 0
    if comp and len(val) >= (9 if (val and val[0] & 2) else 3):
        cap = int.from_bytes(val[5:9], "little") if val[0] & 2 else val[2]
    dst = ctypes.create_string_buffer(max(cap, 1))
    out = ctypes.c_size_t(0)
    status = ctypes.c_int32(0)
    _lib.check(L.qlzx_read_record1(val, len(val), st, crc, int(comp), dst, cap, ctypes.byref(out),
                                   ctypes.byref(status)), "qlzx_read_record1")
    if status.value == _lib.E_CRC:
        return None
    if comp and status.value == _lib.OK:
        return flag - FLAG_COMPRESS, dst.raw[:out.value]
    return flag, val
