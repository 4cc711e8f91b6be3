"""Write-side record encode on the GPU.

Host mirror of the set path between a value arriving and its bytes reaching a
.data chunk:

  Record.TryCompress     store/item.go:120-161  (policy: ver >= 0, no client /
                         compress flag, padded record > 256 B, MIME sniff, a
                         10 KiB trial compress kept when float32(c)/float32(t) <= 0.7,
                         then the whole body)
  NeedCompress           store/item.go:114-118 + NotCompress defaults
                         (store/config_default.go:46-49: audio/wave, audio/mpeg)
  WriteRecord.encodeHeader / getCRC / append   store/datafile.go:66-88, 307-330

The compress runs in qlzx_compress_batch with the value CRC fused (raw state 0),
and the header+key prefix is folded in with qlzx_crc32_combine, because the
header carries the compressed size.  Records come out 256-B padded and laid
out back to back, ready to append.

encode() drives the policy on the host in numpy; encode_batch() is the same step through the C
ABI's qlzx_write_plan / qlzx_write_decide / qlzx_write_finish, with the policy, the sizes, the
offsets and the CRCs kept on the device.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _dev, _lib, batch

# the record format, defined here for the whole package
HDR = 24                   # store/datafile.go:66-88: crc, ts, flag, ver, ksz, vsz
PADDING = 256              # store/item.go:20
FLAG_COMPRESS = 0x00010000
FLAG_CLIENT_COMPRESS = 0x00000010
MAX_KEY_LEN = 250          # config/mc_config.go:6
BODY_MAX = 50 << 20        # config/mc_config.go:7 ("50M")
TRY_COMPRESS_SIZE = 10 * 1024
COMPRESS_RATIO_LIMIT = np.float32(0.7)
NOT_COMPRESS = frozenset({"audio/wave", "audio/mpeg"})


# conf/global.yaml:29-33 (the shipped hstore.data.not_compress); the defaults of
# store/config_default.go:46-49 are NOT_COMPRESS.
NOT_COMPRESS_SHIPPED = frozenset({"audio/mpeg", "audio/wave", "audio/ogg", "audio/midi"})

# The audio/video rows of Go 1.13's http.DetectContentType table (net/http/sniff.go, go.mod:
# go 1.13), in table order: (mask, pattern, answer).  Every row before them needs a
# different first byte ('<' after optional whitespace for HTML/XML, '%', a BOM, or an image
# signature: \x00\x00\x01/\x02\x00, "BM", "GIF8", "RIFF....WEBPVP", \x89PNG, \xFF\xD8\xFF), and
# "RIFF....WEBPVP" differs from the RIFF rows here at offset 8, so none shadows these.
_AV_SIGS = (
    (b"\xFF\xFF\xFF\xFF", b".snd", "audio/basic"),
    (b"\xFF\xFF\xFF\xFF\x00\x00\x00\x00\xFF\xFF\xFF\xFF", b"FORM\x00\x00\x00\x00AIFF", "audio/aiff"),
    (b"\xFF\xFF\xFF", b"ID3", "audio/mpeg"),
    (b"\xFF\xFF\xFF\xFF\xFF", b"OggS\x00", "application/ogg"),   # never "audio/ogg"
    (b"\xFF\xFF\xFF\xFF\xFF\xFF\xFF\xFF", b"MThd\x00\x00\x00\x06", "audio/midi"),
    (b"\xFF\xFF\xFF\xFF\x00\x00\x00\x00\xFF\xFF\xFF\xFF", b"RIFF\x00\x00\x00\x00AVI ", "video/avi"),
    (b"\xFF\xFF\xFF\xFF\x00\x00\x00\x00\xFF\xFF\xFF\xFF", b"RIFF\x00\x00\x00\x00WAVE", "audio/wave"),
)


def sniff(prefix: bytes) -> str | None:
    """The http.DetectContentType answers a NotCompress set of audio types can act on
    (store/item.go:114-118): the masked audio/video signatures of Go 1.13's sniff table.
    None = some other answer (text, HTML, images, archives, octet-stream), which no audio
    entry of NotCompress matches.  Go answers "application/ogg" for Ogg data, so the
    shipped "audio/ogg" entry never fires (store/item_test.go:19 expects exactly that)."""
    p = prefix[:512]
    for mask, pat, ct in _AV_SIGS:
        if len(p) >= len(pat) and all((p[k] & mask[k]) == pat[k] for k in range(len(pat))):
            return ct
    return None


def need_compress(prefix: bytes, not_compress=NOT_COMPRESS) -> bool:
    """store/item.go:114-118."""
    return sniff(prefix) not in not_compress


@dataclass
class Encoded:
    data: torch.Tensor        # uint8 device buffer: the records, back to back
    offset: np.ndarray        # uint64 record offsets
    flag: np.ndarray          # uint32 flags as written (FLAG_COMPRESS added where kept)
    vsz: np.ndarray           # uint32 stored value sizes
    crc: np.ndarray           # uint32 record CRCs


def sniff_many(heads: np.ndarray, lens: np.ndarray, not_compress=NOT_COMPRESS) -> np.ndarray:
    """need_compress for many values at once: heads = the first bytes of each value (uint8
    [n, >= 12]), lens = the value lengths.  Same rows, order and masks as sniff()."""
    n = len(lens)
    undecided = np.ones(n, bool)
    skip = np.zeros(n, bool)
    for mask, pat, name in _AV_SIGS:   # the first matching row decides, as in sniff()
        k = len(pat)
        m = np.frombuffer(mask, np.uint8)[None, :]
        hit = undecided & (lens >= k) & np.all((heads[:, :k] & m) == np.frombuffer(pat, np.uint8)[None, :], axis=1)
        if name in not_compress:
            skip |= hit
        undecided &= ~hit
    if None in not_compress:   # "some other answer" listed: every value without an audio/video row
        skip |= undecided
    return ~skip


@_dev.on_stream
def encode(keys: list[bytes], values: batch.BlockBatch, flags=None, vers=None, ts=None,
           not_compress=NOT_COMPRESS, workspace: batch.Workspace | None = None, stream=None) -> Encoded:
    """TryCompress + encodeHeader + padding for n records whose values live on the device.
    Every per-record step is a device batch or a numpy array operation (no per-record host loop)."""
    L = _lib.lib()
    dev = values.data.device
    n = values.n
    ws = workspace or batch.Workspace(dev)
    flags = np.zeros(n, np.uint32) if flags is None else np.asarray(flags, np.uint32).copy()
    vers = np.zeros(n, np.int32) if vers is None else np.asarray(vers, np.int32)
    ts = np.zeros(n, np.uint32) if ts is None else np.asarray(ts, np.uint32)
    vlen = _dev.readback(values.length).astype(np.int64)
    voff = values.off.cpu().numpy().view(np.uint64)
    klen = np.fromiter(map(len, keys), np.int64, count=n)

    # ---- TryCompress candidates (store/item.go:121-137) ----
    padded = (HDR + klen + vlen + 255) // 256 * 256
    cand = (vers >= 0) & ((flags & (FLAG_CLIENT_COMPRESS | FLAG_COMPRESS)) == 0) & (padded > PADDING)
    ci = np.nonzero(cand)[0]
    if len(ci):
        # MIME sniff (item.go:114-118) on the first bytes of each candidate, gathered from the device
        ok = sniff_many(_gather_heads(values, ci, 16), vlen[ci], not_compress)
        ci = ci[ok]
    is_comp = np.zeros(n, bool)
    c_src = np.zeros(n, np.int8)      # 0: the trial's output buffer, 1: the full compress's
    c_off = np.zeros(n, np.uint64)
    c_len = np.zeros(n, np.int64)
    c_crc = np.zeros(n, np.uint32)    # raw CRC (state 0) of the compressed value
    bufs = [None, None]
    if len(ci):
        tlen = np.minimum(vlen[ci], TRY_COMPRESS_SIZE)
        trial = batch.BlockBatch(values.data, _dev.u64(voff[ci], dev), _dev.u32(tlen, dev))
        crc0 = torch.zeros(len(ci), dtype=torch.int32, device=dev)
        tdst, tcs, tst, tcrc = batch.compress(trial, crc_state=crc0, max_len=int(tlen.max()), workspace=ws)
        tcs_h = _dev.readback(tcs).astype(np.int64)
        if int((tst != 0).sum()):
            raise _lib.QlzxError("trial compress failed on the device")
        keep = (tcs_h.astype(np.float32) / tlen.astype(np.float32)) <= COMPRESS_RATIO_LIMIT   # :145
        full = keep & (vlen[ci] > tlen)      # :149-156: recompress the whole body
        kt = keep & ~full
        bufs[0] = tdst.data
        r = ci[kt]
        is_comp[r] = True
        c_off[r] = tdst.off.cpu().numpy().view(np.uint64)[kt]
        c_len[r] = tcs_h[kt]
        c_crc[r] = _dev.readback(tcrc)[kt] ^ np.uint32(0xFFFFFFFF)
        fi = ci[full]
        if len(fi):
            fsrc = batch.BlockBatch(values.data, _dev.u64(voff[fi], dev), _dev.u32(vlen[fi], dev))
            fcrc0 = torch.zeros(len(fi), dtype=torch.int32, device=dev)
            fdst, fcs, fst, fcrc = batch.compress(fsrc, crc_state=fcrc0, max_len=int(vlen[fi].max()),
                                                 workspace=ws)
            if int((fst != 0).sum()):
                raise _lib.QlzxError("compress failed on the device")
            bufs[1] = fdst.data
            is_comp[fi] = True
            c_src[fi] = 1
            c_off[fi] = fdst.off.cpu().numpy().view(np.uint64)
            c_len[fi] = _dev.readback(fcs).astype(np.int64)
            c_crc[fi] = _dev.readback(fcrc) ^ np.uint32(0xFFFFFFFF)
    # ---- stored value sizes / flags ----
    vsz = np.where(is_comp, c_len, vlen)
    flags = flags + np.where(is_comp, np.uint32(FLAG_COMPRESS), np.uint32(0)).astype(np.uint32)   # :159
    # ---- raw CRC (from state 0) of every stored value ----
    raw_v = c_crc.copy()
    plain = np.nonzero(~is_comp)[0]
    if len(plain):
        c = batch.crc32(batch.BlockBatch(values.data, _dev.u64(voff[plain], dev), _dev.u32(vlen[plain], dev)),
                        init=torch.zeros(len(plain), dtype=torch.int32, device=dev), final_xor=0)
        raw_v[plain] = _dev.readback(c)
    # ---- header[4:24] || key prefixes (16-B aligned staging), their raw CRC state from ~0, and
    # the combine with the value's raw CRC (datafile.go:66-76) ----
    pre_len = (20 + klen).astype(np.int64)
    pre_step = (pre_len + 15) // 16 * 16
    pre_off = np.zeros(n, np.int64)
    if n:
        pre_off[1:] = np.cumsum(pre_step)[:-1]
    pre = np.zeros(int(pre_step.sum()) if n else 0, np.uint8)
    tail = np.zeros(n, dtype=[("ts", "<u4"), ("flag", "<u4"), ("ver", "<i4"), ("ksz", "<u4"), ("vsz", "<u4")])
    tail["ts"], tail["flag"], tail["ver"], tail["ksz"], tail["vsz"] = ts, flags, vers, klen, vsz
    if n:
        pre[(pre_off[:, None] + np.arange(20)[None, :]).reshape(-1)] = tail.view(np.uint8).reshape(n, 20).reshape(-1)
        kall = np.frombuffer(b"".join(keys), np.uint8)
        if kall.size:
            kstart = np.zeros(n, np.int64)
            kstart[1:] = np.cumsum(klen)[:-1]
            pre[np.repeat(pre_off + 20 - kstart, klen) + np.arange(kall.size)] = kall
    pre_d = torch.from_numpy(pre).to(dev)
    s_hk = batch.crc32(batch.BlockBatch(pre_d, _dev.u64(pre_off, dev), _dev.u32(pre_len, dev)), final_xor=0)
    crc_d = torch.zeros(n, dtype=torch.int32, device=dev)
    rv = _dev.u32(raw_v, dev)
    lv = _dev.u32(vsz, dev)
    _lib.check(L.qlzx_crc32_combine(s_hk.data_ptr(), rv.data_ptr(), lv.data_ptr(), n, 0xFFFFFFFF,
                                    crc_d.data_ptr(), batch._stream()), "qlzx_crc32_combine")
    crc = _dev.readback(crc_d).copy()
    # ---- assemble: crc || header tail || key || value, zero padding to 256 (datafile.go:307-330) ----
    rsize = (HDR + klen + vsz + 255) // 256 * 256
    roff = np.zeros(n, np.uint64)
    if n:
        roff[1:] = np.cumsum(rsize)[:-1]
    total = int(rsize.sum())
    out = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)
    # header tail + key (from the prefix staging) at off + 4
    batch.copy_blocks(pre_d, pre_off, pre_len, out, roff + 4)
    # values: raw ones from the value buffer, compressed ones from their compress buffers
    voff_out = roff + HDR + klen.astype(np.uint64)
    if len(plain):
        batch.copy_blocks(values.data, voff[plain], vlen[plain], out, voff_out[plain])
    for b in (0, 1):
        rs = np.nonzero(is_comp & (c_src == b))[0]
        if len(rs):
            batch.copy_blocks(bufs[b], c_off[rs], c_len[rs], out, voff_out[rs])
    # crc field (records are 256-B aligned, so int32 words)
    out.view(torch.int32)[_dev.u64(roff // 4, dev)] = crc_d
    return Encoded(out[:total], roff, flags, vsz.astype(np.uint32), crc)


def not_compress_mask(not_compress) -> int:
    """The QLZX_NC_* mask of a NotCompress set: one bit per row of _AV_SIGS whose answer is
    listed, and NC_OTHER when None ("some other answer") is."""
    mask = 0
    for k, (_, _, name) in enumerate(_AV_SIGS):
        if name in not_compress:
            mask |= 1 << k
    if None in not_compress:
        mask |= _lib.NC_OTHER
    return mask


@dataclass
class EncodedBatch:
    """encode_batch's result; every tensor lives on the device."""
    data: torch.Tensor        # uint8: the records back to back from offset 0 (capacity: the plan's bound)
    offset: torch.Tensor      # int64 record offsets (0 for a record not written)
    flag: torch.Tensor        # int32 flags as written (FLAG_COMPRESS added where kept)
    vsz: torch.Tensor         # int32 stored value sizes
    crc: torch.Tensor         # int32 record CRCs
    status: torch.Tensor      # int32 enum qlzx_write_status
    vhash: torch.Tensor       # int32 Getvhash of the original value
    totals: torch.Tensor      # int32 [3]: records written, bytes written (lo, hi)
    tried: torch.Tensor       # int32 record indices of the trial list (TryCompress's candidates), in order
    counts: tuple[int, int, int, int] = (0, 0, 0, 0)   # OK records, ntry, nkeep, nfull (the two read-backs)


@_dev.on_stream
def encode_batch(keys: batch.BlockBatch, values: batch.BlockBatch, flags=None, vers=None, ts=None,
                 not_compress=NOT_COMPRESS, max_key: int = MAX_KEY_LEN, body_max: int = BODY_MAX,
                 workspace: batch.Workspace | None = None, stream=None, out: torch.Tensor | None = None,
                 out_cap: int | None = None) -> EncodedBatch:
    """TryCompress + encodeHeader + padding for n records whose keys and values live on the device
    (qlzx_write_plan, qlzx_write_decide, qlzx_write_finish around two qlzx_compress_batch calls).
    Sizes, flags, offsets and CRCs stay on the device; the host reads back the plan's and the
    decision's totals only, to size the compress launches and the buffers.  `out` / `out_cap`
    (optional) give the destination and the bytes of it that may be written."""
    L = _lib.lib()
    dev = values.data.device
    n = values.n
    if keys.n != n:
        raise ValueError("keys: one per value")
    ws = workspace or batch.Workspace(dev)
    st_ = batch._stream()
    cap = max(n, 1)
    flags, vers, ts = (torch.zeros(cap, dtype=torch.int32, device=dev) if a is None else _dev.i32(a, dev)
                       for a in (flags, vers, ts))
    i32 = lambda k=cap: torch.empty(k, dtype=torch.int32, device=dev)   # noqa: E731
    i64 = lambda k=cap: torch.empty(k, dtype=torch.int64, device=dev)   # noqa: E731
    status, try_idx, try_off, try_len, try_dst = i32(), i32(), i64(), i32(), i64()
    totals = torch.zeros(7, dtype=torch.int32, device=dev)
    ws_bytes = L.qlzx_write_plan_workspace_size(n)
    wsp = lambda: ws.get(ws_bytes).data_ptr()   # noqa: E731  (the compress calls may grow the workspace)
    _lib.check(L.qlzx_write_plan(values.data.data_ptr(), values.off.data_ptr(), values.length.data_ptr(),
                                 keys.length.data_ptr(), flags.data_ptr(), vers.data_ptr(), n, max_key, body_max,
                                 not_compress_mask(not_compress), status.data_ptr(), try_idx.data_ptr(),
                                 try_off.data_ptr(), try_len.data_ptr(), try_dst.data_ptr(), totals.data_ptr(),
                                 wsp(), ws_bytes, st_), "qlzx_write_plan")
    t = _dev.readback(totals)                              # read-back 1: sizes the trial compress
    nok, ntry, max_try = int(t[0]), int(t[1]), int(t[2])
    trial_bytes, bound = _dev.wide(t, 3), _dev.wide(t, 5)
    tbuf = tcs = tst = tcrc = None
    if ntry:
        tbuf = torch.empty(trial_bytes, dtype=torch.uint8, device=dev)
        trial = batch.BlockBatch(values.data, try_off[:ntry], try_len[:ntry])
        _, tcs, tst, tcrc = batch.compress(trial, batch.BlockBatch(tbuf, try_dst[:ntry], try_len[:ntry]),
                                           crc_state=torch.zeros(ntry, dtype=torch.int32, device=dev),
                                           max_len=max_try, workspace=ws)
    else:
        tcs, tst, tcrc = i32(1), i32(1), i32(1)
    keep = torch.empty(cap, dtype=torch.uint8, device=dev)
    full_idx, full_off, full_len, full_dst = i32(), i64(), i32(), i64()
    totals2 = torch.zeros(5, dtype=torch.int32, device=dev)
    _lib.check(L.qlzx_write_decide(values.off.data_ptr(), values.length.data_ptr(), n, totals.data_ptr(),
                                   try_idx.data_ptr(), try_len.data_ptr(), tcs.data_ptr(), tst.data_ptr(),
                                   keep.data_ptr(), full_idx.data_ptr(), full_off.data_ptr(), full_len.data_ptr(),
                                   full_dst.data_ptr(), totals2.data_ptr(), wsp(), ws_bytes, st_),
               "qlzx_write_decide")
    t2 = _dev.readback(totals2)                            # read-back 2: sizes the full compress
    nkeep, nfull, max_full = int(t2[0]), int(t2[1]), int(t2[2])
    full_bytes = _dev.wide(t2, 3)
    fbuf = None
    if nfull:
        fbuf = torch.empty(full_bytes, dtype=torch.uint8, device=dev)
        fsrc = batch.BlockBatch(values.data, full_off[:nfull], full_len[:nfull])
        _, fcs, fst, fcrc = batch.compress(fsrc, batch.BlockBatch(fbuf, full_dst[:nfull], full_len[:nfull]),
                                           crc_state=torch.zeros(nfull, dtype=torch.int32, device=dev),
                                           max_len=max_full, workspace=ws)
    else:
        fcs, fst, fcrc = i32(1), i32(1), i32(1)
    if out is None:
        out = torch.empty(max(bound, 16), dtype=torch.uint8, device=dev)
    if out_cap is None:
        out_cap = int(out.numel())
    rec_off, flag_out, vsz, crc = i64(), i32(), i32(), i32()
    vh16 = torch.empty(cap, dtype=torch.int16, device=dev)
    totals3 = torch.zeros(3, dtype=torch.int32, device=dev)
    _lib.check(L.qlzx_write_finish(values.data.data_ptr(), values.off.data_ptr(), values.length.data_ptr(),
                                   keys.data.data_ptr(), keys.off.data_ptr(), keys.length.data_ptr(),
                                   flags.data_ptr(), vers.data_ptr(), ts.data_ptr(), n, totals.data_ptr(),
                                   try_idx.data_ptr(), try_len.data_ptr(), try_dst.data_ptr(), tcs.data_ptr(),
                                   tcrc.data_ptr(), keep.data_ptr(), _dev.ptr(tbuf), totals2.data_ptr(),
                                   full_idx.data_ptr(), full_dst.data_ptr(), fcs.data_ptr(), fst.data_ptr(),
                                   fcrc.data_ptr(), _dev.ptr(fbuf), out.data_ptr(), out_cap, status.data_ptr(),
                                   rec_off.data_ptr(), flag_out.data_ptr(), vsz.data_ptr(), crc.data_ptr(),
                                   vh16.data_ptr(), totals3.data_ptr(), wsp(), ws_bytes, st_), "qlzx_write_finish")
    return EncodedBatch(out, rec_off[:n], flag_out[:n], vsz[:n], crc[:n], status[:n],
                        vh16[:n].to(torch.int32) & 0xFFFF, totals3, try_idx[:ntry], (nok, ntry, nkeep, nfull))


_copy = batch.copy_blocks   # the name tools/bench_read.py calls


def _gather_heads(values: batch.BlockBatch, idx: np.ndarray, k: int) -> np.ndarray:
    """The first k bytes of each selected value (zeros past its end), uint8 [len(idx), k]."""
    dev = values.data.device
    sel = _dev.u64(idx, dev)
    off = values.off[sel]
    ln = values.length[sel].to(torch.int64)
    ar = torch.arange(k, device=dev)
    pos = torch.minimum(off.unsqueeze(1) + ar.unsqueeze(0), torch.tensor(values.data.numel() - 1, device=dev))
    h = values.data[pos.reshape(-1)].reshape(len(idx), k)
    return torch.where(ar.unsqueeze(0) < ln.unsqueeze(1), h, torch.zeros_like(h)).cpu().numpy()
