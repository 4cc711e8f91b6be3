"""GPU: the Go level-1 codec (k_dec_go_l1, k_enc_go_l1, qlzx_level1.hip) on the collection of
tests/go_l1_cases.py: hand-assembled streams for every panic site of quicklz.go Decompress and
every token form no encoder emits, header forms, zero-fill cases, every truncation and bit flip
of the small golden level-1 streams, and plaintexts that force each decision of Compress(src, 1).
tests/test_go_l1_cases.py shows on the host, with an independent model, which site or decision
each case reaches, so a pass here is not vacuous.  Expected values are the oracle's.

  route          entry                                          families
  batch decode   qlzx_go_decompress_batch, with dst_cap         all decoder families
                 the same without dst_cap                       the cases that claim <= 8192 bytes
  single decode  qlzx_go_decompress1, quicklz.Decompress        all but the mutants
  batch encode   qlzx_go_l1_compress_batch                      encoder
  single encode  qlzx_compress1 QLZX_F_LEVEL1, quicklz.Compress encoder

Every destination is filled with 0xA5 first (Go's make([]byte, size) zero-fills; the decoder
must do so itself), blocks sit at every offset mod 16 with guard gaps of at least 64 bytes, and
the zero_fill cases are placed at each of the 16 offsets.  The batch calls run twice on one
workspace that held 0xFF before the first call, the second time with the cases in reverse order,
so every lane's hash table must be zeroed by the lane that uses it."""
import ctypes
import functools
from collections import Counter

import numpy as np
import pytest

import go_l1_cases as C
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GAP = 64
NO_CAP_MAX = 8192          # without dst_cap a block needs room for the size its header claims

DECODE = {"panic_sites": 54, "odd_tokens": 61, "headers": 76, "zero_fill": 26 * 16, "mutants": 50724}
DECODE_NO_CAP = {"panic_sites": 54, "odd_tokens": 61, "headers": 75, "zero_fill": 26 * 16, "mutants": 50298}
SINGLE = {"panic_sites": 54, "odd_tokens": 61, "headers": 76, "zero_fill": 26}
ENCODE = {"encoder": 73}
# the oracle's statuses over the batch: OK, E_CORRUPT, E_LEVEL, E_DST_CAP, E_HEADER
STATUSES = {True: {0: 45519, 2: 4561, 3: 204, 4: 607, 6: 440}, False: {0: 45568, 2: 4692, 3: 204, 6: 440}}


def _cap(c):
    return C.claimed_size(c.stream) if c.cap is None else c.cap


@functools.lru_cache(maxsize=None)
def _want(name: str, capped: bool):
    """(status, bytes) of the oracle for a decoder case; without dst_cap the room is the size."""
    c = _by_name()[name]
    return O.decompress_go_l1(c.stream, cap=_cap(c) if capped else C.claimed_size(c.stream))


@functools.lru_cache(maxsize=None)
def _by_name():
    return {c.name: c for c in C.collection()}


def _decode_entries(capped: bool):
    """(case, forced offset mod 16 or None): every decoder case once, the zero_fill cases at
    each of the 16 offsets."""
    out = []
    for c in C.collection():
        if c.stream is None or (not capped and C.claimed_size(c.stream) > NO_CAP_MAX):
            continue
        out += [(c, a) for a in range(16)] if c.family == "zero_fill" else [(c, None)]
    return out


def _layout(rooms, forced):
    """Offsets with a gap of at least GAP before each block, at every offset mod 16."""
    off, pos = [], 0
    for k, (room, a) in enumerate(zip(rooms, forced)):
        pos = (pos + GAP + 15) // 16 * 16 + (k % 16 if a is None else a)
        off.append(pos)
        pos += room
    return off, pos + GAP + 16


def _decode_batch_once(entries, capped, ws):
    import torch
    from gobeansdb_amd import batch
    sizes = [C.claimed_size(c.stream) for c, _ in entries]
    rooms = [_cap(c) if capped else n for (c, _), n in zip(entries, sizes)]
    doff, total = _layout(rooms, [a for _, a in entries])
    assert {o % 16 for o in doff} == set(range(16))
    src = batch.BlockBatch.from_bytes([c.stream for c, _ in entries])
    data = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    dst = batch.BlockBatch(data, torch.tensor(doff, dtype=torch.int64, device="cuda"),
                           torch.tensor(np.asarray(rooms, np.uint32).view(np.int32), device="cuda"))
    cap_t = torch.tensor(np.asarray(rooms, np.uint32).view(np.int32), device="cuda") if capped else None
    dsize, st = batch.go_decompress(src, dst, dst_cap=cap_t, workspace=ws)
    torch.cuda.synchronize()
    out = data.cpu().numpy()
    st = st.cpu().numpy()
    dsize = dsize.cpu().numpy().view(np.uint32)
    bad = []
    untouched = np.ones(len(out), bool)
    for k, ((c, _), o, n) in enumerate(zip(entries, doff, sizes)):
        wst, wdata = _want(c.name, capped)
        if int(st[k]) != wst:
            bad.append((c.name, "status", int(st[k]), wst))
        elif int(dsize[k]) != (n if wst == O.OK else 0):
            bad.append((c.name, "dsize", int(dsize[k]), n))
        elif wst == O.OK and out[o:o + n].tobytes() != wdata:
            got = out[o:o + n].tobytes()
            bad.append((c.name, "bytes", next(j for j in range(n) if got[j] != wdata[j])))
        if wst in (O.OK, O.E_CORRUPT):      # a panic may leave part of [off, off + size) written
            untouched[o:o + n] = False
    touched = np.nonzero(out[untouched] != GUARD)[0]
    assert not bad, (len(bad), len(entries), bad[:12])
    assert touched.size == 0, ("bytes written outside [off, off + size), or on a refused block", touched[:8])
    return Counter(int(s) for s in st)


@pytest.mark.parametrize("capped,count,expect", [pytest.param(True, 51331, DECODE, id="dst_cap_51331cases"),
                                                 pytest.param(False, 50904, DECODE_NO_CAP, id="no_cap_50904cases")])
def test_batch_decode(cuda, capped, count, expect):
    """qlzx_go_decompress_batch, the whole collection in one call (a lane per stream): status,
    dsize and output equal the oracle's; E_HEADER, E_LEVEL and E_DST_CAP leave the block as it
    was, E_CORRUPT writes nothing outside [off, off + size), every guard byte is intact."""
    import torch
    from gobeansdb_amd import _lib, batch
    entries = _decode_entries(capped)
    assert dict(Counter(c.family for c, _ in entries)) == expect and len(entries) == count
    ws = batch.Workspace()
    ws.get(_lib.lib().qlzx_go_decompress_workspace_size(len(entries))).fill_(0xFF)
    seen = _decode_batch_once(entries, capped, ws)
    assert dict(seen) == STATUSES[capped]
    assert _decode_batch_once(entries[::-1], capped, ws) == seen
    torch.cuda.synchronize()


@pytest.mark.parametrize("count", [pytest.param(217, id="single_217cases")])
def test_single_call_decode(cuda, count):
    """qlzx_go_decompress1 and the quicklz.Decompress mirror, one call per case, into a host
    buffer that held 0xA5: the oracle's status and bytes, nothing written on an error and
    nothing past the size."""
    from gobeansdb_amd import _lib
    from gobeansdb_amd.quicklz import Decompress, QuicklzError
    L = _lib.lib()
    cs = [c for c in C.collection() if c.stream is not None and c.family != "mutants"]
    assert dict(Counter(c.family for c in cs)) == SINGLE and len(cs) == count
    bad = []
    for c in cs:
        wst, wdata = _want(c.name, True)
        n, cap = C.claimed_size(c.stream), _cap(c)
        room = min(cap, n)
        dst = ctypes.create_string_buffer(bytes([GUARD]) * (room + GAP))
        r = L.qlzx_go_decompress1(c.stream, len(c.stream), dst, cap)
        got = dst.raw
        if wst == O.OK:
            if r != n or L.qlzx_last_status() != _lib.OK:
                bad.append((c.name, "status", r, L.qlzx_last_status()))
            elif got[:n] != wdata or got[n:] != bytes([GUARD]) * (room - n + GAP) + b"\0":
                bad.append((c.name, "bytes"))
        elif r != _lib.GO_ERROR or L.qlzx_last_status() != wst:
            bad.append((c.name, "error status", r, L.qlzx_last_status(), wst))
        elif got != bytes([GUARD]) * (room + GAP) + b"\0":
            bad.append((c.name, "written on error"))
        # the mirror has no dst_cap; a compressed level-3 stream is the level-3 decoder's
        if n > NO_CAP_MAX:
            continue
        l3 = len(c.stream) >= 3 and (c.stream[0] >> 2) & 3 == 3 and c.stream[0] & 1
        ust, udata = O.decompress(c.stream) if l3 else _want(c.name, False)
        try:
            res = Decompress(c.stream)
        except QuicklzError:
            res = None
        if res != (udata if ust == O.OK else None):
            bad.append((c.name, "quicklz.Decompress", res, ust))
    assert not bad, (len(bad), len(cs), bad[:12])


@functools.lru_cache(maxsize=None)
def _want_enc(name: str) -> bytes:
    return O.compress_go_l1(_by_name()[name].plain)


def _encode_batch_once(sel, ws):
    import torch
    from gobeansdb_amd import batch
    lens = [len(c.plain) for c in sel]
    soff, pos = [], 0
    for k, n in enumerate(lens):                    # every source off the 16-byte grid
        soff.append(pos + 1 + (k * 7) % 15)
        pos = (soff[-1] + n + GAP + 255) // 256 * 256
    host = np.zeros(pos + GAP, np.uint8)
    for o, c in zip(soff, sel):
        host[o:o + len(c.plain)] = np.frombuffer(c.plain, np.uint8)
    doff, total = _layout([n + 400 for n in lens], [None] * len(sel))
    ln = torch.tensor(np.asarray(lens, np.uint32).view(np.int32), device="cuda")
    src = batch.BlockBatch(torch.from_numpy(host).cuda(), torch.tensor(soff, dtype=torch.int64, device="cuda"), ln)
    data = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    dst = batch.BlockBatch(data, torch.tensor(doff, dtype=torch.int64, device="cuda"), ln.clone())
    _, cs, st = batch.go_l1_compress(src, dst, workspace=ws)
    torch.cuda.synchronize()
    out = data.cpu().numpy()
    cs = cs.cpu().numpy().view(np.uint32)
    st = st.cpu().numpy()
    bad = []
    untouched = np.ones(len(out), bool)
    for k, (c, o) in enumerate(zip(sel, doff)):
        want = _want_enc(c.name)
        untouched[o:o + len(c.plain) + 400] = False
        got = out[o:o + int(min(cs[k], len(c.plain) + 400))].tobytes()
        if int(st[k]) != 0:
            bad.append((c.name, "status", int(st[k])))
        elif int(cs[k]) != len(want) or got != want:
            bad.append((c.name, "bytes", int(cs[k]), len(want)))
    touched = np.nonzero(out[untouched] != GUARD)[0]
    assert not bad, (len(bad), len(sel), bad[:12])
    assert touched.size == 0, ("bytes written outside a block's n + 400", touched[:8])


@pytest.mark.parametrize("count", [pytest.param(73, id="encode_73cases")])
def test_batch_encode(cuda, count):
    """qlzx_go_l1_compress_batch: status OK, the oracle's bytes and length (the bail-out at
    margin 0 and -1 and each RLE refusal among them), nothing written outside n + 400."""
    from gobeansdb_amd import _lib, batch
    sel = [c for c in C.collection() if c.plain is not None]
    assert dict(Counter(c.family for c in sel)) == ENCODE and len(sel) == count
    ws = batch.Workspace()
    ws.get(_lib.lib().qlzx_go_l1_workspace_size(len(sel))).fill_(0xFF)
    _encode_batch_once(sel, ws)
    _encode_batch_once(sel[::-1], ws)


@pytest.mark.parametrize("count", [pytest.param(73, id="encode_73cases")])
def test_single_call_encode(cuda, count):
    """qlzx_compress1 with QLZX_F_LEVEL1 and the quicklz.Compress(x, 1) mirror, one call per case."""
    from gobeansdb_amd import _lib
    from gobeansdb_amd.quicklz import Compress
    L = _lib.lib()
    sel = [c for c in C.collection() if c.plain is not None]
    assert dict(Counter(c.family for c in sel)) == ENCODE and len(sel) == count
    bad = []
    for c in sel:
        n, want = len(c.plain), _want_enc(c.name)
        dst = ctypes.create_string_buffer(bytes([GUARD]) * (n + 400 + GAP))
        got = L.qlzx_compress1(c.plain, dst, n, _lib.F_LEVEL1)
        if got != len(want) or dst.raw[:got] != want:
            bad.append((c.name, "bytes", got, len(want), L.qlzx_last_status()))
        elif dst.raw[n + 400:] != bytes([GUARD]) * GAP + b"\0":
            bad.append((c.name, "guard"))
        if Compress(c.plain, 1) != want:
            bad.append((c.name, "quicklz.Compress"))
    assert not bad, (len(bad), len(sel), bad[:12])
