"""GPU: every encoder on the plaintexts of tests/qlz_cases.py, each built to force one decision of
qlz_compress_core (quicklz.c:197-494) -- a token form's edge, a match cut by the end of the block,
a wrapped hash counter, a tie, an evicted slot, a bail-out test passed with margin 0.
tests/test_encoder_cases.py shows on the host that every one of those decisions occurs, for the
workgroup kernels and again beyond 64 KiB for the whole-GPU encoder (its census), so a pass here
is not vacuous.

  route        encoder                                               blocks it takes
  wg4096       k_encode_wg<4096>,  batch call with max_len 4096      n <= 4096
  wg16384      k_encode_wg<16384>, batch call with max_len 16384     n <= 16384
  wg65536      k_encode_wg<65536>, batch call with max_len 65536     n <= 65536
    each with sources and destinations on the 16-byte grid, with destinations off it (no
    speculative stored copy) and with sources off it (no stored proof)
  lane         k_encode_lane, QLZX_F_GO_COMPAT                       n <= 65536, Go's bail-out rule
  huge         the whole-GPU encoder, batch call, max_len > 65536    n > 65536 (and a few small ones
  huge go      the same with QLZX_F_GO_COMPAT                         through the kernels above)
  single call  qlz_compress: the request service up to 65536 bytes, the staged call above

Every case goes to every route that takes it; each test counts what it ran per family against
the constants below.  On every route: status OK, the oracle's bytes and length, the fused CRC
equal to the oracle's from a per-block state, and nothing written outside a block's n + 400."""
import ctypes
import functools
from collections import Counter

import numpy as np
import pytest

import qlz_cases
from oracle import oracle as O

pytestmark = pytest.mark.gpu

WG_MAX_LEN = 65536      # QLZX_WG_MAX_LEN, kSvcMaxLen
GUARD = 0xA5

ALL = {"token_edges": 148, "tail_edges": 61, "table_edges": 22, "compact_edges": 18, "parse_rounds": 21,
       "bail_edges": 74, "huge_edges": 35}
EXPECT = {
    4096: {"token_edges": 132, "tail_edges": 48, "table_edges": 12, "compact_edges": 12, "parse_rounds": 7,
           "bail_edges": 22},
    16384: {"token_edges": 137, "tail_edges": 51, "table_edges": 17, "compact_edges": 15, "parse_rounds": 14,
            "bail_edges": 34},
    65536: {"token_edges": 148, "tail_edges": 54, "table_edges": 22, "compact_edges": 18, "parse_rounds": 21,
            "bail_edges": 54},
    "huge": {"tail_edges": 7, "bail_edges": 20, "huge_edges": 35},
}


@functools.lru_cache(maxsize=None)
def _expected(name: str, go: bool) -> bytes:
    c = next(c for c in qlz_cases.collection() if c.name == name)
    return O.compress_go(c.plain) if go else O.compress(c.plain)


def _route(route, count):
    """The cases of a route, counted per family: the total also stands in the test id."""
    cs = qlz_cases.collection()
    sel = [c for c in cs if (len(c.plain) > WG_MAX_LEN if route == "huge" else len(c.plain) <= route)]
    assert dict(Counter(c.family for c in sel)) == EXPECT[route], route
    assert len(sel) == count, f"{route}: {len(sel)} cases"
    return sel


def _run_batch(sel, max_len, go=False, layout="mixed"):
    """One qlzx_compress_batch call over `sel`, the whole destination buffer filled with GUARD
    first and guard gaps of at least 64 bytes around each block's n + 400.  Layouts:
      mixed          sources 256-byte aligned, destinations at every alignment mod 4, 16 and 256
      aligned        destinations on the 16-byte grid, at every multiple of 16 mod 256
      dst_unaligned  destinations off the 16-byte grid, all of them
      src_unaligned  sources off the 16-byte grid, all of them; destinations as in mixed"""
    import torch
    from gobeansdb_amd import batch
    lens = [len(c.plain) for c in sel]
    soff, pos = [], 0
    for k, n in enumerate(lens):
        soff.append(pos + (1 + (k * 7) % 15 if layout == "src_unaligned" else 0))
        pos = (soff[-1] + n + 64 + 255) // 256 * 256
    host = np.zeros(pos + 64, np.uint8)
    for o, c in zip(soff, sel):
        host[o:o + len(c.plain)] = np.frombuffer(c.plain, np.uint8)
    doff, pos = [], 0
    for k, n in enumerate(lens):
        a = (k * 37) % 256
        if layout == "aligned":
            a = a % 16 * 16
        elif layout == "dst_unaligned" and a % 16 == 0:
            a += 5
        pos = (pos + 64 + 255) // 256 * 256 + a
        doff.append(pos)
        pos += n + 400
    ln = torch.tensor(np.asarray(lens, np.uint32).view(np.int32), device="cuda")
    src = batch.BlockBatch(torch.from_numpy(host).cuda(), torch.tensor(soff, dtype=torch.int64, device="cuda"), ln)
    data = torch.full((pos + 320,), GUARD, dtype=torch.uint8, device="cuda")
    dst = batch.BlockBatch(data, torch.tensor(doff, dtype=torch.int64, device="cuda"), ln.clone())
    states = (np.arange(len(sel), dtype=np.uint64) * 0x9E3779B1 + 0x12345678).astype(np.uint32)
    _, cs, st, crc = batch.compress(src, dst, crc_state=torch.tensor(states.view(np.int32), device="cuda"),
                                    want_crc=True, go_compat=go, max_len=max_len)
    torch.cuda.synchronize()
    out = data.cpu().numpy()
    cs = cs.cpu().numpy().view(np.uint32)
    st = st.cpu().numpy()
    crc = crc.cpu().numpy().view(np.uint32)
    bad = []
    mask = np.ones(len(out), bool)
    for k, (c, o) in enumerate(zip(sel, doff)):
        want = _expected(c.name, go)
        mask[o:o + len(c.plain) + 400] = False
        got = out[o:o + int(min(cs[k], len(c.plain) + 400))].tobytes()
        if int(st[k]) != 0:
            bad.append((c.name, "status", int(st[k])))
        elif int(cs[k]) != len(want) or got != want:
            first = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), None)
            bad.append((c.name, "bytes", int(cs[k]), len(want), first))
        elif int(crc[k]) != O.crc32_write(int(states[k]), want) ^ 0xFFFFFFFF:
            bad.append((c.name, "crc"))
    touched = np.nonzero(out[mask] != GUARD)[0]
    assert not bad, (len(bad), len(sel), bad[:12])
    assert touched.size == 0, ("bytes written outside the blocks", touched[:8])


@pytest.mark.parametrize("layout", ["aligned", "dst_unaligned", "src_unaligned"])
@pytest.mark.parametrize("cap,count", [pytest.param(4096, 233, id="wg4096_233cases"),
                                       pytest.param(16384, 268, id="wg16384_268cases"),
                                       pytest.param(65536, 317, id="wg65536_317cases")])
def test_workgroup_encoder(cuda, cap, count, layout):
    """The three instantiations of k_encode_wg; the small cases go through all of them.  Every
    case (the bail-out edges among them) runs with the stored proof and its speculative copy
    (aligned), with the proof alone (dst_unaligned) and without the proof (src_unaligned)."""
    sel = _route(cap, count)
    assert max(len(c.plain) for c in sel) == cap       # the class bound is met by a block
    _run_batch(sel, cap, layout=layout)


@pytest.mark.parametrize("count", [pytest.param(317, id="lane_317cases")])
def test_lane_encoder_go_compat(cuda, count):
    """The lane encoder, the only Go-compatible path up to 64 KiB: the bail-out test counts the
    header, so the cases that pass quicklz.c:218 with a margin below 9 are stored here."""
    sel = _route(65536, count)
    flipped = sum(_expected(c.name, True)[0] & 1 != _expected(c.name, False)[0] & 1 for c in sel)
    assert flipped >= 20, flipped
    _run_batch(sel, WG_MAX_LEN, go=True)


@pytest.mark.parametrize("go", [False, True], ids=["c_rule", "go_compat"])
@pytest.mark.parametrize("count", [pytest.param(62, id="huge_62cases")])
def test_huge_encoder(cuda, count, go):
    """The whole-GPU encoder on the cases over 64 KiB, mixed with a few small blocks, which the
    same call sends through the workgroup (or, Go-compatible, the lane) encoder."""
    sel = _route("huge", count)
    small = [c for c in qlz_cases.collection() if len(c.plain) <= WG_MAX_LEN][::60]
    mixed = sel[:10] + small[:3] + sel[10:] + small[3:]
    assert len(mixed) == count + 6
    _run_batch(mixed, max(len(c.plain) for c in mixed), go=go)


@pytest.mark.parametrize("count", [pytest.param(379, id="single_379cases")])
def test_single_call(cuda, count):
    """qlz_compress, one call per case: the request service up to 65536 bytes, the staged call
    into the whole-GPU encoder above."""
    from gobeansdb_amd import _lib
    L = _lib.lib()
    cs = qlz_cases.collection()
    assert len(cs) == count and dict(Counter(c.family for c in cs)) == ALL
    bad = []
    for c in cs:
        n = len(c.plain)
        want = _expected(c.name, False)
        dst = ctypes.create_string_buffer(bytes([GUARD]) * (n + 400 + 64))
        got = L.qlz_compress(c.plain, dst, n, None)
        if L.qlzx_last_status() != 0:
            bad.append((c.name, "status", L.qlzx_last_status()))
        elif got != len(want) or dst.raw[:got] != want:
            bad.append((c.name, "bytes", got, len(want)))
        elif dst.raw[n + 400:] != bytes([GUARD]) * 64 + b"\0":
            bad.append((c.name, "guard"))
    assert not bad, (len(bad), len(cs), bad[:12])
