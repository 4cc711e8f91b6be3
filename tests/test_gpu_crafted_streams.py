"""GPU: the five level-3 decoders on the hand-assembled streams of tests/qlz_asm.py -- encodings,
lengths (256-258), offsets (to 131071) and control words that no encoder emits, and invalid
streams one edit away from them.  DESIGN.md §1: every decoder agrees with the oracle and, on
valid streams, with the reference decoder (tests/test_crafted_streams.py pins the same streams to
both on the host).

  route            decoder                                     blocks it takes
  k1k2 uniform     K1 + K2, batch call with max_dsize 16384    dsize <= 16384
  k1k2 mixed       K1 + K2, batch call with max_dsize 65536    dsize <= 65536 (QLZX_FAST_MAX_DSIZE)
    both also with crc_state / want_crc: K2 with the CRC prologue
  lane8            batch call without a workspace              every block
  small            qlz_decompress, request service             csize <= 17408 and dsize <= 32768 (kSmC, kSmD)
  solo             qlz_decompress, request service             the others with csize, dsize <= 65536
  huge (batch)     batch call, max_dsize > 65536, workspace    dsize > 65536
  huge (single)    qlz_decompress, the staged call             dsize > 65536

Every stream goes to every route that takes it; each test counts what it ran per family against
the constants below, so no case can move to another route unnoticed.  A valid stream must give
status OK, the header's dsize and the assembler's plaintext; an invalid one the oracle's status,
and on the batch routes nothing may be written outside the blocks."""
import ctypes
import functools
from collections import Counter

import numpy as np
import pytest

import qlz_asm
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FAST_MAX_DSIZE = 65536      # QLZX_FAST_MAX_DSIZE: K1 + K2
UNIFORM_MAX_DSIZE = 16384   # chunk_blocks(): calls up to here are the uniform regime
SVC_MAX_LEN = 65536         # kSvcMaxLen
SOLO_MAX_CSIZE = 65536      # kSoloMaxCsize
SMALL_MAX_CSIZE = 17408     # kSmC
SMALL_MAX_DSIZE = 32768     # kSmD
GUARD = 0xA5

# cases per family on each route: (valid, invalid)
ALL_VALID = {"forms_S": 143, "forms_M": 52, "forms_L": 20, "chunk_cover": 81, "groups": 15, "lastword": 92,
             "tail": 63, "random": 200}
ALL_INVALID = {"forms_S": 120, "forms_M": 72, "forms_L": 46}
EXPECT = {
    "uniform": ({"forms_S": 143, "chunk_cover": 48, "groups": 13, "lastword": 92, "tail": 63, "random": 98},
                {"forms_S": 120}),
    "mixed": ({"forms_S": 143, "forms_M": 52, "chunk_cover": 81, "groups": 15, "lastword": 92, "tail": 63,
               "random": 160}, {"forms_S": 120, "forms_M": 72}),
    "lane8": (ALL_VALID, ALL_INVALID),
    "small": ({"forms_S": 143, "chunk_cover": 63, "groups": 14, "lastword": 92, "tail": 63, "random": 120},
              {"forms_S": 120}),
    "solo": ({"forms_M": 52, "chunk_cover": 18, "groups": 1, "random": 40}, {"forms_M": 72}),
    "huge": ({"forms_L": 20, "random": 40}, {"forms_L": 46}),
}


def _is_small(csize, dsize):
    return csize <= SMALL_MAX_CSIZE and dsize <= SMALL_MAX_DSIZE


ADMIT = {
    "uniform": lambda csize, dsize: dsize <= UNIFORM_MAX_DSIZE,
    "mixed": lambda csize, dsize: dsize <= FAST_MAX_DSIZE,
    "lane8": lambda csize, dsize: True,
    "small": _is_small,
    "solo": lambda csize, dsize: not _is_small(csize, dsize) and dsize <= SVC_MAX_LEN and csize <= SOLO_MAX_CSIZE,
    "huge": lambda csize, dsize: dsize > FAST_MAX_DSIZE,
}


# a case: (name, family, stream, dsize, expected status, expected bytes or None for an invalid one)
@functools.lru_cache(maxsize=None)
def _cases():
    """Every valid and invalid case with what every decoder owes for it (built once)."""
    out = [(c.name, c.family, c.stream, len(c.plain), O.OK, c.plain) for c in qlz_asm.collection()]
    for i in qlz_asm.invalid_collection():
        st, _ = O.decompress(i.stream, cap=i.dsize)
        assert st == O.E_CORRUPT, i.name
        out.append((i.name, i.family, i.stream, i.dsize, st, None))
    return tuple(out)


def _route(route):
    """The cases the route takes; every block of a single-call route must also be one the
    dispatcher of qlz_decompress sends there, and every case must have some single-call route."""
    sel = [c for c in _cases() if ADMIT[route](len(c[2]), c[3])]
    valid = Counter(c[1] for c in sel if c[5] is not None)
    invalid = Counter(c[1] for c in sel if c[5] is None)
    assert (dict(valid), dict(invalid)) == EXPECT[route], route
    return sel


def _run_batch(sel, max_dsize, general=False, crc=False):
    """One qlzx_decompress_batch call over `sel`: destinations packed at mixed byte alignments
    with guard gaps of at least 64 bytes, the whole buffer filled with GUARD first."""
    import torch
    from gobeansdb_amd import _lib, batch
    L = _lib.lib()
    if not general:   # the workspace batch.decompress passes is the full one: the huge decoder runs
        assert L.qlzx_decompress_workspace_size(len(sel), max_dsize) >= \
            L.qlzx_decompress_workspace_size(len(sel), min(max_dsize, FAST_MAX_DSIZE))
    src = batch.BlockBatch.from_bytes([c[2] for c in sel])
    dsizes = [c[3] for c in sel]
    offs, pos = [], 0
    for k, n in enumerate(dsizes):
        pos = (pos + 64 + 255) // 256 * 256 + (k * 37) % 256   # every alignment mod 4, 16 and 256
        offs.append(pos)
        pos += n
    data = torch.full((pos + 320,), GUARD, dtype=torch.uint8, device="cuda")
    out = batch.BlockBatch(data, torch.tensor(offs, dtype=torch.int64, device="cuda"),
                           torch.tensor(dsizes, dtype=torch.int32, device="cuda"))
    cap = torch.tensor(np.asarray(dsizes, np.uint32).view(np.int32), device="cuda")
    kw = {}
    states = None
    if crc:
        states = (np.arange(len(sel), dtype=np.uint64) * 0x9E3779B1 + 0x12345678).astype(np.uint32)
        kw = dict(crc_state=torch.tensor(states.view(np.int32), device="cuda"), want_crc=True)
    dsz, st, crc_out = batch.decompress(src, out, dst_cap=cap, max_dsize=max_dsize, general=general, **kw)
    torch.cuda.synchronize()
    host = data.cpu().numpy()
    dsz = dsz.cpu().numpy().view(np.uint32)
    st = st.cpu().numpy()
    crcs = crc_out.cpu().numpy().view(np.uint32) if crc else None
    bad = []
    mask = np.ones(len(host), bool)
    for k, (c, o) in enumerate(zip(sel, offs)):
        name, _, stream, n, want_st, want = c
        mask[o:o + n] = False                   # a refused block's own bytes are not compared
        if int(st[k]) != want_st:
            bad.append((name, "status", int(st[k]), want_st))
        elif want is not None and (int(dsz[k]) != n or host[o:o + n].tobytes() != want):
            got = host[o:o + n].tobytes()
            first = next((j for j in range(n) if got[j] != want[j]), None)
            bad.append((name, "bytes", int(dsz[k]), first))
        if crc and int(crcs[k]) ^ 0xFFFFFFFF != O.crc32_write(int(states[k]), stream):
            bad.append((name, "crc"))
    touched = np.nonzero(host[mask] != GUARD)[0]
    assert not bad, (len(bad), len(sel), bad[:12])
    assert touched.size == 0, ("bytes written outside the blocks", touched[:8])


def _counted(route, nvalid, ninvalid):
    """The route's cases, counted: the numbers also stand in the test id."""
    sel = _route(route)
    got = (sum(c[5] is not None for c in sel), sum(c[5] is None for c in sel))
    assert got == (nvalid, ninvalid), f"{route}: {got[0]} valid and {got[1]} invalid streams"
    return sel


@pytest.mark.parametrize("crc", [False, True], ids=["nocrc", "crc"])
@pytest.mark.parametrize("route,max_dsize,nvalid,ninvalid", [
    pytest.param("uniform", UNIFORM_MAX_DSIZE, 457, 120, id="uniform_457valid_120invalid"),
    pytest.param("mixed", FAST_MAX_DSIZE, 606, 192, id="mixed_606valid_192invalid")])
def test_k1_k2(cuda, route, max_dsize, nvalid, ninvalid, crc):
    """K1 + K2 in both chunk regimes, without and with the CRC prologue (the two instantiations
    of K2)."""
    sel = _counted(route, nvalid, ninvalid)
    assert max(c[3] for c in sel) == max_dsize   # the call's bound is met by a block
    _run_batch(sel, max_dsize, crc=crc)


@pytest.mark.parametrize("nvalid,ninvalid", [pytest.param(666, 238, id="666valid_238invalid")])
def test_lane8(cuda, nvalid, ninvalid):
    """The lane-per-block kernel on every stream, the 140 KiB ones included."""
    sel = _counted("lane8", nvalid, ninvalid)
    assert len(sel) == len(_cases())
    _run_batch(sel, max(c[3] for c in sel), general=True)


@pytest.mark.parametrize("nvalid,ninvalid", [pytest.param(60, 46, id="60valid_46invalid")])
def test_huge_batch(cuda, nvalid, ninvalid):
    """The whole-GPU decoder through the batch call: the streams over 64 KiB."""
    sel = _counted("huge", nvalid, ninvalid)
    assert min(c[3] for c in sel) > FAST_MAX_DSIZE
    _run_batch(sel, max(c[3] for c in sel))


def _single(L, stream: bytes, dsize: int):
    """qlz_decompress(stream) -> (status, returned length, bytes, guard untouched)."""
    src = ctypes.create_string_buffer(stream + bytes(16))
    out = ctypes.create_string_buffer(bytes([GUARD]) * (dsize + 64))
    n = L.qlz_decompress(src, out, None)
    return L.qlzx_last_status(), n, out.raw[:dsize], out.raw[dsize:] == bytes([GUARD]) * 64 + b"\0"


@pytest.mark.parametrize("route,nvalid,ninvalid", [
    pytest.param("small", 495, 120, id="small_495valid_120invalid"),
    pytest.param("solo", 111, 72, id="solo_111valid_72invalid"),
    pytest.param("huge", 60, 46, id="huge_60valid_46invalid")])
def test_single_call(cuda, route, nvalid, ninvalid):
    """qlz_decompress, one call per stream: the all-in-LDS small path, the one-workgroup solo
    path and the staged call into the whole-GPU decoder."""
    from gobeansdb_amd import _lib
    L = _lib.lib()
    sel = _counted(route, nvalid, ninvalid)
    bad = []
    for name, _, stream, dsize, want_st, want in sel:
        # the dispatcher's own rule (decompress1): the request path, else the staged batch call
        served = dsize <= SVC_MAX_LEN and len(stream) <= SOLO_MAX_CSIZE
        assert served == (route != "huge"), name
        st, n, got, guard_ok = _single(L, stream, dsize)
        if st != want_st or not guard_ok:
            bad.append((name, "status", st, want_st, guard_ok))
        elif want is not None and (n != dsize or got != want):
            bad.append((name, "bytes", n, next((j for j in range(dsize) if got[j] != want[j]), None)))
        elif want is None and n != 0:
            bad.append((name, "length of a refused stream", n))
    assert not bad, (len(bad), len(sel), bad[:12])
