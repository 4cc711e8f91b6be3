"""GPU: the routing boundaries of the single-call runtime (csrc/qlzx_single.hip).  Every drop-in
picks between the request service (qlzx_service.hip) and the per-thread staged call by the sizes
below; each case sits on one side of a boundary and must equal the oracle there.

  crc32_write        request path up to kSvcIn - 64 = 81856 bytes, staged above
  qlz_decompress     request path for dsize <= 65536 and csize <= 65536 (kSvcMaxLen, kSoloMaxCsize)
  read_record        as qlz_decompress for compressed values; stored values as crc32_write
  qlz_compress       request path up to 65536 bytes (kSvcMaxLen)
  qlzx_compress1     any flag takes the staged call, whatever the size
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from oracle import replay as R

from test_gpu_read_record import _expect

pytestmark = pytest.mark.gpu

SVC_CRC_MAX = (80 << 10) - 64   # kSvcIn - 64
SVC_MAX_LEN = 65536             # kSvcMaxLen == QLZX_FAST_MAX_DSIZE
SOLO_MAX_CSIZE = 65536          # kSoloMaxCsize


@functools.lru_cache(maxsize=None)
def _value(kind: str, n: int) -> bytes:
    if kind == "text":
        return O.gen_text(0x51, n, n)
    return np.random.default_rng(n).bytes(n)


@functools.lru_cache(maxsize=None)
def _stream(kind: str, n: int) -> bytes:
    return O.compress(_value(kind, n))


def _hdr_sizes(c: bytes):
    assert c[0] & 2
    return int.from_bytes(c[1:5], "little"), int.from_bytes(c[5:9], "little")


def _decompress(L, c: bytes):
    _, dsize = _hdr_sizes(c)
    out = ctypes.create_string_buffer(max(dsize, 1))
    n = L.qlz_decompress(c, out, None)
    return L.qlzx_last_status(), out.raw[:n]


# (kind, length, csize of the oracle's stream or None, served by the request path)
DECODE_CASES = [
    ("text", SVC_MAX_LEN, None, True),
    ("text", SVC_MAX_LEN + 1, None, False),
    ("rand", SOLO_MAX_CSIZE - 9, SOLO_MAX_CSIZE, True),       # stored: a 9-byte header
    ("rand", SOLO_MAX_CSIZE - 8, SOLO_MAX_CSIZE + 1, False),
]


def _check_case(kind, n, csize, served):
    c = _stream(kind, n)
    cs, ds = _hdr_sizes(c)
    assert cs == len(c) and ds == n
    if csize is not None:
        assert cs == csize
    assert (ds <= SVC_MAX_LEN and cs <= SOLO_MAX_CSIZE) == served
    return c


@pytest.mark.parametrize("length", [SVC_CRC_MAX - 1, SVC_CRC_MAX, SVC_CRC_MAX + 1])
def test_crc32_write_service_boundary(cuda, length):
    from gobeansdb_amd import _lib
    L = _lib.lib()
    buf = _value("rand", SVC_CRC_MAX + 1)[:length]
    for state in (0x12345678, 0xFFFFFFFF):
        assert L.crc32_write(state, buf, length) == O.crc32_write(state, buf)


@pytest.mark.parametrize("kind,n,csize,served", DECODE_CASES)
def test_qlz_decompress_boundaries(cuda, kind, n, csize, served):
    from gobeansdb_amd import _lib
    L = _lib.lib()
    c = _check_case(kind, n, csize, served)
    st, y = _decompress(L, c)
    assert st == 0 and y == _value(kind, n)


@pytest.mark.parametrize("kind,n,csize,served", DECODE_CASES)
def test_read_record_compressed_boundaries(cuda, kind, n, csize, served):
    from gobeansdb_amd import replay
    c = _check_case(kind, n, csize, served)
    rec = R.make_record(b"key_%d" % n, c, flag=R.FLAG_COMPRESS, ver=3)
    want = _expect(rec)
    assert want == (0, _value(kind, n))
    assert replay.read_record(rec) == want
    bad = bytearray(rec)
    bad[0] ^= 1                     # stored CRC off by a bit
    assert replay.read_record(bytes(bad)) is None


@pytest.mark.parametrize("n", [SVC_CRC_MAX, SVC_CRC_MAX + 1])
def test_read_record_stored_boundary(cuda, n):
    from gobeansdb_amd import replay
    v = _value("rand", SVC_CRC_MAX + 1)[:n]
    rec = R.make_record(b"key_%d" % n, v, flag=0, ver=3)
    want = _expect(rec)
    assert want == (0, v)
    assert replay.read_record(rec) == want
    bad = bytearray(rec)
    bad[0] ^= 1
    assert replay.read_record(bytes(bad)) is None


@pytest.mark.parametrize("n", [SVC_MAX_LEN, SVC_MAX_LEN + 1])
def test_qlz_compress_boundary(cuda, n):
    from gobeansdb_amd import _lib
    L = _lib.lib()
    v = _value("text", n)
    dst = ctypes.create_string_buffer(n + 400)
    got = L.qlz_compress(v, dst, n, None)
    assert dst.raw[:got] == _stream("text", n)


def test_compress1_go_compat_small_is_staged(cuda):
    """A flag keeps qlzx_compress1 off the request path: the staged call at a small size."""
    from gobeansdb_amd import _lib
    L = _lib.lib()
    v = _value("text", 4096)
    dst = ctypes.create_string_buffer(len(v) + 400)
    got = L.qlzx_compress1(v, dst, len(v), _lib.F_GO_COMPAT)
    assert L.qlzx_last_status() == 0
    assert dst.raw[:got] == O.compress_go(v)


def test_staged_buffers_reused_after_trim(cuda):
    """One thread: a staged qlz_decompress of a 200000-byte value (its buffers exceed what a
    thread keeps, so they are released after the call), then a staged crc32_write, then a
    service-sized qlz_decompress.  Each result must be right."""
    from gobeansdb_amd import _lib
    L = _lib.lib()
    st, y = _decompress(L, _stream("text", 200000))
    assert st == 0 and y == _value("text", 200000)
    buf = _value("text", 200000)[:100000]
    assert L.crc32_write(0x9E3779B9, buf, len(buf)) == O.crc32_write(0x9E3779B9, buf)
    st, y = _decompress(L, _stream("text", SVC_MAX_LEN))
    assert st == 0 and y == _value("text", SVC_MAX_LEN)
