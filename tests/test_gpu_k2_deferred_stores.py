"""GPU parity for the seams between K2's batches, chunks and output stores (k_dec_chunk4,
qlzx_decode_k2.h).  Written for the builds that kept a full chunk's dword in registers for up to
four chunks (stored at the next batch start, when one more chunk arrives, before a ragged last
chunk, on an error exit or at the block end) and waited for far bytes only in the chunks that load
them; those builds were measured and not kept.  The cases hold for any
K2 and also cover the lane masks that now carry the items waiting for a marker slot from a batch
into the chunks after it.  The inputs are built for exactly those seams:

* 0, 1, 2 and many chunks completed per 64-item batch (literal-heavy, text, long matches, and
  blocks that switch kind halfway);
* every block end 256 k + r (pending chunks before a ragged chunk, a block ending on a pending
  chunk, no full chunk at all);
* far sources right behind the pending chunks (distances around 14, 15, 16 and 17 chunks), as
  one contiguous run per lane and as runs broken inside a lane's dword;
* destinations at every alignment, in a buffer pre-filled with 0xA5 that must stay 0xA5 outside
  the blocks;
* corrupt streams: status of the oracle, nothing written outside the block, workspace reusable.

Streams come from the oracle's compressor; the few blocks it would store raw (1-4 bytes) are
written as all-literal level-3 streams, which the oracle's decoder accepts.  Every case runs
through batch.decompress without and with the record-CRC prologue (both K2 instantiations).
"""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FILL = 0xA5
CRC = [False, True]


def _periodic(rng, n, period):
    base = rng.integers(0, 256, period, dtype=np.uint8)
    return np.resize(base, n).tobytes()


def _literal_heavy(rng, n):
    """Random bytes with a 16-byte copy from 100 bytes back every 48 bytes: 33 items per 48 bytes,
    so a 64-item batch yields some 93 bytes and most batch trips complete no chunk."""
    a = rng.integers(0, 256, n, dtype=np.uint8)
    for p in range(148, n - 16, 48):
        a[p:p + 16] = a[p - 100:p - 84]
    return a.tobytes()


def _far_runs(rng, n, dist, seg):
    """Random bytes (no match but the planted ones) with `seg`-byte copies from exactly `dist`
    bytes earlier; the segment starts walk through every offset mod 4.  The first `dist` bytes
    are text, so the encoder does not give the block up as incompressible halfway."""
    a = rng.integers(0, 256, n, dtype=np.uint8)
    a[:dist] = np.frombuffer(O.gen_text(dist, seg, dist), np.uint8)
    p, k = dist, 0
    while p + seg <= n:
        p += (k - p) % 4
        if p + seg > n:
            break
        a[p:p + seg] = a[p - dist:p - dist + seg]
        p += seg + int(rng.integers(8, 40))
        k += 1
    return a.tobytes()


def _far_broken(rng, n, dist):
    """Back-to-back short copies (5-8 bytes) from `dist` and `dist` + 17 bytes earlier in turn: a
    lane's four far sources then belong to two matches and form no single run."""
    a = rng.integers(0, 256, n, dtype=np.uint8)
    a[:dist] = np.frombuffer(O.gen_text(dist, 1, dist), np.uint8)
    p, k = dist + 17, 0
    while p + 64 <= n:
        for _ in range(8):
            ln = 5 + (k % 4)
            d = dist + 17 * (k & 1)
            a[p:p + ln] = a[p - d:p - d + ln]
            p += ln
            k += 1
        p += int(rng.integers(4, 24))
    return a.tobytes()


def _all_literal_stream(data: bytes) -> bytes:
    """A level-3 stream of literals only (31 per control word), long header."""
    body = bytearray()
    for i in range(0, len(data), 31):
        body += (0x80000000).to_bytes(4, "little") + data[i:i + 31]
    csize = 9 + len(body)
    return bytes([0x4F]) + csize.to_bytes(4, "little") + len(data).to_bytes(4, "little") + bytes(body)


def _compress(p: bytes) -> bytes:
    c = O.compress(p) if p else b"\0"   # the oracle's compressor takes no empty input
    if not c[0] & 1:   # the encoder stores it raw: K2's stored path, not the one under test
        c = _all_literal_stream(p)
        assert O.decompress(c) == (O.OK, p)
    assert c[0] & 1
    return c


def _offsets(lens, align_of=None):
    """Block offsets with a guard gap before each block; align_of(k) = offset mod 256 of block k."""
    offs, pos = [], 64
    for k, n in enumerate(lens):
        pos = (pos + 255) // 256 * 256 + (align_of(k) if align_of else 0)
        offs.append(pos)
        pos += n + 32
    return offs, pos + 64


def _decode(comp, lens, crc, offs=None, total=None, workspace=None):
    """batch.decompress into a 0xA5-filled buffer -> (status, dsize, host buffer, offsets)."""
    import torch
    from gobeansdb_amd import batch
    if offs is None:
        offs, total = _offsets(lens)
    src = batch.BlockBatch.from_bytes(comp)
    data = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    out = batch.BlockBatch(data, torch.tensor(offs, dtype=torch.int64, device="cuda"),
                           torch.tensor(lens, dtype=torch.int32, device="cuda"))
    kw = {}
    if crc:
        kw = dict(crc_state=torch.full((len(comp),), -1, dtype=torch.int32, device="cuda"),
                  crc_expect=batch.crc32(src))
    dsz, st, _ = batch.decompress(src, out, max_dsize=65536, workspace=workspace, **kw)
    torch.cuda.synchronize()
    return st.cpu().numpy(), dsz.cpu().numpy().view(np.uint32), data.cpu().numpy(), offs


def _assert_guard(host, offs, lens):
    mask = np.ones(len(host), bool)
    for o, n in zip(offs, lens):
        mask[o:o + n] = False
    bad = np.flatnonzero(host[mask] != FILL)
    assert bad.size == 0, f"{bad.size} bytes written outside the blocks"


def _check(plain, comp, crc, align_of=None, workspace=None):
    lens = [len(p) for p in plain]
    offs, total = _offsets(lens, align_of)
    st, dsz, host, offs = _decode(comp, lens, crc, offs, total, workspace)
    assert (st == 0).all(), [(k, int(s)) for k, s in enumerate(st) if s]
    assert (dsz == np.asarray(lens, np.uint32)).all()
    for k, (o, p) in enumerate(zip(offs, plain)):
        assert host[o:o + len(p)].tobytes() == p, (k, len(p))
    _assert_guard(host, offs, lens)


_memo = {}


def _built(name, make):
    """(plain, compressed) of a case set, built and compressed once for both CRC variants."""
    if name not in _memo:
        plain = make()
        _memo[name] = (plain, [_compress(p) for p in plain])
    return _memo[name]


def _chunks_per_trip():
    rng = np.random.default_rng(81)
    kinds = {
        "lit": lambda n, s: _literal_heavy(rng, n),
        "text": lambda n, s: O.gen_text(0x810 + s, s, n),
        "zero": lambda n, s: bytes(n),
        "per": lambda n, s: _periodic(rng, n, (3, 4, 7, 31, 100, 255, 256, 257, 511, 1000)[s % 10]),
    }
    sizes = (300, 777, 1024, 4099, 16384, 40001, 65536)
    out = []
    for s, n in enumerate(sizes):
        for k in kinds.values():
            out.append(k(n, s))
    for s in range(10):
        out.append(_periodic(rng, 9000 + 13 * s, (3, 4, 7, 31, 100, 255, 256, 257, 511, 1000)[s]))
    names = list(kinds)
    s = 0
    for a in names:          # blocks that switch kind halfway
        for b in names:
            if a != b:
                n = (5000, 12289, 33000)[s % 3]
                out.append(kinds[a](n // 2, s) + kinds[b](n - n // 2, s + 1))
                s += 1
    return out


def _block_ends():
    rng = np.random.default_rng(82)
    out = []
    for k in (0, 1, 2, 3, 5, 63):
        for r in (0, 1, 2, 3, 4, 255):
            n = 256 * k + r
            out += [O.gen_text(0x820, n, n), _periodic(rng, n, 5), _literal_heavy(rng, n), bytes(n)]
    return out


FAR_DISTS = (3583, 3584, 3585, 3839, 3840, 3841, 4095, 4096, 4097, 4352, 8000, 30000)


def _far_sources():
    rng = np.random.default_rng(83)
    out = []
    for d in FAR_DISTS:
        n = d + 9000 + d % 251
        out += [_far_runs(rng, n, d, 64), _far_runs(rng, n + 1, d, 11), _far_broken(rng, n + 2, d)]
        text = bytearray(O.gen_text(0x830 + d, d, n + 3))   # the same over text: near and far mixed
        for p in range(d, n - 70, 331):
            text[p:p + 61] = text[p - d:p - d + 61]
        out.append(bytes(text))
    return out


def _placement():
    rng = np.random.default_rng(84)
    out = []
    for k in range(40):
        n = 700 + 397 * k
        out.append((_far_runs(rng, n + 4200, 3841 + k, 32), O.gen_text(0x840, k, n), _periodic(rng, n, 3 + k),
                    _literal_heavy(rng, n))[k % 4])
    return out


@pytest.mark.parametrize("crc", CRC)
def test_chunks_completed_per_batch_trip(cuda, crc):
    _check(*_built("trip", _chunks_per_trip), crc)


@pytest.mark.parametrize("crc", CRC)
def test_block_ends(cuda, crc):
    _check(*_built("ends", _block_ends), crc)


@pytest.mark.parametrize("crc", CRC)
def test_far_sources_behind_pending_chunks(cuda, crc):
    _check(*_built("far", _far_sources), crc)


@pytest.mark.parametrize("crc", CRC)
def test_placement(cuda, crc):
    """Alignments 0..15 first, then k * 23 mod 256; everything outside the blocks stays 0xA5."""
    _check(*_built("place", _placement), crc, align_of=lambda k: k if k < 16 else (k * 23) % 256)


def _corrupt_cases():
    rng = np.random.default_rng(85)
    base = [O.gen_text(0x850, 0, 900), O.gen_text(0x851, 1, 5000), O.gen_text(0x852, 2, 16384),
            _literal_heavy(rng, 3000), _periodic(rng, 4000, 100), _far_runs(rng, 14000, 3841, 64),
            O.gen_text(0x853, 3, 65536)]
    cases = []
    for p in base:
        c = _compress(p)
        hdr = 9 if c[0] & 2 else 3
        b = bytearray(c[:-1])           # cut by one byte, the size field rewritten to match
        if b[0] & 2:
            b[1:5] = len(b).to_bytes(4, "little")
        else:
            b[1] = len(b)
        cases.append((bytes(b), len(p)))
        for _ in range(6):              # one byte of the second half corrupted
            b = bytearray(c)
            q = int(rng.integers(hdr + (len(c) - hdr) // 2, len(c)))
            b[q] ^= int(rng.integers(1, 256))
            cases.append((bytes(b), len(p)))
    return cases


@pytest.mark.parametrize("crc", CRC)
def test_corrupt_streams(cuda, crc):
    from gobeansdb_amd import batch
    if "bad" not in _memo:
        cases = _corrupt_cases()
        _memo["bad"] = (cases, [O.decompress(c) for c, _ in cases])
    cases, want = _memo["bad"]
    comp = [c for c, _ in cases]
    lens = [n for _, n in cases]
    assert all(n >= 3 * 256 and c[0] & 1 for c, n in cases)
    ws = batch.Workspace("cuda")
    st, dsz, host, offs = _decode(comp, lens, crc, workspace=ws)
    assert sum(1 for s, _ in want if s != 0) > len(cases) // 4   # the corruptions were exercised
    for k, ((ost, od), o, n) in enumerate(zip(want, offs, lens)):
        assert int(st[k]) == ost, (k, int(st[k]), ost)
        if ost == 0:
            assert host[o:o + n].tobytes() == od, k
    _assert_guard(host, offs, lens)
    # the same workspace decodes a clean batch afterwards
    _check(*_built("ends", _block_ends), crc, workspace=ws)
