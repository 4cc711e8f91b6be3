"""GPU: the record-file calls over one 4 GiB + 4 MiB buffer whose records lie around 2^31 and
2^32 (tests/wide.py: the buffers; tests/wide_records.py: the two layouts, the decoy records in the
low alias window and the rules that derive the whole buffer's answer from the oracle's answers on
the windows; tests/test_wide_rules.py checks those rules on the host).

Expected values come from oracle/replay.py, oracle/gc.py and tests/hint_model.py run on the window
bytes with offsets shifted by the window start.  Every test asserts its layout's census and that
the decoys are valid other records before it touches the GPU.

The tests at the end produce more than 4 GiB of output (a read's decoder output, a GC destination,
an encode's records and its trial buffer); they allocate those buffers themselves, compare them on
the device in slices and free them before they return."""
import random
import struct

import numpy as np
import pytest

import hint_model as H
import wide
import wide_records as WR
from oracle import gc as G
from oracle import replay as R
from wide import B32, BIG_BYTES

pytestmark = pytest.mark.gpu

widebuf = wide.fixture(out_bytes=1 << 20)      # no test here writes into bigout: the outputs are the calls' own
w = wide.per_test()

LO32, LO31 = WR.WIN32[0], WR.WIN31[0]
OK, ALIGN, EOF_HEADER, KEY_SIZE, VALUE_SIZE, EOF_BODY, CRC = range(7)
KINDS = ("straddle", "starts_at")
CENSUS = {
    "straddle": dict(at31=1, ends_at31=1, straddle31=[], at32=0, ends_at32=0, straddle32=[(True, True)]),
    "starts_at": dict(at31=0, ends_at31=0, straddle31=[(True, True)], at32=1, ends_at32=1, straddle32=[]),
}


def _setup(wb, kind, corrupt=False):
    """The layout on the host, census and decoys asserted, then its windows placed into big."""
    win, _ = WR.layout(kind, corrupt)
    recs, census = WR.facts(win)
    if not corrupt:
        assert {k: census[k] for k in CENSUS[kind]} == CENSUS[kind]
        assert len(recs[LO31]) == len(recs[LO32]) == 120
    for name in ("31", "32"):
        assert census["below" + name] >= 50 and census["above" + name] >= 50
    assert WR.assert_decoys(win, recs) >= 50
    for lo, a in win.items():
        wb.place(wb.big, lo, a)
    return win, recs


def _same_replay(res, rows, win_of):
    """A ReplayResult against oracle rows (absolute offset, sizeBroken, key, ver, flag, value,
    vhash); win_of(offset) -> (window start, window bytes) for the stored header."""
    assert res.n == len(rows)
    off = res.offset.cpu().tolist()
    broken = res.size_broken.cpu().numpy().view(np.uint32).tolist()
    hdr = res.header.cpu().numpy()
    flag = res.flag.cpu().numpy().view(np.uint32).tolist()
    vlen = res.value_len.cpu().tolist()
    vh = res.vhash.cpu().tolist()
    assert off == [r[0] for r in rows]
    assert broken == [r[1] for r in rows]
    bad = []
    for j, (o, _, key, ver, wflag, wval, wvh) in enumerate(rows):
        lo, data = win_of(o)
        stored = struct.unpack_from("<6i", data, o - lo)
        at = o - lo + 24
        if tuple(int(x) for x in hdr[j]) != stored or stored[3] != ver or data[at:at + stored[4]] != key:
            bad.append((j, hex(o), "header"))
        elif (flag[j], vlen[j], vh[j]) != (wflag, len(wval), wvh) or res.value(j) != wval:
            bad.append((j, hex(o), "value", flag[j], wflag, vlen[j], len(wval), vh[j], wvh))
    assert not bad, (len(bad), bad[:8])


def _win_of(win):
    data = {lo: a.tobytes() for lo, a in win.items()}

    def f(o):
        lo = max(k for k in data if k <= o)
        return lo, data[lo]
    return f


@pytest.mark.parametrize("kind", KINDS)
def test_replay_from_the_upper_window(w, kind):
    """replay.index and replay.replay with start = the 2^32 window's start: offsets, rec_broken,
    result[0..3], headers, values and vhash are the oracle's on the window, shifted."""
    from gobeansdb_amd import replay
    win, recs = _setup(w, kind)
    rows, err = WR.replay_rows(win, LO32)
    assert err is None and len(rows) == 120 and rows[0][1] == rows[0][0] - LO32 > 0
    ncand, nvalid = WR.slot_counts(win, BIG_BYTES)
    assert nvalid == 240 + sum(o >= B32 for o, _ in recs[LO32])      # the scan sees every slot, the decoys too
    off, broken, end_error, gc_, gv = replay.index(w.big, start=LO32)
    assert (off.cpu().tolist(), broken.cpu().numpy().view(np.uint32).tolist(), end_error, gc_, gv) == \
        ([r[0] for r in rows], [r[1] for r in rows], False, ncand, nvalid)
    res = replay.replay(w.big, start=LO32)
    assert (res.end_error, res.n_candidates, res.n_valid) == (False, ncand, nvalid)
    _same_replay(res, rows, _win_of(win))


@pytest.mark.parametrize("kind", KINDS)
def test_replay_of_the_whole_buffer(w, kind):
    """replay.index and replay.replay with start = 0: the reader returns the records of A0, of
    the 2^31 window and of the 2^32 window; the first record after each run of zeros carries the
    run in rec_broken (both runs are shorter than 2^32 bytes)."""
    from gobeansdb_amd import replay
    win, recs = _setup(w, kind)
    parts = [(lo, WR.replay_rows(win, lo)[0], WR.last_rsize(win, lo)) for lo in (0, LO31, LO32)]
    rows = WR.join_replays(parts)
    gaps = [r[1] for r in rows if r[1] >= (1 << 30)]
    assert len(gaps) == 2 and all(g < B32 for g in gaps)
    assert len(rows) == 240 + sum(o >= B32 for o, _ in recs[LO32])
    ncand, nvalid = WR.slot_counts(win, BIG_BYTES)
    off, broken, end_error, gc_, gv = replay.index(w.big)
    assert (off.cpu().tolist(), broken.cpu().numpy().view(np.uint32).tolist(), end_error, gc_, gv) == \
        ([r[0] for r in rows], [r[1] for r in rows], False, ncand, nvalid)
    res = replay.replay(w.big)
    assert (res.end_error, res.n_candidates, res.n_valid) == (False, ncand, nvalid)
    _same_replay(res, rows, _win_of(win))


def test_replay_resync_crosses_2_32(w):
    """The last record below 2^32 is corrupted: the resync walks its slots across the line."""
    from gobeansdb_amd import replay
    win, _ = _setup(w, "straddle", corrupt=True)
    rows, err = WR.replay_rows(win, LO32)
    assert err is None and len(rows) == 119
    hit = [r for r in rows[1:] if r[1]]
    assert len(hit) == 1 and hit[0][0] > B32 > hit[0][0] - hit[0][1]
    res = replay.replay(w.big, start=LO32)
    _same_replay(res, rows, _win_of(win))


# ---------------------------------------------------------------- read_records

def _expect(data: bytes, off: int, max_key=R.MAX_KEY_LEN, body_max=R.BODY_MAX):
    from test_gpu_read_batch import _expect as e
    return e(data, off, max_key, body_max)


def _read_rows(res):
    st = res.status.cpu().tolist()
    hdr = res.header.cpu().numpy()
    flag = res.flag.cpu().numpy().view(np.uint32).tolist()
    vh = res.vhash.cpu().tolist()
    dec = res.dec_status.cpu().tolist()
    return [(st[i], tuple(int(x) for x in hdr[i]), flag[i], res.value(i) if st[i] == OK else None, vh[i], dec[i] == 0)
            for i in range(res.n)]


def _check_reads(wb, win32, offsets, size=BIG_BYTES, win31=None, keys=None, **lim):
    """read_records over big[:size] against _expect on the window that holds each offset."""
    from gobeansdb_amd import replay
    res = replay.read_records(wb.big[:size], offsets, keys=keys, **lim)
    rows = _read_rows(res)
    d32 = win32[:size - LO32]
    bad = []
    for i, o in enumerate(offsets):
        lo, data = (LO31, win31) if win31 is not None and LO31 <= o < WR.WIN31[1] else (LO32, d32)
        want = _expect(data, o - lo, **lim)
        if rows[i] != want:
            bad.append((i, hex(o), rows[i][:3], want[:3]))
    assert not bad, (len(bad), bad[:8])
    return res, rows


@pytest.mark.parametrize("kind", KINDS)
def test_read_records(w, kind):
    """Every record of both windows in shuffled order, with keys (every fifth a wrong one), and
    requests that fail above 2^32: an unaligned one, an empty slot, the buffer's end."""
    win, recs = _setup(w, kind)
    win31, win32 = win[LO31].tobytes(), win[LO32].tobytes()
    reqs = [(o, r.key) for o, r in recs[LO31] + recs[LO32]]
    reqs += [(B32 + 128, b"k"), (B32 + (2 << 20), b"k"), (BIG_BYTES, b"k"), (BIG_BYTES + 256, b"k"),
             (BIG_BYTES - 256, b"k")]
    random.Random(5).shuffle(reqs)
    keys = [k if i % 5 else k + b"?" for i, (_, k) in enumerate(reqs)]
    res, rows = _check_reads(w, win32, [o for o, _ in reqs], win31=win31, keys=keys)
    st = {o: r[0] for (o, _), r in zip(reqs, rows)}
    assert (st[B32 + 128], st[B32 + (2 << 20)], st[BIG_BYTES], st[BIG_BYTES + 256], st[BIG_BYTES - 256]) == \
        (ALIGN, KEY_SIZE, EOF_HEADER, EOF_HEADER, KEY_SIZE)
    assert sum(s == OK for s in st.values()) == 240
    real = {o: r.key for o, r in recs[LO31] + recs[LO32]}
    assert res.key_eq.cpu().tolist() == [int(o in real and k == real[o]) for (o, _), k in zip(reqs, keys)]
    assert res.totals[0] == 240


def test_read_boundary_verdicts_above_2_32(w):
    """tests/test_gpu_read_batch.py's test_boundary_verdicts with the records above 2^32: the
    buffer cut inside the last record's body and header, and the crafted sizes."""
    win, recs = _setup(w, "starts_at")
    win32 = bytearray(win[LO32].tobytes())
    (o1, _), (o2, last) = recs[LO32][-2:]
    assert o1 > B32
    end = o2 + 24 + len(last.key) + len(last.body)
    assert len(last.body) > 0
    for size, verdict in ((BIG_BYTES, OK), (end, OK), (end - 1, EOF_BODY), (o2 + 24, EOF_BODY), (o2 + 23, EOF_HEADER),
                          (o2 + 1, EOF_HEADER)):
        _, rows = _check_reads(w, bytes(win32), [o1, o2], size=size)
        assert [r[0] for r in rows] == [OK, verdict], size

    def crafted(ksz, vsz):
        return (struct.pack("<IIiiII", 0x12345678, 1, 0, 2, ksz, vsz) + b"k" * 40).ljust(256, b"\0")
    lim = dict(max_key=30, body_max=8192)
    chunk = crafted(0, 10) + crafted(31, 10) + crafted(5, 8193) + crafted(31, 8193) + crafted(0, 1 << 31) + \
        R.make_record(b"k" * 30, bytes(8192)) + crafted(30, 8192)
    at = B32 + (2 << 20)
    w.place(w.big, at, chunk)
    win32[at - LO32:at - LO32 + len(chunk)] = chunk
    offs = [at + k for k in range(0, 6 * 256, 256)] + [at + len(chunk) - 256]
    size = at + len(chunk)                                  # the last crafted record's body runs past it
    _, rows = _check_reads(w, bytes(win32), offs, size=size, **lim)
    assert [r[0] for r in rows] == [KEY_SIZE, KEY_SIZE, VALUE_SIZE, KEY_SIZE, KEY_SIZE, OK, EOF_BODY]


# ---------------------------------------------------------------- GC rewrite

@pytest.mark.parametrize("kind,dfm,head,nxt", [("straddle", 1 << 30, 0, ()), ("straddle", 4096, 2048, ()),
                                               ("starts_at", 4096, 1024, (512, 3584)), ("starts_at", 8192, 0, ())])
def test_gc_source_above_2_32(w, kind, dfm, head, nxt):
    """rec_off from the replay of the upper window, keep masks and rotation as in
    tests/test_gpu_gc_batch.py; gc.rewrite (the host-planned path) agrees field by field."""
    import torch
    import test_gpu_gc_batch as T
    from gobeansdb_amd import _lib, gc, replay
    win, recs = _setup(w, kind)
    data = win[LO32].tobytes()
    rnd = random.Random(dfm + head)
    keep = [rnd.random() < 0.55 for _ in recs[LO32]]
    above = [k for (o, _), k in zip(recs[LO32], keep) if o >= B32]
    assert sum(above) >= 20 and above.count(False) >= 10
    want_chunks, want_pos = G.gc_rewrite(data, keep, data_file_max=dfm, dst_head=head, next_heads=nxt)
    off = replay.index(w.big, start=LO32)[0]
    assert off.cpu().tolist() == [o for o, _ in recs[LO32]]
    kt = torch.tensor(keep, device=w.device)
    out = T._out(sum(map(len, want_chunks)), w.device)
    res = gc.rewrite_batch(w.big, off, kt, dst_head=head, data_file_max=dfm, next_heads=nxt, out=out)
    torch.cuda.synchronize()
    T._check(res, out, want_chunks, want_pos, [r.crc for (_, r), k in zip(recs[LO32], keep) if k])
    assert res.status.cpu().tolist() == [_lib.GC_WRITTEN if k else _lib.GC_DROPPED for k in keep]
    old, new = gc.rewrite(w.big, off, kt, dst_head=head, data_file_max=dfm, next_heads=nxt), res.result()
    torch.cuda.synchronize()
    assert [c.cpu().numpy().tobytes() for c in new.chunks] == [c.cpu().numpy().tobytes() for c in old.chunks]
    assert new.chunk.tolist() == old.chunk.tolist() and new.offset.tolist() == old.offset.tolist()
    assert new.crc.tolist() == old.crc.tolist() and new.crc_mismatch == old.crc_mismatch == 0


def test_gc_new_off_crosses_2_32(w):
    """dst_head = 2^32 - 1024 in a destination chunk that may grow to 2^40: new_off crosses the
    line while `out`, which holds the bytes from the head on, stays small."""
    import torch
    import test_gpu_gc_batch as T
    from gobeansdb_amd import gc, replay
    win, recs = _setup(w, "straddle")
    data = win[LO32].tobytes()
    keep = [True] * len(recs[LO32])
    head = B32 - 1024
    want_chunks, want_pos = G.gc_rewrite(data, keep, data_file_max=1 << 40, dst_head=head)
    assert len(want_chunks) == 1 and want_pos[0] == (0, head)
    assert sum(p < B32 for _, p in want_pos) >= 1 and sum(p > B32 for _, p in want_pos) >= 100
    off = replay.index(w.big, start=LO32)[0]
    out = T._out(len(want_chunks[0]), w.device)
    res = gc.rewrite_batch(w.big, off, torch.tensor(keep, device=w.device), dst_head=head, data_file_max=1 << 40,
                           out=out)
    torch.cuda.synchronize()
    T._check(res, out, want_chunks, want_pos, [r.crc for _, r in recs[LO32]])


# ---------------------------------------------------------------- hint build

@pytest.mark.parametrize("split_cap", [2, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_hint_build(w, kind, split_cap):
    """hint.build (and so hint.build_split) fed the replay from the upper window: the files are
    hint_model's with every offset reduced mod 2^32 (include/qlzx.h: uint32(rec_off[j])), and
    datasize follows the stated formula with its 32-bit wrap."""
    from test_gpu_hint import _same
    from gobeansdb_amd import hint, replay
    win, recs = _setup(w, kind)
    rows, _ = WR.replay_rows(win, LO32)
    model = WR.hint_records(rows, recs[LO32])
    reduced = sum(m[2] != row[0] for m, row in zip(model, rows))
    assert reduced == sum(o >= B32 for o, _ in recs[LO32]) >= 50
    wrapped = [(m[2] + m[3]) & WR.M32 for m in model if (m[2] + m[3]) >> 32]
    assert len(wrapped) == 1 and (wrapped[0] == 0) == (kind == "starts_at")   # the record that ends at or across 2^32
    kw = dict(split_cap=split_cap, index_interval=128, chunk_id=7)
    want = H.build(model, **kw)
    assert len(want) >= 120 // split_cap
    res = replay.replay(w.big, start=LO32)
    got = hint.build(res, **kw)
    _same(got, want)


# ---------------------------------------------------------------- sources of an encode above 2^32

FC, FCC = 0x10000, 0x10          # FLAG_COMPRESS, FLAG_CLIENT_COMPRESS


def _policy_cases():
    """tests/test_gpu_write_batch.py's test_policy_edges: (value, flag, ver), thirteen of them."""
    from oracle import oracle as O
    texts = {n: O.gen_text(2, n & 0xff, n) for n in (231, 232, 4096, 10240, 10241, 20000)}
    rnd400 = np.random.default_rng(1).integers(0, 256, 400, dtype=np.uint8).tobytes()
    img = O.gen_image(5, 0, 30000)
    return [(texts[231], 0, 0), (texts[232], 0, 0), (b"v" * 255, 0, 0), (rnd400, 0, 0), (texts[4096], 0, 0),
            (texts[10240], 0, 0), (texts[10241], 0, 0), (texts[20000], 0, 0), (img, 0, 0), (texts[4096], 0, -1),
            (texts[4096], FCC, 0), (texts[4096], FC, 0), (b"ID3\x03" + texts[4096], 0, 0)]


def _encode_cases():
    """(key, value, flag, ver): the policy edges under key b"k", then test_alignment_sweep's key
    sizes 1..17 with plain values (the client-compressed flag keeps them raw)."""
    noise = np.random.default_rng(11).integers(0, 256, 6000, dtype=np.uint8).tobytes()
    cases = [(b"k", v, f, ver) for v, f, ver in _policy_cases()]
    for ksz in range(1, 18):
        vlen = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 5000)[ksz % 11]
        cases.append((bytes((ksz + b) & 0xff or 1 for b in range(ksz)), noise[ksz * 7:][:vlen], FCC, ksz))
    return cases


def test_encode_keys_and_values_above_2_32(w):
    """record.encode_batch with every key and every value at all placements of both lines, so
    key_off and val_off pass 2^32; per call the whole output against _expect."""
    import torch
    from test_gpu_write_batch import FILL, _expect
    from gobeansdb_amd import _dev, batch, record
    cases = _encode_cases()
    assert len(cases) == 30
    jobs, kblocks, vblocks = [], [], []
    for i, (k, v, f, ver) in enumerate(cases):
        dk, dv = bytes(b ^ 0x21 for b in k), bytes(b ^ 0x20 for b in v)     # another key, the text in the other case
        kat, vat = wide.all_placements(len(k)), wide.all_placements(len(v))
        for p in range(12):
            ks, vs = kat[(1 - p // 6) * 6 + (p + i) % 6], vat[p]      # the key at the other line: they never overlap
            spans = [("big", ks, len(k)), ("big", vs, len(v))]
            for at, real, decoy in ((ks, k, dk), (vs, v, dv)):
                alias = wide.decoy_tail(at, real, decoy)
                if alias is not None:
                    spans.append(("big", alias[0], len(alias[1])))
            jobs.append(((i, ks, vs), spans))
            kblocks.append((ks, len(k)))
            vblocks.append((vs, len(v)))
    assert wide.census(kblocks) == wide.full_census([len(c[0]) for c in cases])
    assert wide.census(vblocks) == wide.full_census([len(c[1]) for c in cases])
    ws = batch.Workspace(w.device)
    for rnd in wide.rounds(jobs):
        todo = [key for key, _ in rnd]
        sel = [cases[i] for i, _, _ in todo]
        for (i, ks, vs), (k, v, f, ver) in zip(todo, sel):
            w.place_with_decoy(ks, k, bytes(b ^ 0x21 for b in k))
            w.place_with_decoy(vs, v, bytes(b ^ 0x20 for b in v))
        keys = batch.BlockBatch(w.big, _dev.u64([ks for _, ks, _ in todo], w.device),
                                _dev.u32([len(c[0]) for c in sel], w.device))
        vals = batch.BlockBatch(w.big, _dev.u64([vs for _, _, vs in todo], w.device),
                                _dev.u32([len(c[1]) for c in sel], w.device))
        flags, vers, ts = [c[2] for c in sel], [c[3] for c in sel], list(range(7, 7 + len(sel)))
        rows, data, bound = _expect([c[0] for c in sel], [c[1] for c in sel], flags, vers, ts)
        out = torch.full((bound + 512,), FILL, dtype=torch.uint8, device=w.device)
        res = record.encode_batch(keys, vals, flags=flags, vers=vers, ts=ts, out=out, workspace=ws)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got[:len(data)].tobytes() == data and (got[len(data):] == FILL).all(), todo
        assert res.offset.cpu().tolist() == [r[1] for r in rows]
        assert _dev.readback(res.crc).tolist() == [r[5] for r in rows]
        assert res.vhash.cpu().tolist() == [r[6] for r in rows]
        assert res.tried.cpu().tolist() == [j for j, r in enumerate(rows) if r[7]]
        w.restore()


# ---------------------------------------------------------------- more than 4 GiB of output

def _rows_equal(buf, n: int, size: int, row) -> bool:
    """buf[: n * size] is `row` (a device tensor of `size` bytes) n times: compared on the device,
    at most 256 MiB at a time."""
    import torch
    ok = torch.ones((), dtype=torch.bool, device=buf.device)
    step = max(1, wide.SLICE // size)
    for a in range(0, n, step):
        b = min(n, a + step)
        ok &= (buf[a * size:b * size].view(b - a, size) == row).all()
    return bool(ok.item())


def test_read_more_than_4_gib_of_values(w):
    """One compressed 65,536-byte value requested 70,000 times: the plan's output total has a high
    word, comp_dst_off is the exclusive scan (entry 65,536 is exactly 2^32) and every decoded
    block is the value."""
    import torch
    from oracle import oracle as O
    from gobeansdb_amd import _lib, replay
    n, vlen = 70000, 65536
    value = O.gen_text(3, 1, vlen)
    body = O.compress(value)
    assert len(body) < 0.7 * vlen
    rec = R.make_record(b"big64k", body, flag=R.FLAG_COMPRESS, ver=2)
    decoy = R.make_record(b"dcy64k", bytes(len(body)), ver=9)
    at = B32 + (2 << 20)
    assert n * vlen > B32 and 65536 * vlen == B32 and R.read_record_at(decoy, 0) is not None
    w.place(w.big, at, rec)
    w.place(w.big, at - B32, decoy)
    rd = replay.read_records(w.big, [at] * n, keys=[b"big64k"] * n)
    torch.cuda.synchronize()
    assert rd.totals == (n, n, vlen, n * vlen)
    assert bool((rd.status == _lib.RD_OK).all()) and bool((rd.key_eq == 1).all()) and bool((rd.in_out == 1).all())
    assert bool((rd.flag == 0).all()) and bool((rd.value_len == vlen).all())
    assert bool((rd.vhash == R.getvhash(value)).all())
    want_off = torch.arange(n, dtype=torch.int64, device=w.device) * vlen
    assert torch.equal(rd.val_off, want_off) and torch.equal(rd.values.off, want_off)
    assert int(rd.values.off[65536]) == B32
    vt = torch.from_numpy(np.frombuffer(value, np.uint8).copy()).to(w.device)
    assert _rows_equal(rd.values.data, n, vlen, vt)
    for i in (0, 32767, 32768, 65535, 65536, 69999):
        assert rd.value(i) == value, i
    del rd, vt
    torch.cuda.empty_cache()


def _big_value(seed: int) -> bytes:
    """300 bytes short of BodyMax: its record takes 50 MiB less one slot."""
    return np.random.default_rng(seed).integers(0, 256, (50 << 20) - 300, dtype=np.uint8).tobytes()


def test_gc_destination_above_2_32(w):
    """One 50 MiB record listed 85 times ahead of a small chunk (rec_off may repeat): new_off,
    chunk_bytes and the totals pass 2^32; the 85 images are compared on the device, the rest with
    oracle.gc from head 85 * R (tests/test_wide_rules.py: the rule for a repeated record).  The
    small records go through the copy kernel and a 200,000-byte one through the long-record
    kernel, all to destinations above 2^32."""
    import torch
    import test_gpu_gc_batch as T
    from gobeansdb_amd import _lib, gc
    times = 85
    rec = R.make_record(b"fifty_m", _big_value(7), ver=4, ts=1700000000)
    size = len(rec)
    assert size == (50 << 20) - 256 and times * size > B32
    small = WR.chunk(44, 30) + R.make_record(b"long200k", np.random.default_rng(8).integers(
        0, 256, 200000, dtype=np.uint8).tobytes()) + WR.chunk(45, 10)
    srecs = R.stream_all(small)[0]
    keep = [i % 4 != 1 for i in range(len(srecs))]
    assert len(srecs) == 41 and keep[30]
    tail_chunks, tail_pos = G.gc_rewrite(small, keep, data_file_max=1 << 40, dst_head=times * size)
    assert all(p >= times * size > B32 for _, p in tail_pos)
    total = times * size + len(tail_chunks[0])
    src = torch.from_numpy(np.frombuffer(rec + small, np.uint8).copy()).to(w.device)
    out = torch.full((total + T.GUARD,), T.FILL, dtype=torch.uint8, device=w.device)
    rec_off = [0] * times + [size + r.offset for r in srecs]
    res = gc.rewrite_batch(src, torch.tensor(rec_off, dtype=torch.int64, device=w.device),
                           torch.tensor([True] * times + keep, device=w.device), data_file_max=1 << 40, out=out)
    torch.cuda.synchronize()
    written = (res.status == _lib.GC_WRITTEN).cpu().numpy()
    assert written.tolist() == [True] * times + keep
    assert res.new_off.cpu().numpy()[written].tolist() == [k * size for k in range(times)] + [p for _, p in tail_pos]
    assert not res.new_chunk.cpu().numpy().any()
    assert res.chunk_bytes.tolist() == [total]
    t = res.totals
    assert (int(t[2]), int(t[3]), int(t[4]) | int(t[5]) << 32) == (times + sum(keep), 1, total)
    assert (int(t[6]), int(t[7])) == (0, 0)
    assert int(t[5]) == 1
    assert _rows_equal(out, times, size, src[:size])
    assert out[times * size:total].cpu().numpy().tobytes() == tail_chunks[0]
    assert bool((out[total:] == T.FILL).all())
    want_crc = [int.from_bytes(rec[:4], "little")] * times + [r.crc for r, k in zip(srecs, keep) if k]
    assert res.crc.cpu().numpy().view(np.uint32)[written].tolist() == want_crc
    del res, out, src
    torch.cuda.empty_cache()


def test_encode_output_above_2_32(w):
    """85 client-compressed 50 MiB values from one val_off, then the policy edges: rec_off and
    the byte total pass 2^32."""
    import torch
    from test_gpu_write_batch import FILL, _expect
    from gobeansdb_amd import _dev, batch, record
    times = 85
    bigv = _big_value(9)
    image = R.make_record(b"k", bigv, flag=FCC, ver=1, ts=5)
    size = len(image)
    assert size == (50 << 20) - 256 and times * size > B32
    edges = _policy_cases()
    rows, tail, bound = _expect([b"k"] * len(edges), [c[0] for c in edges], [c[1] for c in edges],
                                [c[2] for c in edges], [5] * len(edges))
    total = times * size + len(tail)
    voffs, blob = [0] * times, bytearray(bigv)
    for v, _, _ in edges:
        blob += bytes(7)
        voffs.append(len(blob))
        blob += v
    dev = w.device
    vals = batch.BlockBatch(torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).to(dev), _dev.u64(voffs, dev),
                            _dev.u32([len(bigv)] * times + [len(c[0]) for c in edges], dev))
    n = times + len(edges)
    keys = batch.BlockBatch(torch.from_numpy(np.frombuffer(b"k", np.uint8).copy()).to(dev), _dev.u64([0] * n, dev),
                            _dev.u32([1] * n, dev))
    out = torch.full((total + 4096,), FILL, dtype=torch.uint8, device=dev)
    res = record.encode_batch(keys, vals, flags=[FCC] * times + [c[1] for c in edges],
                              vers=[1] * times + [c[2] for c in edges], ts=[5] * n, out=out, out_cap=total)
    torch.cuda.synchronize()
    t3 = _dev.readback(res.totals)
    assert (int(t3[0]), int(t3[1]) | int(t3[2]) << 32, int(t3[2])) == (n, total, 1)
    assert res.offset.cpu().tolist() == [k * size for k in range(times)] + [times * size + r[1] for r in rows]
    assert res.offset.cpu().tolist()[-1] > B32
    assert _dev.readback(res.crc).tolist() == [int.from_bytes(image[:4], "little")] * times + [r[5] for r in rows]
    assert res.vhash.cpu().tolist() == [R.getvhash(bigv)] * times + [r[6] for r in rows]
    img = torch.from_numpy(np.frombuffer(image, np.uint8).copy()).to(dev)
    assert _rows_equal(out, times, size, img)
    assert out[times * size:total].cpu().numpy().tobytes() == tail
    assert bool((out[total:] == FILL).all())
    del res, out, vals, img
    torch.cuda.empty_cache()


def test_encode_trial_buffer_above_2_32(w):
    """420,000 text values of 10,240 bytes: try_dst_off, the exclusive scan of pad256(10240 + 400)
    = 10,752, passes 2^32 at entry 399,458, and the plan's trial-bytes total has a high word (both
    read from qlzx_write_plan itself, which record.encode_batch does not return).  The entries
    whose trial slot lies below 2^32 hold one value, those at or above it another whose stream has
    another length: a slot address cut to 32 bits lies 5,120 bytes into the slot of an entry of the
    first value, inside its stream, so a compress or a finish that dropped the high word would
    damage those records or build these from other bytes.  Every record is compared."""
    import torch
    from oracle import oracle as O
    from test_gpu_write_batch import FILL, _expect
    from gobeansdb_amd import _dev, _lib, batch, record
    n, vlen, slot = 420000, 10240, 10752
    first = -(-B32 // slot)                       # the first entry whose trial slot starts at or above 2^32
    alias = first * slot - B32
    a, b = O.gen_text(2, vlen & 0xff, vlen), O.gen_text(5, 7, vlen)
    assert slot == (vlen + 400 + 255) // 256 * 256 and first == 399458 and alias == 5120 and n - first > 20000
    (ra,), img_a, _ = _expect([b"k"], [a], [0], [0], [3])
    (rb,), img_b, _ = _expect([b"k"], [b], [0], [0], [3])
    sa, sb = len(img_a), len(img_b)
    assert ra[3] == rb[3] == FC and ra[7] and rb[7]                  # both kept: the trial's output is the value
    assert ra[4] != rb[4] and sa != sb and alias < ra[4]             # other lengths; the aliased write hits a's stream
    total = first * sa + (n - first) * sb
    dev = w.device
    vals = batch.BlockBatch(torch.from_numpy(np.frombuffer(a + b, np.uint8).copy()).to(dev),
                            _dev.u64([0] * first + [vlen] * (n - first), dev), _dev.u32([vlen] * n, dev))
    keys = batch.BlockBatch(torch.from_numpy(np.frombuffer(b"k", np.uint8).copy()).to(dev), _dev.u64([0] * n, dev),
                            _dev.u32([1] * n, dev))
    # the plan alone: try_dst_off and totals as the device leaves them
    L = _lib.lib()
    zeros = torch.zeros(n, dtype=torch.int32, device=dev)
    status, try_idx, try_len = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    try_off, try_dst = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
    totals = torch.zeros(7, dtype=torch.int32, device=dev)
    wsb = L.qlzx_write_plan_workspace_size(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.qlzx_write_plan(vals.data.data_ptr(), vals.off.data_ptr(), vals.length.data_ptr(),
                                 keys.length.data_ptr(), zeros.data_ptr(), zeros.data_ptr(), n, 250, 50 << 20,
                                 record.not_compress_mask(record.NOT_COMPRESS), status.data_ptr(), try_idx.data_ptr(),
                                 try_off.data_ptr(), try_len.data_ptr(), try_dst.data_ptr(), totals.data_ptr(),
                                 ws.data_ptr(), wsb, batch._stream()), "qlzx_write_plan")
    t = _dev.readback(totals)
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    assert (int(t[0]), int(t[1]), int(t[2])) == (n, n, vlen)
    assert torch.equal(try_dst, ar * slot) and int(try_dst[first]) == B32 + alias
    assert torch.equal(try_idx, ar.to(torch.int32)) and torch.equal(try_off, vals.off) and bool((try_len == vlen).all())
    assert int(t[3]) | int(t[4]) << 32 == n * slot and int(t[4]) == 1
    del status, try_idx, try_len, try_off, try_dst, ws
    # the whole call
    out = torch.full((total + 4096,), FILL, dtype=torch.uint8, device=dev)
    res = record.encode_batch(keys, vals, ts=[3] * n, out=out, out_cap=total)
    torch.cuda.synchronize()
    assert res.counts == (n, n, n, 0)
    t3 = _dev.readback(res.totals)
    assert (int(t3[0]), int(t3[1]) | int(t3[2]) << 32) == (n, total)
    want_off = torch.where(ar < first, ar * sa, first * sa + (ar - first) * sb)
    assert torch.equal(res.offset, want_off) and bool((res.status == 0).all()) and bool((res.flag == FC).all())
    for lo, hi, row in ((0, first, ra), (first, n, rb)):
        assert bool((res.crc[lo:hi] == _dev.u32([row[5]], dev)).all()) and bool((res.vhash[lo:hi] == row[6]).all())
        assert bool((res.vsz[lo:hi] == row[4]).all())
    ta = torch.from_numpy(np.frombuffer(img_a, np.uint8).copy()).to(dev)
    tb = torch.from_numpy(np.frombuffer(img_b, np.uint8).copy()).to(dev)
    assert _rows_equal(out, first, sa, ta)
    assert _rows_equal(out[first * sa:], n - first, sb, tb)
    assert bool((out[total:] == FILL).all())
    del res, out, vals, keys, ta, tb
    torch.cuda.empty_cache()
