"""The record-file batch calls past their grid caps and scan carries ("Counts beyond
the grid caps"): record.encode_batch, replay.read_records and gc.rewrite_batch at 1,056,000 items,
encode_batch at 8,192 + 65, and a long list of more than 8,192 segments through the write, the
index, the batched read and the GC rewrite.  Inputs and expectations are tests/scale.py's, whose
rules tests/test_scale_rules.py holds against the models; every comparison is exact and made on
the device where the arrays are large."""
import numpy as np
import pytest
import torch

import scale as S

pytestmark = pytest.mark.gpu
FILL = 0xAA


def _t(a, cuda, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return t if dtype is None else t.to(dtype)


def _packed(blocks, cuda):
    """The blocks back to back behind one odd byte: (device buffer, offsets, lengths as arrays)."""
    lens = np.array([len(b) for b in blocks], np.int64)
    offs = 1 + np.cumsum(lens) - lens
    buf = np.frombuffer(b"\x5c" + b"".join(blocks) + b"\x5c" * 16, np.uint8)
    return _t(buf, cuda), offs, lens


# ------------------------------------------------------------------ writes ----
@pytest.fixture(scope="module")
def writes(cuda):
    """The block's keys and values once on the device, their offsets tiled N / 64 times; the
    expectation uploaded."""
    from gobeansdb_amd import batch
    reps = S.N // S.WRITE_BLOCK
    keys, vals, flags, vers, ts = S.write_block()
    e = S.write_expect(reps)
    kbuf, koff, klen = _packed(keys, cuda)
    vbuf, voff, vlen = _packed(vals, cuda)
    tile = lambda a, dt: _t(np.asarray(a), cuda, dt).repeat(reps)     # noqa: E731
    inp = dict(keys=batch.BlockBatch(kbuf, tile(koff, torch.int64), tile(klen, torch.int32)),
               values=batch.BlockBatch(vbuf, tile(voff, torch.int64), tile(vlen, torch.int32)),
               flags=tile(flags, torch.int32), vers=tile(vers, torch.int32), ts=tile(ts, torch.int32))
    want = {k: _t(getattr(e, k).astype(np.int64), cuda)
            for k in ("status", "offset", "flag", "vsz", "crc", "vhash", "tried")}
    want["block"] = _t(np.frombuffer(e.block, np.uint8), cuda)
    torch.cuda.synchronize()
    yield inp, e, want
    del inp, want
    torch.cuda.empty_cache()


def test_scale_writes(writes):
    """1,056,000 records: the second trip of k_wr_plan / decide / sizes / apply / vhash, and
    k_scan_top's second batch with its carry in every compaction of the write plan (the trial list
    holds 198,000 entries, the records 1,031 tiles).  The data is the block's records tiled."""
    from gobeansdb_amd import record
    inp, e, want = writes
    reps = S.N // S.WRITE_BLOCK
    for k in ("k_wr_plan", "k_wr_decide", "k_wr_sizes", "k_wr_apply", "k_wr_vhash"):
        assert inp["values"].n == S.N > S.over("qlzx_write.hip", k)
    assert S.N > S.SCAN_TOP.over and e.nbytes == len(e.block) * reps and e.nbytes < 320e6
    out = torch.full((e.bound + 512,), FILL, dtype=torch.uint8, device=inp["flags"].device)
    res = record.encode_batch(inp["keys"], inp["values"], flags=inp["flags"], vers=inp["vers"], ts=inp["ts"], out=out)
    torch.cuda.synchronize()
    t3 = res.totals.cpu().numpy().view(np.uint32)
    assert (int(t3[0]), int(t3[1]) | int(t3[2]) << 32) == (e.written, e.nbytes)
    assert res.counts == e.counts
    u32 = lambda t: t.to(torch.int64) & 0xFFFFFFFF     # noqa: E731
    for name, got in (("status", res.status.to(torch.int64)), ("offset", res.offset), ("flag", u32(res.flag)),
                      ("vsz", u32(res.vsz)), ("crc", u32(res.crc)), ("vhash", res.vhash.to(torch.int64)),
                      ("tried", res.tried.to(torch.int64))):
        bad = torch.nonzero(got != want[name])
        assert bad.numel() == 0, (name, int(bad[0]), int(bad.numel()))
    bad = torch.nonzero(out[:e.nbytes].view(reps, len(e.block)) != want["block"][None, :])
    assert bad.numel() == 0, (bad[0].tolist(), int(bad.shape[0]))
    assert bool((out[e.nbytes:] == FILL).all())


def test_scale_writes_wave_cap(cuda):
    """8,192 + 65 records of mixed sizes, out_cap cut inside the last record: a wave of
    k_wr_assemble takes a second record.  Against the write tests' full expectation."""
    from test_gpu_write_batch import NO_SPACE, _run, _shape_inputs
    assert S.WAVE_N > S.over("qlzx_write.hip", "k_wr_assemble")
    keys, vals, flags, vers = _shape_inputs(S.WAVE_N)
    res, rows = _run(keys, vals, flags=flags, vers=vers, ts=list(range(S.WAVE_N)), short=100, seed=S.WAVE_N)
    assert [r[0] for r in rows[-2:]] == [0, NO_SPACE] and len({len(r[2]) for r in rows}) >= 3


# ------------------------------------------------------------------ reads ----
@pytest.fixture(scope="module")
def reads(cuda):
    from test_gpu_read_batch import _expect
    b = S.read_base()
    rows = [_expect(b.data, int(o)) for o in b.offsets]
    idx = S.tile_index(S.N, S.READ_BASE, torch).to(cuda)          # built with torch: no loop over N
    data = _t(np.frombuffer(b.data, np.uint8), cuda)
    offsets = _t(b.offsets, cuda)[idx]
    host_idx = S.tile_index(S.N, S.READ_BASE)
    assert np.array_equal(idx.cpu().numpy(), host_idx)
    wanted = [b.wanted[i] for i in host_idx.tolist()]
    torch.cuda.synchronize()
    yield data, offsets, rows, wanted
    del data, offsets, idx
    torch.cuda.empty_cache()


@pytest.mark.parametrize("with_keys", [False, True])
def test_scale_reads(reads, with_keys):
    """1,056,000 requests over one small chunk: the second trip of k_rd_check (8,192 waves of 64
    requests), of the finish kernels, and k_scan_top's second batch in the read plan's compaction
    (over 330,000 planned requests, each decoded into a place of its own)."""
    from gobeansdb_amd import replay
    data, offsets, rows, wanted = reads
    for k in ("k_rd_check", "k_rp_finish_vals", "k_rp_finish_comp", "k_rp_vhash2"):
        assert offsets.numel() == S.N > S.over("qlzx_read.hip", k)
    assert S.N > S.SCAN_TOP.over
    e = S.read_expect(S.N, rows, with_keys)
    res = replay.read_records(data, offsets, keys=wanted if with_keys else None)
    torch.cuda.synchronize()
    assert res.n == S.N and res.totals == e.totals and res.values.n == e.totals[1] > 300000
    dev = data.device
    cols = [("status", res.status, e.status), ("header", res.header, e.header), ("flag", res.flag, e.flag),
            ("value_len", res.value_len, e.value_len), ("vhash", res.vhash, e.vhash), ("in_out", res.in_out, e.in_out),
            ("val_off", res.val_off, e.val_off), ("dec_ok", res.dec_status == 0, e.dec_ok)]
    if with_keys:
        cols.append(("key_eq", res.key_eq, e.key_eq))
    else:
        assert res.key_eq is None
    for name, got, want in cols:
        w = _t(want, dev).to(got.dtype)
        bad = torch.nonzero((got != w).reshape(S.N, -1).any(dim=1))
        assert bad.numel() == 0, (name, int(bad[0]), int(bad.numel()))
    # the decoded bytes themselves, behind the first batch of both scans
    idx = S.tile_index(S.N, S.READ_BASE)
    late = ([i for i in range(S.N - 3000, S.N) if e.in_out[i]][:5]
            + [i for i in range(S.TWO20, S.TWO20 + 3000) if e.in_out[i]][:5])
    assert len(late) == 10
    for i in late:
        assert res.value(i) == rows[idx[i]][3]


# ------------------------------------------------------------------ gc ----
@pytest.fixture(scope="module")
def gcs(cuda):
    """The million_slots image on the device; the host copy goes, the expectations are arithmetic."""
    import datafile_cases as D
    M = D.million_slots()
    t = torch.from_numpy(M.data).to(cuda)
    crc_block = np.array([int.from_bytes(M.block[o:o + 4], "little") for o in M.block_off.tolist()], np.uint32)
    M = M._replace(data=None)
    shape = S.gc_shape(M)
    torch.cuda.synchronize()
    yield M, t, crc_block, shape, _t(M.offsets, cuda), _t(shape.keep, cuda)
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("variant", ["whole", "max_chunks", "out_cap"])
def test_scale_gc(gcs, variant):
    """gc.rewrite_batch over 1,056,000 records, some 700,000 of them kept: the second trip of
    k_gc_check / k_gc_place, a wave of k_gc_copy with hundreds of records, and k_rp_dstoff (the plan's
    scan of the sizes, one workgroup) with 66,000 sizes per wave.  Six rotations, the last one
    behind record 2^20.  max_chunks: exhausted in the second half; out_cap: one record short.  Every per-record output, every chunk's bytes (and
    through the placement its base), the totals and the whole destination buffer."""
    from gobeansdb_amd import gc
    M, data, crc_block, shape, rec_off, keep = gcs
    for k in ("k_gc_check", "k_gc_place", "k_gc_copy"):
        assert M.nrec == S.N > S.over("qlzx_gc.hip", k)
    assert S.N > S.DSTOFF.over and (S.N + 15) // 16 >= 65536
    whole = S.gc_expect(M, crc_block, shape)
    total = int(whole.chunk_bytes.sum())
    assert len(whole.rotations) >= 5 and whole.rotations[-1] > S.TWO20 and 64 * shape.named[1] > S.TWO20
    kw, e = {}, whole
    if variant == "max_chunks":
        mc = int(whole.new_chunk[S.N // 2]) + 2              # the chunk in use at the middle and one more
        assert mc < len(whole.chunk_bytes) and whole.rotations[mc - 1] > S.N // 2
        kw, e = dict(max_chunks=mc), S.gc_expect(M, crc_block, shape, max_chunks=mc)
        assert int((e.status == S.GC_NO_CHUNK).sum()) > 1000
    elif variant == "out_cap":
        e = S.gc_expect(M, crc_block, shape, out_cap=total - 256)
        assert int((e.status == S.GC_NO_SPACE).sum()) == 1
    dev = data.device
    out = torch.full((total + 4096,), FILL, dtype=torch.uint8, device=dev)
    res = gc.rewrite_batch(data, rec_off, keep, dst_head=shape.dst_head, data_file_max=S.GC_DFM, next_heads=shape.next_heads,
                           out=out[:total - 256] if variant == "out_cap" else out, **kw)
    torch.cuda.synchronize()
    assert [int(x) for x in res.totals] == e.totals
    assert [int(x) for x in res.chunk_bytes] == e.chunk_bytes.tolist()
    for name, got, want in (("status", res.status, e.status), ("new_chunk", res.new_chunk, e.new_chunk),
                            ("new_off", res.new_off, e.new_off), ("crc", res.crc, e.crc.view(np.int32))):
        bad = torch.nonzero(got != _t(want, dev))
        assert bad.numel() == 0, (name, int(bad[0]), int(bad.numel()))
    want = torch.full_like(out, FILL)
    want.view(-1, 256)[_t(e.dst_slot, dev)] = data.view(-1, 256)[_t(e.src_slot, dev)]
    bad = torch.nonzero((out != want).view(-1, 256).any(dim=1))
    assert bad.numel() == 0, (int(bad[0]) * 256, int(bad.numel()))


# ------------------------------------------------------------------ long lists ----
@pytest.fixture(scope="module")
def longs(cuda):
    L = S.long_list()
    vbuf, voff, vlen = _packed(L.vals, cuda)          # the values from byte 1 on: no source is aligned
    kbuf, koff, klen = _packed(L.keys, cuda)
    want = _t(np.frombuffer(L.data, np.uint8), cuda)
    torch.cuda.synchronize()
    yield L, (kbuf, koff, klen), (vbuf, voff, vlen), want
    del vbuf, kbuf, want
    torch.cuda.empty_cache()


def test_scale_long_lists(longs):
    """More than 8,192 segments over the whole long list: g % nw wraps in k_rec_long (the write and
    the GC rewrite) and in k_rp_crc_long (the batched read and the replay's index).  The written
    chunk is read back with one byte flipped in the ninth long value."""
    from gobeansdb_amd import _lib, batch, gc, record, replay
    L, (kbuf, koff, klen), (vbuf, voff, vlen), want = longs
    dev = want.device
    for f, k in (("qlzx_write.hip", "k_rec_long"), ("qlzx_gc.hip", "k_rec_long"), ("qlzx_read.hip", "k_rp_crc_long"),
                 ("qlzx_replay.hip", "k_rp_crc_long")):
        assert L.segments > S.over(f, k) == 8192
    n, total = len(L.keys), len(L.data)
    crcs = [int.from_bytes(r[:4], "little") for r in L.records]
    # the write
    out = torch.full((total + 4096,), FILL, dtype=torch.uint8, device=dev)
    res = record.encode_batch(batch.BlockBatch(kbuf, _t(koff, dev), _t(klen, dev).to(torch.int32)),
                              batch.BlockBatch(vbuf, _t(voff, dev), _t(vlen, dev).to(torch.int32)),
                              flags=L.flags, vers=L.vers, ts=L.ts, out=out, out_cap=total)
    torch.cuda.synchronize()
    assert res.counts == (n, 0, 0, 0) and res.status.cpu().tolist() == [0] * n
    assert res.offset.cpu().tolist() == L.offsets.tolist()
    assert res.crc.cpu().numpy().view(np.uint32).tolist() == crcs
    assert torch.equal(out[:total], want) and bool((out[total:] == FILL).all())
    # the index and the batched read of the written chunk
    chunk = out[:total]
    off, brk, err, ncand, nvalid = replay.index(chunk)
    torch.cuda.synchronize()
    assert not err and (ncand, nvalid) == (n, n) and off.cpu().tolist() == L.offsets.tolist() and not brk.any()
    ninth = 9                                          # the small record stands at 4
    assert L.keys[ninth] == b"lng_8"
    pos = int(L.offsets[ninth]) + 24 + 5 + 11 * (1 << 20) + 3
    chunk[pos] ^= 0x10
    rd = replay.read_records(chunk, off, keys=L.keys)
    torch.cuda.synchronize()
    chunk[pos] ^= 0x10
    ok = [i != ninth for i in range(n)]
    assert rd.status.cpu().tolist() == [_lib.RD_OK if o else _lib.RD_CRC for o in ok]
    assert rd.key_eq.cpu().tolist() == [int(o) for o in ok] and rd.totals[:2] == (n - 1, 0)
    assert rd.header.cpu().numpy().tobytes() == b"".join(r[:24] for r in L.records)
    assert rd.value_len.cpu().tolist() == [len(v) if o else 0 for v, o in zip(L.vals, ok)]
    assert rd.vhash.cpu().tolist() == [S.R.getvhash(v) if o else 0 for v, o in zip(L.vals, ok)]
    assert rd.val_off.cpu().tolist() == [int(a) + 24 + len(k) if o else 0 for a, k, o in zip(L.offsets, L.keys, ok)]
    assert not rd.in_out.any()
    # the GC rewrite, keeping all
    gout = torch.full((total + 4096,), FILL, dtype=torch.uint8, device=dev)
    g = gc.rewrite_batch(chunk, off, torch.ones(n, dtype=torch.bool, device=dev), out=gout)
    torch.cuda.synchronize()
    assert g.status.cpu().tolist() == [_lib.GC_WRITTEN] * n and g.new_off.cpu().tolist() == L.offsets.tolist()
    assert g.crc.cpu().numpy().view(np.uint32).tolist() == crcs and not g.new_chunk.any()
    assert torch.equal(gout[:total], want) and bool((gout[total:] == FILL).all())
    assert [int(x) for x in g.chunk_bytes] == [total]
