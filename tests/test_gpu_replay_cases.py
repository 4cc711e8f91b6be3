"""GPU: the .data replay (gobeansdb_amd/replay.py, csrc/qlzx_replay.hip) on the images of
tests/datafile_cases.py, each built to force one decision of the sequential reader: where Next()
lands against where only nextValid walks, the edges of max_key and body_max (both passed as
parameters), the ends of the file, embedded records, CRC spans around kRpLong and the segment
size, more than 64 long candidates, compressed bodies that do not decode, and two generated
files that push the scans, the destination-offset walk and the pointer doubling past their
batch sizes.  tests/test_datafile_cases.py shows on the host that every file reaches what it
claims and that the oracle returns the rows written down from the layout.

replay.replay's rows equal the oracle's in full (offset, sizeBroken, key, ver, flag and value
after Payload.Decompress, vhash) and end_error; replay.index's offsets, sizeBroken and end_error
equal the written-down rows, its candidate and valid counts those read from the file's headers."""
import numpy as np
import pytest
import torch

import datafile_cases as D
from oracle import replay as R
from tests.test_gpu_replay import _gpu

pytestmark = pytest.mark.gpu


def _case(name):
    return D.many_compressed() if name == "many_compressed" else D.by_name(name)


ALL = D.names() + ["many_compressed"]


@pytest.mark.parametrize("name", ALL)
def test_replay(cuda, name):
    c = _case(name)
    exp_rows, exp_err = R.replay(c.data, c.start, c.max_key, c.body_max)
    got_rows, got_err = _gpu(c.data, c.start, max_key=c.max_key, body_max=c.body_max)
    assert len(got_rows) == len(exp_rows)
    for g, e in zip(got_rows, exp_rows):
        assert g == e
    assert got_err == (exp_err is not None)
    # and the rows written down from the layout, without the oracle in between
    if c.family == "compressed":
        assert [(r[0], r[1], r[2], r[4], r[5]) for r in got_rows] == c.rows
    else:
        assert [r[:3] for r in got_rows] == c.rows
    assert got_err == (c.end_error is not None)


@pytest.mark.parametrize("name", ALL)
def test_index(cuda, name):
    from gobeansdb_amd import replay
    c = _case(name)
    t = torch.from_numpy(np.frombuffer(c.data, dtype=np.uint8).copy()).cuda()
    off, brk, err, ncand, nvalid = replay.index(t, start=c.start, max_key=c.max_key, body_max=c.body_max)
    torch.cuda.synchronize()
    assert off.cpu().tolist() == [r[0] for r in c.rows]
    assert brk.cpu().tolist() == [r[1] for r in c.rows]
    assert err == (c.end_error is not None)
    assert (ncand, nvalid) == D.counts(c)


# ---- million_slots: 262 MiB, built and copied to the device once ----
@pytest.fixture(scope="module")
def million(cuda):
    M = D.million_slots()
    t = torch.from_numpy(M.data).cuda()
    torch.cuda.synchronize()
    M = M._replace(data=None)       # the host copy goes; the expectations are arithmetic
    yield M, t
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("variant", ["intact", "broken", "start"])
def test_million_slots_index(million, variant):
    """Slots and valid records both beyond 1024 tiles of 1024: the tile-sum scan's second batch
    and its carry, in both compactions, and a chain of over a million records for the doubling.
    broken: the two-slot record of block 16450 (slot 1,069,270, valid record 1,052,820: behind
    the first batch of both scans) fails its CRC -- one record fewer, one sizeBroken of 512.
    start: the second slot of the two-slot record of block 9000, in the second half; the first
    record returned has sizeBroken 256."""
    from gobeansdb_amd import replay
    M, t = million
    i = (16450 if variant == "broken" else 9000) * D.MILLION_BLOCK + D.MILLION_TWO_SLOT
    pos = int(M.offsets[i])
    assert int(M.rs[i]) == 512 and pos > len(M.block) * M.reps // 2
    assert variant != "broken" or (pos // 256 > 1048576 and i > 1048576)
    kw = {"intact": {}, "broken": dict(broken_at=i), "start": dict(start=pos + 256)}[variant]
    exp_off, exp_brk = D.tiled_expect(M.offsets, M.rs, **kw)
    if variant == "broken":
        t[pos] = t[pos] ^ 0x40
    try:
        off, brk, err, ncand, nvalid = replay.index(t, start=kw.get("start", 0))
        torch.cuda.synchronize()
    finally:
        if variant == "broken":
            t[pos] = t[pos] ^ 0x40
    assert not err
    assert (ncand, nvalid) == (M.nrec, M.nrec - (variant == "broken"))
    assert np.array_equal(off.cpu().numpy(), exp_off)
    assert np.array_equal(brk.cpu().numpy(), exp_brk)
    assert len(exp_off) == {"intact": M.nrec, "broken": M.nrec - 1, "start": M.nrec - i - 1}[variant]


def test_million_slots_replay(million):
    """The whole replay on the intact file: every per-record field against the block's, tiled."""
    from gobeansdb_amd import replay
    M, t = million
    res = replay.replay(t)
    torch.cuda.synchronize()
    assert res.n == M.nrec and not res.end_error and (res.n_candidates, res.n_valid) == (M.nrec, M.nrec)
    hdr = np.stack([np.frombuffer(M.block[o:o + 24], "<i4") for o in M.block_off.tolist()])
    bodies = [M.block[o + 24 + h[4]: o + 24 + h[4] + h[5]] for o, h in zip(M.block_off.tolist(), hdr)]
    vh = np.asarray([R.getvhash(b) for b in bodies], np.int32)
    H = np.tile(hdr, (M.reps, 1))
    assert np.array_equal(res.offset.cpu().numpy(), M.offsets)
    assert not res.size_broken.cpu().numpy().any()
    assert np.array_equal(res.header.cpu().numpy(), H)
    assert np.array_equal(res.flag.cpu().numpy(), H[:, 2])
    assert np.array_equal(res.value_len.cpu().numpy(), H[:, 5])
    assert np.array_equal(res.vhash.cpu().numpy(), np.tile(vh, M.reps))
    assert not res.in_out.cpu().numpy().any()
    assert np.array_equal(res.val_off.cpu().numpy(), M.offsets + 24 + H[:, 4])
    assert res.values.off.numel() == 0
    j = M.nrec - 7
    assert res.value(j) == bodies[j % D.MILLION_BLOCK]
