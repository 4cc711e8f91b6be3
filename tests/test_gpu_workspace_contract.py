"""GPU: every batch entry point of the C ABI under a hostile workspace (tests/ws_contract.py): exactly
the bytes its caller sized with *_workspace_size(), at base % 256 == 16 (the alignment qlzx.h asks
for and no stricter), between two 64 KiB guards, and poisoned afresh before EVERY call with 0xFF,
0x5A or seeded random bytes.

Nothing new is computed or compared here: each test runs scenario code of the other GPU test files
(their helpers, expected-value functions and test bodies) with the proxy installed, so a pass means
the oracle's bytes, statuses, CRCs and totals, bit-exact, plus intact guards, under each poison.  A
result that changes with the poison is state read before it is written or carried from call to
call (the pairs plan/write, plan/decide/finish and index/plan each get a fresh poison per call); a
touched guard is an array sized too small or a scan that runs past its end.

Each test names the entry points it must reach (@reaches); the proxy counts the calls that came
with a non-null workspace and the test fails if one of them was not among them.  The last test
asserts that the names over the module are exactly the seventeen of ws_contract.ENTRY_POINTS.

The two back-to-back tests at the end use an ordinary shared workspace: the proxy synchronises
around each call, and they are about calls queued without a synchronisation in between."""
import ctypes
import functools
import random
from collections import Counter

import numpy as np
import pytest
import torch

import datafile_cases as D
import test_gpu_codec as CODEC
import test_gpu_crafted_streams as CS
import test_gpu_encoder_cases as EC
import test_gpu_gc_batch as GC
import test_gpu_hint as HINT
import test_gpu_hintlookup as HL
import test_gpu_hintmerge as HM
import test_gpu_level1 as L1
import test_gpu_read_batch as RB
import test_gpu_replay_cases as RC
import test_gpu_write_batch as WB
import ws_contract as W

pytestmark = pytest.mark.gpu

REACHES = {}    # test name -> the entry points it must reach with a non-null workspace
CALLS, LARGEST = Counter(), Counter()   # per entry point over the tests that ran: calls, largest workspace poisoned
every_poison = pytest.mark.parametrize("ws", ["ff", "5a", "random"], indirect=True)
ff_and_random = pytest.mark.parametrize("ws", ["ff", "random"], indirect=True)   # workspaces of gigabytes


@pytest.fixture
def ws(request, cuda, monkeypatch):
    """The proxy with the poison request.param, installed where _lib.lib() finds it."""
    from gobeansdb_amd import _lib
    proxy = W.Proxy(_lib.lib(), request.param)
    monkeypatch.setattr(_lib, "_lib", proxy)
    yield proxy
    for name, calls in proxy.calls.items():     # what the census test prints (pytest -s)
        CALLS[name] += calls
        LARGEST[name] = max(LARGEST[name], proxy.largest[name])


def reaches(*names):
    assert set(names) <= set(W.ENTRY_POINTS)

    def deco(fn):
        REACHES[fn.__name__] = names

        @functools.wraps(fn)
        def run(**kw):
            fn(**kw)
            kw["ws"].require(names)
        return run
    return deco


# ---- qlzx_decompress_batch ----
@every_poison
@pytest.mark.parametrize("route,max_dsize,nvalid,ninvalid", [
    pytest.param("uniform", CS.UNIFORM_MAX_DSIZE, 457, 120, id="uniform_457valid_120invalid"),
    pytest.param("mixed", CS.FAST_MAX_DSIZE, 606, 192, id="mixed_606valid_192invalid")])
@reaches("qlzx_decompress_batch")
def test_decode_k1_k2_crafted_streams(cuda, ws, route, max_dsize, nvalid, ninvalid):
    """K1 + K2 with the CRC prologue.  The invalid streams matter most: K1 stops early, and K2 must
    not consume GroupRecs or a BlkInfo that K1 never wrote."""
    CS._run_batch(CS._counted(route, nvalid, ninvalid), max_dsize, crc=True)


@every_poison
@reaches("qlzx_decompress_batch")
def test_decode_huge_crafted_streams(cuda, ws):
    """The whole-GPU decoder's scratch behind the batch decoder's regions."""
    sel = CS._counted("huge", 60, 46)
    CS._run_batch(sel, max(c[3] for c in sel))
    assert ws.largest["qlzx_decompress_batch"] > 30 * max(c[3] for c in sel)


@ff_and_random
@pytest.mark.parametrize("max_dsize,regions", [(2048, 2), (16385, 3)])
@reaches("qlzx_decompress_batch")
def test_decode_every_region(cuda, ws, max_dsize, regions):
    """More than one region, the full size of qlzx_decompress_workspace_size: two chunks in two
    regions, and three chunks in three with the last chunk's early K1."""
    from gobeansdb_amd import _lib
    n = CODEC._tiny_blocks()["src"].n          # (built through the proxy on the first use: poisoned too)
    full = _lib.lib().qlzx_decompress_workspace_size(n, max_dsize)
    assert full % regions == 0
    before = ws.calls["qlzx_decompress_batch"]
    CODEC._decode_tiny(max_dsize, full, crc=True)
    assert ws.calls["qlzx_decompress_batch"] == before + 1 and ws.largest["qlzx_decompress_batch"] == full


@every_poison
@reaches("qlzx_decompress_batch")
def test_decode_short_workspace_is_the_lane_route(cuda, ws):
    """The documented exception to QLZX_R_WORKSPACE: a workspace one byte below a region decodes
    lane-per-block, and has no use for the bytes it got."""
    from gobeansdb_amd import _lib, batch
    from oracle import oracle as O
    blocks = [O.gen_text(5, i, n) for i, n in enumerate((1, 300, 4096, 16384, 70000))]
    comp = [O.compress(b) for b in blocks]
    L = _lib.lib()
    # a call of one chunk has one region (its size for max_dsize 65536, which larger bounds are clamped to)
    short = L.qlzx_decompress_workspace_size(len(comp), 65536) - 1
    src = batch.BlockBatch.from_bytes(comp)
    out = batch.BlockBatch.empty_for([len(b) for b in blocks])
    dsize = torch.zeros(len(comp), dtype=torch.int32, device="cuda")
    status = torch.full((len(comp),), -1, dtype=torch.int32, device="cuda")
    buf = torch.empty(short, dtype=torch.uint8, device="cuda")
    b = _lib.Blocks(src.data.data_ptr(), src.off.data_ptr(), src.length.data_ptr(), out.data.data_ptr(),
                    out.off.data_ptr(), len(comp))
    rc = L.qlzx_decompress_batch(ctypes.byref(b), None, dsize.data_ptr(), status.data_ptr(), None, None, None,
                                 70000, buf.data_ptr(), short, batch._stream())
    assert rc == _lib.R_OK
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(comp)
    assert out.to_bytes(dsize.cpu().numpy()) == blocks


# ---- qlzx_compress_batch ----
@every_poison
@pytest.mark.parametrize("cap,count", [pytest.param(4096, 233, id="wg4096_233cases"),
                                       pytest.param(65536, 317, id="wg65536_317cases")])
@reaches("qlzx_compress_batch")
def test_encode_workgroup(cuda, ws, cap, count):
    EC._run_batch(EC._route(cap, count), cap, layout="aligned")


@every_poison
@reaches("qlzx_compress_batch")
def test_encode_lane_go_compat(cuda, ws):
    """The lane encoder's slabs (hash tables it must clear itself)."""
    EC._run_batch(EC._route(65536, 317), EC.WG_MAX_LEN, go=True)


@every_poison
@reaches("qlzx_compress_batch")
def test_encode_huge(cuda, ws):
    EC.test_huge_encoder(cuda, 62, False)
    assert ws.largest["qlzx_compress_batch"] > 70 * 65536


# ---- level 1 ----
@every_poison
@reaches("qlzx_go_l1_compress_batch", "qlzx_go_decompress_batch")
def test_level1_both_directions_and_the_corrupt_set(cuda, ws):
    l1 = L1._l1_vectors()
    assert len(l1) == 132
    L1.test_l1_decode_reference_streams(cuda, l1)
    L1.test_l1_compress_matches_oracle(cuda, l1)
    L1.test_l1_corrupt_status_matches_oracle(cuda, l1)


# ---- replay ----
REPLAY_IMAGES = RC.ALL          # every image of tests/datafile_cases.py; the million-slot file is not one of them


@every_poison
@reaches("qlzx_replay_index", "qlzx_replay_plan", "qlzx_decompress_batch")
def test_replay_every_image(cuda, ws):
    assert len(REPLAY_IMAGES) == len(D.names()) + 1 and "million_slots" not in REPLAY_IMAGES
    for name in REPLAY_IMAGES:
        try:
            RC.test_replay(cuda, name)
        except AssertionError as e:
            raise AssertionError(f"image {name}: {e}") from e


@every_poison
@reaches("qlzx_replay_index")
def test_index_every_image(cuda, ws):
    for name in REPLAY_IMAGES:
        try:
            RC.test_index(cuda, name)
        except AssertionError as e:
            raise AssertionError(f"image {name}: {e}") from e


# ---- batched reads ----
@every_poison
@reaches("qlzx_read_plan", "qlzx_decompress_batch")
def test_read_batch(cuda, ws):
    rfile = RB._rfile()
    RB.test_random_file_every_slot(cuda, rfile)
    RB.test_long_records(cuda)          # the long list and the whole-GPU decoder
    RB.test_corruption(cuda, rfile)


# ---- batched writes ----
@every_poison
@reaches("qlzx_write_plan", "qlzx_write_decide", "qlzx_write_finish", "qlzx_compress_batch")
def test_write_batch(cuda, ws):
    texts = WB._texts()
    WB.test_policy_edges(cuda, texts)
    WB.test_long_values(cuda, texts)    # the long list
    WB.test_stored_block(cuda)
    WB.test_batch_shapes(cuda, 1)
    WB.test_batch_shapes(cuda, 1100)    # more than one scan tile


# ---- GC ----
@every_poison
@reaches("qlzx_gc_plan", "qlzx_gc_rewrite", "qlzx_replay_index")
def test_gc_batch(cuda, ws):
    GC.test_matches_oracle_and_rewrite(cuda, 10, 4096, 1024, (512, 3584))   # rotates through three heads
    GC.test_every_tail_length(cuda)
    GC.test_long_records(cuda)
    GC.test_bad_entries(cuda)


# ---- hint build, merge, lookup ----
@every_poison
@reaches("qlzx_hint_plan", "qlzx_hint_write")
def test_hint_build(cuda, ws):
    HINT.test_several_thousand_records(cuda)                    # more than one workgroup sorts
    HINT.test_collisions_one_hash_for_257_distinct_keys(cuda)
    for split_cap in (1, 2, 64):
        HINT.test_cut_at_a_full_buffer(cuda, split_cap)


@every_poison
@reaches("qlzx_hint_merge_plan", "qlzx_hint_merge_write")
def test_hint_merge(cuda, ws):
    HM.test_six_thousand_items_over_five_sources(cuda)
    HM.test_one_hash_for_257_distinct_keys_over_3_sources(cuda, 0x1234567800000000)
    HM.test_bad_file(cuda, "last item cut short", 2)


@every_poison
@reaches("qlzx_hint_lookup")
def test_hint_lookup(cuda, ws):
    HL.test_request_and_file_counts(cuda, 65, 2)    # _check on a _spread case: QLZX_HL_F_LANE and QLZX_HL_F_WAVE
    HL.test_a_file_without_index_entries_is_walked_whole(cuda)


# ---- back to back on one stream, one shared workspace, no synchronisation in between ----
def _positions(off, ln):
    """The device index of every byte of every block (blocks at off[i], ln[i] bytes each)."""
    starts = torch.cumsum(ln, 0) - ln
    rel = torch.arange(int(ln.sum()), device=ln.device) - torch.repeat_interleave(starts, ln)
    return torch.repeat_interleave(off, ln) + rel


def test_back_to_back_decodes_share_a_workspace(cuda):
    """Two qlzx_decompress_batch calls queued on one stream over one workspace: the tiny blocks
    (three chunks, three regions, the early K1) and the same blocks in reverse order.  The second
    call's K1 and order pass start from whatever the first left in every region."""
    from gobeansdb_amd import batch
    t = CODEC._tiny_blocks()
    src, plain, lens = t["src"], t["plain"], t["lens"]
    rev = batch.BlockBatch(src.data, src.off.flip(0).contiguous(), src.length.flip(0).contiguous())
    out1, out2 = batch.BlockBatch.empty_for(lens), batch.BlockBatch.empty_for(lens[::-1])
    shared = batch.Workspace("cuda")
    torch.cuda.synchronize()
    d1, s1, _ = batch.decompress(src, out1, max_dsize=16385, workspace=shared)
    d2, s2, _ = batch.decompress(rev, out2, max_dsize=16385, workspace=shared)
    torch.cuda.synchronize()
    assert int((s1 != 0).sum()) == 0 and int((s2 != 0).sum()) == 0
    assert torch.equal(d1, plain.length) and torch.equal(d2, plain.length.flip(0))
    ln = plain.length.to(torch.int64)
    want = plain.data[_positions(plain.off, ln)]
    assert torch.equal(out1.data[_positions(out1.off, ln)], want)
    assert torch.equal(out2.data[_positions(out2.off.flip(0), ln)], want)    # block j of plain is block n-1-j there


def test_back_to_back_encode_batches_share_a_workspace(cuda):
    """Two record.encode_batch runs over one Workspace, the second smaller than the first and with
    other inputs; nothing is synchronised between them beyond the driver's own two read-backs."""
    from gobeansdb_amd import batch, record
    texts = WB._texts()
    k2 = [b"second%d" % i for i in range(6)]
    v2 = [texts[4096], texts[10241], texts[20000], texts[232], b"", texts[70000]]
    jobs = [WB._shape_inputs(1100), (k2, v2, [0] * 6, [1] * 6)]
    shared = batch.Workspace("cuda")
    runs = []
    for j, (keys, vals, flags, vers) in enumerate(jobs):
        ts = list(range(len(keys)))
        rows, data, bound = WB._expect(keys, vals, flags, vers, ts, record.NOT_COMPRESS, 250, 50 << 20)
        rng = random.Random(j)
        out = torch.full((bound + 512,), WB.FILL, dtype=torch.uint8, device="cuda")
        res = record.encode_batch(WB._pack(keys, rng), WB._pack(vals, rng), flags=flags, vers=vers, ts=ts, out=out,
                                  workspace=shared)
        runs.append((rows, data, out, res))
    torch.cuda.synchronize()
    for rows, data, out, res in runs:
        t3 = res.totals.cpu().numpy().view(np.uint32)
        assert (int(t3[0]), int(t3[1]) | (int(t3[2]) << 32)) == (len(rows), len(data))
        got = out.cpu().numpy()
        assert got[:len(data)].tobytes() == data and (got[len(data):] == WB.FILL).all()
        assert res.status.cpu().tolist() == [r[0] for r in rows]
        assert res.offset.cpu().tolist() == [r[1] for r in rows]
        assert res.crc.cpu().numpy().view(np.uint32).tolist() == [r[5] for r in rows]


# ---- the census ----
def test_census_every_entry_point_is_reached():
    """Every test above fails unless the entry points it names were intercepted with a non-null
    workspace, so their union is what this module covers: exactly the functions of qlzx.h that take
    a workspace.  A new entry point lands in ws_contract.ENTRY_POINTS through the header test of
    tests/test_ws_contract.py and fails here until a scenario reaches it."""
    named = set().union(*REACHES.values())
    assert named == set(W.ENTRY_POINTS) and len(named) == 17
    for name in W.ENTRY_POINTS:
        print(f"{name:28s} {CALLS[name]:6d} calls, largest workspace {LARGEST[name]:12d} bytes")
