#!/usr/bin/env python3
"""The hint build of a replayed chunk (hint.build: qlzx_hint_plan / qlzx_hint_write) next to the
replay that feeds it, on one chunk resident on the device.

Two workloads; the chunk is built on the device by record.encode_batch, as tools/bench_gc.py's:

  mixed   --records-a (131,072) values log-uniform 4-64 KiB, 70 % text / 30 % image-like
  small   --records-b (1,048,576) values of 0-200 random bytes: one 256-B slot a record

A quarter of the records of each are later versions of an earlier key, so the last-version rule and
the runs of equal keyhash are exercised.  For each, in one process: replay.replay, then hint.build on
its result (default SplitCap and IndexIntervalSize: one split), each timed per call after a warm-up
call (host wall, each call ends in a device synchronise; hint.build's one read-back of totals is
inside).  The two ABI calls are also timed on their own with events.  The file is checked for its
shape (numKey = the distinct keys, every record consumed, head consistent with the bytes), not
against the model: tests/test_gpu_hint.py does that.

Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_write import Readbacks, make_values, timed  # noqa: E402


def log(*a):
    print("[hint]", *a, file=sys.stderr, flush=True)


def build_chunk(kind: str, n: int, seed: int, dev):
    """(chunk bytes, distinct keys) on the device: n records written by record.encode_batch, a
    quarter of them later versions of an earlier record's key."""
    from gobeansdb_amd import batch, record
    rng = np.random.default_rng(seed)
    if kind == "small":
        vals = batch.synth("image", seed, rng.integers(0, 201, n), first_id=0, device=dev)
    else:
        vals = make_values(kind, n, seed, dev)
    ident = np.arange(n)
    again = np.nonzero(rng.random(n) < 0.25)[0]
    again = again[again > 0]
    ident[again] = rng.integers(0, again)           # the key of an earlier record
    keys = [b"key_%016x" % (seed * 1000003 + int(i)) for i in ident]
    klen = np.fromiter(map(len, keys), np.int32, count=n)
    koff, _ = batch.pack_offsets(klen, align=1)
    kb = batch.BlockBatch(torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev),
                          torch.from_numpy(koff.view(np.int64)).to(dev), torch.from_numpy(klen).to(dev))
    ts = torch.from_numpy((1700000000 + np.arange(n)).astype(np.uint32).view(np.int32)).to(dev)
    enc = record.encode_batch(kb, vals, vers=torch.from_numpy((np.arange(n) % 7).astype(np.int32)).to(dev), ts=ts)
    t3 = enc.totals.cpu().numpy().view(np.uint32)
    assert int(t3[0]) == n
    return enc.data[:int(t3[1]) | (int(t3[2]) << 32)].clone(), len(set(keys))


def phases(res, reps: int):
    """GPU milliseconds (events) of qlzx_hint_plan and qlzx_hint_write, medians over reps calls."""
    from gobeansdb_amd import _lib, batch
    L = _lib.lib()
    dev = res.data.device
    size, n = int(res.data.numel()), res.n
    result = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev)
    hdr, vh = res.header.contiguous(), res.vhash.to(torch.int16).contiguous()
    item_rec, index_item = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    item_hash, item_off = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
    totals = torch.zeros(10, dtype=torch.int32, device=dev)
    out = torch.empty(16 + 289 * n, dtype=torch.uint8, device=dev)
    wsb = L.qlzx_hint_workspace_size(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    s = batch._stream()
    ms = {"plan": [], "write": []}
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        _lib.check(L.qlzx_hint_plan(res.data.data_ptr(), size, res.offset.data_ptr(), result.data_ptr(), n,
                                    hdr.data_ptr(), None, 0, _lib.HINT_SPLIT_CAP, _lib.HINT_INDEX_INTERVAL, 0,
                                    item_rec.data_ptr(), item_hash.data_ptr(), item_off.data_ptr(),
                                    index_item.data_ptr(), totals.data_ptr(), ws.data_ptr(), wsb, s), "qlzx_hint_plan")
        ev[1].record()
        _lib.check(L.qlzx_hint_write(res.data.data_ptr(), size, res.offset.data_ptr(), n, hdr.data_ptr(),
                                     vh.data_ptr(), 0, item_rec.data_ptr(), item_hash.data_ptr(), item_off.data_ptr(),
                                     index_item.data_ptr(), out.data_ptr(), out.numel(), totals.data_ptr(),
                                     ws.data_ptr(), wsb, s), "qlzx_hint_write")
        ev[2].record()
        torch.cuda.synchronize()
        if it:      # the first call is the warm-up
            ms["plan"].append(ev[0].elapsed_time(ev[1]))
            ms["write"].append(ev[1].elapsed_time(ev[2]))
    return {k: round(float(np.median(v)), 3) for k, v in ms.items()}


def leg(kind: str, n: int, seed: int, reps: int, dev):
    from gobeansdb_amd import hint, replay
    data, nkeys = build_chunk(kind, n, seed, dev)
    torch.cuda.synchronize()
    res = replay.replay(data)
    with Readbacks() as rb:
        splits = hint.build(res)
    torch.cuda.synchronize()
    assert res.n == n and len(splits) == 1
    sp = splits[0]
    assert (sp.consumed, sp.num_key, sp.skipped) == (n, nkeys, 0)
    head = sp.file[:16].cpu().numpy()
    assert int(head[:8].view(np.int64)[0]) == sp.index_offset and int(head[8:12].view(np.uint32)[0]) == nkeys
    assert sp.index_offset + 16 * sp.n_index == int(sp.file.numel()) and sp.n_index > 0
    file_bytes = int(sp.file.numel())
    del splits, sp
    torch.cuda.empty_cache()
    t_rp = timed(lambda: replay.replay(data), reps)
    torch.cuda.empty_cache()
    t_hb = timed(lambda: hint.build(res), reps)
    torch.cuda.empty_cache()
    ph = phases(res, reps)
    rp, hb = float(np.median(t_rp)), float(np.median(t_hb))
    out = {"workload": kind, "records": n, "distinct_keys": nkeys, "chunk_bytes": int(data.numel()),
           "hint_file_bytes": file_bytes, "calls_timed": reps,
           "replay_ms": round(rp * 1e3, 3), "replay_ms_min": round(min(t_rp) * 1e3, 3),
           "hint_build_ms": round(hb * 1e3, 3), "hint_build_ms_min": round(min(t_hb) * 1e3, 3),
           "hint_build_over_replay": round(hb / rp, 3), "hint_build_host_readbacks": rb.count,
           "hint_build_mrec_per_s": round(n / hb / 1e6, 2),
           "abi_gpu_ms": {**ph, "what": "GPU time between events around qlzx_hint_plan and around qlzx_hint_write, "
                                        "called through the C ABI with caller-provided buffers"},
           "what": "median host wall time of a call (every launch, read-back and allocation included); the chunk "
                   "is device-resident before the clock starts; hint.build runs on the replay's result"}
    log(json.dumps(out))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--records-a", type=int, default=131072)
    p.add_argument("--records-b", type=int, default=1048576)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--seed", type=int, default=2031)
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_hint.py needs a GPU"
    from gobeansdb_amd import build
    build.build()
    dev = torch.device("cuda", 0)
    legs = [leg("mixed", a.records_a, a.seed, a.reps, dev), leg("small", a.records_b, a.seed + 1, a.reps, dev)]
    line = json.dumps({
        "metric": "ms per call, hint split file build of a replayed chunk (hint.build)",
        "value": legs[0]["hint_build_ms"], "unit": f"ms, {legs[0]['workload']}",
        "baseline": {"what": "replay.replay of the same chunk, same process", "value": legs[0]["replay_ms"]},
        "legs": legs, "data": "synthetic"})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
