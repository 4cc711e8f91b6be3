#!/usr/bin/env python3
"""The device-resident GC rewrite (gc.rewrite_batch: qlzx_gc_plan / qlzx_gc_rewrite) against
gc.rewrite, on one chunk resident on the device.

Two workloads; the chunk is built on the device by record.encode_batch (TryCompress included), so
its records are what a gobeansdb writer would have stored:

  mixed   --records-a (131,072) values log-uniform 4-64 KiB, 70 % text / 30 % image-like
  small   --records-b (1,048,576) values of 0-600 random bytes: one to three 256-B slots a record

For each, in one process and on the same chunk and keep mask (~70 % kept, as bench.py's gc leg):
gc.rewrite (the baseline: header gather, host planning, qlzx_copy_batch, qlzx_crc32_batch) and
gc.rewrite_batch are run once and compared byte for byte, position by position and CRC by CRC, the
host read-backs of one call are counted (Tensor.cpu / item / tolist / __int__), then each is timed
per call after a warm-up call (host wall, each call ends in a device synchronise).  The two ABI
calls are also timed on their own with events (plan, rewrite) into a caller-provided buffer.

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

from tools.bench_write import HBM_PEAK_GBS, Readbacks, make_values, timed  # noqa: E402


def log(*a):
    print("[gc]", *a, file=sys.stderr, flush=True)


def build_chunk(kind: str, n: int, seed: int, dev):
    """(chunk bytes, record offsets) on the device: n records written by record.encode_batch."""
    from gobeansdb_amd import batch, record
    if kind == "small":
        lens = np.random.default_rng(seed).integers(0, 601, n)
        vals = batch.synth("image", seed, lens, first_id=0, device=dev)
    else:
        vals = make_values(kind, n, seed, dev)
    keys = [b"key_%016x" % (seed * 1000003 + i) for i in range(n)]
    klen = np.fromiter(map(len, keys), np.int32, count=n)
    koff, _ = batch.pack_offsets(klen, align=1)
    kb = batch.BlockBatch(torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev),
                          torch.from_numpy(koff.view(np.int64)).to(dev), torch.from_numpy(klen).to(dev))
    ts = torch.from_numpy((1700000000 + np.arange(n)).astype(np.uint32).view(np.int32)).to(dev)
    enc = record.encode_batch(kb, vals, vers=torch.from_numpy((np.arange(n) % 7).astype(np.int32)).to(dev), ts=ts)
    t3 = enc.totals.cpu().numpy().view(np.uint32)
    nbytes = int(t3[1]) | (int(t3[2]) << 32)
    assert int(t3[0]) == n
    return enc.data[:nbytes].clone(), enc.offset.clone()


def keep_mask(n: int, seed: int, dev):
    """~70 % of the records, from a stream of its own (the value lengths come from `seed`'s)."""
    return torch.from_numpy(np.random.default_rng(seed + 7919).random(n) < 0.7).to(dev)


def phases(data, rec_off, keep, reps: int):
    """GPU milliseconds (events) of qlzx_gc_plan and qlzx_gc_rewrite, medians over reps calls."""
    from gobeansdb_amd import _lib, batch, gc
    L = _lib.lib()
    dev = data.device
    size, n, mc = int(data.numel()), int(rec_off.numel()), 4
    result = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev)
    heads = torch.zeros(mc, dtype=torch.int64, device=dev)
    kp = keep.to(torch.uint8)
    i32 = lambda k=n: torch.empty(k, dtype=torch.int32, device=dev)   # noqa: E731
    i64 = lambda k=n: torch.empty(k, dtype=torch.int64, device=dev)   # noqa: E731
    status, new_chunk, new_off, crc, base, cb, totals = i32(), i32(), i64(), i32(), i64(mc), i64(mc), i32(8)
    out = torch.empty((size + 255) // 256 * 256, dtype=torch.uint8, device=dev)
    wsb = L.qlzx_gc_workspace_size(n, mc)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    s = batch._stream()
    ms = {"plan": [], "rewrite": []}
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        _lib.check(L.qlzx_gc_plan(data.data_ptr(), size, rec_off.data_ptr(), result.data_ptr(), n, kp.data_ptr(),
                                  250, 50 << 20, gc.DATA_FILE_MAX, heads.data_ptr(), mc, status.data_ptr(),
                                  new_chunk.data_ptr(), new_off.data_ptr(), base.data_ptr(), cb.data_ptr(),
                                  totals.data_ptr(), ws.data_ptr(), wsb, s), "qlzx_gc_plan")
        ev[1].record()
        _lib.check(L.qlzx_gc_rewrite(data.data_ptr(), size, rec_off.data_ptr(), result.data_ptr(), n,
                                     heads.data_ptr(), mc, new_chunk.data_ptr(), new_off.data_ptr(), base.data_ptr(),
                                     out.data_ptr(), out.numel(), status.data_ptr(), crc.data_ptr(),
                                     totals.data_ptr(), ws.data_ptr(), wsb, s), "qlzx_gc_rewrite")
        ev[2].record()
        torch.cuda.synchronize()
        if it:      # the first call is the warm-up
            ms["plan"].append(ev[0].elapsed_time(ev[1]))
            ms["rewrite"].append(ev[1].elapsed_time(ev[2]))
    return {k: round(float(np.median(v)), 3) for k, v in ms.items()}


def leg(kind: str, n: int, seed: int, reps: int, dev):
    from gobeansdb_amd import gc
    data, rec_off = build_chunk(kind, n, seed, dev)
    keep = keep_mask(n, seed, dev)
    torch.cuda.synchronize()
    # one call each: outputs equal, read-backs counted
    with Readbacks() as rb_old:
        old = gc.rewrite(data, rec_off, keep)
    torch.cuda.synchronize()
    with Readbacks() as rb_new:
        new = gc.rewrite_batch(data, rec_off, keep)
    torch.cuda.synchronize()
    assert len(old.chunks) == len(new.chunks) == 1 and old.crc_mismatch == 0 and int(new.totals[6]) == 0
    assert torch.equal(new.chunks[0], old.chunks[0]), "rewrite_batch and rewrite differ"
    r = new.result()
    assert np.array_equal(r.chunk, old.chunk) and np.array_equal(r.offset, old.offset)
    assert np.array_equal(r.crc, old.crc)
    kept_bytes, nk = int(old.chunks[0].numel()), int(new.totals[2])
    del old, new, r
    torch.cuda.empty_cache()
    t_old = timed(lambda: gc.rewrite(data, rec_off, keep), reps)
    torch.cuda.empty_cache()
    t_new = timed(lambda: gc.rewrite_batch(data, rec_off, keep), reps)
    torch.cuda.empty_cache()
    ph = phases(data, rec_off, keep, reps)

    def side(ts_, readbacks):
        med = float(np.median(ts_))
        return {"ms_per_call": round(med * 1e3, 3), "ms_per_call_min": round(min(ts_) * 1e3, 3),
                "gib_per_s": round(kept_bytes / med / 2**30, 2), "host_readbacks": readbacks,
                "roofline": {"bound": "hbm", "achieved": round(2 * kept_bytes / med / 1e9, 1), "peak": HBM_PEAK_GBS,
                             "unit": "GB/s", "frac": round(2 * kept_bytes / med / 1e9 / HBM_PEAK_GBS, 4)}}
    a, b = side(t_old, rb_old.count), side(t_new, rb_new.count)
    kern = ph["rewrite"] * 1e-3
    out = {"workload": kind, "records": n, "records_kept": nk, "chunk_bytes": int(data.numel()),
           "kept_bytes": kept_bytes, "calls_timed": reps, "rewrite": a, "rewrite_batch": b,
           "speedup": round(a["ms_per_call"] / b["ms_per_call"], 2),
           "abi_gpu_ms": {**ph, "rewrite_gib_per_s": round(kept_bytes / kern / 2**30, 1),
                          "rewrite_hbm_frac": round(2 * kept_bytes / kern / 1e9 / HBM_PEAK_GBS, 4),
                          "what": "GPU time between events around qlzx_gc_plan and around qlzx_gc_rewrite, called "
                                  "through the C ABI into a caller-provided buffer (no allocation, no read-back)"},
           "what": "algorithmic bytes: every kept record read once and written once, over the median host wall "
                   "time of a call (every launch, read-back and allocation included); the chunk, its record "
                   "offsets and the keep mask are device-resident before the clock starts"}
    log(json.dumps(out))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--records-a", type=int, default=131072)
    p.add_argument("--records-b", type=int, default=1048576)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--seed", type=int, default=2029)
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_gc.py needs a GPU"
    from gobeansdb_amd import build
    build.build()
    dev = torch.device("cuda", 0)
    legs = [leg("mixed", a.records_a, a.seed, a.reps, dev), leg("small", a.records_b, a.seed + 1, a.reps, dev)]
    line = json.dumps({
        "metric": "GiB/s of rewritten records, device-resident GC rewrite of a chunk (gc.rewrite_batch)",
        "value": legs[0]["rewrite_batch"]["gib_per_s"], "unit": f"GiB/s of rewritten records, {legs[0]['workload']}",
        "baseline": {"what": "gc.rewrite, same process, same chunk and keep mask",
                     "value": legs[0]["rewrite"]["gib_per_s"]},
        "legs": legs, "data": "synthetic"})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
