#!/usr/bin/env python3
"""Batched record writes (record.encode_batch), a multi-SET, against record.encode.

Two workloads, values and keys resident on the device before the clock starts:

  text16k   --records-a (262,144) distinct 16 KiB text values: bench.py's record_encode leg
  mixed     --records-b (65,536) values log-uniform 4-64 KiB, 70 % text / 30 % image-like

For each, in one process: record.encode (the baseline: the host drives the policy in numpy) and
record.encode_batch (qlzx_write_plan / decide / finish: sizes, flags, offsets and CRCs stay on the
device) are timed per call (host wall, each call ends in a device synchronise), their outputs are
compared byte for byte on the device and by digest, and the host read-backs of one call are counted
(Tensor.cpu / item / tolist / __int__).  The GPU time inside the two qlzx_compress_batch calls of
encode_batch (events around batch.compress) bounds what this path can win.

Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0
AIM_GIBS = 40.0   # VERDICT.md's aim for f3, GiB/s of values


def log(*a):
    print("[write]", *a, file=sys.stderr, flush=True)


def make_values(kind: str, n: int, seed: int, dev):
    from gobeansdb_amd import batch
    if kind == "text16k":
        return batch.synth("text", seed, [16384] * n, first_id=0, device=dev)
    rng = np.random.default_rng(seed)
    lens = np.exp(rng.uniform(np.log(4096), np.log(65536), n)).astype(np.int64)
    text = rng.random(n) < 0.7
    vals = batch.BlockBatch.empty_for(lens, device=dev)
    for k, idx in (("text", np.nonzero(text)[0]), ("image", np.nonzero(~text)[0])):
        if len(idx):
            sel = torch.from_numpy(idx).to(dev)
            batch.synth(k, seed, lens[idx], first_id=0 if k == "text" else 1 << 40, device=dev,
                        out=batch.BlockBatch(vals.data, vals.off[sel].contiguous(), vals.length[sel].contiguous()))
    return vals


def timed(fn, reps: int):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out


class Readbacks:
    """Counts the device-to-host reads a call makes through torch."""
    NAMES = ("cpu", "item", "tolist", "__int__")

    def __enter__(self):
        self.count, self.depth, self.saved = 0, 0, {}
        for name in self.NAMES:
            orig = getattr(torch.Tensor, name)
            self.saved[name] = orig

            def wrap(t, *a, _orig=orig, **kw):
                if t.is_cuda and self.depth == 0:
                    self.count += 1
                self.depth += 1          # item() under __int__ / tolist() is the same read
                try:
                    return _orig(t, *a, **kw)
                finally:
                    self.depth -= 1
            setattr(torch.Tensor, name, wrap)
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(torch.Tensor, name, orig)


class CompressClock:
    """GPU time inside batch.compress (events on the current stream around each call)."""

    def __enter__(self):
        from gobeansdb_amd import batch
        self.batch, self.orig, self.spans = batch, batch.compress, []

        def wrap(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = self.orig(*a, **kw)
            e1.record()
            self.spans.append((e0, e1))
            return r
        batch.compress = wrap
        return self

    def __exit__(self, *exc):
        self.batch.compress = self.orig

    def ms(self):
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in self.spans]


def digest(t: torch.Tensor) -> str:
    """A position-dependent 64-bit digest of a device byte buffer (length a multiple of 256)."""
    w = t.view(torch.int64)
    idx = torch.arange(1, w.numel() + 1, dtype=torch.int64, device=t.device)
    return "%016x" % ((int((w * (2 * idx + 1)).sum()) ^ (int(w.sum()) << 1)) & 0xFFFFFFFFFFFFFFFF)


def leg(kind: str, n: int, seed: int, reps: int, dev):
    from gobeansdb_amd import batch, record
    vals = make_values(kind, n, seed, dev)
    torch.cuda.synchronize()
    vbytes = int(vals.length.to(torch.int64).sum())
    keys = [b"key_%016x" % (seed * 1000003 + i) for i in range(n)]
    klen = np.fromiter(map(len, keys), np.int32, count=n)
    koff, _ = batch.pack_offsets(klen, align=1)      # keys packed back to back
    kb = batch.BlockBatch(torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev),
                          torch.from_numpy(koff.view(np.int64)).to(dev), torch.from_numpy(klen).to(dev))
    vers = (np.arange(n) % 7).astype(np.int32)
    ts = (1700000000 + np.arange(n)).astype(np.uint32)
    vers_d, ts_d = torch.from_numpy(vers).to(dev), torch.from_numpy(ts.view(np.int32)).to(dev)
    ws = batch.Workspace(dev)
    # one call each: outputs equal, read-backs counted
    with Readbacks() as rb_old:
        old = record.encode(keys, vals, vers=vers, ts=ts, workspace=ws)
    torch.cuda.synchronize()
    with Readbacks() as rb_new:
        new = record.encode_batch(kb, vals, vers=vers_d, ts=ts_d, workspace=ws)
    torch.cuda.synchronize()
    t3 = new.totals.cpu().numpy().view(np.uint32)
    nbytes = int(t3[1]) | (int(t3[2]) << 32)
    assert int(t3[0]) == n and nbytes == int(old.data.numel()), (t3, old.data.numel())
    assert torch.equal(new.data[:nbytes], old.data), "encode_batch and encode differ"
    d_old, d_new = digest(old.data), digest(new.data[:nbytes])
    assert d_old == d_new
    assert np.array_equal(new.offset.cpu().numpy().view(np.uint64), old.offset)
    assert np.array_equal(new.crc.cpu().numpy().view(np.uint32), old.crc)
    ncomp = int((old.flag & 0x10000 != 0).sum())
    counts = new.counts
    del old, new
    torch.cuda.empty_cache()
    t_old = timed(lambda: record.encode(keys, vals, vers=vers, ts=ts, workspace=ws), reps)
    torch.cuda.empty_cache()
    t_new = timed(lambda: record.encode_batch(kb, vals, vers=vers_d, ts=ts_d, workspace=ws), reps)
    with CompressClock() as cc:
        t = time.perf_counter()
        record.encode_batch(kb, vals, vers=vers_d, ts=ts_d, workspace=ws)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        cms = cc.ms()
    alg = vbytes + nbytes

    def side(ts_, readbacks):
        med = float(np.median(ts_))
        return {"ms_per_call": round(med * 1e3, 3), "ms_per_call_min": round(min(ts_) * 1e3, 3),
                "values_gib_per_s": round(vbytes / med / 2**30, 2), "records_per_s": round(n / med),
                "host_readbacks": readbacks,
                "roofline": {"bound": "hbm", "achieved": round(alg / med / 1e9, 1), "peak": HBM_PEAK_GBS,
                             "unit": "GB/s", "frac": round(alg / med / 1e9 / HBM_PEAK_GBS, 4)}}
    a, b = side(t_old, rb_old.count), side(t_new, rb_new.count)
    out = {"workload": kind, "n": n, "value_bytes": vbytes, "record_bytes": nbytes, "stored_compressed": ncomp,
           "tried_kept_full": list(counts[1:]), "calls_timed": reps, "digest": d_new,
           "encode": a, "encode_batch": b,
           "speedup": round(a["ms_per_call"] / b["ms_per_call"], 2),
           "aim_gib_per_s": AIM_GIBS, "aim_met": b["values_gib_per_s"] >= AIM_GIBS,
           "compress_calls": {"gpu_ms": [round(x, 3) for x in cms], "call_wall_ms": round(wall * 1e3, 3),
                              "share_of_call": round(sum(cms) / (wall * 1e3), 3),
                              "what": "GPU time between events around the two qlzx_compress_batch calls of one "
                                      "encode_batch call, over that call's host wall time"},
           "what": "algorithmic bytes: every value byte read once + every record byte written once, over the median "
                   "host wall time of a call (every launch, read-back and allocation included); keys and values "
                   "are device-resident before the clock starts; encode_batch's outputs stay on the device"}
    log(json.dumps(out))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--records-a", type=int, default=262144)
    p.add_argument("--records-b", type=int, default=65536)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--seed", type=int, default=2028)
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_write.py needs a GPU"
    from gobeansdb_amd import build
    build.build()
    dev = torch.device("cuda", 0)
    legs = [leg("text16k", a.records_a, a.seed, a.reps, dev), leg("mixed", a.records_b, a.seed + 1, a.reps, dev)]
    print(json.dumps({
        "metric": "GiB/s of values, batched record writes (record.encode_batch), device-resident keys and values",
        "value": legs[0]["encode_batch"]["values_gib_per_s"], "unit": f"GiB/s of values at n = {legs[0]['n']} x 16 KiB",
        "baseline": {"what": "record.encode, same process, same inputs", "value": legs[0]["encode"]["values_gib_per_s"]},
        "legs": legs, "data": "synthetic"}), flush=True)


if __name__ == "__main__":
    main()
