#!/usr/bin/env python3
"""Batched record reads at known offsets (replay.read_records), a multi-GET over one chunk.

A chunk file of --records records is built on the device (gobeansdb_amd.record.encode: values
log-uniform 4-64 KiB, 70 % text / 30 % image-like, the TryCompress policy, as c4 uses).  For N
in --n (64, 4096, 262144), N distinct record positions in random order are read:

  batched       replay.read_records over the resident chunk (check + CRC, plan, decode, finish)
  single_loop   the same records through replay.read_record, one request-service call each
                (N <= 4096 only; the record bytes are in host memory before the clock starts)
  cpu           oracle/_ref's crc32_write + qlz_decompress + Getvhash over the same records,
                gathered back to back in host memory, on 16 threads (when oracle/_ref is built)

Prints one JSON line.  Checked inside: every request OK and decoded, the delivered bytes equal
the raw sizes, and (N <= 4096) a sample of batched values equals the single-call loop's.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0
PART = 16384   # records encoded per call


def log(*a):
    print("[read]", *a, file=sys.stderr, flush=True)


def build_chunk(nrec: int, seed: int, dev):
    """(chunk on the device, record offsets u64, stored record bytes i64, raw value sizes i64)."""
    from gobeansdb_amd import batch, record
    rng = np.random.default_rng(seed)
    ws = batch.Workspace(dev)
    datas, offs, stored, raws, base = [], [], [], [], 0
    for p0 in range(0, nrec, PART):
        n = min(PART, nrec - p0)
        lens = np.exp(rng.uniform(np.log(4096), np.log(65536), n)).astype(np.int64)
        text = rng.random(n) < 0.7
        vals = batch.BlockBatch.empty_for(lens, device=dev)
        for kind, idx in (("text", np.nonzero(text)[0]), ("image", np.nonzero(~text)[0])):
            if len(idx):
                sel = torch.from_numpy(idx).to(dev)
                batch.synth(kind, seed, lens[idx], first_id=p0 * 7919 + (0 if kind == "text" else 1 << 40), device=dev,
                            out=batch.BlockBatch(vals.data, vals.off[sel].contiguous(), vals.length[sel].contiguous()))
        keys = [b"key_%016x" % (seed * 1000003 + p0 + i) for i in range(n)]
        enc = record.encode(keys, vals, vers=(np.arange(n) % 7).astype(np.int32),
                            ts=(1700000000 + p0 + np.arange(n)).astype(np.uint32), workspace=ws)
        torch.cuda.synchronize()
        datas.append(enc.data)
        offs.append(enc.offset.astype(np.uint64) + np.uint64(base))
        stored.append(24 + 20 + enc.vsz.astype(np.int64))
        raws.append(lens)
        base += int(enc.data.numel())
        assert base % 256 == 0
    return torch.cat(datas), np.concatenate(offs), np.concatenate(stored), np.concatenate(raws)


def timed(fn, reps: int):
    """Per-call host wall times (each call ends in a device synchronise), after one warm-up."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out


def cpu_leg(host: np.ndarray, nrec: int, seconds: float):
    """The reference record loop over `host` (the selected records back to back, 256-B padded)."""
    from bench import host_cpus
    from oracle import oracle as O
    Q, C = O.ref_if_built(), O.crc_ref_if_built()
    if Q is None or C is None:
        return None
    L = O.lib()
    usable, nproc, model = host_cpus()
    nthr = max(1, min(16, usable, nrec))
    dec = ctypes.cast(Q.qlz_decompress, ctypes.c_void_p).value
    crc = ctypes.cast(C.crc32_write, ctypes.c_void_p).value
    # cuts at record starts: walk the headers once
    starts, pos = [], 0
    while pos + 24 <= len(host):
        starts.append(pos)
        ksz, vsz = struct.unpack_from("<II", host, pos + 16)
        pos += (24 + ksz + vsz + 255) & ~255
    assert len(starts) == nrec
    cuts = np.asarray([starts[nrec * t // nthr] for t in range(nthr)] + [len(host)], np.uint64)
    bad = ctypes.c_uint64(0)
    best, reps, t_end = None, 0, time.time() + seconds
    while time.time() < t_end or reps == 0:
        ns = L.orc_bench_replay(dec, crc, host.ctypes.data, cuts.ctypes.data, nthr, 1, ctypes.byref(bad))
        if bad.value:
            raise RuntimeError(f"reference loop: {bad.value} records failed CRC/decompress")
        best = ns if best is None else min(best, ns)
        reps += 1
    return {"records_per_s": round(nrec / (best * 1e-9)), "ms": round(best * 1e-6, 3), "threads": nthr, "passes": reps,
            "nproc": nproc, "cpu_model": model, "kind": "reference crc32_write + qlz_decompress (output malloc per "
            "value) + Getvhash, contiguous record ranges per thread, best pass"}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--records", type=int, default=262144)
    p.add_argument("--n", type=int, nargs="+", default=[64, 4096, 262144])
    p.add_argument("--seed", type=int, default=2027)
    p.add_argument("--cpu-seconds", type=float, default=3.0)
    p.add_argument("--no-cpu", action="store_true")
    p.add_argument("--single-max", type=int, default=4096)
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_read.py needs a GPU"
    from gobeansdb_amd import replay, batch, build
    build.build()
    dev = torch.device("cuda", 0)
    t0 = time.time()
    chunk, rec_off, stored, raw = build_chunk(a.records, a.seed, dev)
    log(f"chunk: {a.records} records, {chunk.numel() / 2**20:.0f} MiB, raw values {raw.sum() / 2**20:.0f} MiB, "
        f"built in {time.time() - t0:.1f}s")
    ws = batch.Workspace(dev)
    rng = np.random.default_rng(a.seed + 1)
    legs = []
    for n in a.n:
        n = min(n, a.records)
        pick = rng.permutation(a.records)[:n]
        offs = torch.from_numpy(rec_off[pick].view(np.int64)).to(dev)
        keys = [b"key_%016x" % (a.seed * 1000003 + int(i)) for i in pick]
        res = replay.read_records(chunk, offs, keys=keys, workspace=ws)
        torch.cuda.synchronize()
        assert int((res.status != 0).sum()) == 0 and int((res.dec_status != 0).sum()) == 0
        assert int((res.key_eq != 1).sum()) == 0 and int(((res.flag & 0x10000) != 0).sum()) == 0
        vbytes = int(res.value_len.to(torch.int64).sum())
        assert vbytes == int(raw[pick].sum()), "delivered bytes"
        ncomp, maxd, out_bytes = res.totals[1:]
        written = int(res.values.length.to(torch.int64).sum())
        read = int(stored[pick].sum())
        reps = max(5, min(200, (1 << 20) // n))
        ts = timed(lambda: replay.read_records(chunk, offs, workspace=ws), reps)
        tk = timed(lambda: replay.read_records(chunk, offs, keys=keys, workspace=ws), max(3, reps // 4))
        med, best = float(np.median(ts)), float(min(ts))
        leg = {"n": n, "compressed": ncomp, "max_dsize": maxd, "calls_timed": reps,
               "ms_per_call": round(med * 1e3, 4), "ms_per_call_min": round(best * 1e3, 4),
               "us_per_record": round(med * 1e6 / n, 4), "records_per_s": round(n / med),
               "values_gib_per_s": round(vbytes / med / 2**30, 3),
               "with_keys_ms_per_call": round(float(np.median(tk)) * 1e3, 4),
               "roofline": {"bound": "hbm", "achieved": round((read + written) / med / 1e9, 2), "peak": HBM_PEAK_GBS,
                            "unit": "GB/s", "frac": round((read + written) / med / 1e9 / HBM_PEAK_GBS, 5),
                            "what": "algorithmic bytes over the median call time (host wall, the plan's read-back "
                                    "and every launch included): record bytes read once + decoded value bytes "
                                    "written once; raw values are delivered in place",
                            "bytes_read": read, "bytes_written": written}}
        host_recs = None
        if n <= a.single_max or not a.no_cpu:   # the selected records in host memory, request order
            ln = (stored[pick] + 255) // 256 * 256
            dst = np.zeros(n + 1, np.int64)
            dst[1:] = np.cumsum(ln)
            gathered = torch.zeros(int(dst[-1]), dtype=torch.uint8, device=dev)
            from gobeansdb_amd import record
            record._copy(chunk, rec_off[pick], stored[pick].astype(np.uint32), gathered, dst[:-1].astype(np.uint64))
            host_recs = gathered.cpu().numpy()
            del gathered
        if n <= a.single_max:
            recs = [host_recs[int(dst[i]): int(dst[i]) + int(stored[pick[i]])].tobytes() for i in range(n)]
            got = [replay.read_record(r) for r in recs[: min(n, 64)]]   # warm-up, and the cross-check
            for i, g in enumerate(got):
                assert g == (int(res.flag[i]), res.value(i)), f"request {i}: batched != single call"
            t = time.perf_counter()
            for r in recs:
                replay.read_record(r)
            one = time.perf_counter() - t
            leg["single_loop"] = {"ms": round(one * 1e3, 3), "us_per_record": round(one * 1e6 / n, 3),
                                  "records_per_s": round(n / one),
                                  "batched_speedup": round(one / med, 2),
                                  "what": "replay.read_record per record (host CRC fold of header + key, "
                                          "qlzx_read_record1 through the request service), one thread, record "
                                          "bytes already in host memory; checked equal to the batched values on "
                                          "the first 64"}
        if not a.no_cpu:
            cpu = cpu_leg(host_recs, n, a.cpu_seconds)
            leg["cpu"] = cpu
            if cpu:
                leg["cpu"]["batched_speedup"] = round(cpu["ms"] * 1e-3 / med, 2)
        legs.append(leg)
        log(json.dumps(leg))
        del res
    print(json.dumps({
        "metric": "records/s, batched reads at known offsets (replay.read_records), device-resident chunk",
        "value": legs[-1]["records_per_s"], "unit": f"records/s at N = {legs[-1]['n']}",
        "config": {"records": a.records, "chunk_bytes": int(chunk.numel()), "raw_value_bytes": int(raw.sum()),
                   "values": "log-uniform 4-64 KiB, 70 % text / 30 % image-like, TryCompress policy",
                   "positions": "N distinct record starts in random order", "seed": a.seed},
        "legs": legs, "data": "synthetic"}), flush=True)


if __name__ == "__main__":
    main()
