#!/usr/bin/env python3
"""The hint merge of a bucket's split files (hint.merge: qlzx_hint_merge_plan /
qlzx_hint_merge_write) on files resident on the device, next to the hint.build calls that produced
them.

Two shapes; every source is the one split hint.build makes of a chunk of one-slot records (values
of 0-200 bytes, written on the device by record.encode_batch as tools/bench_hint.py's "small"):

  splits  --files-a (8) files of --items-a (131,072) items
  chunks  --files-b (4) files of --items-b (1,048,576) items

A chunk's keys are distinct; they are drawn from a universe 1.5 times a chunk's size, so about two
thirds of every file's keys are in any other file as well and the winner rule has work to do.  For
each shape, in one process: hint.build of every chunk (timed after a warm-up build, summed),
then hint.merge of the files timed per call after a warm-up call (host wall, each call ends in a
device synchronise; the read-back of totals is inside).  The two ABI calls are also timed on their
own with events.  The merged file is checked for its shape (numKey = the distinct keys over all
files, head consistent with the bytes), not against the model: tests/test_gpu_hintmerge.py does
that.  There is no CPU baseline: the reference's merge needs Go.

Prints one JSON line; --out also writes it to a file.
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

from tools.bench_write import Readbacks, timed  # noqa: E402

HBM_BYTES_PER_S = 8e12


def log(*a):
    print("[hintmerge]", *a, file=sys.stderr, flush=True)


def build_chunk(n: int, ident: np.ndarray, seed: int, dev):
    """A chunk of n one-slot records with the keys key_<ident>, on the device."""
    from gobeansdb_amd import batch, record
    rng = np.random.default_rng(seed)
    vals = batch.synth("image", seed, rng.integers(0, 201, n), first_id=0, device=dev)
    keys = [b"key_%016x" % int(i) for i in ident]
    klen = np.fromiter(map(len, keys), np.int32, count=n)
    koff, _ = batch.pack_offsets(klen, align=1)
    kb = batch.BlockBatch(torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev),
                          torch.from_numpy(koff.view(np.int64)).to(dev), torch.from_numpy(klen).to(dev))
    ts = torch.from_numpy((1700000000 + np.arange(n)).astype(np.uint32).view(np.int32)).to(dev)
    enc = record.encode_batch(kb, vals, vers=torch.from_numpy((np.arange(n) % 7).astype(np.int32)).to(dev), ts=ts)
    t3 = enc.totals.cpu().numpy().view(np.uint32)
    assert int(t3[0]) == n
    return enc.data[:int(t3[1]) | (int(t3[2]) << 32)].clone()


def phases(files, chunk_ids, reps: int):
    """GPU milliseconds (events) of qlzx_hint_merge_plan and qlzx_hint_merge_write, medians over reps calls."""
    from gobeansdb_amd import _lib, batch
    L = _lib.lib()
    dev = files[0].device
    lens = [int(f.numel()) for f in files]
    offs = np.cumsum([0] + lens[:-1]).astype(np.int64)
    hints = torch.cat(files)
    nbytes, n_files = int(hints.numel()), len(files)
    room = sum(x - 16 for x in lens)
    cap = room // 23
    off_d, len_d = torch.from_numpy(offs).to(dev), torch.tensor(lens, dtype=torch.int64, device=dev)
    chunk_d = torch.tensor(chunk_ids, dtype=torch.int32, device=dev)
    item_src, item_off = (torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(2))
    item_chunk, index_item, coll_item = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
    totals = torch.zeros(12, dtype=torch.int32, device=dev)
    out = torch.empty(16 + room + 16 * cap, dtype=torch.uint8, device=dev)
    wsb = L.qlzx_hint_merge_workspace_size(nbytes, n_files, cap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    s = batch._stream()
    ms = {"plan": [], "write": []}
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        _lib.check(L.qlzx_hint_merge_plan(hints.data_ptr(), nbytes, off_d.data_ptr(), len_d.data_ptr(),
                                          chunk_d.data_ptr(), n_files, cap, _lib.HINT_INDEX_INTERVAL,
                                          item_src.data_ptr(), item_chunk.data_ptr(), item_off.data_ptr(),
                                          index_item.data_ptr(), coll_item.data_ptr(), totals.data_ptr(),
                                          ws.data_ptr(), wsb, s), "qlzx_hint_merge_plan")
        ev[1].record()
        _lib.check(L.qlzx_hint_merge_write(hints.data_ptr(), nbytes, cap, item_src.data_ptr(), item_chunk.data_ptr(),
                                           item_off.data_ptr(), index_item.data_ptr(), out.data_ptr(), out.numel(),
                                           totals.data_ptr(), ws.data_ptr(), wsb, s), "qlzx_hint_merge_write")
        ev[2].record()
        torch.cuda.synchronize()
        if it:      # the first call is the warm-up
            ms["plan"].append(ev[0].elapsed_time(ev[1]))
            ms["write"].append(ev[1].elapsed_time(ev[2]))
    t = totals.cpu().numpy().view(np.uint32)
    assert t[_lib.HM_STATUS] == _lib.HM_OK
    return {k: round(float(np.median(v)), 3) for k, v in ms.items()}, cap, wsb


def leg(name: str, n_files: int, n: int, seed: int, reps: int, dev):
    from gobeansdb_amd import hint, replay
    rng = np.random.default_rng(seed)
    universe = n + n // 2
    files, every, build_s = [], set(), 0.0
    for c in range(n_files):
        ident = rng.permutation(universe)[:n] + seed * 1000003
        every.update(ident.tolist())
        res = replay.replay(build_chunk(n, ident, seed + c, dev))
        if c == 0:
            hint.build(res, chunk_id=c)            # the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        splits = hint.build(res, chunk_id=c)
        torch.cuda.synchronize()
        build_s += time.perf_counter() - t0
        assert len(splits) == 1 and splits[0].num_key == n
        files.append(splits[0].file.clone())
        del res, splits
        torch.cuda.empty_cache()
    chunk_ids = list(range(n_files))
    with Readbacks() as rb:
        m = hint.merge(files, chunk_ids)
    torch.cuda.synchronize()
    assert m.num_key == len(every) and m.items_read == n_files * n and m.collisions == []
    head = m.file[:16].cpu().numpy()
    assert int(head[:8].view(np.int64)[0]) == m.index_offset and int(head[8:12].view(np.uint32)[0]) == m.num_key
    assert m.index_offset + 16 * m.n_index == int(m.file.numel()) and m.n_index > 0
    file_bytes, item_bytes = int(m.file.numel()), m.index_offset - 16
    del m
    torch.cuda.empty_cache()
    t_m = timed(lambda: hint.merge(files, chunk_ids), reps)
    torch.cuda.empty_cache()
    t_gc = timed(lambda: hint.merge(files, chunk_ids, write=False), reps)
    torch.cuda.empty_cache()
    ph, cap, wsb = phases(files, chunk_ids, reps)
    med = float(np.median(t_m))
    moved = file_bytes + item_bytes                 # the file written, its items read from the sources
    out = {"shape": name, "files": n_files, "items_per_file": n, "items_read": n_files * n, "cap": cap,
           "source_bytes": sum(int(f.numel()) for f in files), "merged_keys": len(every),
           "merged_file_bytes": file_bytes, "workspace_bytes": wsb, "calls_timed": reps,
           "hint_merge_ms": round(med * 1e3, 3), "hint_merge_ms_min": round(min(t_m) * 1e3, 3),
           "hint_merge_plan_only_ms": round(float(np.median(t_gc)) * 1e3, 3),
           "hint_merge_host_readbacks": rb.count,
           "hint_merge_mitem_per_s": round(n_files * n / med / 1e6, 2),
           "hint_build_of_the_sources_ms": round(build_s * 1e3, 3),
           "hint_merge_over_hint_build": round(med / build_s, 3),
           "abi_gpu_ms": {**ph, "what": "GPU time between events around qlzx_hint_merge_plan and around "
                                        "qlzx_hint_merge_write, called through the C ABI with caller-provided buffers"},
           "write_bytes_moved": moved,
           "write_fraction_of_8TBps": round(moved / (ph["write"] * 1e-3) / HBM_BYTES_PER_S, 4),
           "what": "median host wall time of a call (packing the files into one buffer, every launch, read-back and "
                   "allocation included); the files are device-resident before the clock starts; "
                   "hint_build_of_the_sources_ms sums one timed hint.build per source chunk in the same process"}
    log(json.dumps(out))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--files-a", type=int, default=8)
    p.add_argument("--items-a", type=int, default=131072)
    p.add_argument("--files-b", type=int, default=4)
    p.add_argument("--items-b", type=int, default=1048576)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--seed", type=int, default=2032)
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_hintmerge.py needs a GPU"
    from gobeansdb_amd import build
    build.build()
    dev = torch.device("cuda", 0)
    legs = [leg("splits", a.files_a, a.items_a, a.seed, a.reps, dev),
            leg("chunks", a.files_b, a.items_b, a.seed + 1, a.reps, dev)]
    line = json.dumps({
        "metric": "ms per call, hint merge of device-resident split files (hint.merge)",
        "value": legs[0]["hint_merge_ms"], "unit": f"ms, {legs[0]['files']} files of {legs[0]['items_per_file']} items",
        "baseline": {"what": "hint.build of the same sources, same process (no CPU merge baseline: the reference "
                             "needs Go)", "value": legs[0]["hint_build_of_the_sources_ms"]},
        "legs": legs, "data": "synthetic"})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
