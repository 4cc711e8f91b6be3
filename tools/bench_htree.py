#!/usr/bin/env python3
"""The HTree build of a bucket from its split files (htree.build: qlzx_htree_plan /
qlzx_htree_write) on files resident on the device, next to hint.merge on the same files.

Two shapes, tools/bench_hintmerge.py's (its build_chunk makes the chunks; one record in seven has
ver 0, which updateHtreeFromHint applies as a remove):

  splits  --files-a (8) files of --items-a (131,072) items
  chunks  --files-b (4) files of --items-b (1,048,576) items

with --depth (1) and --height (3).  For each shape, in one process: hint.build of every chunk,
then htree.build (plan + write) and htree.build(write=False) (the plan alone) timed per call after
a warm-up call (host wall, each call ends in a device synchronise; the read-back of totals is
inside), and hint.merge on the same files timed the same way: both read the same bytes and sort
the same number of items.  The two ABI calls are also timed on their own with events.  The tree is
checked for its shape (ops read, the file's length from the slots, the root's count = the slots),
not against the model: tests/test_gpu_htree.py does that.  There is no CPU baseline: the
reference's bucket open needs Go.

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

from tools.bench_hintmerge import build_chunk  # noqa: E402
from tools.bench_write import Readbacks, timed  # noqa: E402


def log(*a):
    print("[htree]", *a, file=sys.stderr, flush=True)


def phases(files, chunk_ids, depth: int, height: int, reps: int):
    """GPU milliseconds (events) of qlzx_htree_plan and qlzx_htree_write, medians over reps calls."""
    from gobeansdb_amd import _lib, batch, htree
    L = _lib.lib()
    dev = files[0].device
    klen, nleaf = htree.geometry(depth, height)
    lens = [int(f.numel()) for f in files]
    offs = np.cumsum([0] + lens[:-1]).astype(np.int64)
    hints = torch.cat(files)
    nbytes, n_files = int(hints.numel()), len(files)
    cap = sum(x - 16 for x in lens) // 23
    off_d, len_d = torch.from_numpy(offs).to(dev), torch.tensor(lens, dtype=torch.int64, device=dev)
    chunk_d = torch.tensor(chunk_ids, dtype=torch.int32, device=dev)
    nodes = htree.level_base(height)
    node_count = torch.empty(nodes, dtype=torch.int32, device=dev)
    node_hash = torch.empty(nodes, dtype=torch.int16, device=dev)
    leaf_first = torch.empty(nleaf + 1, dtype=torch.int32, device=dev)
    slot_src = torch.empty(cap, dtype=torch.int64, device=dev)
    slot_chunk = torch.empty(cap, dtype=torch.int32, device=dev)
    totals = torch.zeros(10, dtype=torch.int32, device=dev)
    out = torch.empty(10 * nleaf + (klen + 11) * cap, dtype=torch.uint8, device=dev)
    wsb = L.qlzx_htree_workspace_size(nbytes, n_files, cap, height)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    s = batch._stream()
    ms = {"plan": [], "write": []}
    for it in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        _lib.check(L.qlzx_htree_plan(hints.data_ptr(), nbytes, off_d.data_ptr(), len_d.data_ptr(),
                                     chunk_d.data_ptr(), n_files, cap, depth, height, node_count.data_ptr(),
                                     node_hash.data_ptr(), leaf_first.data_ptr(), slot_src.data_ptr(),
                                     slot_chunk.data_ptr(), totals.data_ptr(), ws.data_ptr(), wsb, s),
                   "qlzx_htree_plan")
        ev[1].record()
        _lib.check(L.qlzx_htree_write(hints.data_ptr(), nbytes, cap, depth, height, node_count.data_ptr(),
                                      node_hash.data_ptr(), leaf_first.data_ptr(), slot_src.data_ptr(),
                                      slot_chunk.data_ptr(), out.data_ptr(), out.numel(), totals.data_ptr(),
                                      ws.data_ptr(), wsb, s), "qlzx_htree_write")
        ev[2].record()
        torch.cuda.synchronize()
        if it:      # the first call is the warm-up
            ms["plan"].append(ev[0].elapsed_time(ev[1]))
            ms["write"].append(ev[1].elapsed_time(ev[2]))
    t = totals.cpu().numpy().view(np.uint32)
    assert t[_lib.HT_STATUS] == _lib.HT_OK
    return {k: round(float(np.median(v)), 3) for k, v in ms.items()}, cap, wsb


def leg(name: str, n_files: int, n: int, seed: int, depth: int, height: int, reps: int, dev):
    from gobeansdb_amd import hint, htree, replay
    rng = np.random.default_rng(seed)
    universe = n + n // 2
    files = []
    for c in range(n_files):
        ident = rng.permutation(universe)[:n] + seed * 1000003
        res = replay.replay(build_chunk(n, ident, seed + c, dev))
        splits = hint.build(res, chunk_id=c)
        assert len(splits) == 1 and splits[0].num_key == n
        files.append(splits[0].file.clone())
        del res, splits
        torch.cuda.empty_cache()
    chunk_ids = list(range(n_files))
    klen, nleaf = htree.geometry(depth, height)
    with Readbacks() as rb:
        t = htree.build(files, chunk_ids, depth, height)
    torch.cuda.synchronize()
    assert t.n_ops == n_files * n == t.n_set + t.n_remove and 0 < t.n_slots <= t.n_set
    assert int(t.file.numel()) == 10 * nleaf + (klen + 11) * t.n_slots
    assert t.node(0, 0)[0] == t.n_slots == int(t.leaf_first[-1])
    shape = {"n_set": t.n_set, "n_remove": t.n_remove, "n_slots": t.n_slots, "file_bytes": int(t.file.numel())}
    del t
    torch.cuda.empty_cache()
    t_b = timed(lambda: htree.build(files, chunk_ids, depth, height), reps)
    torch.cuda.empty_cache()
    t_p = timed(lambda: htree.build(files, chunk_ids, depth, height, write=False), reps)
    torch.cuda.empty_cache()
    t_m = timed(lambda: hint.merge(files, chunk_ids), reps)
    torch.cuda.empty_cache()
    t_mp = timed(lambda: hint.merge(files, chunk_ids, write=False), reps)
    torch.cuda.empty_cache()
    ph, cap, wsb = phases(files, chunk_ids, depth, height, reps)
    med = float(np.median(t_b))
    out = {"shape": name, "files": n_files, "items_per_file": n, "ops_read": n_files * n, "cap": cap,
           "depth": depth, "height": height, **shape,
           "source_bytes": sum(int(f.numel()) for f in files), "workspace_bytes": wsb, "calls_timed": reps,
           "htree_build_ms": round(med * 1e3, 3), "htree_build_ms_min": round(min(t_b) * 1e3, 3),
           "htree_plan_only_ms": round(float(np.median(t_p)) * 1e3, 3),
           "htree_host_readbacks": rb.count,
           "htree_mop_per_s": round(n_files * n / med / 1e6, 2),
           "hint_merge_ms": round(float(np.median(t_m)) * 1e3, 3),
           "hint_merge_plan_only_ms": round(float(np.median(t_mp)) * 1e3, 3),
           "htree_build_over_hint_merge": round(med / float(np.median(t_m)), 3),
           "abi_gpu_ms": {**ph, "what": "GPU time between events around qlzx_htree_plan and around "
                                        "qlzx_htree_write, called through the C ABI with caller-provided buffers"},
           "what": "median host wall time of a call (packing the files into one buffer, every launch, read-back and "
                   "allocation included); the files are device-resident before the clock starts; hint_merge_* are "
                   "hint.merge on the same files in the same process"}
    log(json.dumps(out))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--files-a", type=int, default=8)
    p.add_argument("--items-a", type=int, default=131072)
    p.add_argument("--files-b", type=int, default=4)
    p.add_argument("--items-b", type=int, default=1048576)
    p.add_argument("--depth", type=int, default=1)
    p.add_argument("--height", type=int, default=3)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--seed", type=int, default=2032)
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_htree.py needs a GPU"
    from gobeansdb_amd import build
    build.build()
    dev = torch.device("cuda", 0)
    legs = [leg("splits", a.files_a, a.items_a, a.seed, a.depth, a.height, a.reps, dev),
            leg("chunks", a.files_b, a.items_b, a.seed + 1, a.depth, a.height, a.reps, dev)]
    line = json.dumps({
        "metric": "ms per call, HTree build from device-resident split files (htree.build)",
        "value": legs[0]["htree_build_ms"], "unit": f"ms, {legs[0]['files']} files of {legs[0]['items_per_file']} items",
        "baseline": {"what": "hint.merge of the same files, same process (no CPU baseline: the reference needs Go)",
                     "value": legs[0]["hint_merge_ms"]},
        "legs": legs, "data": "synthetic"})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
