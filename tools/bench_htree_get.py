#!/usr/bin/env python3
"""The queries over a built HTree (include/qlzx_htree_get.h) on trees resident on the device.

Every number is GPU time between events around one ABI call with caller-provided buffers (no
allocation, no read-back inside), the median over --reps calls after a warm-up call, as
tools/bench_htree.py times its two calls.

  get sweep   a tree of --items (1,048,576) items at (depth, height) = (1, 3) and (2, 5): 4,096
              and 16 items per leaf; then (1, 4) with --items and a quarter of them: 256 and 64 per
              leaf.  n = 64 ... 1,048,576 keys (nine in ten present), hashes given; each kernel shape
              (QLZX_HTG_F_WAVE / QLZX_HTG_F_LANE) is timed at every n, and their outputs compared.
  old route   the same keys through qlzx_hint_lookup over the merged hint file of the same items
              (hint.merge of the tree's source), hashes given, the shape by n as the library picks it.
  index       qlzx_htree_index of the tree's image, and of the same image with a ver < 0 item in
              every 16th leaf (its count one less: the places cannot be proven from that leaf on).
  gc          tools/bench_gc.py's two chunks (131,072 mixed records, 1,048,576 small ones), the tree
              built from the chunk's own hints: qlzx_gc_liveness, qlzx_gc_plan, qlzx_gc_rewrite
              and qlzx_htree_move, each timed on its own.

The results are checked for their shape (found counts, totals), not against the model:
tests/test_gpu_htree_get.py does that.  Prints one JSON line; --out also writes it to a file.
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

from tools.bench_gc import build_chunk  # noqa: E402

SWEEP = (64, 1024, 4096, 16384, 65536, 262144, 1048576)


def log(*a):
    print("[htree_get]", *a, file=sys.stderr, flush=True)


def gpu_ms(call, reps: int) -> float:
    """Median GPU milliseconds between events around call(), after one warm-up call."""
    ms = []
    for it in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        if it:
            ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 4)


def source_file(n: int, seed: int, dev):
    """A hint file of n items with distinct random keyhashes in keyhash order, every key the one
    byte "k", no index section (a reader takes the items to the file's end): (file, keyhashes)."""
    rng = np.random.default_rng(seed)
    kh = np.unique(rng.integers(0, 1 << 63, int(n * 1.01) + 16, dtype=np.uint64) * np.uint64(2) + np.uint64(1))
    kh = np.sort(rng.permutation(kh)[:n])
    assert len(kh) == n
    item = np.dtype([("kh", "<u8"), ("chunk", "<u4"), ("off", "<u4"), ("ver", "<i4"), ("vhash", "<u2"), ("ksz", "u1"),
                     ("key", "u1")])
    assert item.itemsize == 24
    a = np.zeros(n, item)
    a["kh"], a["off"], a["ver"], a["ksz"], a["key"] = kh, (np.arange(n, dtype=np.uint32) % (1 << 23)) * 256, 1, 1, ord("k")
    a["vhash"] = rng.integers(0, 1 << 16, n)
    head = np.zeros(1, np.dtype([("io", "<i8"), ("nk", "<u4"), ("ds", "<u4")]))
    head["nk"] = n
    raw = np.concatenate([head.view(np.uint8), a.view(np.uint8)])
    return torch.from_numpy(raw).to(dev), kh


def get_call(image, keyhash, n: int, flags: int):
    """(call, outputs): qlzx_htree_get of the first n hashes into buffers of its own."""
    from gobeansdb_amd import _lib, batch
    L = _lib.lib()
    dev = image.file.device
    out = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4)]
    vhash = torch.zeros(n, dtype=torch.int16, device=dev)
    slot = torch.zeros(n, dtype=torch.int32, device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    wsb = L.qlzx_htree_get_workspace_size(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def call():
        _lib.check(L.qlzx_htree_get(image.file.data_ptr(), int(image.file.numel()), image.leaf_first.data_ptr(),
                                    image.depth, image.height, None, None, None, keyhash.data_ptr(), n, flags,
                                    out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                    vhash.data_ptr(), slot.data_ptr(), totals.data_ptr(), ws.data_ptr(), wsb,
                                    batch._stream()), "qlzx_htree_get")
    return call, (*out, vhash, slot, totals)


def lookup_call(merged, keys, keyhash, n: int):
    """qlzx_hint_lookup of the first n hashes over the one merged file."""
    from gobeansdb_amd import _dev, _lib, batch
    L = _lib.lib()
    dev = merged.device
    nbytes = int(merged.numel())
    off_d, len_d = _dev.u64([0], dev), _dev.u64([nbytes], dev)
    chunk_d, flag_d = _dev.u32([0], dev), _dev.u32([_lib.HL_FILE_MERGED], dev)
    o = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(5)]
    vhash = torch.zeros(n, dtype=torch.int16, device=dev)
    item_src = torch.zeros(n, dtype=torch.int64, device=dev)
    totals = torch.zeros(4, dtype=torch.int32, device=dev)
    wsb = L.qlzx_hint_lookup_workspace_size(n, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def call():
        _lib.check(L.qlzx_hint_lookup(merged.data_ptr(), nbytes, off_d.data_ptr(), len_d.data_ptr(), chunk_d.data_ptr(),
                                      flag_d.data_ptr(), 1, keys.data.data_ptr(), keys.off.data_ptr(),
                                      keys.length.data_ptr(), keyhash.data_ptr(), n, _lib.HL_F_BOUNDED,
                                      o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(),
                                      o[4].data_ptr(), vhash.data_ptr(), item_src.data_ptr(), totals.data_ptr(),
                                      ws.data_ptr(), wsb, batch._stream()), "qlzx_hint_lookup")
    return call, totals


def index_call(file, depth: int, height: int):
    from gobeansdb_amd import _lib, batch, htree
    L = _lib.lib()
    _, nleaf = htree.geometry(depth, height)
    leaf_first = torch.empty(nleaf + 1, dtype=torch.int32, device=file.device)
    totals = torch.zeros(4, dtype=torch.int32, device=file.device)
    wsb = L.qlzx_htree_index_workspace_size(height)
    ws = torch.empty(wsb, dtype=torch.uint8, device=file.device)

    def call():
        _lib.check(L.qlzx_htree_index(file.data_ptr(), int(file.numel()), depth, height, leaf_first.data_ptr(),
                                      totals.data_ptr(), ws.data_ptr(), wsb, batch._stream()), "qlzx_htree_index")
    return call, leaf_first, totals


def with_deleted_items(image, klen: int):
    """The image with the first item of every 16th non-empty-leaf given ver = -1 and the leaf's
    count one less, as HTree.set leaves a delete: a copy, on the device."""
    raw = image.file.cpu().numpy().copy()
    first = image.leaf_first.cpu().numpy().astype(np.int64)
    nleaf = len(first) - 1
    leaves = np.arange(0, nleaf, 16)
    leaves = leaves[first[leaves + 1] > first[leaves]]
    at = 6 * nleaf + 4 * (leaves + 1) + (klen + 11) * first[leaves] + klen      # the first item's ver
    for b in range(4):
        raw[at + b] = 0xFF
    counts = raw[:6 * nleaf].reshape(nleaf, 6)[:, :4].copy().view("<u4").reshape(nleaf)
    counts[leaves] -= 1
    raw[:6 * nleaf].reshape(nleaf, 6)[:, :4] = counts.view(np.uint8).reshape(nleaf, 4)
    return torch.from_numpy(raw).to(image.file.device), len(leaves)


def sweep(depth: int, height: int, n_items: int, seed: int, reps: int, dev):
    from gobeansdb_amd import _lib, batch, hint, htree
    file, kh = source_file(n_items, seed, dev)
    built = htree.build([file], [0], depth, height)
    image = built.image()
    assert built.n_slots == n_items
    merged = hint.merge([file], [0]).file
    klen, nleaf = htree.geometry(depth, height)
    rng = np.random.default_rng(seed + 1)
    nmax = max(SWEEP)
    ask = kh[rng.integers(0, n_items, nmax)]
    absent = rng.random(nmax) < 0.1
    ask[absent] = ask[absent] - np.uint64(1)                           # the items' hashes are odd: an even one is absent
    keyhash = torch.from_numpy(ask.view(np.int64)).to(dev)
    keys = batch.BlockBatch.from_bytes([b"k"] * nmax, device=dev)
    rows = []
    for n in SWEEP:
        row = {"n": n}
        outs = {}
        for name, flag in (("wave", _lib.HTG_F_WAVE), ("lane", _lib.HTG_F_LANE)):
            call, outs[name] = get_call(image, keyhash, n, flag)
            row[f"get_{name}_ms"] = gpu_ms(call, reps)
        assert all(torch.equal(a, b) for a, b in zip(outs["wave"], outs["lane"])), "the two shapes differ"
        found = int(outs["wave"][6][0])
        assert found == n - int(absent[:n].sum())
        call, totals = lookup_call(merged, keys, keyhash, n)
        row["hint_lookup_ms"] = gpu_ms(call, reps)
        assert int(totals[0]) == found, (totals.tolist(), found)
        call, _ = get_call(image, keyhash, n, 0)
        row["get_ms"] = gpu_ms(call, reps)
        row["found"] = found
        row["get_over_hint_lookup"] = round(row["get_ms"] / row["hint_lookup_ms"], 3)
        log(json.dumps(row))
        rows.append(row)
    # the index: the image as written, and with ver < 0 items
    call, leaf_first, totals = index_call(image.file, depth, height)
    ms_plain = gpu_ms(call, reps)
    assert torch.equal(leaf_first, image.leaf_first) and totals.tolist()[:3] == [n_items, nleaf, 0]
    odd, n_odd = with_deleted_items(image, klen)
    call, leaf_first, totals = index_call(odd, depth, height)
    ms_odd = gpu_ms(call, max(reps // 2, 1))
    assert torch.equal(leaf_first, image.leaf_first) and totals.tolist()[:3] == [n_items, nleaf, 0]
    out = {"depth": depth, "height": height, "items": n_items, "leaves": nleaf, "items_per_leaf": n_items / nleaf,
           "image_bytes": int(image.file.numel()), "merged_hint_bytes": int(merged.numel()), "calls_timed": reps,
           "sweep": rows, "index_ms": ms_plain, "index_with_deleted_items_ms": ms_odd, "leaves_with_a_deleted_item": n_odd}
    log(json.dumps({k: v for k, v in out.items() if k != "sweep"}))
    return out


def gc_leg(kind: str, n: int, seed: int, depth: int, height: int, reps: int, dev):
    from gobeansdb_amd import _lib, batch, gc, hint, htree, replay
    L = _lib.lib()
    data, rec_off = build_chunk(kind, n, seed, dev)
    res = replay.replay(data)
    assert res.n == n
    splits = hint.build(res, chunk_id=5)
    built = htree.build([sp.file for sp in splits], [5] * len(splits), depth, height)
    image = built.image()
    del res
    torch.cuda.empty_cache()
    size, mc = int(data.numel()), 4
    result = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev)
    i32 = lambda k=n: torch.empty(k, dtype=torch.int32, device=dev)   # noqa: E731
    i64 = lambda k=n: torch.empty(k, dtype=torch.int64, device=dev)   # noqa: E731
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    verdict, tree_ver, slot, ask, lt, mt = i32(), i32(), i32(), i32(), i32(8), i32(2)
    vhash = torch.empty(n, dtype=torch.int16, device=dev)
    status, new_chunk, new_off, crc, base, cb, totals = i32(), i32(), i64(), i32(), i64(mc), i64(mc), i32(8)
    heads = torch.zeros(mc, dtype=torch.int64, device=dev)
    ids = torch.tensor([9, 10, 11, 12], dtype=torch.int32, device=dev)
    out = torch.empty((size + 255) // 256 * 256, dtype=torch.uint8, device=dev)
    wl, wg, wm = L.qlzx_gc_liveness_workspace_size(n), L.qlzx_gc_workspace_size(n, mc), L.qlzx_htree_move_workspace_size(n)
    ws = torch.empty(max(wl, wg, wm), dtype=torch.uint8, device=dev)
    s = batch._stream()
    file = image.file.clone()                                          # the move rewrites it: from the same state each time

    def liveness():
        _lib.check(L.qlzx_gc_liveness(data.data_ptr(), size, rec_off.data_ptr(), result.data_ptr(), n, 250, 50 << 20,
                                      5, file.data_ptr(), int(file.numel()), image.leaf_first.data_ptr(), depth,
                                      height, None, 0, keep.data_ptr(), verdict.data_ptr(), vhash.data_ptr(),
                                      tree_ver.data_ptr(), slot.data_ptr(), ask.data_ptr(), lt.data_ptr(),
                                      ws.data_ptr(), wl, s), "qlzx_gc_liveness")

    def plan():
        _lib.check(L.qlzx_gc_plan(data.data_ptr(), size, rec_off.data_ptr(), result.data_ptr(), n, keep.data_ptr(),
                                  250, 50 << 20, gc.DATA_FILE_MAX, heads.data_ptr(), mc, status.data_ptr(),
                                  new_chunk.data_ptr(), new_off.data_ptr(), base.data_ptr(), cb.data_ptr(),
                                  totals.data_ptr(), ws.data_ptr(), wg, s), "qlzx_gc_plan")

    def rewrite():
        _lib.check(L.qlzx_gc_rewrite(data.data_ptr(), size, rec_off.data_ptr(), result.data_ptr(), n,
                                     heads.data_ptr(), mc, new_chunk.data_ptr(), new_off.data_ptr(), base.data_ptr(),
                                     out.data_ptr(), out.numel(), status.data_ptr(), crc.data_ptr(),
                                     totals.data_ptr(), ws.data_ptr(), wg, s), "qlzx_gc_rewrite")

    def move():
        _lib.check(L.qlzx_htree_move(file.data_ptr(), int(file.numel()), image.leaf_first.data_ptr(), depth, height,
                                     result.data_ptr(), n, verdict.data_ptr(), status.data_ptr(), slot.data_ptr(),
                                     new_chunk.data_ptr(), new_off.data_ptr(), ids.data_ptr(), mc, mt.data_ptr(),
                                     ws.data_ptr(), wm, s), "qlzx_htree_move")

    ms = {}
    ms["liveness"] = gpu_ms(liveness, reps)
    ms["plan"] = gpu_ms(plan, reps)
    ms["rewrite"] = gpu_ms(rewrite, reps)                              # rewrite settles status: plan is not run again
    ms["move"] = gpu_ms(move, reps)
    t = lt.cpu().numpy().view(np.uint32).tolist()
    m = mt.cpu().numpy().view(np.uint32).tolist()
    assert t[0] == n and t[1] == t[7] == built.n_slots and t[2] == 0 and t[6] == 0 and t[1] + t[4] == n
    assert m == [t[1], 0] and int(totals[2]) == t[1] and int(totals[6]) == 0
    out = {"workload": kind, "records": n, "chunk_bytes": size, "depth": depth, "height": height,
           "tree_items": built.n_slots, "records_kept": t[7], "not_in_tree": t[4], "calls_timed": reps, "abi_gpu_ms": ms,
           "what": "the tree is built from the chunk's own hints: every record with ver > 0 is NEWEST; hashes "
                   "computed on the device from the records' keys"}
    log(json.dumps(out))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--items", type=int, default=1048576)
    p.add_argument("--records-a", type=int, default=131072)
    p.add_argument("--records-b", type=int, default=1048576)
    p.add_argument("--reps", type=int, default=9)
    p.add_argument("--seed", type=int, default=2029)
    p.add_argument("--skip-gc", action="store_true")
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_htree_get.py needs a GPU"
    from gobeansdb_amd import _lib, build
    build.build()
    dev = torch.device("cuda", 0)
    trees = [sweep(1, 3, a.items, a.seed, a.reps, dev), sweep(2, 5, a.items, a.seed + 1, a.reps, dev),
             # between the two: 256 and 64 items per leaf, where the two shapes cross
             sweep(1, 4, a.items, a.seed + 2, a.reps, dev), sweep(1, 4, a.items // 4, a.seed + 3, a.reps, dev)]
    legs = [] if a.skip_gc else [gc_leg("mixed", a.records_a, a.seed, 1, 3, a.reps, dev),
                                 gc_leg("small", a.records_b, a.seed + 1, 1, 3, a.reps, dev)]
    at = next(r for r in trees[0]["sweep"] if r["n"] == 4096)
    line = json.dumps({
        "metric": "GPU ms per call, qlzx_htree_get of 4,096 keys over a 1,048,576-item tree at depth 1, height 3",
        "value": at["get_ms"], "unit": "ms",
        "baseline": {"what": "qlzx_hint_lookup of the same keys over the merged hint file of the same items",
                     "value": at["hint_lookup_ms"]},
        "lane_shape_rule": {"items_per_leaf_at_most": _lib.HTG_LANE_LEAF, "n_at_least": _lib.HTG_LANE_FROM,
                            "n_per_item_of_a_leaf_at_least": _lib.HTG_LANE_PER_ITEM},
        "trees": trees, "gc": legs, "data": "synthetic"})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
