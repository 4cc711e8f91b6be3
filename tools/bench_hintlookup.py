#!/usr/bin/env python3
"""Key lookups through a bucket's hint files (hint.lookup: qlzx_hint_lookup) on files resident on
the device, next to the hint.merge of the same files and the replay.read_records that follows a
lookup.

The bucket: --files (8) chunks of --items (131,072) one-slot records each (tools/bench_hintmerge.py's
"splits" shape: keys distinct inside a chunk, drawn from a universe 1.5 times its size), one split
file per chunk from hint.build, and the file hint.merge makes of them.  The requests: --requests
(4,096 and 262,144) keys, half of them stored somewhere in the bucket, half absent.  Per request
count, in one process:

  layouts  "splits": the 8 split files, newest chunk first; "merged": the merged file alone
  modes    the reference as it is (flags 0) and QLZX_HL_F_BOUNDED
  shapes   the wave-per-request kernel (QLZX_HL_F_WAVE) and the lane-per-request one
           (QLZX_HL_F_LANE), and, bounded, the library's own choice by the request count; all
           alternating call by call

Every combination is timed through the C ABI with caller-provided buffers: GPU milliseconds between
events, the median of --reps calls after a warm-up call.  hint.lookup's host wall time (packing,
upload of the file table, read-back of totals) is timed bounded, with the library's choice of
kernel.  The two shapes must give the same seven outputs; in bounded mode the found keys are exactly
the stored half and the two layouts name the same (chunk, offset).  The positions found in the newest chunk, the one whose data
is kept, then go to replay.read_records with the keys (key_eq must be 1).  hint.merge of the same
files is timed in the same run for orientation.  There is no CPU baseline: the reference's lookup
needs Go.

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
from tools.bench_write import timed  # noqa: E402


def log(*a):
    print("[hintlookup]", *a, file=sys.stderr, flush=True)


def key_batch(keys, dev):
    from gobeansdb_amd import batch
    klen = np.fromiter(map(len, keys), np.int32, count=len(keys))
    koff, _ = batch.pack_offsets(klen, align=1)
    return batch.BlockBatch(torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev),
                            torch.from_numpy(koff.view(np.int64)).to(dev), torch.from_numpy(klen).to(dev))


class Abi:
    """qlzx_hint_lookup over one layout with buffers made once."""

    def __init__(self, files, chunk_ids, merged, kb):
        from gobeansdb_amd import _lib, batch
        self.L, self._lib, self.kb = _lib.lib(), _lib, kb
        dev = kb.data.device
        lens = [int(f.numel()) for f in files]
        offs = np.cumsum([0] + lens[:-1]).astype(np.int64)
        self.hints = torch.cat(files)
        self.nf, self.n = len(files), kb.n
        self.off_d, self.len_d = torch.from_numpy(offs).to(dev), torch.tensor(lens, dtype=torch.int64, device=dev)
        self.chunk_d = torch.tensor(chunk_ids, dtype=torch.int32, device=dev)
        self.flag_d = torch.tensor([_lib.HL_FILE_MERGED if i == merged else 0 for i in range(self.nf)],
                                   dtype=torch.int32, device=dev)
        self.out = [torch.zeros(self.n, dtype=dt, device=dev)
                    for dt in (torch.int32,) * 5 + (torch.int16, torch.int64)]
        self.totals = torch.zeros(4, dtype=torch.int32, device=dev)
        self.wsb = self.L.qlzx_hint_lookup_workspace_size(self.n, self.nf)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=dev)
        self.stream = batch._stream()

    def call(self, flags):
        kb = self.kb
        self._lib.check(self.L.qlzx_hint_lookup(
            self.hints.data_ptr(), int(self.hints.numel()), self.off_d.data_ptr(), self.len_d.data_ptr(),
            self.chunk_d.data_ptr(), self.flag_d.data_ptr(), self.nf, kb.data.data_ptr(), kb.off.data_ptr(),
            kb.length.data_ptr(), None, self.n, flags, *[o.data_ptr() for o in self.out], self.totals.data_ptr(),
            self.ws.data_ptr(), self.wsb, self.stream), "qlzx_hint_lookup")

    def results(self, flags):
        self.call(flags)
        torch.cuda.synchronize()
        return [o.clone() for o in self.out], [int(x) for x in self.totals.cpu().numpy().view(np.uint32)]

    def gpu_ms(self, flag_sets, reps):
        """Median GPU ms per flag set, the sets alternating call by call."""
        ms = {f: [] for f in flag_sets}
        for it in range(reps + 1):
            for f in flag_sets:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                self.call(f)
                ev[1].record()
                torch.cuda.synchronize()
                if it:      # the first round is the warm-up
                    ms[f].append(ev[0].elapsed_time(ev[1]))
        return {f: round(float(np.median(v)), 4) for f, v in ms.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--files", type=int, default=8)
    p.add_argument("--items", type=int, default=131072)
    p.add_argument("--requests", type=int, nargs="+", default=[4096, 262144])
    p.add_argument("--reps", type=int, default=9)
    p.add_argument("--seed", type=int, default=2033)
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_hintlookup.py needs a GPU"
    from gobeansdb_amd import _lib, build, hint, replay
    build.build()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(a.seed)
    n, nf, universe = a.items, a.files, a.items + a.items // 2
    base = a.seed * 1000003
    files, idents, newest = [], [], None
    for c in range(nf):
        ident = rng.permutation(universe)[:n] + base
        idents.append(ident)
        data = build_chunk(n, ident, a.seed + c, dev)
        splits = hint.build(replay.replay(data), chunk_id=c)
        assert len(splits) == 1 and splits[0].num_key == n
        files.append(splits[0].file.clone())
        newest = data if c == nf - 1 else None
        del splits
        torch.cuda.empty_cache()
    chunk_ids = list(range(nf))
    every = np.unique(np.concatenate(idents))
    merged = hint.merge(files, chunk_ids)
    assert merged.num_key == len(every)
    t_merge = timed(lambda: hint.merge(files, chunk_ids), a.reps)
    log("hint.merge ms", round(float(np.median(t_merge)) * 1e3, 3))
    layouts = {"splits": (files[::-1], chunk_ids[::-1], None), "merged": ([merged.file], [0], 0)}
    B, LANE, WAVE = _lib.HL_F_BOUNDED, _lib.HL_F_LANE, _lib.HL_F_WAVE
    names = {WAVE: "reference_wave", LANE: "reference_lane", B | WAVE: "bounded_wave", B | LANE: "bounded_lane",
             B: "bounded_by_n"}
    legs = []
    for nreq in a.requests:
        hit = rng.choice(every, nreq // 2)
        miss = base + universe + rng.permutation(4 * nreq)[:nreq - nreq // 2]       # outside the universe
        order = rng.permutation(nreq)
        ids = np.concatenate([hit, miss])[order]
        stored = np.concatenate([np.ones(len(hit), bool), np.zeros(len(miss), bool)])[order]
        keys = [b"key_%016x" % int(i) for i in ids]
        kb = key_batch(keys, dev)
        leg = {"requests": nreq, "stored": int(stored.sum()), "absent": int((~stored).sum())}
        where = {}
        for lname, (lf, lc, lm) in layouts.items():
            abi = Abi(lf, lc, lm, kb)
            res = {f: abi.results(f) for f in names}
            for b in (0, B):                                        # the two shapes agree
                assert res[b | WAVE][1] == res[b | LANE][1]
                assert all(torch.equal(x, y) for x, y in zip(res[b | WAVE][0], res[b | LANE][0]))
            out_b, tot_b = res[B]
            assert tot_b == res[B | LANE][1] and all(torch.equal(x, y) for x, y in zip(out_b, res[B | LANE][0]))
            status = out_b[0].cpu().numpy()
            assert ((status == _lib.HL_FOUND) == stored).all() and tot_b == [int(stored.sum()), int((~stored).sum()), 0, 0]
            where[lname] = (out_b[2].cpu().numpy(), out_b[3].cpu().numpy())
            ms = abi.gpu_ms(list(names), a.reps)
            wall = timed(lambda: hint.lookup(lf, lc, kb, merged=lm, bounded=True), a.reps)
            leg[lname] = {"files": len(lf), "hint_bytes": int(abi.hints.numel()), "workspace_bytes": abi.wsb,
                          "abi_gpu_ms": {names[f]: ms[f] for f in names},
                          "mreq_per_s_bounded_wave": round(nreq / ms[B | WAVE] / 1e3, 2),
                          "mreq_per_s_bounded_lane": round(nreq / ms[B | LANE] / 1e3, 2),
                          "totals_reference": dict(zip(("found", "miss", "err", "bad_file"), res[WAVE][1])),
                          "totals_bounded": dict(zip(("found", "miss", "err", "bad_file"), tot_b)),
                          "hint_lookup_bounded_host_wall_ms": round(float(np.median(wall)) * 1e3, 3)}
            log(nreq, lname, json.dumps(leg[lname]))
            if lname == "splits":                                   # the newest chunk's records, read back by key
                chunk = out_b[2].cpu().numpy().view(np.uint32)
                sel = np.flatnonzero((status == _lib.HL_FOUND) & (chunk == nf - 1))
                offs = (out_b[3].to(torch.int64) & 0xFFFFFFFF)[torch.from_numpy(sel).to(dev)]
                want = [keys[i] for i in sel]
                rd = replay.read_records(newest, offs, keys=want)
                torch.cuda.synchronize()
                assert int((rd.status != 0).sum()) == 0 and int(rd.key_eq.sum()) == len(sel)
                t_rd = timed(lambda: replay.read_records(newest, offs, keys=want), a.reps)
                leg["read_records_of_the_newest_chunk"] = {"records": len(sel),
                                                           "host_wall_ms": round(float(np.median(t_rd)) * 1e3, 3)}
            del abi
        assert (where["splits"][0] == where["merged"][0]).all() and (where["splits"][1] == where["merged"][1]).all()
        legs.append(leg)
    first = legs[-1]["splits"]["abi_gpu_ms"]
    line = json.dumps({
        "metric": "GPU ms per call, hint lookup over device-resident hint files (qlzx_hint_lookup)",
        "value": first["bounded_by_n"],
        "unit": f"ms, {legs[-1]['requests']} requests over {nf} split files of {n} items, bounded",
        "lane_from": _lib.HL_LANE_FROM,
        "baseline": {"what": "hint.merge of the same files, same process, host wall ms (no CPU lookup baseline: the "
                             "reference needs Go)", "value": round(float(np.median(t_merge)) * 1e3, 3)},
        "files": nf, "items_per_file": n, "merged_keys": int(merged.num_key), "calls_timed": a.reps,
        "legs": legs, "data": "synthetic",
        "what": "abi_gpu_ms: GPU time between events around one qlzx_hint_lookup call (key hash, file heads and the "
                "search kernel), median, the five flag sets alternating call by call; host_wall_ms: median wall "
                "time of the Python call, every launch, upload, read-back and allocation included"})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
