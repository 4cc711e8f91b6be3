"""GPU: the block calls with offsets at and beyond 2^31 and 2^32 (tests/wide.py has the layout:
one 4 GiB + 4 MiB source `big`, one destination `bigout` of the same size full of the guard byte,
the windows W31 and W32 around the two lines and the alias window A0).

Every call goes through batch.BlockBatch(data, off, length) over the whole buffer, so the Python
mirror's own offset handling is under test with the kernels.  Every block stands at all six
placements of both boundaries (wide.placements); each test counts them (wide.census) and shows on
the host, before the first GPU call, that the answer it expects differs from the one the decoy in
A0 gives -- what an implementation that drops an offset's high word would return.

  read-only sources (crc32, keyhash, vhash, the source side of copy_blocks): the windows hold
      random bytes, A0 other random bytes; the blocks are slices of them and may overlap.
  written destinations and structured sources (copy_blocks, synth, decompress, compress, level 1):
      the placements of different blocks overlap, so the jobs run in rounds of disjoint spans
      (wide.rounds), one call per round; after each call every byte of bigout outside the round's
      blocks is compared with the guard byte, A0 included.
"""
import functools
import json
import os
import zlib

import numpy as np
import pytest

import hint_model as H
import qlz_asm
import qlz_cases
import wide
from oracle import oracle as O
from oracle import replay as R
from wide import B31, B32

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

widebuf = wide.fixture()
w = wide.per_test()

CRC_LENGTHS = (1, 3, 4, 63, 64, 65, 4095, 4096, 4097, 70000, 200000)
FAST_MAX_DSIZE = 65536      # QLZX_FAST_MAX_DSIZE: K1 + K2
UNIFORM_MAX_DSIZE = 16384   # calls up to here are the uniform regime
WG_MAX_LEN = 65536          # QLZX_WG_MAX_LEN


# ---------------------------------------------------------------- read-only sources: slices of random windows

@functools.lru_cache(maxsize=None)
def _windows():
    rng = np.random.default_rng(0x31D0)
    return tuple((lo, rng.integers(0, 256, hi - lo, dtype=np.uint8)) for lo, hi in (wide.W31, wide.W32, wide.A0))


def _real(s: int, n: int) -> bytes:
    """big[s : s + n] as the windows define it."""
    for lo, a in _windows():
        if lo <= s and s + n <= lo + len(a):
            return a[s - lo:s - lo + n].tobytes()
    raise AssertionError(("outside the windows", s, n))


def _alias(s: int, n: int) -> bytes:
    """The same block with every address at or above 2^32 reduced by 2^32."""
    k = min(n, max(0, B32 - s))
    return _real(s, k) + _real(s + k - B32, n - k)


def _fill_windows(wb):
    for lo, a in _windows():
        wb.place(wb.big, lo, a)


def _slices(lengths, answer):
    """(start, n) of every length at all twelve placements and what `answer(bytes, index)` owes for
    each; census and decoy difference asserted here, on the host."""
    blocks = [(s, n) for n in lengths for s in wide.all_placements(n)]
    assert wide.census(blocks) == wide.full_census(lengths)
    want = [answer(_real(s, n), i) for i, (s, n) in enumerate(blocks)]
    above = [i for i, (s, n) in enumerate(blocks) if s + n > B32]
    assert len(above) == sum(5 if n > 1 else 3 for n in lengths)
    for i in above:
        assert answer(_alias(*blocks[i]), i) != want[i], ("the decoy gives the same answer", blocks[i])
    return blocks, want


def _batch_of(wb, blocks, data=None):
    from gobeansdb_amd import _dev, batch
    assert all(s + n > 0 for s, n in blocks)
    return batch.BlockBatch(wb.big if data is None else data, _dev.u64([s for s, _ in blocks], wb.device),
                            _dev.u32([n for _, n in blocks], wb.device))


def test_crc32(w):
    """batch.crc32 (k_crc32 -> wave_crc: the short path, the 64-lane path and the segmented one
    from 128 KiB) with the default and a per-block init and both final_xor values."""
    import torch
    from gobeansdb_amd import _dev, batch
    nblk = 12 * len(CRC_LENGTHS)
    init = (np.arange(nblk, dtype=np.uint64) * 0x9E3779B1 + 0x0BADC0DE).astype(np.uint32)
    blocks, want_z = _slices(CRC_LENGTHS, lambda b, i: zlib.crc32(b))
    _, want_0 = _slices(CRC_LENGTHS, lambda b, i: O.crc32_write(int(init[i]), b))
    assert want_z[5] == O.crc32_write(0xFFFFFFFF, _real(*blocks[5])) ^ 0xFFFFFFFF     # the two references agree
    _fill_windows(w)
    src = _batch_of(w, blocks)
    init_t = _dev.u32(init, w.device)
    got_z = _dev.readback(batch.crc32(src)).tolist()
    got_0 = _dev.readback(batch.crc32(src, init=init_t, final_xor=0)).tolist()
    got_f = _dev.readback(batch.crc32(src, init=init_t, final_xor=0xFFFFFFFF)).tolist()
    torch.cuda.synchronize()
    bad = [(blocks[i], k) for k, got, want in (("zlib", got_z, want_z), ("init", got_0, want_0),
                                                ("init_xor", got_f, [x ^ 0xFFFFFFFF for x in want_0]))
           for i in range(nblk) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:12])


def test_keyhash(w):
    """hint.keyhash (qlzx_keyhash_batch) against hint_model.keyhash."""
    from gobeansdb_amd import hint
    blocks, want = _slices((1, 4, 5, 250, 255), lambda b, i: H.keyhash(b))
    _fill_windows(w)
    got = hint.keyhash(_batch_of(w, blocks)).cpu().numpy().view(np.uint64).tolist()
    bad = [(blocks[i], hex(got[i]), hex(want[i])) for i in range(len(blocks)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:12])


def test_vhash(w):
    """qlzx_vhash_batch against oracle/replay.getvhash, on both sides of its 1024-byte switch.
    An empty value has no decoy (its hash reads no byte): it stands at the starts of a one-byte
    block and is counted apart."""
    import torch
    from gobeansdb_amd import _lib, batch
    blocks, want = _slices((1, 1023, 1024, 1025, 5000), lambda b, i: R.getvhash(b))
    empty = [(s, 0) for s in wide.all_placements(1)]
    assert sum(s >= B32 for s, _ in empty) == 3 and sum(B31 <= s < B32 - wide.MIB for s, _ in empty) == 3
    blocks, want = blocks + empty, want + [R.getvhash(b"")] * len(empty)
    _fill_windows(w)
    b = _batch_of(w, blocks)
    out = torch.zeros(b.n, dtype=torch.int16, device=w.device)
    _lib.check(_lib.lib().qlzx_vhash_batch(b.data.data_ptr(), b.off.data_ptr(), b.length.data_ptr(), b.n,
                                           out.data_ptr(), batch._stream()), "qlzx_vhash_batch")
    got = [int(x) & 0xFFFF for x in out.cpu().numpy()]
    bad = [(blocks[i], got[i], want[i]) for i in range(len(blocks)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:12])


# ---------------------------------------------------------------- written destinations: rounds of disjoint spans

def _pairs(k: int):
    """For item k: (source placement, destination placement) indices, each of the twelve once on
    either side, the pairing turning with k so that the two sides vary independently."""
    return [(i, (i + 1 + 5 * k) % 12) for i in range(12)]


def _check_census(src_blocks, src_lengths, dst_blocks, dst_lengths):
    if src_blocks is not None:
        assert wide.census(src_blocks) == wide.full_census(src_lengths)
    assert wide.census(dst_blocks) == wide.full_census(dst_lengths)


def test_copy_blocks(w):
    """batch.copy_blocks (qlzx_copy_batch): the source at one boundary and the destination at
    the other, in both directions; the source side reads slices of the random windows."""
    import torch
    from gobeansdb_amd import batch
    jobs, srcs, dsts = [], [], []
    for k, n in enumerate(CRC_LENGTHS):
        for bs, bd in ((B31, B32), (B32, B31)):
            for i in range(6):
                s, d = wide.placements(n, bs)[i], wide.placements(n, bd)[(i + k) % 6]
                jobs.append(((s, d, n), [("out", d, n)]))
                srcs.append((s, n))
                dsts.append((d, n))
    _check_census(srcs, CRC_LENGTHS, dsts, CRC_LENGTHS)
    for s, n in srcs:
        if s + n > B32:
            assert _alias(s, n) != _real(s, n)
    _fill_windows(w)
    plan = wide.rounds(jobs)
    assert sum(len(r) for r in plan) == 12 * len(CRC_LENGTHS)
    bad = []
    for rnd in plan:
        todo = [key for key, _ in rnd]
        for s, d, n in todo:
            w.wrote(w.bigout, d, n)
        batch.copy_blocks(w.big, [s for s, _, _ in todo], [n for _, _, n in todo], w.bigout, [d for _, d, _ in todo])
        torch.cuda.synchronize()
        bad += [(s, d, n) for s, d, n in todo if w.fetch(w.bigout, d, n) != _real(s, n)]
        wide.assert_untouched(w.bigout, [(d, n) for _, d, n in todo])
        w.restore(only=w.bigout)
    assert not bad, (len(bad), bad[:12])
    wide.assert_untouched(w.bigout, [])


@pytest.mark.parametrize("kind", ["text", "image"])
def test_synth(w, kind):
    """batch.synth (qlzx_synth_batch) into bigout: block i of a call is gen(seed, first_id + i)."""
    import torch
    from gobeansdb_amd import batch
    lengths, seed = (5, 777, 16384), 0x5EED
    gen = O.gen_text if kind == "text" else O.gen_image
    jobs = [((d, n), [("out", d, n)]) for n in lengths for d in wide.all_placements(n)]
    _check_census(None, None, [key for key, _ in jobs], lengths)
    first, bad = 1000, []
    for rnd in wide.rounds(jobs):
        todo = [key for key, _ in rnd]
        for d, n in todo:
            w.wrote(w.bigout, d, n)
        batch.synth(kind, seed, [n for _, n in todo], first_id=first, device=w.device, out=_batch_of(w, todo, w.bigout))
        torch.cuda.synchronize()
        bad += [(d, n) for i, (d, n) in enumerate(todo) if w.fetch(w.bigout, d, n) != gen(seed, first + i, n)]
        wide.assert_untouched(w.bigout, todo)
        w.restore()
        first += len(todo)
    assert not bad, (len(bad), bad[:12])
    wide.assert_untouched(w.bigout, [])


def _codec_jobs(items):
    """items: (payload, decoy, destination length, key).  Each item at every source and every
    destination placement (_pairs); a job's spans are its source, its decoy in A0 and its
    destination.  Returns the jobs ((key, source start, destination start), spans)."""
    jobs, srcs, dsts = [], [], []
    for k, (payload, decoy, room, key) in enumerate(items):
        sat, dat = wide.all_placements(len(payload)), wide.all_placements(room)
        for i, j in _pairs(k):
            s, d = sat[i], dat[j]
            spans = [("big", s, len(payload)), ("out", d, room)]
            alias = wide.decoy_tail(s, payload, decoy)
            if alias is not None:
                spans.append(("big", alias[0], len(alias[1])))
            jobs.append(((key, s, d), spans))
            srcs.append((s, len(payload)))
            dsts.append((d, room))
    _check_census(srcs, [len(p) for p, _, _, _ in items], dsts, [r for _, _, r, _ in items])
    assert len({d % 16 for d, _ in dsts}) >= 3       # destinations on and off the 16-byte grid
    return jobs


# -- decompress

@functools.lru_cache(maxsize=None)
def _streams():
    """(name, family, stream, dsize, status, plaintext or None) of every crafted stream."""
    out = [(c.name, c.family, c.stream, len(c.plain), O.OK, c.plain) for c in qlz_asm.collection()]
    for i in qlz_asm.invalid_collection():
        st, _ = O.decompress(i.stream, cap=i.dsize)
        assert st == O.E_CORRUPT, i.name
        out.append((i.name, i.family, i.stream, i.dsize, st, None))
    return tuple(out)


ROUTES = {   # route: (admits(csize, dsize), the families of its valid streams)
    "uniform": (lambda c, d: d <= UNIFORM_MAX_DSIZE,
                {"forms_S", "chunk_cover", "groups", "lastword", "tail", "random"}),
    "mixed": (lambda c, d: d <= FAST_MAX_DSIZE,
              {"forms_S", "forms_M", "chunk_cover", "groups", "lastword", "tail", "random"}),
    "lane8": (lambda c, d: True,
              {"forms_S", "forms_M", "forms_L", "chunk_cover", "groups", "lastword", "tail", "random"}),
    "huge": (lambda c, d: d > FAST_MAX_DSIZE, {"forms_L", "random"}),
}


def _pick(route):
    """The first valid stream of every family the route admits and its first two invalid ones."""
    admits, families = ROUTES[route]
    sel = [c for c in _streams() if admits(len(c[2]), c[3])]
    valid = {}
    for c in sel:
        if c[5] is not None:
            valid.setdefault(c[1], c)
    assert set(valid) == families, route
    invalid = [c for c in sel if c[5] is None][:2]
    assert len(invalid) == 2
    return list(valid.values()), invalid


def _run_decode(wb, route, max_dsize, general=False, crc=False):
    import torch
    from gobeansdb_amd import _dev, batch
    valid, invalid = _pick(route)
    items = []
    for k, c in enumerate(valid + invalid):
        decoy = valid[(k + 1) % len(valid)] if c[5] is not None else valid[0]
        assert (decoy[4], decoy[5]) != (c[4], c[5])          # another status or another plaintext
        items.append((c[2], decoy[2], c[3], c))
    jobs = _codec_jobs(items)
    ws, bad = batch.Workspace(wb.device), []
    for rnd in wide.rounds(jobs):
        todo = [key for key, _ in rnd]
        for c, s, d in todo:
            decoy = next(it[1] for it in items if it[3] is c)
            wb.place_with_decoy(s, c[2], decoy)
            wb.wrote(wb.bigout, d, c[3])
        src = _batch_of(wb, [(s, len(c[2])) for c, s, _ in todo])
        out = _batch_of(wb, [(d, c[3]) for c, _, d in todo], wb.bigout)
        kw, states = {}, None
        if crc:
            states = (np.arange(len(todo), dtype=np.uint64) * 0x9E3779B1 + 0x12345678).astype(np.uint32)
            kw = dict(crc_state=_dev.u32(states, wb.device), want_crc=True)
        dsz, st, crc_out = batch.decompress(src, out, dst_cap=_dev.u32([c[3] for c, _, _ in todo], wb.device),
                                            max_dsize=max_dsize, general=general, workspace=ws, **kw)
        torch.cuda.synchronize()
        dsz, st = _dev.readback(dsz), st.cpu().numpy()
        crcs = _dev.readback(crc_out) if crc else None
        for k, (c, s, d) in enumerate(todo):
            name, _, stream, n, want_st, want = c
            if int(st[k]) != want_st:
                bad.append((name, s, d, "status", int(st[k]), want_st))
            elif want is not None and (int(dsz[k]) != n or wb.fetch(wb.bigout, d, n) != want):
                bad.append((name, s, d, "bytes", int(dsz[k])))
            if crc and int(crcs[k]) ^ 0xFFFFFFFF != O.crc32_write(int(states[k]), stream):
                bad.append((name, s, d, "crc"))
        wide.assert_untouched(wb.bigout, [(d, c[3]) for c, _, d in todo])   # a refused block's own bytes are free
        wb.restore()
    assert not bad, (len(bad), bad[:12])
    wide.assert_untouched(wb.bigout, [])


@pytest.mark.parametrize("crc", [False, True], ids=["nocrc", "crc"])
@pytest.mark.parametrize("route,max_dsize", [("uniform", UNIFORM_MAX_DSIZE), ("mixed", FAST_MAX_DSIZE)])
def test_decompress_k1_k2(w, route, max_dsize, crc):
    """K1 + K2 in both chunk regimes, without and with the CRC prologue."""
    _run_decode(w, route, max_dsize, crc=crc)


def test_decompress_lane8(w):
    """The lane-per-block kernel (no workspace), the streams over 64 KiB included."""
    _run_decode(w, "lane8", max(c[3] for c in _streams()), general=True)


def test_decompress_huge(w):
    """The whole-GPU decoder through the batch call."""
    _run_decode(w, "huge", max(c[3] for c in _streams()))


# -- compress

@functools.lru_cache(maxsize=None)
def _plain_150k() -> bytes:
    return qlz_cases.text(150, 150000)


def _first_per_family(cap):
    """The first case of every family the class admits, and the first one as long as the class
    allows: the bound of the call is met by a block."""
    first = {}
    for c in qlz_cases.collection():
        if len(c.plain) <= cap:
            first.setdefault(c.family, c)
    full = next(c for c in qlz_cases.collection() if len(c.plain) == cap)
    picked = list(first.values())
    return [(c.name, c.plain) for c in picked + [full] * (full not in picked)]


def _run_encode(wb, plains, max_len, go=False):
    """plains: (name, plaintext).  The oracle's bytes, the length, the fused CRC from a per-block
    state, and the guard outside each block's n + 400."""
    import torch
    from gobeansdb_amd import _dev, batch
    comp = O.compress_go if go else O.compress
    want = {name: comp(p) for name, p in plains}
    items = []
    for k, (name, p) in enumerate(plains):
        dname, decoy = plains[(k + 1) % len(plains)]
        assert want[dname] != want[name]
        items.append((p, decoy, len(p) + 400, name))
    jobs = _codec_jobs(items)
    by_name = {it[3]: it for it in items}
    ws, bad = batch.Workspace(wb.device), []
    for rnd in wide.rounds(jobs):
        todo = [key for key, _ in rnd]
        for name, s, d in todo:
            p, decoy, room, _ = by_name[name]
            wb.place_with_decoy(s, p, decoy)
            wb.wrote(wb.bigout, d, room)
        lens = [len(by_name[name][0]) for name, _, _ in todo]
        src = _batch_of(wb, [(s, n) for (_, s, _), n in zip(todo, lens)])
        dst = _batch_of(wb, [(d, n) for (_, _, d), n in zip(todo, lens)], wb.bigout)
        states = (np.arange(len(todo), dtype=np.uint64) * 0x9E3779B1 + 0x12345678).astype(np.uint32)
        _, cs, st, crc = batch.compress(src, dst, crc_state=_dev.u32(states, wb.device), want_crc=True,
                                        go_compat=go, max_len=max_len, workspace=ws)
        torch.cuda.synchronize()
        cs, st, crc = _dev.readback(cs), st.cpu().numpy(), _dev.readback(crc)
        for k, (name, s, d) in enumerate(todo):
            exp = want[name]
            if int(st[k]) != 0:
                bad.append((name, s, d, "status", int(st[k])))
            elif int(cs[k]) != len(exp) or wb.fetch(wb.bigout, d, len(exp)) != exp:
                bad.append((name, s, d, "bytes", int(cs[k]), len(exp)))
            elif int(crc[k]) != O.crc32_write(int(states[k]), exp) ^ 0xFFFFFFFF:
                bad.append((name, s, d, "crc"))
        wide.assert_untouched(wb.bigout, [(d, n + 400) for (_, _, d), n in zip(todo, lens)])
        wb.restore()
    assert not bad, (len(bad), bad[:12])
    wide.assert_untouched(wb.bigout, [])


@pytest.mark.parametrize("cap", [4096, 16384, 65536])
def test_compress_workgroup(w, cap):
    """k_encode_wg<cap>: the first case of every family the class admits."""
    plains = _first_per_family(cap)
    assert len(plains) == 6 + (cap > 4096) and max(len(p) for _, p in plains) == cap
    _run_encode(w, plains, cap)


def test_compress_lane_go_compat(w):
    """k_encode_lane, the Go-compatible path up to 64 KiB."""
    plains = _first_per_family(WG_MAX_LEN)
    assert len(plains) == 7
    _run_encode(w, plains, WG_MAX_LEN, go=True)


def test_compress_huge(w):
    """The whole-GPU encoder: a 70,000-byte case of qlz_cases and 150,000 bytes of its text."""
    c = next(c for c in qlz_cases.collection() if len(c.plain) == 70000)
    _run_encode(w, [(c.name, c.plain), ("text_150000", _plain_150k())], 150000)


# -- Go level 1

L1_NAMES = ("text_5", "rand_13", "ab_33", "runs_100", "text_255", "image_300", "zeros_1000", "text_4097",
            "runs_16384", "text_65536")


@functools.lru_cache(maxsize=None)
def _l1():
    man = json.load(open(os.path.join(GOLDEN, "golden_l1.json")))
    blob = open(os.path.join(GOLDEN, "qlz_l1_vectors.bin"), "rb").read()
    get = lambda span: blob[span[0]:span[0] + span[1]]  # noqa: E731
    by = {v["name"]: (get(v["input"]), get(v["ref"])) for v in man["vectors"]}
    return [(n,) + by[n] for n in L1_NAMES]


def test_go_l1_compress(w):
    """batch.go_l1_compress on ten golden plaintexts: the level-1 oracle's stream, as in
    tests/test_gpu_level1.py."""
    import torch
    from gobeansdb_amd import _dev, batch
    vec = _l1()
    want = {name: O.compress_go_l1(data) for name, data, _ in vec}
    items = [(data, vec[(k + 1) % len(vec)][1], len(data) + 400, name) for k, (name, data, _) in enumerate(vec)]
    assert all(want[vec[(k + 1) % len(vec)][0]] != want[vec[k][0]] for k in range(len(vec)))
    by_name = {it[3]: it for it in items}
    ws, bad = batch.Workspace(w.device), []
    for rnd in wide.rounds(_codec_jobs(items)):
        todo = [key for key, _ in rnd]
        for name, s, d in todo:
            p, decoy, room, _ = by_name[name]
            w.place_with_decoy(s, p, decoy)
            w.wrote(w.bigout, d, room)
        lens = [len(by_name[name][0]) for name, _, _ in todo]
        src = _batch_of(w, [(s, n) for (_, s, _), n in zip(todo, lens)])
        dst = _batch_of(w, [(d, n) for (_, _, d), n in zip(todo, lens)], w.bigout)
        _, cs, st = batch.go_l1_compress(src, dst, workspace=ws)
        torch.cuda.synchronize()
        cs, st = _dev.readback(cs), st.cpu().numpy()
        for k, (name, s, d) in enumerate(todo):
            exp = want[name]
            if int(st[k]) != 0 or int(cs[k]) != len(exp) or w.fetch(w.bigout, d, len(exp)) != exp:
                bad.append((name, s, d, int(st[k]), int(cs[k]), len(exp)))
        wide.assert_untouched(w.bigout, [(d, n + 400) for (_, _, d), n in zip(todo, lens)])
        w.restore()
    assert not bad, (len(bad), bad[:12])
    wide.assert_untouched(w.bigout, [])


def test_go_decompress(w):
    """batch.go_decompress on the ten golden level-1 streams: their plaintexts."""
    import torch
    from gobeansdb_amd import _dev, batch
    vec = _l1()
    plain = {name: data for name, data, _ in vec}
    items = [(ref, vec[(k + 1) % len(vec)][2], len(data), name) for k, (name, data, ref) in enumerate(vec)]
    assert all(vec[(k + 1) % len(vec)][1] != vec[k][1] for k in range(len(vec)))
    by_name = {it[3]: it for it in items}
    ws, bad = batch.Workspace(w.device), []
    for rnd in wide.rounds(_codec_jobs(items)):
        todo = [key for key, _ in rnd]
        for name, s, d in todo:
            ref, decoy, room, _ = by_name[name]
            w.place_with_decoy(s, ref, decoy)
            w.wrote(w.bigout, d, room)
        src = _batch_of(w, [(s, len(by_name[name][0])) for name, s, _ in todo])
        rooms = [(d, by_name[name][2]) for name, _, d in todo]
        out = _batch_of(w, rooms, w.bigout)
        dsz, st = batch.go_decompress(src, out, dst_cap=_dev.u32([n for _, n in rooms], w.device), workspace=ws)
        torch.cuda.synchronize()
        dsz, st = _dev.readback(dsz), st.cpu().numpy()
        for k, (name, s, d) in enumerate(todo):
            exp = plain[name]
            if int(st[k]) != 0 or int(dsz[k]) != len(exp) or w.fetch(w.bigout, d, len(exp)) != exp:
                bad.append((name, s, d, int(st[k]), int(dsz[k]), len(exp)))
        wide.assert_untouched(w.bigout, rooms)
        w.restore()
    assert not bad, (len(bad), bad[:12])
    wide.assert_untouched(w.bigout, [])
