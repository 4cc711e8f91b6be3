"""The plaintexts of tests/qlz_cases.py on the host: the instrumented model (tests/qlz_model.py)
equals the oracle on every one of them, in the plain and the Go mode, the oracle equals the
compiled reference where that is built, and the census below shows that every decision of the
compressor the collection is meant to force really occurs -- at an item start, in the encoder
size classes the table at CENSUS names (and says why).  The census is what keeps tests/test_gpu_encoder_cases.py from
passing vacuously.  No GPU."""
import ctypes
import functools
from collections import Counter

import numpy as np
import pytest

import qlz_asm
import qlz_cases
import qlz_model
from oracle import oracle as O

# (length, offset) pairs at which the token form changes (quicklz.c:377-406)
EDGE_PAIRS = ({(3, 63), (3, 64), (3, 16383), (3, 16384), (18, 40), (19, 40), (33, 50), (34, 50), (33, 2000),
               (34, 2000), (254, 300), (255, 300)} | {(L, off) for L in range(4, 19) for off in (1023, 1024)})
FAR = (131069, 131070)


@functools.lru_cache(maxsize=None)
def analysed(name: str):
    """(case, oracle stream, oracle Go stream, model report, disassembly) of a case, once."""
    if not BY_NAME:
        BY_NAME.update({c.name: c for c in qlz_cases.collection()})
    c = BY_NAME[name]
    s, g = O.compress(c.plain), O.compress_go(c.plain)
    core, rep = qlz_model.parse(c.plain)
    assert qlz_model.finish(c.plain, core, rep.margins) == s, f"{name}: the model differs from the oracle"
    assert qlz_model.finish(c.plain, core, rep.margins, bias=9) == g, f"{name}: the model differs (Go rule)"
    return c, s, g, rep, qlz_asm.disassemble(s)


BY_NAME = {}


def features(name: str) -> set:
    """What the compressor does on this case, named: the rows of CENSUS."""
    c, s, g, rep, (dsize, items, tests) = analysed(name)
    n = len(c.plain)
    f = set()
    f.add("stored" if items is None else "compressed")
    f.add("hdr3" if n < 216 else "hdr9")
    if items is None:
        f.add("stored_at_first_test" if len(rep.margins) == 1 else "stored_at_later_test")
        return f
    assert tests == rep.margins, name
    for j, (ip, tl, ml, off) in enumerate(items):
        if not tl:
            continue
        f.add(f"form{tl}")
        if (ml, off) in EDGE_PAIRS:
            f.add(f"match_{ml}_{off}")
            if j % 31 in (0, 30, 15):
                f.add(f"match_{ml}_{off}_bit{j % 31}")
        if ip == c.tags.get("at") and (ml, off) == c.tags.get("match"):
            f.add(f"planted_{ml}_{off}")
        if "split" in c.tags and (ip, ml) == c.tags["split"][:2] and items[j + 1][2:] == (45, off):
            f.add("planted_split_255_45")
        if off in FAR:
            f.add(f"match_off_{off}")
        if c.plain[ip] < 0x80:                     # the carrier: zeros, text, filler
            continue
        if off == 3:
            f.add("match_off_3")
        if ml == 255 and j + 1 < len(items) and items[j + 1][0] == ip + 255 and items[j + 1][2:] == (45, off):
            f.add("split_255_45")
        if off < ml:
            f.add("overlap_period3" if off == 3 else "overlap")
        if ip == n - 11:
            f.add("match_at_n-11")
    last = max((ip for ip, tl, _, _ in items if tl), default=-1)
    if "at" in c.tags and c.tags["at"] >= n - 10:
        assert last < c.tags["at"]
        f.add("repeat_in_tail_not_searched")
    for ev in rep.ev:
        f.add(ev)
    for at in c.tags.get("ats", ()):               # the probes of compact_edges
        f.add(f"at:viable_{rep.at[at][1]}")
        f |= {f"at:{e}" for e in rep.at[at][2]}
    if c.tags.get("at") in rep.at:                 # what happens at the planted item start itself
        rank, viable, evs = rep.at[c.tags["at"]]
        f |= {f"at:{e}" for e in evs} | {f"at:viable_{viable}"}
        if "wrap_rank" in c.tags:
            assert rank == c.tags["wrap_rank"], name
            f.add(f"at:rank_{rank}")
    for lim in rep.limits:
        if lim <= 12:
            f.add(f"limit_cut_{lim}")
    for k in (9, 10, 11, 16):
        if k in rep.viable:
            f.add(f"viable_{k}")
    if "band" in c.tags:
        share = rep.repeat_share
        f.add("share_lt20" if share < 0.20 else "share_35_55" if 0.35 <= share <= 0.55 else "share_gt70")
        assert share < 0.20 or 0.35 <= share <= 0.55 or share > 0.70, name
    if tests:
        m = min(tests)
        if m <= 2:
            f.add("margin_le2")
        if m == 0:
            f.add("margin0")
            f.add("margin0_first_test" if tests.index(0) == 0 else "margin0_later_test")
        if m <= 8:
            assert g[0] & 1 == 0, name
            f.add("go_stored_c_compressed")
        else:
            assert g[0] & 1 == 1, name
        if m == 9:
            f.add("margin9_first_test" if tests.index(9) == 0 else "margin9_later_test")
    if c.family == "parse_rounds" and n <= 65536:
        rounds, notes = qlz_model.walker_rounds(c.plain)
        f.add(f"rounds_{rounds}" if rounds <= 4 else "rounds_over_4")
        f |= {f"walker_{x}" for x in notes}
    if n in (65537, 65545, 65546, 65547, 131081, 131082):
        f.add(f"n_{n}")
    return f


def test_disassembler_on_assembled_streams():
    """Every valid hand-assembled stream disassembles to the assembler's own item list, and
    replaying the items gives the plaintext."""
    cases = qlz_asm.collection()
    for c in cases:
        dsize, items, tests = qlz_asm.disassemble(c.stream)
        want = [(it.op, len(it.tok) if it.is_match else 0, it.ml, it.off) for it in c.asm.items]
        assert dsize == len(c.plain) and items == want, c.name
        assert qlz_asm.replay(c.stream, items) == c.plain, c.name
    assert len(cases) >= 600


def test_disassembler_margins():
    """The margins are the ones of quicklz.c:218: a block of text with noise bails out exactly
    when the model sees a negative one, and a stored stream has no items."""
    t = bytes(x % 7 for x in qlz_asm.XorShift64(3).bytes(2000))
    dsize, items, tests = qlz_asm.disassemble(O.compress(t))
    assert dsize == 2000 and items and tests and min(tests) > 0
    assert tests == qlz_model.compress(t)[1].margins
    r = qlz_asm.XorShift64(4).bytes(2000)
    assert qlz_asm.disassemble(O.compress(r)) == (2000, None, [])
    assert qlz_model.compress(r)[1].margins[-1] < 0


def test_model_equals_oracle_on_plain_sizes():
    """The model on the sizes around its own switches, before it is trusted on the cases."""
    rng = qlz_asm.XorShift64(9)
    for n in (1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14, 31, 32, 215, 216, 217, 300):
        for d in (rng.bytes(n), bytes(n), bytes(x % 3 for x in rng.bytes(n)), O.gen_text(5, n, n)):
            assert qlz_model.compress(d)[0] == O.compress(d), n
            assert qlz_model.compress(d, bias=9)[0] == O.compress_go(d), n


@pytest.mark.parametrize("family", list(qlz_cases.FAMILIES))
def test_cases_model_oracle_reference(family):
    """Model == oracle (both modes), oracle == the compiled reference (plain mode, where built),
    and the oracle's own decoder returns the plaintext."""
    Q = O.ref_if_built()
    n = 0
    for c in qlz_cases.collection():
        if c.family != family:
            continue
        _, s, g, rep, _ = analysed(c.name)
        assert O.decompress(s) == (O.OK, c.plain), c.name
        assert O.decompress(g) == (O.OK, c.plain), c.name
        if Q is not None:
            src = np.frombuffer(c.plain, np.uint8)
            dst = np.zeros(len(c.plain) + 400, np.uint8)
            scratch = np.zeros(528400, np.uint8)
            Q.qlz_compress.restype = ctypes.c_size_t
            Q.qlz_compress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
            r = Q.qlz_compress(src.ctypes.data, dst.ctypes.data, len(c.plain), scratch.ctypes.data)
            assert dst[:r].tobytes() == s, c.name
        n += 1
    assert n >= 10


# feature: the least number of cases that must show it, per encoder size class.  A class is left
# out of a row for one of two reasons.  The feature cannot occur in it: an offset of 16383 needs
# more than 16384 bytes, the offset limit more than 128 KiB, and the compact loop and the walkers
# exist only in the workgroup kernels, up to 65536 bytes.  Or the row is one of the many token-edge
# pairs, cut limits and counter ranks that are planted once, at no more than 4096 bytes, because the
# three workgroup kernels are one template and tests/test_gpu_encoder_cases.py sends every small
# case through all three of them; a handful are repeated at 16384 and 65536 bytes all the same.
# The whole-GPU encoder shares none of that code (its own token table, candidate loop and bail-out
# test), so what applies to it is planted again beyond position 65536 and has a "huge" row: every
# token edge but the middle lengths of (L, 1023 / 1024), the ranks 256..272 and every cut limit.
ALL4 = {4096: 1, 16384: 1, 65536: 1, "huge": 1}
WG3 = {4096: 1, 16384: 1, 65536: 1}
SMALL = {4096: 1}
SMALL_HUGE = {4096: 1, "huge": 1}
HUGE = {"huge": 1}
BIG_PAIRS = {(3, 16383), (3, 16384)}                      # need more than 16384 bytes
WIDE_PAIRS = {(3, 64), (18, 1023), (19, 40), (34, 50), (255, 300)}   # also planted at 16384 and 65536
CENSUS = {}
for _p in sorted(EDGE_PAIRS):                           # token_edges: every pair, at every place in a word
    _row = {65536: 1} if _p in BIG_PAIRS else WG3 if _p in WIDE_PAIRS else SMALL
    CENSUS[f"planted_{_p[0]}_{_p[1]}"] = dict(_row, huge=1) if _p in qlz_cases.HUGE_PAIRS else _row
    for _bit in (0, 30, 15):
        CENSUS[f"match_{_p[0]}_{_p[1]}_bit{_bit}"] = {65536: 1} if _p in BIG_PAIRS else SMALL
CENSUS.update({
    "planted_split_255_45": {4096: 3, "huge": 1}, "match_off_3": SMALL, "overlap_period3": SMALL, "overlap": SMALL,
    "form1": ALL4, "form2": ALL4, "form3": ALL4, "form4": ALL4, "stored": ALL4, "compressed": ALL4,
    # tail_edges (a limit below 7 cannot occur: ip <= n - 11)
    "limit_cut_7": ALL4, "limit_cut_8": ALL4, "limit_cut_9": SMALL_HUGE, "limit_cut_10": SMALL_HUGE,
    "limit_cut_11": SMALL_HUGE, "limit_cut_12": SMALL_HUGE, "match_at_n-11": ALL4, "repeat_in_tail_not_searched": ALL4, "hdr3": SMALL, "hdr9": ALL4,
    # table_edges: at the planted item start itself
    "at:rank_256": ALL4, "at:rank_257": ALL4, "at:rank_271": SMALL_HUGE, "at:rank_272": SMALL_HUGE, "at:rank_517": SMALL,
    "at:wrap_hides": {4096: 4, 16384: 2, 65536: 2, "huge": 2}, "at:wrap_hides_0": ALL4, "at:tie": ALL4,
    "at:evicted": ALL4, "at:collision": ALL4, "minoffset": ALL4, "at:long_recent_wins": ALL4,
    "long_over_short": ALL4,
    # compact_edges
    "at:viable_9": WG3, "at:viable_10": WG3, "at:viable_11": WG3, "at:viable_16": WG3, "at:long_older_wins": WG3,
    "share_lt20": WG3, "share_35_55": WG3, "share_gt70": WG3,
    # parse_rounds
    "rounds_1": WG3, "rounds_2": WG3, "rounds_3": WG3, "rounds_4": WG3, "rounds_over_4": {4096: 2, 16384: 2, 65536: 2},
    "walker_cover": WG3, "walker_merge": WG3,
    # bail_edges
    "margin0": {4096: 4, 16384: 2, 65536: 4, "huge": 4}, "margin0_first_test": ALL4, "margin0_later_test": ALL4,
    "margin9_first_test": ALL4, "margin9_later_test": ALL4, "margin_le2": ALL4, "go_stored_c_compressed": ALL4,
    "stored_at_first_test": ALL4, "stored_at_later_test": ALL4,
    # huge_edges
    "match_off_131069": HUGE, "match_off_131070": {"huge": 2}, "at:far_reject": {"huge": 3},
    "at:far_reject_nearer": HUGE, "n_65537": HUGE, "n_65545": HUGE, "n_65546": HUGE, "n_65547": HUGE, "n_131081": HUGE, "n_131082": HUGE,
})


def test_census():
    """Every decision the collection is built for occurs, in every class it applies to."""
    got = Counter()
    for c in qlz_cases.collection():
        cls = qlz_cases.size_class(len(c.plain))
        for f in features(c.name):
            got[f, cls] += 1
    missing = [(f, cls, got[f, cls], need) for f, row in CENSUS.items() for cls, need in row.items()
               if got[f, cls] < need]
    assert not missing, missing
    assert len(CENSUS) >= 60


def test_planted_events_per_case():
    """What a builder plants occurs in that very case, not merely somewhere in its class: the
    source is still read after 15 later insertions into its bucket and gone after 16 and 17; the
    tie, the collision and each compact probe's tie stand at the planted item start; a planted
    match is the item at its position, and over 64 KiB that position lies beyond 65536."""
    n = 0
    for c in qlz_cases.collection():
        t = c.tags
        if t.get("kind") == "evict":
            assert ("at:evicted" in features(c.name)) == (t["between"] >= 16), c.name
            rep = analysed(c.name)[3]
            assert rep.at[t["at"]][0] == t["between"] + 1, c.name
        elif t.get("kind") in ("tie", "tie3"):
            assert "at:tie" in features(c.name), c.name
        elif t.get("kind") == "collision":
            assert "at:collision" in features(c.name), c.name
        elif "ats" in t:
            rep = analysed(c.name)[3]
            for at, k in zip(t["ats"], t["counts"]):
                assert rep.at[at][1] == k and {"tie", "long_older_wins"} <= set(rep.at[at][2]), (c.name, k)
        elif "match" in t:
            assert "planted_%d_%d" % t["match"] in features(c.name), c.name
        elif "split" in t:
            assert "planted_split_255_45" in features(c.name), c.name
        elif "wrap_rank" in t:
            assert ("at:wrap_hides" in features(c.name)) == (t["wrap_rank"] & 255 < 16), c.name
        elif "far" in t:
            assert ("at:far_reject" in features(c.name)) == (t["far"] >= 131071), c.name
        else:
            continue
        if len(c.plain) > 65536 and "at" in t:
            assert t["at"] > 65536, c.name
        n += 1
    assert n >= 200


def test_gpu_routes_cover_every_case():
    """The route tables of tests/test_gpu_encoder_cases.py, checked where no GPU is needed: the
    per-family counts of every route are the ones its test states, every case has exactly one of
    the routes wg65536 / huge, and each workgroup class has a block of exactly its bound."""
    import test_gpu_encoder_cases as G
    cs = qlz_cases.collection()
    for route, fams in G.EXPECT.items():
        sel = G._route(route, sum(fams.values()))
        if route != "huge":
            assert max(len(c.plain) for c in sel) == route
    assert len(G._route(65536, 317)) + len(G._route("huge", 62)) == len(cs) == sum(G.ALL.values())
    assert dict(Counter(c.family for c in cs)) == G.ALL
    assert max(len(c.plain) for c in cs) <= 143360 and sum(len(c.plain) for c in cs) < 16 << 20
