"""Host: the collection of tests/go_l1_cases.py through the independent model of quicklz.go
level 1 (tests/go_l1_model.py) and through the oracle (oracle/qlz_oracle_l1.c).

The model and the oracle must agree on every case: status and output of Decompress, bytes of
Compress(src, 1).  The model's report then says what each case reaches, and the census below
pins it, so that tests/test_gpu_go_l1_cases.py, which compares the kernels with the oracle on
the same cases, cannot pass vacuously.

Census (the constants CASES, STATUS, SITES_PANICKED, DEC_EVENTS and ENC_EVENTS below):
  cases     panic_sites 54, odd_tokens 61, headers 76, zero_fill 26, encoder 73, mutants 50724
  mutants   45110 decode OK, 4405 E_CORRUPT, 600 E_DST_CAP, 414 E_HEADER, 195 E_LEVEL
  sites     nine of the eleven panic, each in a case with a neighbour one byte away that gets
            past it; `literal` and `rehash_first` cannot panic (go_l1_cases.py says why) and
            do not in any of the 50,941 streams
  events    every decode event occurs on an odd_tokens stream that decodes OK; every encoder
            event occurs, but of the RLE exception's five byte tests only source[src-3] and
            source[src-2] can fail alone
  zero-fill 16 odd_tokens and 6 zero_fill results change when the destination starts as 0xA5
  bail-out  margin 0 (kept) and margin -1 (stored) are both reached
The file takes about 7 s on one core; most of it is the mutants through the model.
"""
from collections import Counter

import pytest

import go_l1_cases as C
import go_l1_model as M
from oracle import oracle as O

E_DST_CAP = 4

CASES = {"panic_sites": 54, "odd_tokens": 61, "headers": 76, "zero_fill": 26, "encoder": 73, "mutants": 50724}

# decode status per family: {status: cases}
STATUS = {
    "panic_sites": {0: 21, 2: 31, 6: 2},
    "odd_tokens": {0: 57, 2: 4},
    "headers": {0: 27, 2: 9, 3: 9, 4: 7, 6: 24},
    "zero_fill": {0: 19, 2: 7},
    "mutants": {0: 45110, 2: 4405, 3: 195, 4: 600, 6: 414},
}
# the site of every panic per family
SITES_PANICKED = {
    "panic_sites": {"cword": 2, "fetch_cword": 4, "fetch_match": 4, "header": 2, "len_byte": 1, "literal_ahead": 5,
                    "match_copy": 3, "rehash_loop": 7, "tail": 5},
    "odd_tokens": {"match_copy": 3, "rehash_loop": 1},
    "headers": {"cword": 5, "fetch_cword": 3, "header": 24, "tail": 1},
    "zero_fill": {"cword": 7},
    "mutants": {"cword": 398, "fetch_cword": 289, "fetch_match": 363, "header": 414, "literal_ahead": 1792,
                "match_copy": 709, "rehash_loop": 2, "tail": 852},
}
# decode events per family: cases in which the event occurs on a stream that decodes OK
DEC_EVENTS = {
    "panic_sites": {"fetch_never_loaded": 2, "header3": 1, "long_len_0": 2, "long_len_1": 1, "long_len_2": 1,
                    "long_len_3": 2, "overlap": 2, "rehash_past_dst": 7, "short_len_3": 1, "tail_cword_skip": 1,
                    "unwritten_bucket": 2},
    "odd_tokens": {"fetch_never_loaded": 9, "header3": 3, "long_len_0": 8, "long_len_1": 3, "long_len_17": 1,
                   "long_len_18": 1, "long_len_2": 3, "long_len_255": 1, "long_len_3": 11, "overlap": 21,
                   "rehash_past_dst": 25, "short_len_17": 2, "short_len_3": 3, "stale_fetch": 1,
                   "stored_short_body": 1, "tail_cword_skip": 9, "unwritten_bucket": 18},
    "headers": {"header3": 9, "stored_short_body": 11},
    "zero_fill": {"long_len_0": 6, "long_len_1": 6, "long_len_255": 1, "overlap": 6, "rehash_past_dst": 6,
                  "stored_short_body": 13, "unwritten_bucket": 6},
    "mutants": {"header3": 15611, "long_len_0": 3, "long_len_255": 150, "overlap": 6605, "rehash_past_dst": 7495,
                "short_len_17": 110, "short_len_3": 7495, "stored_short_body": 2485, "tail_cword_skip": 8772,
                "unwritten_bucket": 3863},
}
# encoder events: cases of the encoder family in which the event occurs
ENC_EVENTS = {"collision": 9, "counter0": 3, "cut_by_remaining": 8, "last_cword_full": 4, "len_17": 1, "len_18": 1,
              "len_255": 7, "len_3": 11, "len_4": 2, "len_5": 2, "len_6": 2, "minoffset_1": 12, "minoffset_2": 2,
              "rle_lits01": 6, "rle_lits2": 6, "rle_m2": 2, "rle_m3": 4, "rle_src3": 4, "rle_taken": 7, "stored": 5}

UNREACHABLE = ("literal", "rehash_first")
RLE_CANNOT_FAIL_ALONE = ("rle_m1", "rle_p1", "rle_p2")

# name -> (stored, [(src - 3*(len>>2), margin) at every full control word])
BAIL_EXPECT = {
    "bail_margin_0": (False, [(8, 0)]),
    "bail_margin_minus1": (True, [(6, -1)]),
    "bail_at_threshold_behind_kept": (False, [(0, -7)]),
    "bail_at_threshold_behind_stored": (True, [(-100, -9), (-39, 0), (0, -1), (31, -6)]),
    "bail_at_threshold_ahead_kept": (False, [(-55, 0), (0, 6)]),
    "bail_at_threshold_ahead_stored": (True, [(-102, -7), (-41, 2), (0, 2), (31, -3)]),
    "bail_threshold_plus1_stored": (True, [(1, -8)]),
    "bail_threshold_plus1_kept": (False, [(-52, 0), (1, 5)]),
}

# encoder cases named after one decision: the events each must show
ENC_PINS = {
    "counter0_bucket0": ["counter0"], "minoffset_1": ["minoffset_1"], "minoffset_2": ["minoffset_2"],
    "rle_taken_from_start": ["rle_taken", "rle_src3", "rle_lits2"], "rle_taken_mid": ["rle_taken"],
    "rle_src3_alone": ["rle_src3"], "rle_lits2_after_match": ["rle_lits2", "rle_taken"],
    "rle_m3_alone": ["rle_m3"], "rle_m2_alone": ["rle_m2"],
    "match_3": ["len_3"], "match_4": ["len_4"], "match_5": ["len_5"], "match_6": ["len_6"], "match_17": ["len_17"],
    "match_18": ["len_18"], "match_255": ["len_255"], "match_256_split": ["len_255"], "match_300_split": ["len_255"],
    "cut_remaining_7": ["cut_by_remaining"], "cut_remaining_8": ["cut_by_remaining"],
    "cut_remaining_254": ["cut_by_remaining"], "last_cword_full_31": ["last_cword_full"],
    "last_cword_full_with_match": ["last_cword_full"], "stored_random_4096": ["stored"],
}


def _cap(c):
    return C.claimed_size(c.stream) if c.cap is None else c.cap


def model_decode(stream, cap, fill=0):
    """The model's Decompress under the project's status mapping, which adds one rule Go has
    not: a size above dst_cap is E_DST_CAP, after the header and level checks and before any
    decoding.  The model is not run then (a mutant's header may claim gigabytes)."""
    size = C.claimed_size(stream)
    if size > cap and len(stream) and ((stream[0] >> 2) & 3) in (1, 3):
        return E_DST_CAP, None, M.Report()
    return M.decompress(stream, fill)


@pytest.fixture(scope="module")
def decoded():
    """name -> (case, model status, model output, report, oracle status, oracle output), once."""
    out = {}
    for c in C.collection():
        if c.stream is None:
            continue
        st, data, rep = model_decode(c.stream, _cap(c))
        ost, odata = O.decompress_go_l1(c.stream, cap=_cap(c))
        out[c.name] = (c, st, data, rep, ost, odata)
    return out


@pytest.fixture(scope="module")
def encoded():
    """name -> (case, model stream, report, oracle stream), once."""
    return {c.name: (c,) + M.compress(c.plain) + (O.compress_go_l1(c.plain),)
            for c in C.collection() if c.plain is not None}


def test_case_counts():
    assert dict(Counter(c.family for c in C.collection())) == CASES
    assert [n for n in C.ZERO_FILL_SIZES] == [1, 15, 16, 17, 31, 33, 4101]


def test_decoder_model_equals_oracle(decoded):
    bad = []
    for name, (c, st, data, rep, ost, odata) in decoded.items():
        if st != ost or (st == M.OK and data != odata):
            bad.append((name, st, ost))
    assert not bad, (len(bad), bad[:10])


def test_encoder_model_equals_oracle_and_decodes_back(encoded):
    for name, (c, s, rep, o) in encoded.items():
        assert s == o, name
        st, back, _ = M.decompress(s)
        assert (st, back) == (M.OK, c.plain), name
        assert O.decompress_go_l1(s) == (O.OK, c.plain), name


def test_decode_census(decoded):
    status, sites, events = {}, {}, {}
    for name, (c, st, data, rep, ost, odata) in decoded.items():
        status.setdefault(c.family, Counter())[st] += 1
        if rep.site:
            sites.setdefault(c.family, Counter())[rep.site] += 1
        if st == M.OK:
            for e in rep.events:
                events.setdefault(c.family, Counter())[e] += 1
    status, sites, events = ({f: dict(sorted(v.items())) for f, v in d.items()} for d in (status, sites, events))
    assert status == STATUS
    assert sites == SITES_PANICKED
    assert events == DEC_EVENTS
    for site in UNREACHABLE:
        assert all(site not in v for v in sites.values())
    # every decode event on at least one odd_tokens stream that decodes OK
    assert sorted(events["odd_tokens"]) == sorted(M.DEC_EVENTS)


def test_panic_pairs(decoded):
    """Every reachable site: a case that panics there and, one source byte or one in the
    header's size away, a neighbour that gets past it."""
    pairs = {}
    for name, (c, st, data, rep, ost, odata) in decoded.items():
        if c.family != "panic_sites":
            continue
        site, tag, role = name.split("/")
        assert site == c.site
        if c.panics:
            assert rep.site == site and st in (M.E_HEADER, M.E_CORRUPT), name
        else:
            assert rep.site != site, name
        pairs.setdefault((site, tag), {})[role] = c.stream
    for (site, tag), p in pairs.items():
        if "passes" not in p:
            continue
        a, b = p["panics"], p["passes"]
        if len(a) == len(b):                        # one byte differs; the size field by one
            diff = [k for k in range(len(a)) if a[k] != b[k]]
            assert len(diff) == 1, (site, tag)
            if diff[0] == (5 if a[0] & 2 else 2):
                assert abs(a[diff[0]] - b[diff[0]]) == 1, (site, tag)
        else:                                       # a truncation: the neighbour has one byte more
            assert len(b) == len(a) + 1 and b[:len(a)] == a, (site, tag)
        if "ok" in p:
            assert decoded[f"{site}/{tag}/ok"][1] == M.OK and p["ok"][:len(b)][9:] == b[9:], (site, tag)
    reachable = set(M.SITES) - set(UNREACHABLE)
    assert {s for (s, _), p in pairs.items() if "passes" in p} == reachable
    # every site has a neighbour, or the whole stream of one, that decodes OK
    assert {s for (s, t), p in pairs.items() for r in ("passes", "ok")
            if r in p and decoded[f"{s}/{t}/{r}"][1] == M.OK} == reachable


def test_zero_fill_dependence(decoded):
    """What removing the decoder's zero-fill would change: the cases whose result differs when
    the destination starts as 0xA5, as it does in the GPU tests."""
    dep = Counter()
    names = []
    for name, (c, st, data, rep, ost, odata) in decoded.items():
        if c.family in ("odd_tokens", "zero_fill", "panic_sites") and st == M.OK:
            st5, data5, _ = M.decompress(c.stream, fill=0xA5)
            if (st5, data5) != (st, data):
                dep[c.family] += 1
                names.append(name)
    assert dict(dep) == {"panic_sites": 1, "odd_tokens": 16, "zero_fill": 6}, (dep, names)
    for n in ("odd/long_len_1_dst0", "odd/long_len_2_dst0", "odd/self_copy_5", "odd/self_copy_9"):
        assert n in names
    for size in C.ZERO_FILL_SIZES[1:]:
        assert f"zf/self_copy_{size}" in names


def test_encode_census(encoded):
    events = Counter()
    for name, (c, s, rep, o) in encoded.items():
        for e in rep.events:
            events[e] += 1
    assert dict(events) == ENC_EVENTS
    assert sorted(events) == sorted(set(M.ENC_EVENTS) - set(RLE_CANNOT_FAIL_ALONE))
    for name, evs in ENC_PINS.items():
        rep = encoded["enc/" + name][2]
        for e in evs:
            assert rep.events[e] >= 1, (name, e)
    assert sorted({n for _, _, rep, _ in encoded.values() for n in rep.cut} & {7, 8, 254}) == [7, 8, 254]
    assert {len(c.plain) for c, _, _, _ in encoded.values()} >= set(range(1, 13))
    assert max(len(c.plain) for c, _, _, _ in encoded.values()) == 4096


def test_rle_refusals_alone(encoded):
    """Each refusal of the RLE exception with every other term true: lits == 2, src == 3,
    source[src-3] and source[src-2]; the other three byte tests hold whenever src == o + 1."""
    alone = Counter()
    for name, (c, s, rep, o) in encoded.items():
        for lits, src, eq in rep.rle:
            assert eq[2:] == (True, True, True), name
            terms = {"lits": lits >= 3, "src": src > 3, "m3": eq[0], "m2": eq[1]}
            false = [k for k, v in terms.items() if not v]
            if len(false) == 1:
                alone[false[0] + ("2" if false[0] == "lits" and lits == 2 else "")] += 1
            if not false:
                alone["taken"] += 1
    assert set(alone) == {"lits2", "src", "m3", "m2", "taken"}, alone


def test_bail_out_margins(encoded):
    assert sorted(BAIL_EXPECT) == sorted(C.BAIL_CASES)
    for name, (stored, margins) in BAIL_EXPECT.items():
        c, s, rep, o = encoded["enc/" + name]
        assert rep.margins == margins, name
        assert (rep.events["stored"] == 1) == stored and bool(s[0] & 1) != stored, name
    tested = [m for _, _, rep, _ in encoded.values() for d, m in rep.margins if d > 0]
    assert 0 in tested and -1 in tested
