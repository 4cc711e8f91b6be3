"""Known answers that pin tests/hint_model.py (no GPU).  Go is not installed where the goldens are
made and MurmurHash3 is not in the reference tree, so no golden file comes from the compiled
reference: the model is pinned by published MurmurHash3_x86_32 answers, the reference's own fnv1a
answer (store/htree_test.go:18-23), two worked files, and the reader side of the reference
(loadHintIndex + hintFileIndex.get finds every item: store/hint_test.go:81)."""
import random

import hint_model as H

KH_TEST = 0xafd071e5ba6bd213
RECORDS = [(KH_TEST, b"test", 0, 256, 1, 0x1234),
           (7, b"b", 256, 512, -2, 0xbeef),
           (KH_TEST, b"test", 1024, 256, 3, 0x00ff),
           (7, b"a", 1280, 256, 1, 1)]
FILE_A = ("5b00000000000000030000000006000007000000000000000000000000050000010000000100016107000000000000000000"
          "000000010000feffffffefbe016213d26bbae571d0af000000000004000003000000ff0004746573740700000000000000"
          "10000000000000000700000000000000280000000000000013d26bbae571d0af4000000000000000")
FILE_B = ("4300000000000000020000000005000007000000000000000000000000010000feffffffefbe016213d26bbae571d0af00"
          "0000000004000003000000ff000474657374")


def test_murmur3_known_answers():
    for text, want in ((b"", 0), (b"hello", 0x248bfa47), (b"hello, world", 0x149bbb7f), (b"test", 0xba6bd213),
                       (b"Hello, world!", 0xc0363e43),
                       (b"The quick brown fox jumps over the lazy dog", 0x2e4ff723)):
        assert H.murmur3_32(text) == want, text


def test_fnv1a_and_keyhash_known_answers():
    assert H.fnv1a(b"test") == 2949673445
    assert H.keyhash(b"test") == KH_TEST
    assert H.keyhash(b"\xe4\xb8\xad\xff") == 0x3d722a51c990d5e1      # bytes >= 0x80: the sign extension


def test_worked_file_every_item_indexed():
    sp = H.build_split(RECORDS, split_cap=1 << 20, index_interval=128)
    assert (sp.consumed, sp.num_key, sp.datasize, sp.n_index) == (4, 3, 1536, 3)
    assert sp.file.hex() == FILE_A


def test_worked_file_cut_at_split_cap():
    sp = H.build_split(RECORDS, split_cap=2, index_interval=4096)
    assert (sp.consumed, sp.num_key, sp.datasize, sp.n_index) == (3, 2, 1280, 0)
    assert sp.file.hex() == FILE_B
    splits = H.build(RECORDS, split_cap=2, index_interval=4096)
    assert [s.consumed for s in splits] == [3, 1] and splits[1].datasize == 1536


def _random_records(rnd, n, nkeys, nhash):
    keys = [bytes(rnd.getrandbits(8) for _ in range(rnd.randint(1, 40))) for _ in range(nkeys)]
    keys += [k[:max(1, len(k) // 2)] for k in keys[:nkeys // 4]]          # prefixes of other keys
    hashes = {k: rnd.randrange(nhash) if nhash else H.keyhash(k) for k in keys}
    out, off = [], 0
    for _ in range(n):
        k = rnd.choice(keys)
        size = 256 * rnd.randint(1, 4)
        off += 256 * rnd.randint(0, 2)
        out.append((hashes[k], k, off, size, rnd.randint(-3, 9), rnd.getrandbits(16)))
        off += size
    return out


def test_every_item_is_found_through_the_index():
    rnd = random.Random(5)
    for case in range(60):
        recs = _random_records(rnd, rnd.randint(1, 120), rnd.randint(1, 40), rnd.choice((0, 0, 3, 1 << 40)))
        interval = rnd.choice((128, 279, 280, 303, 400, 1000, 4096))
        for sp in H.build(recs, split_cap=rnd.choice((1, 2, 7, 1 << 20)), index_interval=interval):
            items = H.read_items(sp.file)
            assert len(items) == sp.num_key == H.read_head(sp.file)[1]
            assert [(i.keyhash, i.key) for i in items] == sorted((i.keyhash, i.key) for i in items)
            index = H.load_index(sp.file)
            assert len(index) == sp.n_index
            for it in items:
                assert H.get(sp.file, index, it.keyhash, it.key) == it, (case, it)


def test_split_semantics_against_the_set_formulation():
    """The grouping / cut / last-member formulation the device code uses, against HintBuffer.Set."""
    rnd = random.Random(11)
    for case in range(200):
        recs = _random_records(rnd, rnd.randint(1, 60), rnd.randint(1, 12), rnd.choice((0, 2, 3)))
        cap, first = rnd.choice((1, 2, 3, 5, 100)), rnd.randint(0, 3)
        sp = H.build_split(recs, first, cap, 128, max_offset=rnd.choice((0, 10 ** 6)))
        seen, c = [], len(recs)
        for j in range(first, len(recs)):
            g = (recs[j][0], recs[j][1])
            if g not in seen:
                if len(seen) == cap:
                    c = j
                    break
                seen.append(g)
        assert sp.consumed == max(c - first, 0), case
        last = {}
        for j in range(first, c):
            last[(recs[j][0], recs[j][1])] = j
        want = [recs[last[g]] for g in sorted(last)]
        assert [(i.keyhash, i.key, i.offset, i.ver, i.vhash) for i in H.read_items(sp.file)] == \
            [(r[0], r[1], r[2], r[4], r[5]) for r in want] if want else sp.file == b""
