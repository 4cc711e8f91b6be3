"""Record what the *reference* decoder makes of the hand-assembled streams of tests/qlz_asm.py.

Run in the build container (needs /root/reference):  python tests/golden/make_golden_streams.py

Every valid stream of qlz_asm.collection() goes through the reference qlz_decompress
(quicklz/quicklz.c as gobeansdb builds it, compiled by oracle/Makefile into
oracle/_ref/libqlzref.so).  streams.json holds, per stream, its name, its length and SHA-256, the
length the reference returned and the SHA-256 of the reference's output.  The streams themselves
are rebuilt from their names by the tests (tests/test_crafted_streams.py), which check both
hashes: that the stream is the one the reference saw, and that the assembler's own plaintext is
what the reference decoded.

Only data is written (names, lengths and hashes); no reference source.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import qlz_asm  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    if O.ref() is None:
        sys.exit("oracle/_ref/libqlzref.so is not built (needs /root/reference)")
    rows = []
    for c in qlz_asm.collection():
        out = O.ref_decompress(c.stream)
        assert out == c.plain, c.name           # the reference agrees with the assembler
        rows.append({"name": c.name, "stream_len": len(c.stream),
                     "stream_sha256": hashlib.sha256(c.stream).hexdigest(),
                     "ref_len": len(out), "ref_sha256": hashlib.sha256(out).hexdigest()})
    with open(os.path.join(HERE, "streams.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_streams.py",
                   "reference": "quicklz/quicklz.c qlz_decompress at level 3 (oracle/_ref/libqlzref.so)",
                   "streams": rows}, f, indent=0)
        f.write("\n")
    print(f"{len(rows)} streams, {sum(r['stream_len'] for r in rows)} stream bytes, "
          f"{sum(r['ref_len'] for r in rows)} decoded bytes")


if __name__ == "__main__":
    main()
