"""The HTree query entry points (qlzx_htree_index, qlzx_htree_get, qlzx_gc_liveness, qlzx_htree_move
and their workspace-size functions): declared in include/qlzx_htree_get.h, exported, bound, and
their argument checks answer before any HIP call (no GPU)."""
import re
import subprocess

import pytest

from gobeansdb_amd import _lib, build

CALLS = {"qlzx_htree_index", "qlzx_htree_get", "qlzx_gc_liveness", "qlzx_htree_move"}
NAMES = CALLS | {n + "_workspace_size" for n in CALLS}
P = 0x1000          # a fake non-null pointer: a call that got past its checks would need a device
IMAGE, DATA = 0x10000, 0x100000
BYTES = 0x8000
BIG = 1 << 30

ARGS = {
    "qlzx_htree_index": ["image", "bytes", "depth", "height", "leaf_first", "totals", "workspace", "workspace_bytes",
                         "stream"],
    "qlzx_htree_get": ["image", "bytes", "leaf_first", "depth", "height", "keys", "key_off", "key_len", "keyhash", "n",
                       "flags", "status", "chunk", "offset", "ver", "vhash", "slot", "totals", "workspace",
                       "workspace_bytes", "stream"],
    "qlzx_gc_liveness": ["data", "size", "rec_off", "result", "cap", "max_key", "body_max", "src_chunk", "image",
                         "bytes", "leaf_first", "depth", "height", "keyhash", "flags", "keep", "verdict", "vhash",
                         "tree_ver", "slot", "ask_idx", "totals", "workspace", "workspace_bytes", "stream"],
    "qlzx_htree_move": ["image", "bytes", "leaf_first", "depth", "height", "result", "cap", "verdict", "gc_status",
                        "slot", "new_chunk", "new_off", "dst_chunk_id", "max_chunks", "totals", "workspace",
                        "workspace_bytes", "stream"],
}
SCALARS = dict(bytes=BYTES, depth=1, height=3, n=5, cap=5, flags=0, size=0x4000, max_key=250, body_max=50 << 20,
               src_chunk=3, max_chunks=4, workspace_bytes=BIG, stream=None)
POINTERS = dict(image=IMAGE, data=DATA)
MAY_BE_NULL = {"qlzx_htree_index": set(), "qlzx_htree_get": {"keys", "key_off", "key_len", "keyhash"},
               "qlzx_gc_liveness": {"keyhash"}, "qlzx_htree_move": set()}


def _L():
    build.build()
    return _lib.lib()


def _args(name, **kw):
    a = {k: SCALARS[k] if k in SCALARS else POINTERS.get(k, P) for k in ARGS[name]}
    a.update(kw)
    return list(a.values())


def _need(L, name):
    size = getattr(L, name + "_workspace_size")
    return size(SCALARS["height"]) if name == "qlzx_htree_index" else size(5)


def test_declared_in_their_own_header_exported_and_bound():
    L = _L()
    assert NAMES == set(_lib.header_functions(_lib.HTREE_GET_HEADER))
    assert not NAMES & set(_lib.header_functions())                     # qlzx.h keeps its functions
    assert not NAMES & set(_lib.header_functions(_lib.HTREE_HEADER))    # and so does qlzx_htree.h
    assert '#include "qlzx_htree.h"' in open(_lib.HTREE_GET_HEADER).read()
    for n in NAMES:
        assert hasattr(L, n) and getattr(L, n).argtypes is not None, n
    for n in CALLS:
        assert len(getattr(L, n).argtypes) == len(ARGS[n]), n
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert NAMES <= {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "qlzx_htree_get.h" in open(build.__file__).read()           # the header enters the source hash


def test_names():
    text = open(_lib.HTREE_GET_HEADER).read()
    assert "enum qlzx_htg_status { QLZX_HTG_MISS = 0, QLZX_HTG_FOUND };" in text
    assert "enum qlzx_htg_file { QLZX_HTG_OK = 0, QLZX_HTG_BAD_FILE };" in text
    assert "enum { QLZX_HTG_F_LANE = 1, QLZX_HTG_F_WAVE = 2 };" in text
    assert "enum qlzx_gl_verdict { QLZX_GL_BAD = 0, QLZX_GL_NEWEST, QLZX_GL_OTHER_POS, QLZX_GL_NOT_IN_TREE };" in text
    assert "enum { QLZX_GL_F_BEGIN_GT_0 = 1 };" in text
    assert int(re.search(r"#define QLZX_HTG_LANE_FROM (\w+?)u?\n", text).group(1), 0) == _lib.HTG_LANE_FROM
    assert int(re.search(r"#define QLZX_HTG_LANE_LEAF (\w+?)u?\n", text).group(1), 0) == _lib.HTG_LANE_LEAF
    assert int(re.search(r"#define QLZX_HTG_LANE_PER_ITEM (\w+?)u?\n", text).group(1), 0) == _lib.HTG_LANE_PER_ITEM
    assert (_lib.HTG_LANE_FROM, _lib.HTG_LANE_LEAF, _lib.HTG_LANE_PER_ITEM) == (4096, 64, 256)
    assert "#define QLZX_HTG_NO_SLOT 0xFFFFFFFFu" in text and _lib.HTG_NO_SLOT == 0xFFFFFFFF
    assert [_lib.HTG_MISS, _lib.HTG_FOUND] == [0, 1] and _lib.HTG_NAMES == ["HTG_MISS", "HTG_FOUND"]
    assert [_lib.HTG_OK, _lib.HTG_BAD_FILE] == [0, 1]
    assert [_lib.HTG_N_FOUND, _lib.HTG_N_MISS] == [0, 1]
    assert [_lib.HTG_ITEMS, _lib.HTG_N_LEAF, _lib.HTG_STATUS, _lib.HTG_STATUS_LEAF] == list(range(4))
    assert (_lib.HTG_F_LANE, _lib.HTG_F_WAVE) == (1, 2)
    assert [_lib.GL_BAD, _lib.GL_NEWEST, _lib.GL_OTHER_POS, _lib.GL_NOT_IN_TREE] == list(range(4))
    assert _lib.GL_NAMES == ["GL_BAD", "GL_NEWEST", "GL_OTHER_POS", "GL_NOT_IN_TREE"]
    assert [_lib.GL_N_RECORDS, _lib.GL_N_NEWEST, _lib.GL_N_OTHER_POS, _lib.GL_N_OTHER_POS_DELETED,
            _lib.GL_N_NOT_IN_TREE, _lib.GL_N_NOT_IN_TREE_KEPT, _lib.GL_N_BAD, _lib.GL_N_KEEP] == list(range(8))
    assert _lib.GL_F_BEGIN_GT_0 == 1 and [_lib.HTM_MOVED, _lib.HTM_SKIPPED] == [0, 1]
    from gobeansdb_amd import gc, htree
    assert all(callable(f) for f in (htree.load_image, htree.get, htree.move, htree.HTreeBuilt.image, gc.liveness))
    assert list(htree.HTreeImage.__dataclass_fields__) == ["file", "leaf_first", "n_items", "depth", "height"]
    assert list(gc.GCLiveness.__dataclass_fields__) == ["keep", "verdict", "vhash", "tree_ver", "slot", "ask_idx",
                                                        "totals"]


def test_workspace_sizes_positive_and_monotone():
    L = _L()
    heights = [L.qlzx_htree_index_workspace_size(h) for h in range(1, 7)]
    assert heights == sorted(heights) and heights[0] > 0 and heights[-1] > 16 << 20
    for size in (L.qlzx_htree_get_workspace_size, L.qlzx_gc_liveness_workspace_size,
                 L.qlzx_htree_move_workspace_size):
        got = [size(n) for n in (1, 1024, 1025, 1 << 20, 1 << 24)]
        assert got == sorted(got) and got[0] > 0


@pytest.mark.parametrize("name", sorted(CALLS))
def test_argument_checks_run_before_any_hip_call(name):
    L = _L()
    fn, fname = getattr(L, name), name.encode()
    for arg in ARGS[name]:
        if arg in SCALARS or arg == "workspace" or arg in MAY_BE_NULL[name]:
            continue
        assert fn(*_args(name, **{arg: None})) == _lib.R_BAD_ARG, arg
        assert fname in L.qlzx_last_error(), arg
    for bad in (dict(depth=3), dict(height=0), dict(height=7), dict(depth=0xFFFFFFFF), dict(image=IMAGE + 8),
                dict(bytes=1 << 36)):
        assert fn(*_args(name, **bad)) == _lib.R_BAD_ARG, bad
        assert fname in L.qlzx_last_error()
    need = _need(L, name)
    assert fn(*_args(name, workspace_bytes=need - 1)) == _lib.R_WORKSPACE
    assert fname in L.qlzx_last_error()
    assert fn(*_args(name, workspace=None)) == _lib.R_WORKSPACE
    assert fname in L.qlzx_last_error()
    assert fn(*_args(name, workspace=P + 8)) == _lib.R_WORKSPACE       # 16-byte aligned
    assert fname in L.qlzx_last_error()
    # a null image of no bytes is no error: the call gets past that check (asked with a short workspace)
    assert fn(*_args(name, image=None, bytes=0, workspace_bytes=1)) == _lib.R_WORKSPACE


def test_the_keys_may_be_null_only_with_hashes():
    L = _L()
    assert L.qlzx_htree_get(*_args("qlzx_htree_get", keys=None, key_off=None, key_len=None,
                                   workspace_bytes=1)) == _lib.R_WORKSPACE
    for arg in ("keys", "key_off", "key_len"):
        assert L.qlzx_htree_get(*_args("qlzx_htree_get", keyhash=None, **{arg: None})) == _lib.R_BAD_ARG, arg
        assert b"qlzx_htree_get" in L.qlzx_last_error()
    assert L.qlzx_htree_get(*_args("qlzx_htree_get", keyhash=None, workspace_bytes=1)) == _lib.R_WORKSPACE
    assert L.qlzx_gc_liveness(*_args("qlzx_gc_liveness", keyhash=None, workspace_bytes=1)) == _lib.R_WORKSPACE


def test_flags_and_alignment():
    L = _L()
    for flags in (3, 4, 0x80000000):
        assert L.qlzx_htree_get(*_args("qlzx_htree_get", flags=flags)) == _lib.R_BAD_ARG, flags
        assert b"qlzx_htree_get" in L.qlzx_last_error()
    for flags in (1, 2):
        assert L.qlzx_htree_get(*_args("qlzx_htree_get", flags=flags, workspace_bytes=1)) == _lib.R_WORKSPACE
    assert L.qlzx_gc_liveness(*_args("qlzx_gc_liveness", flags=2)) == _lib.R_BAD_ARG
    assert L.qlzx_gc_liveness(*_args("qlzx_gc_liveness", flags=1, workspace_bytes=1)) == _lib.R_WORKSPACE
    assert L.qlzx_gc_liveness(*_args("qlzx_gc_liveness", data=DATA + 8)) == _lib.R_BAD_ARG
    assert b"qlzx_gc_liveness" in L.qlzx_last_error() and b"aligned" in L.qlzx_last_error()
    assert L.qlzx_gc_liveness(*_args("qlzx_gc_liveness", data=None, size=0, workspace_bytes=1)) == _lib.R_WORKSPACE


def test_zero_work_returns_ok_whatever_the_other_arguments():
    L = _L()
    assert L.qlzx_htree_get(*_args("qlzx_htree_get", n=0, image=None, totals=None, workspace=None, depth=9)) == \
        _lib.R_OK
    assert L.qlzx_gc_liveness(*_args("qlzx_gc_liveness", cap=0, image=None, totals=None, workspace=None,
                                     depth=9)) == _lib.R_OK
    assert L.qlzx_htree_move(*_args("qlzx_htree_move", cap=0, image=None, totals=None, workspace=None, depth=9)) == \
        _lib.R_OK
