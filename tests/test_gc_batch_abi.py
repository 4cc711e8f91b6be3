"""The GC rewrite entry points (qlzx_gc_workspace_size, qlzx_gc_plan, qlzx_gc_rewrite): declared,
exported, and their argument checks answer before any HIP call (no GPU)."""
import subprocess

from gobeansdb_amd import _lib, build

NAMES = {"qlzx_gc_workspace_size", "qlzx_gc_plan", "qlzx_gc_rewrite"}
P = 0x1000          # a fake non-null pointer: a call that got past its checks would need a device
DATA, OUT = 0x10000, 0x100000       # 16-B aligned and, with SIZE / out_cap below, disjoint
SIZE = 0x8000
BIG = 1 << 30

PLAN = ["data", "size", "rec_off", "result", "cap", "keep", "max_key", "body_max", "data_file_max", "chunk_head",
        "max_chunks", "gc_status", "new_chunk", "new_off", "chunk_base", "chunk_bytes", "totals", "workspace",
        "workspace_bytes", "stream"]
REWRITE = ["data", "size", "rec_off", "result", "cap", "chunk_head", "max_chunks", "new_chunk", "new_off",
           "chunk_base", "out", "out_cap", "gc_status", "crc", "totals", "workspace", "workspace_bytes", "stream"]
SCALARS = dict(size=SIZE, cap=4, max_key=250, body_max=50 << 20, data_file_max=4000 << 20, max_chunks=3,
               out_cap=SIZE, workspace_bytes=BIG, stream=None)
POINTERS = dict(data=DATA, out=OUT)


def _L():
    build.build()
    return _lib.lib()


def _args(names, **kw):
    a = {k: SCALARS[k] if k in SCALARS else POINTERS.get(k, P) for k in names}
    a.update(kw)
    return list(a.values())


def test_declared_and_exported():
    L = _L()
    assert NAMES <= set(_lib.header_functions())
    for n in NAMES:
        assert hasattr(L, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert NAMES <= {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_status_names():
    assert [_lib.GC_WRITTEN, _lib.GC_DROPPED, _lib.GC_BAD_RECORD, _lib.GC_NO_CHUNK, _lib.GC_NO_SPACE] == list(range(5))
    assert len(_lib.GC_NAMES) == 5 and _lib.GC_NAMES[_lib.GC_NO_SPACE] == "GC_NO_SPACE"
    text = open(_lib.HEADER).read()
    assert ("enum qlzx_gc_status { QLZX_GC_WRITTEN = 0, QLZX_GC_DROPPED, QLZX_GC_BAD_RECORD, QLZX_GC_NO_CHUNK, "
            "QLZX_GC_NO_SPACE };") in text


def test_workspace_size_positive_and_monotone():
    L = _L()
    by_cap = [L.qlzx_gc_workspace_size(n, 1) for n in (0, 1, 1024, 1025, 1 << 20)]
    by_chunks = [L.qlzx_gc_workspace_size(1000, c) for c in (1, 2, 64, 500, 998)]
    for sizes in (by_cap, by_chunks):
        assert all(s > 0 for s in sizes)
        assert sizes == sorted(sizes)
    assert by_cap[-1] > by_cap[0] and by_chunks[-1] > by_chunks[0]


def _common_checks(fn, fname, names):
    L = _L()
    for name in names:
        if name in SCALARS or name == "workspace":
            continue
        assert fn(*_args(names, **{name: None})) == _lib.R_BAD_ARG, name
        assert fname in L.qlzx_last_error()
    need = L.qlzx_gc_workspace_size(SCALARS["cap"], SCALARS["max_chunks"])
    assert fn(*_args(names, workspace_bytes=need - 1)) == _lib.R_WORKSPACE
    assert fname in L.qlzx_last_error()
    assert fn(*_args(names, workspace=None)) == _lib.R_WORKSPACE
    for bad in (0, 999):                                   # 1 .. MAX_NUM_CHUNK
        assert fn(*_args(names, max_chunks=bad)) == _lib.R_BAD_ARG, bad
        assert fname in L.qlzx_last_error()
    assert fn(*_args(names, data=DATA + 8)) == _lib.R_BAD_ARG          # 16-B loads
    assert fname in L.qlzx_last_error()
    # no capacity: nothing to do, whatever the other pointers
    assert fn(*_args(names, cap=0, data=None, rec_off=None, totals=None, workspace=None, max_chunks=0)) == _lib.R_OK


def test_plan_argument_checks_run_before_any_hip_call():
    L = _L()
    _common_checks(L.qlzx_gc_plan, b"qlzx_gc_plan", PLAN)
    # sizes that would not fit 32 bits
    assert L.qlzx_gc_plan(*_args(PLAN, body_max=0xffffffff - 300)) == _lib.R_BAD_ARG


def test_rewrite_argument_checks_run_before_any_hip_call():
    L = _L()
    _common_checks(L.qlzx_gc_rewrite, b"qlzx_gc_rewrite", REWRITE)
    assert L.qlzx_gc_rewrite(*_args(REWRITE, out=OUT + 4)) == _lib.R_BAD_ARG      # 16-B stores
    assert b"qlzx_gc_rewrite" in L.qlzx_last_error()
    # a chunk cannot be rewritten onto itself: any overlap of [out, out + out_cap) with the source
    for out, out_cap in ((DATA, SIZE), (DATA + SIZE - 16, SIZE), (DATA - 0x1000, 0x1010), (DATA + 16, 16)):
        assert L.qlzx_gc_rewrite(*_args(REWRITE, out=out, out_cap=out_cap)) == _lib.R_BAD_ARG, (out, out_cap)
        assert b"overlaps" in L.qlzx_last_error()
    # touching ranges do not overlap: that call gets past the checks, so only its checks are asked
    # with a workspace that is too small
    for out, out_cap in ((DATA + SIZE, SIZE), (DATA - 0x1000, 0x1000)):
        assert L.qlzx_gc_rewrite(*_args(REWRITE, out=out, out_cap=out_cap, workspace_bytes=1)) == _lib.R_WORKSPACE
