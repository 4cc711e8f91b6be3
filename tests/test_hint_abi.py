"""The hint build entry points (qlzx_keyhash_batch, qlzx_hint_workspace_size, qlzx_hint_plan,
qlzx_hint_write): declared, exported, and their argument checks answer before any HIP call (no GPU)."""
import subprocess

from gobeansdb_amd import _lib, build

NAMES = {"qlzx_keyhash_batch", "qlzx_hint_workspace_size", "qlzx_hint_plan", "qlzx_hint_write"}
P = 0x1000          # a fake non-null pointer: a call that got past its checks would need a device
DATA, OUT = 0x10000, 0x100000
SIZE = 0x8000
BIG = 1 << 30

PLAN = ["data", "size", "rec_off", "result", "cap", "hdr", "keyhash", "first", "split_cap", "index_interval",
        "max_offset_in", "item_rec", "item_hash", "item_off", "index_item", "totals", "workspace", "workspace_bytes",
        "stream"]
WRITE = ["data", "size", "rec_off", "cap", "hdr", "vhash", "chunk_id", "item_rec", "item_hash", "item_off",
         "index_item", "out", "out_cap", "totals", "workspace", "workspace_bytes", "stream"]
SCALARS = dict(size=SIZE, cap=4, first=0, split_cap=1 << 20, index_interval=4096, max_offset_in=0, chunk_id=0,
               out_cap=SIZE, workspace_bytes=BIG, stream=None)
POINTERS = dict(data=DATA, out=OUT)
OPTIONAL = {"keyhash"}      # NULL: the default key hash


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


def test_names():
    assert [_lib.HINT_CONSUMED, _lib.HINT_NUM_KEY, _lib.HINT_N_INDEX, _lib.HINT_DATASIZE, _lib.HINT_INDEX_OFF_LO,
            _lib.HINT_INDEX_OFF_HI, _lib.HINT_BYTES_LO, _lib.HINT_BYTES_HI, _lib.HINT_STATUS,
            _lib.HINT_SKIPPED] == list(range(10))
    assert _lib.HINT_NO_SPACE == 1 and "#define QLZX_HINT_NO_SPACE 1" in open(_lib.HEADER).read()
    assert (_lib.HINT_SPLIT_CAP, _lib.HINT_INDEX_INTERVAL) == (1 << 20, 4096)
    from gobeansdb_amd import hint
    assert callable(hint.keyhash) and callable(hint.build_split) and callable(hint.build)


def test_workspace_size_positive_and_monotone():
    L = _L()
    sizes = [L.qlzx_hint_workspace_size(n) for n in (0, 1, 1024, 1025, 1 << 20, 1 << 24)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]


def _common_checks(fn, fname, names):
    L = _L()
    for name in names:
        if name in SCALARS or name == "workspace" or name in OPTIONAL:
            continue
        assert fn(*_args(names, **{name: None})) == _lib.R_BAD_ARG, name
        assert fname in L.qlzx_last_error()
    need = L.qlzx_hint_workspace_size(SCALARS["cap"])
    assert fn(*_args(names, workspace_bytes=need - 1)) == _lib.R_WORKSPACE
    assert fname in L.qlzx_last_error()
    assert fn(*_args(names, workspace=None)) == _lib.R_WORKSPACE
    assert fname in L.qlzx_last_error()
    assert fn(*_args(names, size=0xfffffff0 * 256)) == _lib.R_BAD_ARG      # record offsets would not fit
    assert fname in L.qlzx_last_error()
    # a null chunk of no bytes is no error: the call gets past that check (asked with a short workspace)
    assert fn(*_args(names, data=None, size=0, workspace_bytes=1)) == _lib.R_WORKSPACE
    # no capacity: nothing to do, whatever the other pointers
    assert fn(*_args(names, cap=0, data=None, rec_off=None, totals=None, workspace=None, split_cap=0)) == _lib.R_OK


def test_plan_argument_checks_run_before_any_hip_call():
    L = _L()
    _common_checks(L.qlzx_hint_plan, b"qlzx_hint_plan", PLAN)
    assert L.qlzx_hint_plan(*_args(PLAN, split_cap=0)) == _lib.R_BAD_ARG
    assert b"qlzx_hint_plan" in L.qlzx_last_error() and b"split_cap" in L.qlzx_last_error()
    # keyhash is optional: null gets past the pointer checks
    assert L.qlzx_hint_plan(*_args(PLAN, keyhash=None, workspace_bytes=1)) == _lib.R_WORKSPACE


def test_write_argument_checks_run_before_any_hip_call():
    L = _L()
    _common_checks(L.qlzx_hint_write, b"qlzx_hint_write", WRITE)
    assert L.qlzx_hint_write(*_args(WRITE, out=OUT + 8)) == _lib.R_BAD_ARG      # 16-B stores
    assert b"qlzx_hint_write" in L.qlzx_last_error()
    # no room at all is the device's verdict (totals[8]), not an argument error
    assert L.qlzx_hint_write(*_args(WRITE, out=None, out_cap=0, workspace_bytes=1)) == _lib.R_WORKSPACE


def test_keyhash_argument_checks():
    L = _L()
    assert L.qlzx_keyhash_batch(None, None, None, 0, None, None) == _lib.R_OK
    for k in range(4):
        a = [P, P, P, 3, P, None]
        a[k if k < 3 else 4] = None
        assert L.qlzx_keyhash_batch(*a) == _lib.R_BAD_ARG
        assert b"qlzx_keyhash_batch" in L.qlzx_last_error()
