"""The hint merge entry points (qlzx_hint_merge_workspace_size, qlzx_hint_merge_plan,
qlzx_hint_merge_write): declared, exported, bound, and their argument checks answer before any HIP
call (no GPU)."""
import subprocess

from gobeansdb_amd import _lib, build

NAMES = {"qlzx_hint_merge_workspace_size", "qlzx_hint_merge_plan", "qlzx_hint_merge_write"}
P = 0x1000          # a fake non-null pointer: a call that got past its checks would need a device
HINTS, OUT = 0x10000, 0x100000
BYTES = 0x8000
BIG = 1 << 30

PLAN = ["hints", "bytes", "file_off", "file_len", "file_chunk", "n_files", "cap", "index_interval", "item_src",
        "item_chunk", "item_off", "index_item", "coll_item", "totals", "workspace", "workspace_bytes", "stream"]
WRITE = ["hints", "bytes", "cap", "item_src", "item_chunk", "item_off", "index_item", "out", "out_cap", "totals",
         "workspace", "workspace_bytes", "stream"]
SCALARS = dict(bytes=BYTES, n_files=3, cap=4, index_interval=4096, out_cap=BYTES, workspace_bytes=BIG, stream=None)
POINTERS = dict(hints=HINTS, out=OUT)


def _L():
    build.build()
    return _lib.lib()


def _args(names, **kw):
    a = {k: SCALARS[k] if k in SCALARS else POINTERS.get(k, P) for k in names}
    a.update(kw)
    return list(a.values())


def test_declared_exported_and_bound():
    L = _L()
    assert NAMES <= set(_lib.header_functions())
    for n in NAMES:
        assert hasattr(L, n) and getattr(L, n).argtypes is not None, n
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert NAMES <= {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_names():
    assert [_lib.HM_OK, _lib.HM_NO_SPACE, _lib.HM_BAD_FILE, _lib.HM_TOO_MANY, _lib.HM_UNSORTED] == list(range(5))
    assert _lib.HM_NAMES == ["HM_OK", "HM_NO_SPACE", "HM_BAD_FILE", "HM_TOO_MANY", "HM_UNSORTED"]
    assert "enum qlzx_hm_status { QLZX_HM_OK = 0, QLZX_HM_NO_SPACE, QLZX_HM_BAD_FILE, QLZX_HM_TOO_MANY, " \
           "QLZX_HM_UNSORTED };" in open(_lib.HEADER).read()
    # entries 1..8 of totals sit where qlzx_hint_plan has them
    assert [_lib.HM_NUM_KEY, _lib.HM_N_INDEX, _lib.HM_DATASIZE, _lib.HM_INDEX_OFF_LO, _lib.HM_INDEX_OFF_HI,
            _lib.HM_BYTES_LO, _lib.HM_BYTES_HI, _lib.HM_STATUS] == \
        [_lib.HINT_NUM_KEY, _lib.HINT_N_INDEX, _lib.HINT_DATASIZE, _lib.HINT_INDEX_OFF_LO, _lib.HINT_INDEX_OFF_HI,
         _lib.HINT_BYTES_LO, _lib.HINT_BYTES_HI, _lib.HINT_STATUS]
    assert (_lib.HM_ITEMS_READ, _lib.HM_STATUS_SOURCE, _lib.HM_N_COLLISION) == (0, 9, 10)
    from gobeansdb_amd import hint
    assert callable(hint.merge) and callable(hint.merge_packed)
    assert {"file", "num_key", "datasize", "index_offset", "n_index", "items_read", "collisions"} == \
        set(hint.HintMerged.__dataclass_fields__)


def test_workspace_size_positive_and_monotone():
    L = _L()
    caps = [L.qlzx_hint_merge_workspace_size(BYTES, 2, n) for n in (0, 1, 1024, 1025, 1 << 20, 1 << 24)]
    assert all(s > 0 for s in caps)
    assert caps == sorted(caps) and caps[-1] > caps[0]
    files = [L.qlzx_hint_merge_workspace_size(BYTES, n, 1024) for n in (0, 1, 65, 1000, 1 << 20)]
    assert files == sorted(files) and files[-1] > files[0]


def _common_checks(fn, fname, names, need):
    L = _L()
    for name in names:
        if name in SCALARS or name == "workspace":
            continue
        assert fn(*_args(names, **{name: None})) == _lib.R_BAD_ARG, name
        assert fname in L.qlzx_last_error()
    assert fn(*_args(names, workspace_bytes=need - 1)) == _lib.R_WORKSPACE
    assert fname in L.qlzx_last_error()
    assert fn(*_args(names, workspace=None)) == _lib.R_WORKSPACE
    assert fname in L.qlzx_last_error()
    # a null buffer of no bytes is no error: the call gets past that check (asked with a short workspace)
    assert fn(*_args(names, hints=None, bytes=0, workspace_bytes=1)) == _lib.R_WORKSPACE
    # no capacity: nothing to do, whatever the other pointers
    assert fn(*_args(names, cap=0, hints=None, item_src=None, totals=None, workspace=None)) == _lib.R_OK


def test_plan_argument_checks_run_before_any_hip_call():
    L = _L()
    need = L.qlzx_hint_merge_workspace_size(BYTES, SCALARS["n_files"], SCALARS["cap"])
    _common_checks(L.qlzx_hint_merge_plan, b"qlzx_hint_merge_plan", PLAN, need)
    assert L.qlzx_hint_merge_plan(*_args(PLAN, n_files=0, file_off=None, totals=None, workspace=None)) == _lib.R_OK


def test_write_argument_checks_run_before_any_hip_call():
    L = _L()
    need = L.qlzx_hint_merge_workspace_size(BYTES, 1, SCALARS["cap"])
    _common_checks(L.qlzx_hint_merge_write, b"qlzx_hint_merge_write", WRITE, need)
    assert L.qlzx_hint_merge_write(*_args(WRITE, out=OUT + 8)) == _lib.R_BAD_ARG      # 16-B stores
    assert b"qlzx_hint_merge_write" in L.qlzx_last_error() and b"aligned" in L.qlzx_last_error()
    # no room at all is the device's verdict (totals[8]), not an argument error
    assert L.qlzx_hint_merge_write(*_args(WRITE, out=None, out_cap=0, workspace_bytes=1)) == _lib.R_WORKSPACE
