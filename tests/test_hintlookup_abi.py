"""The hint lookup entry points (qlzx_hint_lookup_workspace_size, qlzx_hint_lookup): declared,
exported, bound, and their argument checks answer before any HIP call (no GPU)."""
import subprocess

from gobeansdb_amd import _lib, build

NAMES = {"qlzx_hint_lookup_workspace_size", "qlzx_hint_lookup"}
P = 0x1000          # a fake non-null pointer: a call that got past its checks would need a device
HINTS = 0x10000
BYTES = 0x8000
BIG = 1 << 30

ARGS = ["hints", "bytes", "file_off", "file_len", "file_chunk", "file_flags", "n_files", "keys", "key_off", "key_len",
        "keyhash", "n", "flags", "status", "hit_file", "chunk", "offset", "ver", "vhash", "item_src", "totals",
        "workspace", "workspace_bytes", "stream"]
SCALARS = dict(bytes=BYTES, n_files=3, n=5, flags=0, workspace_bytes=BIG, stream=None)
POINTERS = dict(hints=HINTS)
OPTIONAL = {"keyhash"}   # NULL: getKeyHashDefalut


def _L():
    build.build()
    return _lib.lib()


def _args(**kw):
    a = {k: SCALARS[k] if k in SCALARS else POINTERS.get(k, P) for k in ARGS}
    a.update(kw)
    return list(a.values())


def test_declared_exported_and_bound():
    L = _L()
    assert NAMES <= set(_lib.header_functions())
    for n in NAMES:
        assert hasattr(L, n) and getattr(L, n).argtypes is not None, n
    assert len(L.qlzx_hint_lookup.argtypes) == len(ARGS)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert NAMES <= {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_names():
    assert [_lib.HL_MISS, _lib.HL_FOUND, _lib.HL_ERR, _lib.HL_BAD_FILE] == list(range(4))
    assert _lib.HL_NAMES == ["HL_MISS", "HL_FOUND", "HL_ERR", "HL_BAD_FILE"]
    text = open(_lib.HEADER).read()
    assert "enum qlzx_hl_status { QLZX_HL_MISS = 0, QLZX_HL_FOUND, QLZX_HL_ERR, QLZX_HL_BAD_FILE };" in text
    assert f"#define QLZX_HL_FILE_MERGED {_lib.HL_FILE_MERGED}u" in text
    assert f"#define QLZX_HL_F_BOUNDED {_lib.HL_F_BOUNDED}u" in text
    assert f"#define QLZX_HL_F_LANE {_lib.HL_F_LANE}u" in text
    assert f"#define QLZX_HL_F_WAVE {_lib.HL_F_WAVE}u" in text
    assert f"#define QLZX_HL_LANE_FROM {_lib.HL_LANE_FROM}u" in text
    # totals = {found, miss, err, bad_file}
    assert (_lib.HL_N_FOUND, _lib.HL_N_MISS, _lib.HL_N_ERR, _lib.HL_N_BAD_FILE) == (0, 1, 2, 3)
    from gobeansdb_amd import hint
    assert callable(hint.lookup) and callable(hint.lookup_packed)
    assert {"status", "hit_file", "chunk", "offset", "ver", "vhash", "item_src", "totals"} == \
        set(hint.HintLookup.__dataclass_fields__)


def test_workspace_size_positive_and_monotone():
    L = _L()
    by_n = [L.qlzx_hint_lookup_workspace_size(n, 2) for n in (0, 1, 64, 65, 1 << 12, 1 << 18, 1 << 24)]
    assert all(s > 0 for s in by_n)
    assert by_n == sorted(by_n) and by_n[-1] > by_n[0]
    by_files = [L.qlzx_hint_lookup_workspace_size(1024, n) for n in (0, 1, 65, 1000, 1 << 20)]
    assert all(s > 0 for s in by_files)
    assert by_files == sorted(by_files) and by_files[-1] > by_files[0]


def test_argument_checks_run_before_any_hip_call():
    L = _L()
    fn, fname = L.qlzx_hint_lookup, b"qlzx_hint_lookup"
    need = L.qlzx_hint_lookup_workspace_size(SCALARS["n"], SCALARS["n_files"])
    for name in ARGS:
        if name in SCALARS or name in OPTIONAL or name == "workspace":
            continue
        assert fn(*_args(**{name: None})) == _lib.R_BAD_ARG, name
        assert fname in L.qlzx_last_error()
    for flags in (8, 1 << 31, _lib.HL_F_LANE | _lib.HL_F_WAVE):
        assert fn(*_args(flags=flags)) == _lib.R_BAD_ARG
        assert fname in L.qlzx_last_error() and b"flag" in L.qlzx_last_error()
    for kw in (dict(workspace_bytes=need - 1), dict(workspace=None)):
        assert fn(*_args(**kw)) == _lib.R_WORKSPACE
        assert fname in L.qlzx_last_error()
    # a null keyhash and a null buffer of no bytes are no errors: the call gets past those checks
    # (asked with a short workspace)
    assert fn(*_args(keyhash=None, workspace_bytes=1)) == _lib.R_WORKSPACE
    assert fn(*_args(hints=None, bytes=0, workspace_bytes=1)) == _lib.R_WORKSPACE
    for flags in (_lib.HL_F_BOUNDED, _lib.HL_F_LANE, _lib.HL_F_WAVE, _lib.HL_F_BOUNDED | _lib.HL_F_LANE,
                  _lib.HL_F_BOUNDED | _lib.HL_F_WAVE):
        assert fn(*_args(flags=flags, workspace_bytes=1)) == _lib.R_WORKSPACE
    # no request, or no file (every request a miss): nothing to do, whatever the other pointers
    assert fn(*_args(n=0, hints=None, keys=None, status=None, totals=None, workspace=None)) == _lib.R_OK
    assert fn(*_args(n_files=0, file_off=None, status=None, totals=None, workspace=None)) == _lib.R_OK
