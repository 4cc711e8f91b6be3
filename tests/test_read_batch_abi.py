"""The batched-read entry points (qlzx_read_plan_workspace_size, qlzx_read_plan, qlzx_read_finish):
declared, exported, and their argument checks answer before any HIP call (no GPU)."""
import ctypes
import subprocess

from gobeansdb_amd import _lib, build

NAMES = {"qlzx_read_plan_workspace_size", "qlzx_read_plan", "qlzx_read_finish"}
P = 0x1000          # a fake non-null pointer: a call that got past its checks would need a device
SIZE = 1 << 20


def _L():
    build.build()
    return _lib.lib()


def test_declared_and_exported():
    L = _L()
    assert NAMES <= set(_lib.header_functions())
    for n in NAMES:
        assert hasattr(L, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert NAMES <= {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_status_names():
    assert [_lib.RD_OK, _lib.RD_ALIGN, _lib.RD_EOF_HEADER, _lib.RD_KEY_SIZE, _lib.RD_VALUE_SIZE, _lib.RD_EOF_BODY,
            _lib.RD_CRC] == list(range(7))
    assert len(_lib.RD_NAMES) == 7 and _lib.RD_NAMES[_lib.RD_CRC] == "RD_CRC"


def test_workspace_size_positive_and_monotone():
    L = _L()
    sizes = [L.qlzx_read_plan_workspace_size(n) for n in (0, 1, 1024, 1025, 1 << 20)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)


def _plan_args(n=4, **kw):
    """Positional arguments of qlzx_read_plan, every pointer fake and non-null, no keys."""
    a = dict(data=P, size=SIZE, rec_off=P, n=n, max_key=250, body_max=50 << 20, want_key=None, want_key_off=None,
             want_key_len=None, rd_status=P, key_eq=None, hdr=P, comp_idx=P, comp_off=P, comp_len=P, comp_dsize=P,
             comp_dst_off=P, totals=P, workspace=P, workspace_bytes=1 << 30, stream=None)
    a.update(kw)
    return list(a.values())


def test_plan_argument_checks_run_before_any_hip_call():
    L = _L()
    for name in ("data", "rec_off", "rd_status", "hdr", "comp_idx", "comp_off", "comp_len", "comp_dsize",
                 "comp_dst_off", "totals"):
        assert L.qlzx_read_plan(*_plan_args(**{name: None})) == _lib.R_BAD_ARG, name
        assert b"qlzx_read_plan" in L.qlzx_last_error()
    # the wanted keys come as all three or none, and key_eq goes with them
    for part in ({"want_key": P}, {"want_key_off": P}, {"want_key_len": P}, {"want_key": P, "want_key_off": P},
                 {"want_key": P, "want_key_len": P}, {"want_key_off": P, "want_key_len": P}):
        assert L.qlzx_read_plan(*_plan_args(key_eq=P, **part)) == _lib.R_BAD_ARG, part
    all3 = {"want_key": P, "want_key_off": P, "want_key_len": P}
    assert L.qlzx_read_plan(*_plan_args(key_eq=None, **all3)) == _lib.R_BAD_ARG
    assert L.qlzx_read_plan(*_plan_args(key_eq=P)) == _lib.R_BAD_ARG
    # a chunk whose slot numbers do not fit
    assert L.qlzx_read_plan(*_plan_args(size=0xfffffff0 * 256)) == _lib.R_BAD_ARG
    # a short or missing workspace
    need = L.qlzx_read_plan_workspace_size(4)
    assert L.qlzx_read_plan(*_plan_args(workspace_bytes=need - 1)) == _lib.R_WORKSPACE
    assert L.qlzx_read_plan(*_plan_args(workspace=None)) == _lib.R_WORKSPACE
    assert L.qlzx_read_plan(*_plan_args(key_eq=P, workspace_bytes=need - 1, **all3)) == _lib.R_WORKSPACE


def test_finish_argument_checks_run_before_any_hip_call():
    L = _L()
    names = ["data", "rec_off", "n", "rd_status", "totals", "comp_idx", "comp_status", "comp_dsize", "comp_dst_off",
             "outbuf", "flag", "value_len", "in_out", "val_off", "vhash", "dec_status", "stream"]
    base = {k: P for k in names}
    base.update(n=4, stream=None)
    for name in names:
        if name in ("data", "outbuf", "n", "stream"):   # nullable: unread when nothing passed / decoded
            continue
        args = dict(base, **{name: None})
        assert L.qlzx_read_finish(*args.values()) == _lib.R_BAD_ARG, name
    # no requests: nothing to do, whatever the pointers
    assert L.qlzx_read_finish(*dict(base, n=0, rec_off=None, flag=None).values()) == _lib.R_OK
