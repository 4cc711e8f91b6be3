"""The batched-write entry points (qlzx_write_plan_workspace_size, qlzx_write_plan, qlzx_write_decide,
qlzx_write_finish): declared, exported, and their argument checks answer before any HIP call (no GPU)."""
import subprocess

from gobeansdb_amd import _lib, build, record

NAMES = {"qlzx_write_plan_workspace_size", "qlzx_write_plan", "qlzx_write_decide", "qlzx_write_finish"}
P = 0x1000          # a fake non-null pointer: a call that got past its checks would need a device
BIG = 1 << 30

PLAN = ["values", "val_off", "val_len", "key_len", "flag", "ver", "n", "max_key", "body_max", "not_compress",
        "wr_status", "try_idx", "try_off", "try_len", "try_dst_off", "totals", "workspace", "workspace_bytes", "stream"]
DECIDE = ["val_off", "val_len", "n", "totals", "try_idx", "try_len", "try_csize", "try_status", "keep", "full_idx",
          "full_off", "full_len", "full_dst_off", "totals2", "workspace", "workspace_bytes", "stream"]
FINISH = ["values", "val_off", "val_len", "keys", "key_off", "key_len", "flag", "ver", "ts", "n", "totals", "try_idx",
          "try_len", "try_dst_off", "try_csize", "try_crc", "keep", "trial_buf", "totals2", "full_idx",
          "full_dst_off", "full_csize", "full_status", "full_crc", "full_buf", "out", "out_cap", "wr_status",
          "rec_off", "flag_out", "vsz", "crc", "vhash", "totals3", "workspace", "workspace_bytes", "stream"]
SCALARS = dict(n=4, max_key=250, body_max=50 << 20, not_compress=_lib.NC_DEFAULT, out_cap=BIG, workspace_bytes=BIG,
               stream=None)
NULLABLE = {"trial_buf", "full_buf", "vhash"}      # unread when their list is empty / not wanted


def _L():
    build.build()
    return _lib.lib()


def _args(names, **kw):
    a = {k: SCALARS.get(k, P) for k in names}
    a.update(kw)
    return list(a.values())


def test_declared_and_exported():
    L = _L()
    assert NAMES <= set(_lib.header_functions())
    for n in NAMES:
        assert hasattr(L, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert NAMES <= {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_status_and_mask_names():
    assert [_lib.WR_OK, _lib.WR_KEY_SIZE, _lib.WR_VALUE_SIZE, _lib.WR_NO_SPACE] == list(range(4))
    assert len(_lib.WR_NAMES) == 4 and _lib.WR_NAMES[_lib.WR_NO_SPACE] == "WR_NO_SPACE"
    bits = [_lib.NC_AUDIO_BASIC, _lib.NC_AUDIO_AIFF, _lib.NC_AUDIO_MPEG, _lib.NC_APPLICATION_OGG, _lib.NC_AUDIO_MIDI,
            _lib.NC_VIDEO_AVI, _lib.NC_AUDIO_WAVE, _lib.NC_OTHER]
    assert bits == [1 << k for k in range(8)]
    # the bits follow record._AV_SIGS row by row, and the header says the same
    assert [ct for _, _, ct in record._AV_SIGS] == ["audio/basic", "audio/aiff", "audio/mpeg", "application/ogg",
                                                    "audio/midi", "video/avi", "audio/wave"]
    assert record.not_compress_mask(record.NOT_COMPRESS) == _lib.NC_DEFAULT == 0x44
    assert record.not_compress_mask(record.NOT_COMPRESS_SHIPPED) == 0x54      # "audio/ogg" names no row
    assert record.not_compress_mask({None}) == _lib.NC_OTHER and record.not_compress_mask(()) == 0
    text = open(_lib.HEADER).read()
    for k, name in enumerate(("AUDIO_BASIC", "AUDIO_AIFF", "AUDIO_MPEG", "APPLICATION_OGG", "AUDIO_MIDI", "VIDEO_AVI",
                              "AUDIO_WAVE", "OTHER")):
        assert f"#define QLZX_NC_{name} 0x{1 << k:02x}u" in text
    assert "QLZX_WR_OK = 0, QLZX_WR_KEY_SIZE, QLZX_WR_VALUE_SIZE, QLZX_WR_NO_SPACE" in text


def test_workspace_size_positive_and_monotone():
    L = _L()
    sizes = [L.qlzx_write_plan_workspace_size(n) for n in (0, 1, 1024, 1025, 1 << 20)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)


def _null_checks(fn, fname, names):
    L = _L()
    for name in names:
        if name in SCALARS or name in NULLABLE or name == "workspace":
            continue
        assert fn(*_args(names, **{name: None})) == _lib.R_BAD_ARG, name
        assert fname in L.qlzx_last_error()
    need = L.qlzx_write_plan_workspace_size(4)
    assert fn(*_args(names, workspace_bytes=need - 1)) == _lib.R_WORKSPACE
    assert fname in L.qlzx_last_error()
    assert fn(*_args(names, workspace=None)) == _lib.R_WORKSPACE


def test_plan_argument_checks_run_before_any_hip_call():
    L = _L()
    _null_checks(L.qlzx_write_plan, b"qlzx_write_plan", PLAN)
    # sizes that would not fit 32 bits
    assert L.qlzx_write_plan(*_args(PLAN, body_max=0xffffffff - 300)) == _lib.R_BAD_ARG
    # no records: nothing to do, whatever the other pointers
    assert L.qlzx_write_plan(*_args(PLAN, n=0, values=None, wr_status=None, workspace=None)) == _lib.R_OK
    assert L.qlzx_write_plan(*_args(PLAN, n=0, totals=None)) == _lib.R_BAD_ARG


def test_decide_argument_checks_run_before_any_hip_call():
    L = _L()
    _null_checks(L.qlzx_write_decide, b"qlzx_write_decide", DECIDE)
    assert L.qlzx_write_decide(*_args(DECIDE, n=0, keep=None, try_csize=None, workspace=None)) == _lib.R_OK
    assert L.qlzx_write_decide(*_args(DECIDE, n=0, totals2=None)) == _lib.R_BAD_ARG


def test_finish_argument_checks_run_before_any_hip_call():
    L = _L()
    _null_checks(L.qlzx_write_finish, b"qlzx_write_finish", FINISH)
    assert L.qlzx_write_finish(*_args(FINISH, out=P + 4)) == _lib.R_BAD_ARG      # 16-B stores
    assert L.qlzx_write_finish(*_args(FINISH, n=0, out=None, rec_off=None, workspace=None)) == _lib.R_OK
    assert L.qlzx_write_finish(*_args(FINISH, n=0, totals3=None)) == _lib.R_BAD_ARG
