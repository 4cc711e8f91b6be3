"""The workspace contract of the batch C ABI, the part that needs no GPU: the proxy's table is the
header's, its guard logic finds what it should (on CPU tensors), and every entry point answers a
workspace that is one byte short or off the documented 16-byte alignment with QLZX_R_WORKSPACE
before any HIP call (fake pointers: a call that got past its checks would need a device).
tests/test_gpu_workspace_contract.py runs the kernels under the proxy."""
import ctypes
import re

import pytest
import torch

import ws_contract as W
from gobeansdb_amd import _lib, build

P = 0x1000                          # a fake non-null pointer, 16-B aligned
DATA, OUT = 0x10000, 0x100000       # 16-B aligned and, with SIZE / out_cap below, disjoint
SIZE = 0x8000
BIG = 1 << 40
N = 4
SCALARS = dict(size=SIZE, start=0, max_key=250, body_max=50 << 20, cap=N, n=N, n_files=2, bytes=SIZE, max_chunks=3,
               data_file_max=4000 << 20, out_cap=SIZE, first=0, split_cap=1024, index_interval=4096, max_offset_in=0,
               chunk_id=0, flags=0, not_compress=0, max_dsize=16384, max_len=4096, stream=None)
POINTERS = dict(data=DATA, out=OUT)


def _L():
    build.build()
    return _lib.lib()


def _prototypes():
    """{function: [(parameter name, is a pointer)]} for every qlzx_* prototype of include/qlzx.h."""
    text = open(_lib.HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    out = {}
    for name, params in re.findall(r"\b(qlzx_[A-Za-z0-9_]*)\s*\(([^;{]*)\)\s*;", text):
        ps = [p.strip() for p in params.split(",")]
        out[name] = [] if ps == ["void"] else [(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", p)[-1], "*" in p) for p in ps]
    return out


def _need(L, name):
    """What the entry point's own *_workspace_size() asks for the SCALARS above."""
    S = SCALARS
    if name == "qlzx_decompress_batch":
        return L.qlzx_decompress_workspace_size(N, S["max_dsize"])
    if name == "qlzx_compress_batch":
        return L.qlzx_compress_workspace_size(N, S["max_len"])
    if name == "qlzx_go_l1_compress_batch":
        return L.qlzx_go_l1_workspace_size(N)
    if name == "qlzx_go_decompress_batch":
        return L.qlzx_go_decompress_workspace_size(N)
    if name == "qlzx_replay_index":
        return L.qlzx_replay_workspace_size(S["size"])
    if name == "qlzx_replay_plan":
        return L.qlzx_replay_plan_workspace_size(S["cap"])
    if name == "qlzx_read_plan":
        return L.qlzx_read_plan_workspace_size(N)
    if name.startswith("qlzx_write_"):
        return L.qlzx_write_plan_workspace_size(N)
    if name.startswith("qlzx_gc_"):
        return L.qlzx_gc_workspace_size(S["cap"], S["max_chunks"])
    if name == "qlzx_hint_merge_plan":
        return L.qlzx_hint_merge_workspace_size(S["bytes"], S["n_files"], S["cap"])
    if name == "qlzx_hint_merge_write":      # "the plan's workspace, for one source at the least"
        return L.qlzx_hint_merge_workspace_size(S["bytes"], 1, S["cap"])
    if name == "qlzx_hint_lookup":
        return L.qlzx_hint_lookup_workspace_size(N, S["n_files"])
    assert name in ("qlzx_hint_plan", "qlzx_hint_write"), name
    return L.qlzx_hint_workspace_size(S["cap"])


def _args(name, workspace, workspace_bytes, keep):
    """Arguments that pass every check of `name` but the workspace's.  keep: objects that must
    outlive the call (the qlzx_blocks struct)."""
    out = []
    for pname, pointer in _prototypes()[name]:
        if pname == "b":
            keep.append(_lib.Blocks(P, P, P, P, P, N))
            out.append(ctypes.byref(keep[-1]))
        elif pname == "workspace":
            out.append(workspace)
        elif pname == "workspace_bytes":
            out.append(workspace_bytes)
        elif pointer and pname != "stream":
            out.append(POINTERS.get(pname, P))
        else:
            out.append(SCALARS[pname])
    return out


def test_the_proxys_table_is_the_headers():
    """Exactly the functions with a workspace_bytes parameter, each with (workspace,
    workspace_bytes, stream) as its last three: what the proxy's argument surgery relies on."""
    protos = _prototypes()
    assert set(protos) == {n for n in _lib.header_functions() if n.startswith("qlzx_")}
    with_ws = {n for n, ps in protos.items() if any(p == "workspace_bytes" for p, _ in ps)}
    assert with_ws == set(W.ENTRY_POINTS) and len(W.ENTRY_POINTS) == 17
    for n in with_ws:
        assert [p for p, _ in protos[n][-3:]] == ["workspace", "workspace_bytes", "stream"], n
        assert len(getattr(_lib.lib(), n).argtypes) == len(protos[n]), n


def test_header_states_the_alignment_and_no_state():
    text = " ".join(open(_lib.HEADER).read().replace(" *", " ").split())
    assert "`workspace` must be 16-byte aligned" in text
    assert W.BASE_ALIGN == 16
    # write, GC, hint and hint merge: one workspace serves the calls of a group, nothing travels in it
    assert text.count("no state is carried in it") == 4


# ---- the guard logic, on CPU tensors ----
def _guarded(nbytes, poison, at=0):
    buf = torch.empty(W.buffer_bytes(nbytes) + at, dtype=torch.uint8)[at:]
    base = W.base_offset(buf.data_ptr())
    W.fill(buf, base, nbytes, poison)
    return buf, base


@pytest.mark.parametrize("at", [0, 1, 17, 255])
def test_the_base_sits_at_the_documented_alignment_and_no_stricter(at):
    buf, base = _guarded(1000, "ff", at)
    assert (buf.data_ptr() + base) % 256 == W.BASE_ALIGN
    assert W.GUARD_BYTES <= base and base + 1000 + W.GUARD_BYTES <= buf.numel()


@pytest.mark.parametrize("poison", list(W.POISONS))
@pytest.mark.parametrize("nbytes", [0, 1, 4096, 100001])
def test_guards_untouched_and_workspace_writes_pass(poison, nbytes):
    buf, base = _guarded(nbytes, poison)
    ws = buf[base:base + nbytes]
    if W.POISONS[poison] is not None:
        assert bool((ws == W.POISONS[poison]).all())
    elif nbytes >= 4096:      # seeded: the same bytes every time, and not one value
        again, base2 = _guarded(nbytes, poison)
        assert torch.equal(ws, again[base2:base2 + nbytes])
        assert ws.unique().numel() > 200
    assert W.first_touched(buf, base, nbytes) is None
    W.check("f", buf, base, nbytes)
    if nbytes:                # every byte of the workspace is the call's to write
        ws.fill_(W.GUARD_FILL ^ 0xFF)
        ws[0], ws[-1] = 0, 1
        W.check("f", buf, base, nbytes)


@pytest.mark.parametrize("nbytes", [0, 4096, 100001])
@pytest.mark.parametrize("where", ["last byte before the base", "first byte of the front guard",
                                   "first byte past the workspace", "last byte of the back guard", "both guards"])
def test_one_changed_guard_byte_is_reported_with_its_offset(where, nbytes):
    buf, base = _guarded(nbytes, "5a")
    want = {"last byte before the base": -1, "first byte of the front guard": -W.GUARD_BYTES,
            "first byte past the workspace": nbytes, "last byte of the back guard": nbytes + W.GUARD_BYTES - 1,
            "both guards": -7}[where]
    buf[base + want] ^= 0x01
    if where == "both guards":
        buf[base + nbytes + 300] = 0
    assert W.first_touched(buf, base, nbytes) == want
    with pytest.raises(W.GuardTouched, match="qlzx_some_call") as e:
        W.check("qlzx_some_call", buf, base, nbytes)
    assert (e.value.name, e.value.offset, e.value.workspace_bytes) == ("qlzx_some_call", want, nbytes)
    assert f"offset {want} " in str(e.value)


def test_the_proxy_forwards_what_it_does_not_guard():
    """The size functions, the single-call symbols and a null workspace go to the library as they
    are (no device is touched: the proxy allocates only for a non-null workspace)."""
    L = _L()
    X = W.Proxy(L, "ff")
    assert X.qlzx_decompress_workspace_size(5, 65536) == L.qlzx_decompress_workspace_size(5, 65536) == 171264
    assert X.qlz_get_setting(0) == 3
    keep = []
    for name in W.ENTRY_POINTS:          # a null workspace: the library's own answer, nothing counted
        if name != "qlzx_decompress_batch":      # (that one decodes without a workspace: it would launch)
            assert getattr(X, name)(*_args(name, None, BIG, keep)) == _lib.R_WORKSPACE, name
    assert not X.calls and not X.bytes
    with pytest.raises(AssertionError, match="never reached"):
        X.require(["qlzx_gc_plan"])


# ---- QLZX_R_WORKSPACE before any launch ----
@pytest.mark.parametrize("name", [n for n in W.ENTRY_POINTS if n != "qlzx_decompress_batch"])
def test_one_byte_short_is_refused(name):
    L = _L()
    fn, need, keep = getattr(L, name), _need(L, name), []
    assert need > 0
    assert fn(*_args(name, P, need - 1, keep)) == _lib.R_WORKSPACE
    assert name.encode() in L.qlzx_last_error()
    assert fn(*_args(name, None, BIG, keep)) == _lib.R_WORKSPACE


@pytest.mark.parametrize("name", W.ENTRY_POINTS)
@pytest.mark.parametrize("off", [1, 4, 8, 15, 16 + 8])
def test_a_base_off_the_16_byte_grid_is_refused(name, off):
    """Level 1 always asked for 16 bytes; now every entry point does, with a size that is enough."""
    L = _L()
    keep = []
    assert getattr(L, name)(*_args(name, P + off, BIG, keep)) == _lib.R_WORKSPACE
    assert name.encode() in L.qlzx_last_error()
    if "_go_" not in name:
        assert b"not 16-byte aligned" in L.qlzx_last_error()


def test_decompress_takes_a_short_workspace_as_no_workspace():
    """The documented exception: a workspace below one region is not an error, the call decodes
    lane-per-block.  That route launches, so here only what the argument checks alone decide: an
    empty batch is QLZX_R_OK whatever the workspace, and a short aligned workspace is never
    QLZX_R_WORKSPACE material -- the size check sits in no argument check of this call (the GPU test
    test_decode_short_workspace_is_the_lane_route runs the route)."""
    L = _L()
    empty = _lib.Blocks(P, P, P, P, P, 0)
    for ws, nbytes in ((P, 0), (P, 1), (None, 0), (P + 8, BIG)):
        assert L.qlzx_decompress_batch(ctypes.byref(empty), None, P, P, None, None, None, 16384, ws, nbytes,
                                       None) == _lib.R_OK
    assert L.qlzx_decompress_batch(None, None, P, P, None, None, None, 16384, P, BIG, None) == _lib.R_BAD_ARG
