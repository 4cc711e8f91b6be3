"""gobeansdb_amd._dev on the CPU device: the conversions every driver's uploads go through keep the
ABI's unsigned values bit for bit, whatever they arrive as."""
import inspect

import numpy as np
import pytest
import torch

from gobeansdb_amd import _dev, batch

EDGES64 = [0, 1 << 31, (1 << 32) - 1, 1 << 63, (1 << 64) - 1]
EDGES32 = EDGES64[:3]   # the ones 32 bits hold


def _bits(t: torch.Tensor, width: int) -> list[int]:
    return [int(x) & ((1 << width) - 1) for x in t.tolist()]


@pytest.mark.parametrize("fn, width, edges, udt, dt", [
    (_dev.u64, 64, EDGES64, np.uint64, torch.int64),
    (_dev.u32, 32, EDGES32, np.uint32, torch.int32),
    (_dev.i32, 32, EDGES32, np.uint32, torch.int32),
])
def test_round_trip_from_list_ndarray_and_tensor(fn, width, edges, udt, dt):
    arr = np.asarray(edges, dtype=udt)
    signed = torch.from_numpy(arr.view(np.int64 if width == 64 else np.int32).copy())
    inputs = [edges, arr, signed]
    if width == 32:
        inputs.append(torch.tensor(edges, dtype=torch.int64))   # a wider tensor holding the values
    for v in inputs:
        t = fn(v, "cpu")
        assert t.dtype == dt and t.is_contiguous() and t.device.type == "cpu"
        assert _bits(t, width) == edges
        assert np.array_equal(t.numpy().view(udt), arr)
    assert fn(arr[::2], "cpu").is_contiguous() and _bits(fn(arr[::2], "cpu"), width) == edges[::2]
    assert fn(signed[::2], "cpu").is_contiguous() and _bits(fn(signed[::2], "cpu"), width) == edges[::2]
    assert fn([], "cpu").numel() == 0 and fn([], "cpu").dtype == dt


def test_i32_keeps_negative_values():
    assert _dev.i32([-3, 7], "cpu").tolist() == [-3, 7]
    assert _dev.i32(np.asarray([-1, -(1 << 31)], np.int32), "cpu").tolist() == [-1, -(1 << 31)]


def test_wide_readback_ptr():
    assert _dev.wide([0xFFFFFFFF, 0xFFFFFFFF], 0) == (1 << 64) - 1
    assert _dev.wide([0, 1], 0) == 1 << 32
    assert _dev.wide(np.asarray([9, 0xFFFFFFFF, 0, 5, 1], np.uint32), 1) == 0xFFFFFFFF
    assert _dev.wide(np.asarray([9, 0xFFFFFFFF, 0, 5, 1], np.uint32), 3) == (1 << 32) + 5
    back = _dev.readback(torch.tensor([-1, 0, -(1 << 31)], dtype=torch.int32))
    assert back.dtype == np.uint32 and back.tolist() == [0xFFFFFFFF, 0, 1 << 31]
    assert _dev.ptr(None) is None
    assert _dev.ptr(torch.zeros(0, dtype=torch.uint8)) is None
    assert _dev.ptr(torch.zeros(4, dtype=torch.uint8)[:0]) is None
    t = torch.zeros(4, dtype=torch.uint8)
    assert _dev.ptr(t) == t.data_ptr() != 0
    assert batch._ptr is _dev.ptr and callable(batch._stream)


def test_on_stream_takes_the_stream_by_position_or_keyword(monkeypatch):
    entered = []

    class Ctx:
        def __init__(self, s):
            self.s = s

        def __enter__(self):
            entered.append(self.s)

        def __exit__(self, *a):
            entered.append(None)
            return False

    monkeypatch.setattr(torch.cuda, "stream", Ctx)

    @_dev.on_stream
    def f(a, b=2, stream=None, c=4):
        """doc"""
        return a, b, stream, c, len(entered)

    assert f(1) == (1, 2, None, 4, 0) and entered == []
    assert f(1, stream="s", c=5) == (1, 2, None, 5, 1) and entered == ["s", None]
    assert f(1, 3, "t", 6) == (1, 3, None, 6, 3) and entered == ["s", None, "t", None]
    assert f(1, 3, None, 6) == (1, 3, None, 6, 4)
    assert f.__doc__ == "doc" and list(inspect.signature(f).parameters) == ["a", "b", "stream", "c"]


def test_public_signatures_keep_stream():
    from gobeansdb_amd import gc, hint, record, replay
    for fn in (batch.decompress, batch.compress, batch.go_l1_compress, batch.go_decompress, batch.crc32, batch.synth,
               replay.index, replay.replay, replay.read_records, record.encode, record.encode_batch, gc.rewrite,
               gc.rewrite_batch, hint.keyhash, hint.build_split, hint.build, hint.merge_packed, hint.merge,
               hint.lookup_packed, hint.lookup):
        assert inspect.signature(fn).parameters["stream"].default is None, fn.__name__
    assert replay.HDR == record.HDR == gc.HDR == 24 and replay.FLAG_COMPRESS == record.FLAG_COMPRESS
    assert (replay.MAX_KEY_LEN, replay.BODY_MAX) == (record.MAX_KEY_LEN, record.BODY_MAX) == (250, 50 << 20)
