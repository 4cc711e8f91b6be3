"""The workspace contract of the batch C ABI (include/qlzx.h), made checkable: a proxy around the
loaded library that hands every entry point a workspace of EXACTLY the byte count its caller
passed, at the weakest base alignment the header allows, between two guards, and filled with a
poison first.

What the header promises and this checks:
  - the byte count the matching *_workspace_size() returns is enough: a store before the base or
    past workspace_bytes lands in a guard and is reported with the entry point and the offset;
  - nothing needs a value on entry and no state travels in the workspace between calls: every call
    gets a freshly poisoned one, so a counter, a status or a list slot that is read before it is
    written shows in the results the tests compare anyway.

A test installs the proxy with monkeypatch on gobeansdb_amd._lib._lib: _lib.lib() returns that
global, so the Python drivers and the tests' raw L.qlzx_* calls both go through it.  The proxy
synchronises the device around every intercepted call (it compares the guards after it), so it
says nothing about calls in flight together: tests of that use an ordinary workspace.

fill() / first_touched() know nothing of the device: tests/test_ws_contract.py runs them on CPU
tensors."""
from __future__ import annotations

import functools
from collections import Counter

import torch

# every function of include/qlzx.h whose last three parameters are (workspace, workspace_bytes, stream)
ENTRY_POINTS = (
    "qlzx_decompress_batch", "qlzx_compress_batch", "qlzx_go_l1_compress_batch", "qlzx_go_decompress_batch",
    "qlzx_replay_index", "qlzx_replay_plan", "qlzx_read_plan",
    "qlzx_write_plan", "qlzx_write_decide", "qlzx_write_finish",
    "qlzx_gc_plan", "qlzx_gc_rewrite",
    "qlzx_hint_plan", "qlzx_hint_write", "qlzx_hint_merge_plan", "qlzx_hint_merge_write", "qlzx_hint_lookup",
)

GUARD_BYTES = 64 << 10
GUARD_FILL = 0xC3          # differs from every poison below and from the tests' own fills (0xAA, 0xA5, 0x5C)
BASE_ALIGN = 16            # the alignment qlzx.h asks of `workspace`, and no stricter: base % 256 == 16
_SLACK = 256 + BASE_ALIGN  # room to put the base at 256 k + BASE_ALIGN whatever the allocation's address

# name -> fill byte, or None for seeded random bytes.  0xFF makes every counter huge and every
# status -1 (kPending); 0x5A is a plausible small positive in every byte lane.
POISONS = {"ff": 0xFF, "5a": 0x5A, "random": None}
RANDOM_SEED = 0x51A7


class GuardTouched(AssertionError):
    """A byte outside [base, base + workspace_bytes) changed.  offset is relative to the base:
    negative in the guard before it, >= workspace_bytes in the guard behind it."""

    def __init__(self, name: str, offset: int, workspace_bytes: int):
        self.name, self.offset, self.workspace_bytes = name, offset, workspace_bytes
        where = "before the base" if offset < 0 else "past workspace_bytes"
        super().__init__(f"{name}: byte at workspace offset {offset} ({where}; workspace_bytes = {workspace_bytes}) "
                         "was written")


def buffer_bytes(workspace_bytes: int) -> int:
    """Bytes to allocate for guard + workspace + guard at any address."""
    return _SLACK + 2 * GUARD_BYTES + workspace_bytes


def base_offset(address: int) -> int:
    """Offset of the workspace base in a buffer that starts at `address`: a whole guard before it,
    and the base at 256 k + BASE_ALIGN."""
    return GUARD_BYTES + (BASE_ALIGN - (address + GUARD_BYTES)) % 256


def _views(buf: torch.Tensor, base: int, workspace_bytes: int):
    return (buf[base - GUARD_BYTES:base], buf[base:base + workspace_bytes],
            buf[base + workspace_bytes:base + workspace_bytes + GUARD_BYTES])


def fill(buf: torch.Tensor, base: int, workspace_bytes: int, poison: str) -> None:
    """Guards to GUARD_FILL, the workspace to the poison."""
    assert base >= GUARD_BYTES and base + workspace_bytes + GUARD_BYTES <= buf.numel()
    front, ws, back = _views(buf, base, workspace_bytes)
    front.fill_(GUARD_FILL)
    back.fill_(GUARD_FILL)
    value = POISONS[poison]
    if value is not None:
        ws.fill_(value)
    elif workspace_bytes:
        ws.random_(0, 256, generator=torch.Generator(device=buf.device).manual_seed(RANDOM_SEED))


def first_touched(buf: torch.Tensor, base: int, workspace_bytes: int):
    """The workspace offset of the first guard byte that is no longer GUARD_FILL, or None."""
    front, _, back = _views(buf, base, workspace_bytes)
    for guard, at in ((front, -GUARD_BYTES), (back, workspace_bytes)):
        bad = guard != GUARD_FILL
        if bool(bad.any()):
            return at + int(bad.nonzero()[0])
    return None


def check(name: str, buf: torch.Tensor, base: int, workspace_bytes: int) -> None:
    off = first_touched(buf, base, workspace_bytes)
    if off is not None:
        raise GuardTouched(name, off, workspace_bytes)


class Proxy:
    """Stands in for the ctypes library object.  The ENTRY_POINTS, called with a non-null
    workspace, get a guarded and poisoned one of the caller's own workspace_bytes; everything else
    (a null workspace, the size functions, the single-call symbols) is forwarded untouched."""

    def __init__(self, real, poison: str, device="cuda"):
        assert poison in POISONS
        self._real, self._poison, self._device = real, poison, device
        self.calls = Counter()      # intercepted calls per entry point (non-null workspace only)
        self.bytes = Counter()      # workspace bytes poisoned per entry point, summed over its calls
        self.largest = Counter()    # the largest single workspace per entry point

    def __getattr__(self, name):
        f = getattr(self._real, name)
        return functools.partial(self._call, name, f) if name in ENTRY_POINTS else f

    def _call(self, name, f, *args):
        ws, nbytes = args[-3], args[-2]
        ws = getattr(ws, "value", ws)
        if not ws:
            return f(*args)
        nbytes = int(getattr(nbytes, "value", nbytes))
        buf = torch.empty(buffer_bytes(nbytes), dtype=torch.uint8, device=self._device)
        base = base_offset(buf.data_ptr())
        assert (buf.data_ptr() + base) % 256 == BASE_ALIGN
        fill(buf, base, nbytes, self._poison)
        torch.cuda.synchronize()    # the call may run on any stream
        self.calls[name] += 1
        self.bytes[name] += nbytes
        self.largest[name] = max(self.largest[name], nbytes)
        rc = f(*args[:-3], buf.data_ptr() + base, nbytes, args[-1])   # never a larger size than the caller's
        torch.cuda.synchronize()
        check(name, buf, base, nbytes)
        return rc

    def require(self, names) -> None:
        """The census of one test: each of `names` was intercepted with a non-null workspace."""
        missing = [n for n in names if not self.calls[n]]
        assert not missing, ("never reached with a workspace", missing, dict(self.calls))
