"""Poisoned, guard-banded allocations for the device entries' workspaces and outputs.

Every HIP entry of the package writes into memory the Python side takes from ``torch.empty`` (or ``empty_like`` /
``new_empty`` / ``empty_strided``).  What such a buffer holds is whatever the caching allocator hands back, so a kernel
that reads a workspace word it has not written, leaves an output element unwritten, or writes past its region can pass
every parity test by luck.  Inside ``poisoned_allocations(pattern)`` every ``empty``-family request is served from a flat
``uint8`` block filled with ``pattern`` and framed by ``guard`` bytes of it on both sides; ``check_guards()`` (run again
when the context is left) reports any guard byte that changed, with the call site that allocated the block.

    0x00  what a fresh segment of the caching allocator most likely holds
    0xFF  NaN in fp64 and fp32, -1 in the integer types, 255 / True in uint8 / bool
    0x7F  a huge finite value: 1.4e306 in fp64, 3.4e38 in fp32, 0x7F7F7F7F in int32

``torch.zeros``, ``torch.full`` and the other constructors with a defined content are left alone.  A helper module,
not a conftest: only the tests that import it are affected.
"""
import contextlib
import os
import sys

import numpy as np
import torch

PATTERNS = (0x00, 0xFF, 0x7F)

_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep
_THIS = os.path.abspath(__file__)


def _call_site():
    """First stack frame outside torch and outside this module: the line that asked for the buffer."""
    f = sys._getframe(2)
    while f is not None:
        fn = os.path.abspath(f.f_code.co_filename)
        if fn != _THIS and not fn.startswith(_TORCH_DIR):
            return f"{fn}:{f.f_lineno} ({f.f_code.co_name})"
        f = f.f_back
    return "<unknown>"


def _size(args, kw):
    if "size" in kw:
        s = kw["size"]
    elif len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        s = args[0]
    else:
        s = args
    return tuple(int(v) for v in s)


class _Block:
    __slots__ = ("base", "nbytes", "guard", "site", "shape", "dtype")

    def __init__(self, base, nbytes, guard, site, shape, dtype):
        self.base, self.nbytes, self.guard, self.site, self.shape, self.dtype = base, nbytes, guard, site, shape, dtype


class PoisonedAllocations:
    """State of one ``poisoned_allocations`` context: the live guard-banded blocks, in allocation order."""

    def __init__(self, pattern, guard, devices=("cuda",)):
        if not 0 <= int(pattern) <= 255:
            raise ValueError("pattern is one byte")
        if guard <= 0 or guard % 256:
            raise ValueError("guard must be a positive multiple of 256 bytes (vector loads stay aligned)")
        self.pattern, self.guard, self.devices = int(pattern), int(guard), tuple(devices)
        self.blocks = []
        self._orig = {}

    # --- allocation -------------------------------------------------------------------------------------------
    def _fill(self, t):
        if t.numel() > 0:
            raw = self._orig["empty"](0, dtype=torch.uint8, device=t.device)
            raw.set_(t.untyped_storage())
            raw.fill_(self.pattern)
        return t

    def _guarded(self, shape, dtype, device, requires_grad=False):
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        device = torch.device(device) if device is not None else self._orig["empty"](0).device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        numel = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        nbytes = numel * self._orig["empty"](0, dtype=dtype).element_size()
        if device.type not in self.devices or nbytes == 0:
            return None
        g = self.guard
        base = self._orig["empty"](nbytes + 2 * g, dtype=torch.uint8, device=device)
        base.fill_(self.pattern)
        view = base[g:g + nbytes].view(dtype).view(shape)
        self.blocks.append(_Block(base, nbytes, g, _call_site(), tuple(shape), dtype))
        if requires_grad:
            view.requires_grad_(True)
        return view

    @staticmethod
    def _plain(kw, allowed):
        """Only the keywords a guarded block can honour; anything else (out=, pin_memory, a non-default layout or memory
        format) takes the unguarded path."""
        for k, v in kw.items():
            if k in allowed:
                continue
            if k == "layout" and v in (None, torch.strided):
                continue
            if k == "memory_format" and v in (None, torch.contiguous_format, torch.preserve_format):
                continue
            if k == "pin_memory" and not v:
                continue
            return False
        return True

    def empty(self, *args, **kw):
        if self._plain(kw, ("size", "dtype", "device", "requires_grad")):
            t = self._guarded(_size(args, kw), kw.get("dtype"), kw.get("device"), kw.get("requires_grad", False))
            if t is not None:
                return t
        return self._fill(self._orig["empty"](*args, **kw))

    def empty_like(self, input, *args, **kw):
        if not args and input.is_contiguous() and self._plain(kw, ("dtype", "device", "requires_grad")):
            t = self._guarded(tuple(input.shape), kw.get("dtype") or input.dtype, kw.get("device") or input.device,
                              kw.get("requires_grad", False))
            if t is not None:
                return t
        return self._fill(self._orig["empty_like"](input, *args, **kw))

    def new_empty(self, src, *args, **kw):
        if self._plain(kw, ("size", "dtype", "device", "requires_grad")):
            t = self._guarded(_size(args, kw), kw.get("dtype") or src.dtype, kw.get("device") or src.device,
                              kw.get("requires_grad", False))
            if t is not None:
                return t
        return self._fill(self._orig["new_empty"](src, *args, **kw))

    def empty_strided(self, size, stride, *args, **kw):
        size, stride = tuple(int(v) for v in size), tuple(int(v) for v in stride)
        contiguous, acc = True, 1
        for n, s in zip(reversed(size), reversed(stride)):
            if n != 1 and s != acc:
                contiguous = False
            acc *= n
        if not args and contiguous and self._plain(kw, ("dtype", "device", "requires_grad")):
            t = self._guarded(size, kw.get("dtype"), kw.get("device"), kw.get("requires_grad", False))
            if t is not None:
                return t
        return self._fill(self._orig["empty_strided"](size, stride, *args, **kw))

    # --- checking ---------------------------------------------------------------------------------------------
    def check_guards(self):
        """Synchronises, then asserts that every guard byte of every live block still holds the pattern."""
        if not self.blocks:
            return
        if any(b.base.is_cuda for b in self.blocks):
            torch.cuda.synchronize()
        g = self.guard
        by_dev = {}
        for i, b in enumerate(self.blocks):
            by_dev.setdefault(b.base.device, []).append(i)
        for dev, idx in by_dev.items():
            bands = torch.stack([torch.cat([self.blocks[i].base[:g], self.blocks[i].base[g + self.blocks[i].nbytes:]])
                                 for i in idx])
            bad = (bands != self.pattern).any(1).cpu().numpy()
            if not bad.any():
                continue
            msgs = []
            for k in np.nonzero(bad)[0]:
                b = self.blocks[idx[k]]
                band = bands[k].cpu().numpy()
                first = int(np.nonzero(band != self.pattern)[0][0])
                off = first - g if first < g else b.nbytes + (first - g)      # relative to the start of the buffer
                side = "before" if first < g else "after"
                msgs.append(f"{b.site}: {b.nbytes}-byte buffer {b.shape} {b.dtype}: guard byte {side} it changed, "
                            f"first at offset {off} (0x{int(band[first]):02x}, pattern 0x{self.pattern:02x})")
            raise AssertionError("guard band corrupted:\n  " + "\n  ".join(msgs))

    def release(self):
        self.blocks = []


@contextlib.contextmanager
def poisoned_allocations(pattern, guard=4096, devices=("cuda",)):
    """Serves every ``empty``-family request on one of ``devices`` (device types) from a pattern-filled, guard-banded
    block (see the module docstring); requests elsewhere are only filled with the pattern.  Yields the state
    (``.check_guards()``, ``.blocks``).  Leaving the context normally checks the guards; the blocks stay alive until then,
    so asynchronous launches never see their buffers recycled."""
    st = PoisonedAllocations(pattern, guard, devices)
    st._orig = {"empty": torch.empty, "empty_like": torch.empty_like, "new_empty": torch.Tensor.new_empty,
                "empty_strided": torch.empty_strided}
    torch.empty, torch.empty_like, torch.empty_strided = st.empty, st.empty_like, st.empty_strided
    torch.Tensor.new_empty = lambda self, *a, **k: st.new_empty(self, *a, **k)
    ok = False
    try:
        yield st
        ok = True
    finally:
        torch.empty, torch.empty_like, torch.empty_strided = (st._orig["empty"], st._orig["empty_like"],
                                                              st._orig["empty_strided"])
        torch.Tensor.new_empty = st._orig["new_empty"]
        try:
            if ok:
                st.check_guards()
        finally:
            st.release()


def equals_pattern(a, pattern):
    """Boolean mask of the elements of numpy array ``a`` whose every byte is ``pattern``."""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return np.zeros(a.shape, bool)
    b = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)) if a.ndim else a.reshape(1).view(np.uint8)
    return (b == pattern).all(-1)
