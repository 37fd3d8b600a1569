"""What a test of one C-ABI entry needs: the loaded library, pointers and small ctypes arrays, and the guarded output buffer that says
"this kernel wrote nothing outside its output".  Test infrastructure; tests/test_parity_harness.py holds the guard to its word on the CPU."""
from __future__ import annotations

import ctypes
import functools

import torch

NAN, INF = float("nan"), float("inf")
CAR_E_ARG = -1
P_ = ctypes.c_void_p
F32, F64 = torch.float32, torch.float64
MARGIN = 256                  # elements in front of and behind every guarded buffer: keeps the 16- and 256-byte alignment of 4-byte elements
SENTINEL = -0x5a5a5a5b        # what guards an integer buffer


@functools.lru_cache(maxsize=None)
def lib():
    from cross_attention_renderer_amd import _lib as L
    return L.load()


def dev():
    return torch.device("cuda:0")


def ptr(t):
    return None if t is None else P_(t.data_ptr())


def stream():
    return P_(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def ptrs(ts):
    return (P_ * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def up4(n):
    return (n + 3) & ~3


class Guarded:
    """A tensor of `shape` whose rows (the last dimension, `cols` wide) lie `ld >= cols` elements apart, `offset` elements behind the
    front margin, inside a buffer that holds the guard value — NaN, or SENTINEL for an integer dtype — everywhere: in both margins, in
    the offset gap, in the row padding and, unless `fill` or `init` says otherwise, in the payload itself.

    view    the rows on the device, [..., ld]
    ptr     where they start
    get()   the [..., cols] payload on the host, after checking that nothing around it was written"""

    def __init__(self, shape, ld=None, offset=0, dtype=torch.float32, fill=None, init=None, device=None):
        self.shape = tuple(shape)
        self.cols = self.shape[-1]
        self.ld = ld or self.cols
        self.rows = 1
        for d in self.shape[:-1]:
            self.rows *= d
        assert self.ld >= self.cols and offset >= 0
        self.guard = NAN if dtype.is_floating_point else SENTINEL
        self.front, n = MARGIN + offset, self.rows * self.ld
        self.full = torch.full((self.front + n + MARGIN,), self.guard, dtype=dtype, device=dev() if device is None else device)
        self.view = self.full[self.front:self.front + n].view(*self.shape[:-1], self.ld)
        if fill is not None:
            self.view[..., :self.cols] = fill
        if init is not None:
            self.view[..., :self.cols] = init.reshape(self.shape).to(self.full.device)

    @property
    def ptr(self):
        return P_(self.view.data_ptr())

    def _is_guard(self, t):
        return torch.isnan(t) if self.guard != self.guard else t == self.guard

    def untouched(self):
        """The whole buffer, payload included, still holds the guard value."""
        return bool(self._is_guard(self.full).all())

    def margins_untouched(self):
        """Both margins and the offset gap still hold the guard value."""
        return bool(self._is_guard(self.full[:self.front]).all()) and bool(self._is_guard(self.full[self.front + self.rows * self.ld:]).all())

    def get(self, what=""):
        f = self.full.cpu()
        end = self.front + self.rows * self.ld
        assert bool(self._is_guard(f[:self.front]).all()), f"{what}: wrote in front of the buffer"
        assert bool(self._is_guard(f[end:]).all()), f"{what}: wrote behind the buffer"
        v = f[self.front:end].view(self.rows, self.ld)
        assert bool(self._is_guard(v[:, self.cols:]).all()), f"{what}: wrote into the row padding"
        return v[:, :self.cols].reshape(self.shape).clone()


def exact_then_twice(nbytes, run, what, same=True):
    """An entry's size entry and its launcher agree: `run(work, work_bytes)` — one call of the entry over the Guarded `work`, returning its
    outputs as host tensors — over a NaN-filled guarded workspace of exactly `nbytes`, then over one twice as large.  Nothing is written outside either
    workspace, and the outputs of the two calls are the same bytes (same=False: for an entry whose two runs need not be, `run` judges each
    call itself).  Returns the first call's outputs."""
    assert nbytes > 0 and nbytes % 4 == 0, (what, nbytes, lib().car_last_error())
    outs = []
    for scale in (1, 2):
        work = Guarded((scale * nbytes // 4,))
        assert work.view.data_ptr() % 16 == 0
        outs.append(tuple(run(work, scale * nbytes)))
        torch.cuda.synchronize()
        assert work.margins_untouched(), f"{what}: wrote outside a workspace of {scale} x {nbytes} bytes"
    assert len(outs[0]) == len(outs[1]) > 0
    for i, (a, b) in enumerate(zip(*outs) if same else ()):
        a, b = torch.as_tensor(a), torch.as_tensor(b)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).clone().view(torch.uint8), b.reshape(-1).clone().view(torch.uint8)), \
            f"{what}: output {i} differs between the exact workspace and the larger one"
    return outs[0]


def rows_out(rows, ld, offset=0, device=None):
    """`rows` rows at a stride of ld floats and a guard row behind them, all NaN."""
    return Guarded((rows + 1, ld), offset=offset, device=device)


def take_rows(out, rows, width, what):
    """The rows' windows; everything else of the buffer must still be NaN."""
    got = out.view[:rows, :width].clone()
    out.view[:rows, :width] = NAN
    assert out.untouched(), f"{what}: wrote outside the rows' windows (padding columns, the guard row or the margins)"
    return got.cpu()
