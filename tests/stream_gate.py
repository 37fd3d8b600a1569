"""The stream contract's instrument ("All work is enqueued asynchronously on `stream` ... No call synchronises the device", include/car_hip.h):
a bounded device-side delay — the gate — on a side stream, behind which a step's real inputs, the poison of its outputs and the call itself
are enqueued.  A launch, memset or copy that the call issues on any OTHER stream does not wait for the gate: it runs early, reads the decoy the
input buffers still hold and has its writes overwritten by the poison, so the step's result differs from the eager one on the real inputs.
Test infrastructure; tests/test_stream_gate.py holds it to its word (a stray launch is seen, a correct one passes).

The order on the side stream `s` (run_gated):
    gate | event | real inputs -> the buffers (device to device) | poison of every output and workspace | the call | clones of the outputs
and the step is CONCLUSIVE only if the event behind the gate has not happened when the host has finished enqueuing all of it.  The gate is
`torch.cuda._sleep` (a kernel that counts device clock cycles and ends on its own), or a fixed chain of matmuls; never a kernel that waits for
the host.  Every gate is capped (CAP_MS): nothing here can hang.
"""
from __future__ import annotations

import contextlib
import ctypes
import json
import os
import time
from typing import Callable, List, Optional, Sequence

import torch

import abi_harness as A

MARGIN_FACTOR = 8            # the project's margin: a gate lasts 8 x the wall time the warm call took ungated
FLOOR_MS = 4.0               # ... and at least this (a call of a few microseconds still needs a gate the host cannot outlast by jitter)
CAP_MS = 400.0               # the hard upper length of any gate, the four-fold retry included
RETRY = 4                    # an inconclusive step is repeated once with a gate this many times as long
KINDS = ("sleep", "matmul")

_cal = {}                    # kind -> units per millisecond (clock cycles of _sleep, matmuls of the chain)
_kind = "sleep"              # what gate() enqueues; instrument()'s must-see checks may move it to the chain
LOG: List[dict] = []         # one record per gated step, for profiles/stream_order.md (tools print it; nothing reads it back)


class Inconclusive(AssertionError):
    """The gate had ended before the host finished enqueuing the step, twice: the step showed nothing, and that is a failure."""


def use(kind: str) -> None:
    global _kind
    assert kind in KINDS
    _kind = kind


def kind() -> str:
    return _kind


def _chain_operands():
    if "ops" not in _cal:
        g = torch.Generator().manual_seed(0)
        _cal["ops"] = (torch.randn(512, 512, generator=g).to(A.dev()) / 512 ** 0.5, torch.empty(512, 512, device=A.dev()))
    return _cal["ops"]


def _enqueue(kind_: str, units: int) -> None:
    """`units` of delay on the current stream."""
    if kind_ == "sleep":
        torch.cuda._sleep(int(units))
    else:
        a, out = _chain_operands()
        for _ in range(int(units)):
            torch.mm(a, a, out=out)


def units_per_ms(kind_: Optional[str] = None) -> float:
    """Calibrated once per process on the default stream: how many clock cycles (or matmuls) one millisecond of gate takes."""
    kind_ = kind_ or _kind
    if kind_ not in _cal:
        probe = 2_000_000 if kind_ == "sleep" else 64
        _enqueue(kind_, probe)                                  # warm: the first matmul loads its kernel
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _enqueue(kind_, probe)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.0, f"the {kind_} gate took no time: it does not delay this device"
        _cal[kind_] = probe / ms
    return _cal[kind_]


def log(rec: dict) -> None:
    LOG.append(rec)
    if os.environ.get("CAR_STREAM_LOG"):                         # how profiles/stream_order.md is made: one JSON line per gated step
        with open(os.environ["CAR_STREAM_LOG"], "a") as f:
            f.write(json.dumps(rec) + "\n")


def gate_ms_for(ungated_ms: float) -> float:
    """The gate's length for a step whose warm, ungated run took `ungated_ms` of wall time."""
    return min(max(MARGIN_FACTOR * ungated_ms, FLOOR_MS), CAP_MS / RETRY)


def gate(stream: torch.cuda.Stream, ms: float) -> torch.cuda.Event:
    """Enqueues a gate of `ms` milliseconds (capped) on `stream` and returns the event recorded behind it."""
    ms = min(ms, CAP_MS)
    units = max(1, int(ms * units_per_ms()))
    with torch.cuda.stream(stream):
        _enqueue(_kind, units)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def gated(stream: torch.cuda.Stream, ungated_ms: float, step: Callable[[], object], what: str, reset: Callable[[], None] = lambda: None):
    """`step()` — host code that only enqueues — behind a gate on `stream`; (step's value, the record).  Conclusive or Inconclusive:
    the gate's event must still be pending when step() has returned; if not, once more behind a gate four times as long (`reset()` first)."""
    ms = gate_ms_for(ungated_ms)
    for attempt in (0, 1):
        torch.cuda.synchronize()
        ev = gate(stream, ms)
        value = step()
        conclusive = not ev.query()
        stream.synchronize()
        torch.cuda.synchronize()
        rec = dict(what=what, kind=_kind, ungated_ms=round(ungated_ms, 3), gate_ms=round(min(ms, CAP_MS), 3), attempt=attempt, conclusive=conclusive)
        log(rec)
        if conclusive:
            return value, rec
        ms *= RETRY
        reset()
    raise Inconclusive(f"{what}: the gate ({rec['gate_ms']} ms of {_kind}) had ended before the host finished enqueuing the step — inconclusive, "
                       "which is not a pass")


# ---- one C-ABI call as a case --------------------------------------------------------------------------------------------------------------------
class Built:
    """The buffers of one call, made on the default stream, and the call itself.

    inp(real, decoy)   a float input: the device buffer the call reads (it holds the DECOY until a run copies the real values in)
    idx(t)             an index-like input (sample tables, index lists, records, flags): never decoyed
    out(shape, ...)    a guarded output, poisoned with NaN / SENTINEL before every run
    work(nbytes, zero) a guarded workspace, poisoned with NaN — or with zeros where it holds counters or indices
    call               call(stream_pointer): enqueues the entry (or the entries of the row); raises on a negative status"""

    def __init__(self):
        self.inputs, self.outputs, self.works, self.keep = [], [], [], []
        self.extra_poison, self.extra_out = [], []                  # (tensor, value) poisoned, and plain tensors cloned, beside the guarded ones
        self.call: Callable[[ctypes.c_void_p], None] = None
        self.bound: Optional[Callable[[Sequence[torch.Tensor], Sequence[torch.Tensor]], None]] = None   # None: bit-identical
        self.loose: Sequence[int] = ()                                                                       # outputs exempt from "the decoy matters"

    def inp(self, real: torch.Tensor, decoy: torch.Tensor) -> torch.Tensor:
        assert real.shape == decoy.shape and real.dtype == decoy.dtype and (real.dtype.is_floating_point or real.dtype == torch.uint8), \
            "only float data and uint8 images have a decoy; index-like inputs go through idx()"
        assert bool((torch.isfinite(decoy) | ~torch.isfinite(real)).all()), "a decoy is a valid input, never NaN (but where the real input holds padding)"
        real, decoy = real.to(A.dev()).contiguous(), decoy.to(A.dev()).contiguous()
        buf = decoy.clone()
        self.inputs.append((buf, real, decoy))
        return buf

    def inout(self, real: torch.Tensor, decoy: torch.Tensor) -> torch.Tensor:
        """An input the call overwrites in place with a result: loaded like an input, cloned like an output."""
        buf = self.inp(real, decoy)
        self.extra_out.append(buf)
        return buf

    def idx(self, t: torch.Tensor) -> torch.Tensor:
        t = t.to(A.dev()).contiguous()
        self.keep.append(t)
        return t

    def keep_host(self, obj):
        """A host array the call reads (flags, sizes, pointer tables): kept alive with the case, never decoyed."""
        self.keep.append(obj)
        return obj

    def out(self, shape, dtype=torch.float32, zero: bool = False, **kw) -> A.Guarded:
        """zero: an output the entry ADDS into and its caller zeroes first — its poison is that zero (margins and padding: the guard)."""
        g = A.Guarded(shape, dtype=dtype, **kw)
        g.zero = zero
        self.outputs.append(g)
        return g

    def out_bytes(self, n: int, fill: int = 0x5a) -> "Bytes":
        g = Bytes(n, fill)
        self.outputs.append(g)
        return g

    def work(self, nbytes: int, zero: bool = False) -> A.Guarded:
        assert nbytes > 0 and nbytes % 4 == 0, nbytes
        g = A.Guarded((nbytes // 4,))
        self.works.append((g, zero))
        return g

    # the three steps every run enqueues on the current stream
    def load(self, which: str) -> None:
        for buf, real, decoy in self.inputs:
            buf.copy_(real if which == "real" else decoy)

    def poison(self) -> None:
        for g in self.outputs:
            g.full.fill_(g.guard)
            if getattr(g, "zero", False):
                g.view[..., :g.cols] = 0
        for t, value in self.extra_poison:
            t.fill_(value)
        for g, zero in self.works:
            g.full.fill_(g.guard)
            if zero:
                g.view.zero_()

    def clones(self) -> List[torch.Tensor]:
        return [g.view[..., :g.cols].clone() for g in self.outputs] + [t.clone() for t in self.extra_out]

    def margins_untouched(self) -> bool:
        return all(g.margins_untouched() for g in self.outputs) and all(g.margins_untouched() for g, _ in self.works)


class Bytes:
    """A uint8 output (abi_harness.Guarded's sentinel needs four bytes): `n` bytes between two margins, everything poisoned with `fill`."""

    def __init__(self, n: int, fill: int):
        self.guard, self.cols, self.n = fill, n, n
        self.full = torch.full((2 * A.MARGIN + n,), fill, dtype=torch.uint8, device=A.dev())
        self.view = self.full[A.MARGIN:A.MARGIN + n]

    @property
    def ptr(self):
        return A.P_(self.view.data_ptr())

    def margins_untouched(self) -> bool:
        return bool((self.full[:A.MARGIN] == self.guard).all()) and bool((self.full[A.MARGIN + self.n:] == self.guard).all())


def stream_ptr(stream: Optional[torch.cuda.Stream]) -> ctypes.c_void_p:
    return ctypes.c_void_p(None if stream is None else stream.cuda_stream)


def run_eager(b: Built, which: str = "real"):
    """The reference: the call on the default stream with the `which` inputs, everything ready.  (outputs on the host, wall milliseconds)"""
    b.load(which)
    b.poison()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b.call(A.stream())
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    outs = [t.cpu() for t in b.clones()]
    assert b.margins_untouched(), "the eager run wrote outside a guarded buffer"
    return outs, ms


def run_gated(b: Built, stream: torch.cuda.Stream, ungated_ms: float, what: str, hand: object = "same", poison: bool = True):
    """The call behind a gate on `stream`: the buffers hold the decoy; behind the gate come the real inputs, the poison, the call and the
    clones.  `hand`: the stream the call is GIVEN — "same" (the contract), None (the null stream) or another stream (both only for showing
    that the instrument sees a stray launch).  (outputs on the host, the record)"""
    given = stream if isinstance(hand, str) else hand

    def reset():
        b.load("decoy")
        torch.cuda.synchronize()

    def step():
        with torch.cuda.stream(stream):
            b.load("real")
            if poison:
                b.poison()
            b.call(stream_ptr(given))
            return b.clones()

    reset()
    outs, rec = gated(stream, ungated_ms, step, what, reset)
    return [t.cpu() for t in outs], rec


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


def differing_fraction(a: torch.Tensor, b: torch.Tensor) -> float:
    """The share of entries whose BITS differ (NaN against NaN of the same bits is no difference)."""
    if a.numel() == 0:
        return 0.0
    w = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return float((a.reshape(-1).contiguous().view(w) != b.reshape(-1).contiguous().view(w)).float().mean())


def decoy_matters(real: Sequence[torch.Tensor], decoy: Sequence[torch.Tensor], loose: Sequence[int] = ()) -> None:
    """The condition on every case: the eager result on the decoy differs from the one on the real inputs in more than half of the entries of
    every float output — a case cannot hide a stray launch behind inputs that do not matter.  The entries of an output are those the call
    wrote: what still holds the NaN poison after BOTH runs (the part of a shared table another packer owns, row padding) is nobody's output."""
    for i, (r, d) in enumerate(zip(real, decoy)):
        if r.dtype.is_floating_point and i not in loose:
            written = ~(torch.isnan(r) & torch.isnan(d))
            assert bool(written.any()), f"output {i}: nothing was written"
            f = differing_fraction(r[written], d[written])
            assert f > 0.5, f"output {i}: the decoy changes only {f:.1%} of the {int(written.sum())} entries the call wrote"


def check_case(b: Built, stream: torch.cuda.Stream, what: str):
    """A row's three assertions — conclusive, the result, the margins — and the condition on its decoy.  Returns the record.  Whatever
    happens, the buffers hold the real inputs again afterwards (a row's inputs may be somebody else's tensors: a module's parameters)."""
    try:
        return _check_case(b, stream, what)
    finally:
        b.load("real")
        torch.cuda.synchronize()


def _check_case(b: Built, stream: torch.cuda.Stream, what: str):
    run_eager(b)                                                   # warm: module load, caches, the allocator
    want, ms = run_eager(b, "real")
    decoy, _ = run_eager(b, "decoy")
    decoy_matters(want, decoy, b.loose)
    got, rec = run_gated(b, stream, ms, what)                      # raises Inconclusive
    assert b.margins_untouched(), f"{what}: wrote outside a guarded buffer on the side stream"
    if b.bound is None:
        for i, (g, w) in enumerate(zip(got, want)):
            assert same_bits(g, w), (f"{what}: output {i} behind the gate differs from the eager one in {differing_fraction(g, w):.1%} of its entries "
                                     "— something the call enqueued did not wait for the stream it was given")
    else:
        b.bound(got, want)
    return rec


# ---- the package under a side stream: a spy on the checked handle --------------------------------------------------------------------------------
class Spy:
    """Records every C entry called through a handle, with the stream it was handed (its last argument, where the prototype ends in the
    stream).  install() puts a recording wrapper over each such function ON the handle object itself, so a handle somebody captured
    earlier (RenderEngine.lib, the training run's record, the loader's state) is spied on like a fresh `_lib.api()`."""

    def __init__(self, handle, signatures):
        self._handle, self._sig, self.calls, self._saved = handle, signatures, [], {}

    def _wrap(self, name, fn):
        def spied(*a):
            st = a[-1]
            self.calls.append((name, getattr(st, "value", st) or 0))
            return fn(*a)
        spied.__name__ = name
        return spied

    def install(self):
        for name, (res, args) in self._sig.items():
            if res is ctypes.c_int and args and args[-1] is ctypes.c_void_p:
                fn = getattr(self._handle, name)
                self._saved[name] = fn
                setattr(self._handle, name, self._wrap(name, fn))
        return self

    def remove(self):
        for name, fn in self._saved.items():
            setattr(self._handle, name, fn)
        self._saved = {}

    def strays(self, stream: torch.cuda.Stream):
        return [(n, hex(s)) for n, s in self.calls if s != stream.cuda_stream]

    def entries(self):
        return sorted({n for n, _ in self.calls})


@contextlib.contextmanager
def spied():
    """The package's checked handle under a Spy for the duration."""
    from cross_attention_renderer_amd import _lib as L
    spy = Spy(L.api(), all_signatures()).install()
    try:
        yield spy
    finally:
        spy.remove()


def all_signatures():
    from cross_attention_renderer_amd import _lib as L
    out = {}
    for n in dir(L):
        if n.endswith("SIGNATURES"):
            out.update(getattr(L, n))
    return out


def stream_entries():
    """Every entry whose prototype ends in the stream: an int status whose last parameter is the `void* stream`."""
    return sorted(n for n, (res, args) in all_signatures().items() if res is ctypes.c_int and args and args[-1] is ctypes.c_void_p
                  and n not in NOT_A_STREAM)


NOT_A_STREAM = ()            # an entry whose last void* is something else would be named here (there is none)


# ---- which entries an entry calls: read from the sources -------------------------------------------------------------------------------------------
def _strip_comments_and_strings(src: str) -> str:
    import re
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return re.sub(r'"(?:\\.|[^"\\])*"', '""', src)


def function_bodies(src: str) -> dict:
    """{identifier: body text} of every top-level definition of a translation unit (namespaces and extern "C" blocks are looked through):
    every identifier that is followed by `(` in a definition's header names its body — an over-approximation (attributes such as
    __launch_bounds__ name it too) that costs nothing, since only names that are called elsewhere are ever looked up."""
    import re
    src = _strip_comments_and_strings(src)
    bodies, depth, head_start, body_start, transparent, names = {}, 0, 0, 0, [], []
    for i, ch in enumerate(src):
        if ch == "{":
            if depth == len(transparent):
                head = src[head_start:i]
                if re.search(r'(\bnamespace\b[^;{}()]*|extern\s*""\s*)$', head):
                    transparent.append(depth)
                    depth += 1
                    head_start = i + 1
                    continue
                body_start, names = i, re.findall(r"\b([A-Za-z_]\w*)\s*\(", head)
            depth += 1
        elif ch == "}":
            depth -= 1
            if transparent and depth == transparent[-1]:
                transparent.pop()
                head_start = i + 1
            elif depth == len(transparent):
                for n in names:
                    bodies[n] = bodies.get(n, "") + src[body_start:i + 1]
                head_start = i + 1
        elif ch == ";" and depth == len(transparent):
            head_start = i + 1
    return bodies


def entry_calls(csrc_dir: str) -> dict:
    """{stream entry: the stream entries it reaches}, through static helpers and helpers of other units, read from csrc/*.hip and *.h."""
    import re
    bodies = {}
    for f in sorted(os.listdir(csrc_dir)):
        if f.endswith((".hip", ".h")):
            for n, body in function_bodies(open(os.path.join(csrc_dir, f)).read()).items():
                bodies[n] = bodies.get(n, "") + body
    entries = set(stream_entries())
    reach = {}
    for e in entries:
        seen, todo, found = {e}, [e], set()
        while todo:
            for callee in set(re.findall(r"\b([A-Za-z_]\w*)\s*\(", bodies.get(todo.pop(), ""))):
                if callee in entries and callee != e:
                    found.add(callee)
                if callee in bodies and callee not in seen:
                    seen.add(callee)
                    todo.append(callee)
        reach[e] = found
    return reach


ENQUEUES = r"hipLaunchKernelGGL|<<<|hipMemsetAsync|hipMemcpyAsync|CAR_LAUNCH_LDS"       # every way the library puts work on a stream


def launch_sites(csrc_dir: str) -> dict:
    """{stream entry: {function: the number of enqueue sites written in its body}} over the entry itself and the helpers it reaches WITHOUT
    passing through another entry (those are the other entry's).  Sites, as written in the source: a site inside a loop or a branch counts
    once.  The entry's own name is the key of the sites in its own body."""
    import re
    bodies = {}
    for f in sorted(os.listdir(csrc_dir)):
        if f.endswith((".hip", ".h")):
            src = open(os.path.join(csrc_dir, f)).read()
            src = re.sub(r"^[ \t]*#[ \t]*define(?:[^\n]*\\\n)*[^\n]*", " ", src, flags=re.M)        # a macro's own text is no site: its uses are
            for n, body in function_bodies(src).items():
                bodies[n] = bodies.get(n, "") + body
    entries = set(stream_entries())
    out = {}
    for e in entries:
        seen, todo, sites = {e}, [e], {}
        while todo:
            fn = todo.pop()
            body = bodies.get(fn, "")
            n = len(re.findall(ENQUEUES, body))
            if n:
                sites[fn] = n
            for callee in set(re.findall(r"\b([A-Za-z_]\w*)\s*\(", body)):
                if callee in bodies and callee not in seen and callee not in entries:
                    seen.add(callee)
                    todo.append(callee)
        out[e] = sites
    return out


# ---- the instrument held to its word, once per process: which gate sees a stray launch ----------------------------------------------------------------
def add_case() -> Built:
    """out = alpha a + beta b over [257, 131] rows at a stride of 136 (more than one block, odd sizes, padded rows): elementwise, floats only —
    a stray launch can read nothing it must not."""
    M, N, LD = 257, 131, 136
    g = torch.Generator().manual_seed(11)
    b = Built()
    a_, b_ = (b.inp(torch.randn(M, LD, generator=g), torch.randn(M, LD, generator=g)) for _ in range(2))
    out = b.out((M, N), ld=LD)
    lib = A.lib()

    def call(st):
        assert lib.car_add(out.ptr, LD, A.ptr(a_), LD, 0.75, A.ptr(b_), LD, -1.5, M, N, st) == 0, lib.car_last_error()
    b.call = call
    return b


def sees_strays(b: Built, s, other, ms: float) -> dict:
    """The two must-see checks under the current kind of gate: {hand: seen}.  car_add behind a gate on `s`, handed NULL or a second side
    stream: without the poison the stray launch's own output survives and is the eager result on the DECOY; with it the output is the poison.
    Either way it differs from the real one."""
    want, _ = run_eager(b, "real")
    decoy, _ = run_eager(b, "decoy")
    decoy_matters(want, decoy)
    seen = {}
    for name, hand in (("NULL", None), ("second side stream", other)):
        bare, _ = run_gated(b, s, ms, f"car_add handed the {name}, no poison", hand=hand, poison=False)
        full, _ = run_gated(b, s, ms, f"car_add handed the {name}", hand=hand)
        seen[name] = same_bits(bare[0], decoy[0]) and not same_bits(bare[0], want[0]) and bool(torch.isnan(full[0]).all())
    return seen


_instrument = {}


def instrument() -> dict:
    """Chooses, once per process, the gate under which both must-see checks see the stray launch: `_sleep`, else the matmul chain.  Every
    module that gates anything calls this first, whatever order the files run in; where neither gate sees it this raises — a blind instrument
    never lets a gated test pass quietly.  -> {"streams": (s, other), "case", "ms", "report"}"""
    if "error" in _instrument:
        raise AssertionError(_instrument["error"])
    if "got" not in _instrument:
        s, other = torch.cuda.Stream(), torch.cuda.Stream()
        b = add_case()
        run_eager(b)
        _, ms = run_eager(b)
        report = {}
        for k in KINDS:
            use(k)
            report[k] = sees_strays(b, s, other, ms)
            if all(report[k].values()):
                _instrument["got"] = dict(streams=(s, other), case=b, ms=ms, report=report)
                break
        else:
            use("sleep")
            _instrument["error"] = f"instrument blind on this runtime: a launch on another stream did not overtake the gate ({report})"
            raise AssertionError(_instrument["error"])
    return _instrument["got"]


# ---- which stream an enqueue site is handed: read from the source text ------------------------------------------------------------------------------
_STREAM_ARG = {"hipLaunchKernelGGL": 4, "CAR_LAUNCH_LDS": 5, "hipMemsetAsync": 3, "hipMemcpyAsync": 4}


def _split_args(text: str, start: int, open_: str, close: str):
    """The top-level, comma-separated arguments of the bracket that opens at text[start]."""
    depth, args, cur, i = 0, [], [], start
    while i < len(text):
        ch = text[i]
        if ch in "([{" or (open_ == "<<<" and text.startswith("<<<", i)):
            if open_ == "<<<" and text.startswith("<<<", i):
                i += 2
            depth += 1
            if depth > 1:
                cur.append(ch)
        elif ch in ")]}" or (close == ">>>" and depth == 1 and text.startswith(">>>", i)):
            depth -= 1
            if depth == 0:
                args.append("".join(cur).strip())
                return args
            cur.append(ch)
        elif ch == "," and depth == 1:
            args.append("".join(cur).strip())
            cur = []
        elif depth >= 1:
            cur.append(ch)
        i += 1
    return args


def streams_in(body: str) -> list:
    """The stream written at every enqueue site of `body`, in order, casts removed and a local `hipStream_t st = (hipStream_t)stream;`
    followed back to what it was made from: "stream" is the entry's own parameter, anything else is what the source says ("0", a name)."""
    import re

    def bare(x):
        x = re.sub(r"static_cast\s*<\s*hipStream_t\s*>\s*\((.*)\)$", r"\1", x.strip())
        return re.sub(r"^\(\s*hipStream_t\s*\)\s*", "", x).strip()
    alias = {m.group(1): bare(m.group(2)) for m in re.finditer(r"hipStream_t\s+(\w+)\s*=\s*([^;]+);", body)}
    found = []
    for m in re.finditer(r"\b(hipLaunchKernelGGL|CAR_LAUNCH_LDS|hipMemsetAsync|hipMemcpyAsync)\s*\(|<<<", body):
        if m.group(0) == "<<<":
            args, at = _split_args(body, m.start(), "<<<", ">>>"), 3
        else:
            args, at = _split_args(body, m.end() - 1, "(", ")"), _STREAM_ARG[m.group(1)]
        x = bare(args[at]) if at < len(args) else "?"
        found.append((m.start(), alias.get(x, x)))
    return [x for _, x in sorted(found)]


def site_streams(csrc_dir: str) -> dict:
    """{stream entry: streams_in(its own body)}."""
    import re
    out, entries = {}, set(stream_entries())
    for f in sorted(os.listdir(csrc_dir)):
        if f.endswith(".hip"):
            src = re.sub(r"^[ \t]*#[ \t]*define(?:[^\n]*\\\n)*[^\n]*", " ", open(os.path.join(csrc_dir, f)).read(), flags=re.M)
            for n, body in function_bodies(src).items():
                if n in entries:
                    out[n] = streams_in(body)
    return out
