"""The stream-order instrument (tests/stream_gate.py) held to its word, and one neighbouring promise of the same header paragraph.

CPU: the bookkeeping of a case (what is loaded, poisoned and cloned), the gate's sizing rule, the spy, and "car_last_error() returns a
thread-local message".  GPU: behind a gate on a side stream `s`, car_add handed the NULL stream or a second side stream instead of `s` MUST be
seen — it overtakes the gate, reads the decoy and is overwritten by the poison — and car_add handed `s` must pass, bit-identical and
conclusive.  A runtime on which the stray launch is not seen (streams that share one hardware queue would serialise it behind the gate) makes
this module fail with "instrument blind on this runtime"; the rows of tests/test_stream_order_hip.py mean nothing there."""
import ctypes
import threading

import pytest
import torch

import abi_harness as A
import stream_gate as SG


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------------------
def test_gate_length_rule():
    """8 x the ungated wall time, a floor, and a cap that the four-fold retry stays under."""
    assert SG.gate_ms_for(1.0) == 8.0 and SG.gate_ms_for(0.01) == SG.FLOOR_MS
    assert SG.gate_ms_for(1e6) * SG.RETRY == SG.CAP_MS
    assert SG.MARGIN_FACTOR == 8 and SG.RETRY == 4 and SG.CAP_MS <= 500.0


def cpu_case():
    b = SG.Built()
    dev = torch.device("cpu")
    real, decoy = torch.arange(6.0).reshape(2, 3), -torch.arange(6.0).reshape(2, 3) - 1
    # the builder's device is the GPU; on the CPU the same bookkeeping over host tensors
    buf = decoy.clone()
    b.inputs.append((buf, real, decoy))
    out = A.Guarded((2, 3), ld=4, device=dev)
    cnt = A.Guarded((8,), device=dev)
    nan = A.Guarded((8,), device=dev)
    b.outputs.append(out)
    b.works += [(cnt, True), (nan, False)]
    return b, buf, out, cnt, nan


def test_case_bookkeeping_on_the_host():
    """load() swaps real and decoy in place, poison() refills outputs and workspaces (zeros where asked, the guard elsewhere, margins always the
    guard), clones() are the payload columns, and a write into a margin is seen."""
    b, buf, out, cnt, nan = cpu_case()
    p = buf.data_ptr()
    assert torch.equal(buf, b.inputs[0][2])
    b.load("real")
    assert torch.equal(buf, b.inputs[0][1]) and buf.data_ptr() == p
    out.view[..., :3] = 1.0
    cnt.view[:] = 5.0
    nan.view[:] = 5.0
    b.poison()
    assert out.untouched() and nan.untouched() and bool((cnt.view == 0).all()) and cnt.margins_untouched()
    out.view[..., :3] = buf
    got, = b.clones()
    assert got.shape == (2, 3) and torch.equal(got, b.inputs[0][1])
    assert b.margins_untouched()
    cnt.full[0] = 0.0
    assert not b.margins_untouched()


def test_decoys_are_valid_floats():
    b = SG.Built()
    with pytest.raises(AssertionError):
        b.inp(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))          # index-like inputs are never decoyed
    with pytest.raises(AssertionError, match="never NaN"):
        b.inp(torch.zeros(2), torch.tensor([0.0, float("nan")]))


def test_decoy_must_matter():
    a = torch.arange(8.0)
    SG.decoy_matters([a], [a + 1])
    with pytest.raises(AssertionError, match="changes only"):
        SG.decoy_matters([a], [torch.where(a < 4, a + 1, a)])                                 # exactly half is not "more than half"
    SG.decoy_matters([a.int()], [a.int()])                                                    # integer outputs are not held to it
    nan = torch.full((4,), float("nan"))
    half_written = torch.cat([a, nan])                                                        # what both runs left poisoned is no output entry
    SG.decoy_matters([half_written], [torch.cat([a + 1, nan])])
    with pytest.raises(AssertionError, match="nothing was written"):
        SG.decoy_matters([nan], [nan])
    assert SG.differing_fraction(nan, nan) == 0.0 and SG.differing_fraction(nan, torch.zeros(4)) == 1.0
    assert SG.same_bits(nan, nan) and not SG.same_bits(torch.zeros(1), -torch.zeros(1))


def test_spy_records_the_stream_of_stream_entries_only():
    class Real:
        def car_add(self, *a):
            return 0

        def car_version(self):
            return 300
    handle = Real()
    captured = handle                                                 # a handle somebody kept before the spy came
    spy = SG.Spy(handle, {k: v for k, v in SG.all_signatures().items() if k in ("car_add", "car_version")}).install()
    assert captured.car_version() == 300 and spy.calls == []
    captured.car_add(*([None] * 10), ctypes.c_void_p(0x10))
    handle.car_add(*([None] * 10), None)

    class S:
        cuda_stream = 0x10
    assert spy.calls == [("car_add", 0x10), ("car_add", 0)] and spy.strays(S) == [("car_add", "0x0")] and spy.entries() == ["car_add"]
    spy.remove()
    handle.car_add(*([None] * 10), None)
    assert len(spy.calls) == 2


def test_last_error_is_thread_local():
    """include/car_hip.h: "car_last_error() returns a thread-local message".  Two host threads each provoke a refusal of their own (arguments
    that fail before any launch) at the same time, and each reads its own text back — the loader's assembler thread relies on it."""
    import __graft_entry__ as ge
    ge.build()
    lib = A.lib()
    calls = {"null": (lambda: lib.car_linear(None, 4, None, 4, 4, None, 4, 1, 0, None), b"null pointer"),
             "act": (lambda: lib.car_linear_x3_masked(None, 4, None, None, 4, 32, None, 32, 8, 0, None, 32, None), b"act")}
    assert calls["null"][1] not in (calls["act"][0]() and lib.car_last_error()) and calls["act"][1] not in (calls["null"][0]() and lib.car_last_error())
    refused, read = threading.Barrier(2), threading.Barrier(2)
    seen = {}

    def worker(name):
        call, _ = calls[name]
        texts = []
        for _ in range(20):
            refused.wait(timeout=30)
            code = call()
            read.wait(timeout=30)                                 # both refusals have happened before either text is read
            texts.append((code, lib.car_last_error()))
        seen[name] = texts

    threads = [threading.Thread(target=worker, args=(n,)) for n in calls]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert set(seen) == set(calls)
    for name, (_, word) in calls.items():
        other = next(w for n, (_, w) in calls.items() if n != name)
        for code, text in seen[name]:
            assert code == A.CAR_E_ARG and word in text and other not in text, (name, text)
    # and the main thread, which refused nothing since, still reads its own last message
    assert calls["null"][1] in lib.car_last_error()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def streams():
    return SG.instrument()["streams"]


@pytest.fixture(scope="module")
def instrument():
    """stream_gate.instrument(): the gate that sees a stray launch on this runtime (`_sleep`, else the matmul chain), chosen once per process
    by the two must-see checks; neither sees it: "instrument blind on this runtime", here and in every module that gates anything."""
    got = SG.instrument()
    print(f"stream gate: {SG.kind()} sees both stray launches ({SG.units_per_ms():.0f} units / ms); {got['report']}")
    return got["case"], got["ms"], got["report"]


@pytest.mark.gpu
def test_a_stray_launch_is_seen(instrument):
    _, _, report = instrument
    assert all(report[SG.kind()].values()), report


@pytest.mark.gpu
def test_a_correct_launch_passes(instrument, streams):
    b, _, _ = instrument
    rec = SG.check_case(b, streams[0], "car_add handed its own stream")
    assert rec["conclusive"]


@pytest.mark.gpu
def test_an_ended_gate_is_inconclusive(instrument, streams):
    """A step that outlasts its gate on the host (here: it synchronises the stream itself, as a call that broke "No call synchronises the
    device" would) is never a pass."""
    s = streams[0]
    with pytest.raises(SG.Inconclusive):
        SG.gated(s, 0.0, lambda: s.synchronize(), "a step that synchronises")
