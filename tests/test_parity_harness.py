"""The parity suites' own tools on the CPU: every corner of parity_rule.ratio that the suites' former private versions read differently,
the tolerance rule, and abi_harness.Guarded / take_rows firing on a write into each region they guard."""
import pytest
import torch

import abi_harness as abi
import parity_rule as PR
from abi_harness import NAN, Guarded

INF = float("inf")
D = lambda *v: torch.tensor(v, dtype=torch.float64)


# ---- ratio ------------------------------------------------------------------------------------------------------------------------------------
def test_ratio_is_the_worst_error_over_its_bound():
    assert PR.ratio(torch.tensor([1.0, 2.5, -1.0]), D(1.0, 2.0, -1.5), D(4.0, 1.0, 0.25)) == 2.0


def test_a_zero_bound_demands_a_zero_error():
    assert PR.ratio(torch.tensor([3.0, 1.0]), D(3.0, 1.5), D(0.0, 1.0)) == 0.5
    assert PR.ratio(torch.tensor([3.0, 1.0]), D(3.0 + 2.0 ** -40, 1.5), D(0.0, 1.0)) == INF


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
@pytest.mark.parametrize("bound", [1.0, 0.0])
def test_a_non_finite_result_is_infinitely_wrong(bad, bound):
    for kw in ({}, {"bound_ok": "finite"}, {"bound_ok": "nonzero"}, {"all_finite": True}):
        assert PR.ratio(torch.tensor([1.0, bad]), D(1.0, 2.0), D(1.0, bound), **kw) == INF, kw


def test_all_finite_sees_what_a_mask_or_a_nan_bound_would_hide():
    got, ref, mask = torch.tensor([1.0, NAN]), D(1.0, 2.0), torch.tensor([True, False])
    assert PR.ratio(got, ref, D(1.0, 1.0), mask) == 0.0
    assert PR.ratio(got, ref, D(1.0, 1.0), mask, all_finite=True) == INF
    assert PR.ratio(got, ref, D(1.0, -1.0), bound_ok="nonzero") != INF                  # -inf or NaN, entry by entry
    assert PR.ratio(got, ref, D(1.0, -1.0), bound_ok="nonzero", all_finite=True) == INF


def test_equal_infinities_agree_only_when_asked_to():
    got, ref = torch.tensor([1.0, INF, -INF]), D(1.0, INF, -INF)
    for bound in (D(1.0, 1.0, 1.0), D(1.0, 0.0, 0.0)):
        assert PR.ratio(got, ref, bound) == INF
        assert PR.ratio(got, ref, bound, equal_inf=True) == 0.0
    assert PR.ratio(got, D(1.0, -INF, INF), D(1.0, 1.0, 1.0), equal_inf=True) == INF
    assert PR.ratio(got, ref, D(1.0, 1.0, 1.0), equal_inf=True, all_finite=True) == INF


@pytest.mark.parametrize("bound_ok,inf_bound,nan_bound,negative", [("positive", 0.0, INF, INF), ("finite", INF, INF, INF), ("nonzero", 0.0, NAN, -2.0)])
def test_a_bound_that_is_not_finite_and_positive(bound_ok, inf_bound, nan_bound, negative):
    """An error of 1 over a bound of +inf, NaN and -0.5: divided by, or held to a zero error, as the keyword says."""
    got, ref = torch.tensor([1.0]), D(2.0)
    for bound, want in ((INF, inf_bound), (NAN, nan_bound), (-0.5, negative)):
        r = PR.ratio(got, ref, D(bound), bound_ok=bound_ok)
        assert r == want or (r != r and want != want), (bound, r, want)
        assert PR.ratio(ref, ref, D(bound), bound_ok=bound_ok) == 0.0 or bound != bound  # no error: nothing to hold against any bound


def test_a_mask_selects_the_entries_and_none_selected_gives_zero():
    got, ref, bound = torch.tensor([[1.0, 2.0], [3.0, 9.0]]), D(1.0, 2.0, 3.5, 4.0).view(2, 2), D(1.0)
    assert PR.ratio(got, ref, bound) == 5.0
    assert PR.ratio(got, ref, bound, torch.tensor([[True], [False]])) == 0.0
    assert PR.ratio(got, ref, bound, torch.tensor([[True, True], [True, False]])) == 0.5
    assert PR.ratio(got, ref, bound, torch.zeros(2, 2, dtype=torch.bool)) == 0.0
    assert PR.ratio(got[:0], ref[:0], bound) == 0.0


def test_the_error_form_agrees_with_the_pair_form():
    g = PR.gen(3)
    got, ref = torch.randn(7, 5, generator=g), torch.randn(7, 5, generator=g, dtype=torch.float64)
    bound = torch.rand(7, 5, generator=g, dtype=torch.float64)
    bound[2, 3] = 0.0
    got[2, 3] = ref[2, 3].float()
    ref[2, 3] = got[2, 3].double()
    mask = torch.rand(7, 5, generator=g) < 0.5
    for kw in ({}, {"mask": mask}, {"bound_ok": "finite"}, {"bound_ok": "nonzero", "mask": mask}):
        assert PR.error_ratio((got.double() - ref).abs(), bound, **kw) == PR.ratio(got, ref, bound, **kw), kw
    assert PR.error_ratio(D(NAN), D(1.0)) == INF and PR.error_ratio(D(1.0), D(0.0)) == INF and PR.error_ratio(D(0.0), D(0.0)) == 0.0


def test_tolerance():
    assert PR.tolerance(0) == 2.0 ** -19
    assert PR.tolerance(1e-3) == 8e-3
    assert (PR.FLOOR, PR.FACTOR) == (2.0 ** -22, 8.0)


def test_judge_holds_every_entry_to_every_deciding_yardstick(capsys):
    ref, bound = D(1.0, 2.0), D(1.0, 1.0)
    got = torch.tensor([1.0, 2.0 + 2.0 ** -20])                                           # ratio 2^-20: 4 x the floor, half the least tolerance
    PR.judge("t", "c", {"": ((got, ref, bound), 0.0)}, also={"other": 1e-9})
    PR.judge("t", "c", {"a": ((got, ref, bound), {"fp32": 1e-6, "fp16-emulation": 0.0}), "b": (2.0 ** -19, 0.0)}, finite=True)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "[parity] t c: 0.500 (kernel 9.54e-07 fp32 0.00e+00 tol 1.91e-06; other 1.00e-09 tol 1.91e-06)"
    assert lines[1] == ("[parity] t c: a=0.119 (kernel 9.54e-07 fp32 1.00e-06 tol 8.00e-06; fp16-emulation 0.00e+00 tol 1.91e-06: 0.5000) "
                        "b=1.000 (kernel 1.91e-06 fp32 0.00e+00 tol 1.91e-06)  ABOVE HALF THE TOLERANCE")
    got = torch.tensor([1.0, 2.0 + 2.0 ** -18])                                           # ratio 2^-18: under 8e-6, over the floor's 2^-19
    with pytest.raises(AssertionError):
        PR.judge("t", "c", {"": ((got, ref, bound), {"fp32": 1e-6, "fp16-emulation": 2.0 ** -24})})      # the tighter one decides
    PR.judge("t", "c", {"": ((got, ref, bound), 1e-6)}, also={"fp16-emulation": 2.0 ** -24})              # printed only
    PR.judge("t", "c", {"": ([(ref, ref, bound), (got, ref, bound)], 1e-6)})
    with pytest.raises(AssertionError):
        PR.judge("t", "c", {"": ([(got, ref, bound), (ref, ref, bound)], 2.0 ** -24)})                     # the worst of a list counts
    with pytest.raises(AssertionError, match="not finite"):
        PR.judge("t", "c", {"x": ((torch.tensor([1.0, INF]), D(1.0, INF), bound), 1.0)}, finite=True, ratio=lambda *a: 0.0)


# ---- Guarded ------------------------------------------------------------------------------------------------------------------------------------
ROWS, COLS, LD, OFFSET = 3, 5, 8, 2
FRONT = abi.MARGIN + OFFSET
# flat index into .full of: the last element of the front margin, the offset gap, the first padding column of the last row, the first
# element of the back margin
OUTSIDE = {"front margin": abi.MARGIN - 1, "offset gap": abi.MARGIN + OFFSET - 1, "row padding": FRONT + (ROWS - 1) * LD + COLS, "back margin": FRONT + ROWS * LD}
PAYLOAD = {"first": FRONT, "last": FRONT + (ROWS - 1) * LD + COLS - 1}
MESSAGE = {"front margin": "in front of the buffer", "offset gap": "in front of the buffer", "row padding": "into the row padding", "back margin": "behind the buffer"}


def _guarded(dtype, **kw):
    return Guarded((ROWS, COLS), LD, OFFSET, dtype=dtype, device="cpu", **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32], ids=["float32", "int32"])
def test_guarded_layout_and_a_fresh_buffer(dtype):
    g = _guarded(dtype)
    assert g.untouched() and g.margins_untouched()
    assert g.full.numel() == 2 * abi.MARGIN + OFFSET + ROWS * LD and g.view.shape == (ROWS, LD)
    assert g.ptr.value == g.full.data_ptr() + 4 * FRONT == g.view.data_ptr()
    got = g.get("fresh")
    assert got.shape == (ROWS, COLS)
    assert bool(torch.isnan(got).all()) if dtype == torch.float32 else bool((got == abi.SENTINEL).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32], ids=["float32", "int32"])
@pytest.mark.parametrize("where", list(OUTSIDE))
def test_guarded_fires_on_a_write_outside_the_payload(where, dtype):
    g = _guarded(dtype)
    g.full[OUTSIDE[where]] = 1
    assert not g.untouched()
    assert g.margins_untouched() == (where == "row padding")
    with pytest.raises(AssertionError, match=f"x: wrote {MESSAGE[where]}"):
        g.get("x")


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32], ids=["float32", "int32"])
@pytest.mark.parametrize("where", list(PAYLOAD))
def test_guarded_lets_a_payload_write_through(where, dtype):
    g = _guarded(dtype)
    g.full[PAYLOAD[where]] = 7
    assert g.margins_untouched() and not g.untouched()
    got = g.get("x")
    assert got.reshape(-1)[0 if where == "first" else -1] == 7 and int((got == 7).sum()) == 1


def test_guarded_fill_and_init_reach_the_payload_only():
    g = _guarded(torch.float32, fill=0.0)
    assert g.margins_untouched() and bool(torch.isnan(g.view[:, COLS:]).all()) and bool((g.get() == 0).all())
    init = torch.arange(ROWS * COLS, dtype=torch.float32)
    g = _guarded(torch.float32, init=init)
    assert torch.equal(g.get(), init.view(ROWS, COLS))
    g = Guarded((2, 3, 4), device="cpu")                                                  # ld = cols: the view has the shape itself
    assert g.view.shape == (2, 3, 4) and g.get().shape == (2, 3, 4) and g.full.numel() == 2 * abi.MARGIN + 24
    assert Guarded((6,), device="cpu").get().shape == (6,)


# ---- rows_out / take_rows -----------------------------------------------------------------------------------------------------------------------
def test_take_rows_hands_back_the_windows_and_fires_on_the_guard_row():
    rows, width, ld = 4, 6, 8
    out = abi.rows_out(rows, ld, offset=1, device="cpu")
    assert out.view.shape == (rows + 1, ld) and out.untouched()
    out.view[:rows, :width] = 2.0
    assert bool((abi.take_rows(out, rows, width, "y") == 2.0).all()) and out.untouched()
    for at in ((rows, 0), (0, width), (rows - 1, ld - 1)):                                # the guard row, the padding of the first and of the last row
        out = abi.rows_out(rows, ld, device="cpu")
        out.view[:rows, :width] = 2.0
        out.view[at] = 0.0
        with pytest.raises(AssertionError, match="y: wrote outside the rows' windows"):
            abi.take_rows(out, rows, width, "y")
    out = abi.rows_out(rows, ld, device="cpu")
    out.full[-abi.MARGIN] = 0.0
    with pytest.raises(AssertionError):
        abi.take_rows(out, rows, width, "y")
