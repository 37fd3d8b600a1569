"""The acceptance rule of the kernel parity suites, stated once: the error-over-bound ratio, the tolerance it is held to, and the
``[parity]`` line that reports both.  Test infrastructure: no GPU, no ctypes.

    ratio      = max over entries of |got - ref64| / bound          bound: the float64 sum of magnitudes that goes with the value
    tolerance  = FACTOR x max(ratio of a yardstick on the same inputs, FLOOR)

The yardstick is a run of the same formula in the arithmetic the kernel is entitled to (the float32 restatement; for the fp16 and bf16
entries the CPU emulation of that arithmetic), judged against the same float64 reference and bound, never against the kernel."""
from __future__ import annotations

import torch

INF = float("inf")
FLOOR = 2.0 ** -22
# 4: the kernels' operands keep 22 bits against fp32's 24 (csrc/car_split.h: |x - hi - lo| < 2^-21 |x|);
# 2: the spread of a maximum over a few thousand entries.
FACTOR = 8.0


def tolerance(r_yardstick: float) -> float:
    """What the kernel's ratio may reach: 8 x max(the yardstick's ratio on the same inputs, 2^-22)."""
    return FACTOR * max(r_yardstick, FLOOR)


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def error_ratio(err, bound, mask=None, *, bound_ok: str = "positive") -> float:
    """max over the masked entries of err / bound, err >= 0 given; a non-finite error is infinitely wrong; an entry whose bound is not
    divided by demands a zero error.  `bound_ok` says which bounds are divided by:
      "positive"  bound > 0, +inf included (a NaN or negative bound counts as zero);
      "finite"    bound > 0 and finite;
      "nonzero"   bound != 0 (a negative or NaN bound is divided by).
    No entry left (an empty tensor, a mask that selects nothing) gives 0."""
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, INF))
    bound = bound.expand_as(err)
    ok = {"positive": bound > 0, "finite": torch.isfinite(bound) & (bound > 0), "nonzero": bound != 0}[bound_ok]
    r = torch.where(ok, err / torch.where(ok, bound, torch.ones_like(bound)), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, INF)))
    if mask is not None:
        r = r[mask.expand_as(r)]
    return r.max().item() if r.numel() else 0.0


def ratio(got, ref64, bound, mask=None, *, equal_inf: bool = False, bound_ok: str = "positive", all_finite: bool = False) -> float:
    """error_ratio of |got - ref64|.  equal_inf: entries where got == ref64 agree, equal infinities among them (otherwise inf - inf is a
    non-finite error).  all_finite: a non-finite entry anywhere in `got`, masked or not, makes the whole comparison infinitely wrong."""
    if all_finite and not bool(torch.isfinite(got).all()):
        return INF
    got, ref64 = got.double(), ref64.double()
    err = (got - ref64).abs()
    if equal_inf:
        err = torch.where(got == ref64, torch.zeros_like(err), err)
    return error_ratio(err, bound, mask, bound_ok=bound_ok)


def judge(test: str, case: str, entries: dict, what: str = "fp32", also=None, extra: str = "", finite: bool = False, ratio=ratio) -> None:
    """Prints the ``[parity] <test> <case>: ...`` line and holds every entry's ratio to tolerance(yardstick).

    entries: {name: (kernel, yardstick)}.  kernel: (got, ref64, bound[, mask]) for ratio(), a list of such tuples (the worst one counts),
    or a ratio already taken.  yardstick: the ratio of the run named `what`, or {name: ratio} of several that all decide, the first of
    them the one the leading quotient is taken against.  also: {name: ratio} of yardsticks that are printed with the tolerance they would
    give and decide nothing.  finite: assert first that every `got` is finite.  ratio: the suite's reading of ratio() where it sets
    keywords.  An entry named "" is printed without its name."""
    parts, bad, half = [], [], False
    for name, (rk, yard) in entries.items():
        if not isinstance(rk, float):
            pairs = [rk] if isinstance(rk, tuple) else rk
            assert not finite or all(bool(torch.isfinite(p[0]).all()) for p in pairs), (test, case, name, "not finite")
            rk = max(ratio(*p) for p in pairs)
        yards = list((yard if isinstance(yard, dict) else {what: yard}).items())
        (w0, r0), tol0 = yards[0], tolerance(yards[0][1])
        text = f"{rk / tol0:.3f} (kernel {rk:.2e} {w0} {r0:.2e} tol {tol0:.2e}"
        for w, r in yards[1:]:
            text += f"; {w} {r:.2e} tol {tolerance(r):.2e}: {rk / tolerance(r):.4f}"
        for w, r in (also or {}).items():
            text += f"; {w} {r:.2e} tol {tolerance(r):.2e}"
        parts.append((f"{name}=" if name else "") + text + extra + ")")
        half = half or rk > tol0 / 2
        for w, r in yards:
            if not rk <= tolerance(r):
                bad.append((name, w, rk, tolerance(r)))
    print(f"[parity] {test} {case}: " + " ".join(parts) + ("  ABOVE HALF THE TOLERANCE" if half else ""))
    assert not bad, (test, case, bad)
