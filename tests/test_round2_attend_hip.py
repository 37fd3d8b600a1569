"""car_attend_round2 (csrc/car_round2_attend.hip): the second attention round in one kernel — the folded bilinear logits of
car_round2_logits_from_g, the softmax over the ray's V * P samples and ebar = sum_s w_s e_s — through the C ABI

  * against the two launches it replaces (car_round2_logits_from_g, then car_attend on those logits) on the same inputs: logits, weights
    and ebar bit for bit;
  * against fp64: the logits within 4e-6 of the magnitudes that enter the sums (the bound of
    test_hip_parity.py::test_second_round_bilinear_form_matches_the_two_layers, whose inputs and weight scalings these are), the weights
    and ebar by test_attention_hip.py's rule for given logits (2e-5 of the sum of the terms' magnitudes, tests/attention_reference.py);
  * edge cases (a one-hot ray, a ray of constant logits, logit_out = NULL), the refusals, and the whole forward in both render precisions
    with engine.second_round_merged True against False.

Shapes: one ray (fewer rays than workgroups), odd ray counts (a last batch of one ray), three 32-sample tiles per view (P = 96), and
twelve scenes (uh is indexed by scene and ray and shared by the scene's views).  Every output lies in a NaN-filled buffer with margins."""
import pytest
import torch

import abi_harness as abi
import attention_reference as A
from abi_harness import CAR_E_ARG, Guarded
from parity_rule import error_ratio as _ratio

pytestmark = pytest.mark.gpu

V = 2
D = 576
TOL = 2e-5                                   # tests/test_attention_hip.py: fp32 sums against fp64, times the sum of the terms' magnitudes
LOGIT_TOL = 4e-6                             # test_second_round_bilinear_form_matches_the_two_layers
SHAPES = [(1, 1, 32, 1.0), (1, 5, 32, 1.0), (2, 33, 64, 30.0), (1, 7, 96, 1e-3), (12, 3, 64, 1.0)]       # (b, R, P, wscale)


def _inputs(b, R, P, wscale, g_edit=None, uh_edit=None):
    """g, uh and the four layers as test_second_round_bilinear_form_matches_the_two_layers makes them (V = 2), and e rows 576 wide."""
    S = b * V * R * P
    g_ = torch.Generator().manual_seed(S)
    rnd = lambda *sh: torch.randn(*sh, generator=g_)
    x = dict(b=b, R=R, P=P)
    x["g"] = rnd(S, 16) * torch.logspace(-2, 1, S).unsqueeze(1)
    x["uh"] = rnd(b * R, 128)
    x["wr1"], x["br1"] = rnd(128, 144) / 4, rnd(128)
    x["wr2"], x["br2"] = rnd(128, 128) / 128 ** 0.5 * wscale, rnd(128)
    x["wq1"], x["bq1"] = rnd(128, 16) / 4, rnd(128)
    x["wq2"], x["bq2"] = rnd(128, 128) / 128 ** 0.5 / wscale, rnd(128)
    x["e"] = rnd(b * V, R, P, D)
    if g_edit is not None:
        g_edit(x["g"].view(b * V, R, P, 16))
    if uh_edit is not None:
        uh_edit(x["uh"].view(b, R, 128))
    return x


def _run(x, merged=True, want_logits=True):
    """The merged entry, or the two launches it replaces.  Returns host tensors: logit [b*V, R, P] (None when not asked for), w, z [b, R, D]."""
    from cross_attention_renderer_amd import _lib as L
    lib = abi.lib()
    dev = abi.dev()
    b, R, P = x["b"], x["R"], x["P"]
    S = b * V * R * P
    d = {k: x[k].contiguous().to(dev) for k in ("g", "uh", "wr1", "br1", "wr2", "br2", "wq1", "bq1", "wq2", "bq2", "e")}
    st = abi.stream()
    wp, bp = torch.empty(lib.car_round2q_packed_floats(), device=dev), torch.empty(lib.car_round2q_bias_floats(), device=dev)
    L.check(lib.car_round2q_pack(abi.ptr(d["wr1"]), abi.ptr(d["br1"]), abi.ptr(d["wr2"]), abi.ptr(d["br2"]), abi.ptr(d["wq1"]), abi.ptr(d["bq1"]), abi.ptr(d["wq2"]),
                                 abi.ptr(d["bq2"]), abi.ptr(wp), abi.ptr(bp), st), "car_round2q_pack")
    logit, w, z = Guarded((S,)), Guarded((S,)), Guarded((b * R * D,))
    if merged:
        L.check(lib.car_attend_round2(abi.ptr(d["g"]), abi.ptr(d["uh"]), abi.ptr(wp), abi.ptr(bp), abi.ptr(d["e"]), D, b, V, R, P, w.ptr, z.ptr, D,
                                      logit.ptr if want_logits else None, st), "car_attend_round2")
    else:
        L.check(lib.car_round2_logits_from_g(abi.ptr(d["g"]), abi.ptr(d["uh"]), abi.ptr(wp), abi.ptr(bp), b, V, R, P, logit.ptr, st), "car_round2_logits_from_g")
        L.check(lib.car_attend(logit.ptr, None, 128, abi.ptr(d["e"]), D, b, V, R, P, None, 0.0, w.ptr, z.ptr, D, 1, None, None, None, None, st), "car_attend")
    torch.cuda.synchronize()
    if merged and not want_logits:
        assert logit.untouched()
    return {"logit": logit.get("logit").view(b * V, R, P) if (want_logits or not merged) else None,
            "w": w.get("w").view(b * V, R, P), "z": z.get("z").view(b, R, D)}


_cache = {}


def _case(b, R, P, wscale):
    """Inputs and both forms' outputs of a shape, computed once and shared by the tests that read them."""
    key = (b, R, P, wscale)
    if key not in _cache:
        x = _inputs(b, R, P, wscale)
        _cache[key] = (x, _run(x, merged=True), _run(x, merged=False))
    return _cache[key]


@pytest.mark.parametrize("b,R,P,wscale", SHAPES)
def test_merged_round_equals_the_two_launches_bit_for_bit(b, R, P, wscale):
    _, got, two = _case(b, R, P, wscale)
    for k in ("logit", "w", "z"):
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k], two[k]), f"{k}: max |diff| {(got[k] - two[k]).abs().max().item():.3e}"


@pytest.mark.parametrize("b,R,P,wscale", SHAPES)
def test_merged_round_against_fp64(b, R, P, wscale):
    x, got, _ = _case(b, R, P, wscale)
    d = lambda t: t.double()
    S = b * V * R * P
    ray = torch.arange(S) // P                                              # (scene-view, ray) -> (scene, ray)
    ray = (ray // R // V) * R + ray % R
    y = torch.relu(d(x["g"]) @ d(x["wr1"][:, 128:]).T + d(x["br1"]) + d(x["uh"])[ray])
    xx = torch.relu(d(x["g"]) @ d(x["wq1"]).T + d(x["bq1"]))
    q2, qry = y @ d(x["wr2"]).T + d(x["br2"]), xx @ d(x["wq2"]).T + d(x["bq2"])
    want = (q2 * qry).sum(1) / 16
    q2b, qb = y.abs() @ d(x["wr2"]).abs().T + d(x["br2"]).abs(), xx.abs() @ d(x["wq2"]).abs().T + d(x["bq2"]).abs()
    bound = (q2b * qb).sum(1) / 16
    r_logit = ((d(got["logit"]).reshape(-1) - want).abs() / bound).max().item() / LOGIT_TOL
    # the softmax and the value average for the logits the kernel itself made (test_attention_hip.py's rule for given logits)
    ref = A.forward(got["logit"], x["e"], V)
    w = d(got["w"])
    r_w = _ratio((w - ref["w"]).abs(), TOL * ref["w"].clamp_min(2.0 ** -100))
    r_sum = ((A.ray_major(w, b, V).sum(-1) - 1.0).abs() / TOL).max().item()
    r_z = _ratio((d(got["z"]) - ref["z"]).abs(), TOL * ref["Bz"])
    print(f"[parity] round2_attend b={b} R={R} P={P} wscale={wscale}: logit={r_logit:.3f} w={r_w:.3f} wsum={r_sum:.3f} z={r_z:.3f}")
    assert r_logit <= 1.0 and r_w <= 1.0 and r_sum <= 1.0 and r_z <= 1.0


def test_null_logit_out_changes_no_other_output():
    x, got, _ = _case(2, 33, 64, 30.0)
    quiet = _run(x, merged=True, want_logits=False)
    assert torch.equal(quiet["w"], got["w"]) and torch.equal(quiet["z"], got["z"])


def test_one_hot_ray_and_constant_ray():
    """Ray 2: uh is blown up until one sample's logit leads the ray by more than 100 — the weights are one-hot and ebar is that row of e,
    exactly.  Ray 1: every sample carries the same g, so the logits are constant — the weights are exactly 1 / (V P) (a power of two)."""
    b, R, P = 1, 5, 32

    def g_edit(g):                                                          # [b*V, R, P, 16]
        g[:, 1, :, :] = g[0, 1, 0, :].clone()

    def uh_edit(uh):                                                        # [b, R, 128]
        uh[0, 2] *= 1e4

    x = _inputs(b, R, P, 1.0, g_edit=g_edit, uh_edit=uh_edit)
    got, two = _run(x, merged=True), _run(x, merged=False)
    for k in ("logit", "w", "z"):
        assert torch.equal(got[k], two[k]), k
    lr = A.ray_major(two["logit"], b, V)                                    # [b, R, V*P]
    top2 = lr[0, 2].topk(2).values
    assert (top2[0] - top2[1]).item() > 100.0, "the planted ray does not dominate: the inputs of this test are wrong"
    hot = int(lr[0, 2].argmax())
    wr = A.ray_major(got["w"], b, V)
    one_hot = torch.zeros(V * P)
    one_hot[hot] = 1.0
    assert torch.equal(wr[0, 2], one_hot)
    assert torch.equal(got["z"][0, 2], A.ray_major(x["e"], b, V)[0, 2, hot])
    assert bool((lr[0, 1] == lr[0, 1, 0]).all()), "equal g rows gave different logits"
    assert torch.equal(wr[0, 1], torch.full((V * P,), 1.0 / (V * P)))


def test_refusals_write_nothing():
    lib = abi.lib()
    dev = abi.dev()
    b, R, P = 1, 3, 32
    S = b * V * R * 64
    g, uh, e = torch.zeros(S * 16, device=dev), torch.zeros(b * R * 128, device=dev), torch.zeros(S * D, device=dev)
    wp, bp = torch.zeros(lib.car_round2q_packed_floats(), device=dev), torch.zeros(lib.car_round2q_bias_floats(), device=dev)
    logit, w, z = Guarded((S,)), Guarded((S,)), Guarded((b * R * D,))
    st = abi.stream()
    call = lambda g_, uh_, wp_, bp_, e_, D_, P_, w_, z_: lib.car_attend_round2(g_, uh_, wp_, bp_, e_, D_, b, V, R, P_, w_, z_, D, logit.ptr, st)
    ok = (abi.ptr(g), abi.ptr(uh), abi.ptr(wp), abi.ptr(bp), abi.ptr(e))
    assert call(*ok, D, 8, w.ptr, z.ptr) == CAR_E_ARG and b"P" in lib.car_last_error()
    assert call(*ok, D, 40, w.ptr, z.ptr) == CAR_E_ARG
    assert call(*ok, 512, P, w.ptr, z.ptr) == CAR_E_ARG and b"576" in lib.car_last_error()
    for i in range(5):
        args = list(ok)
        args[i] = None
        assert call(*args, D, P, w.ptr, z.ptr) == CAR_E_ARG and b"null pointer" in lib.car_last_error()
    assert call(*ok, D, P, None, z.ptr) == CAR_E_ARG and call(*ok, D, P, w.ptr, None) == CAR_E_ARG
    torch.cuda.synchronize()
    assert logit.untouched() and w.untouched() and z.untouched()


def _forward(precision, merged):
    """The one-call forward of fixture t2_c2 (P = 64) with the second round merged or split; outputs on the host and the stage names."""
    from cross_attention_renderer_amd.engine import RenderEngine
    from golden_util import load_case
    from hip_harness import build_module, to_device
    dev = abi.dev()
    c, inp, z, sd, _ = load_case("t2_c2")
    m = build_module(c, sd, dev)
    m._engine = RenderEngine(m)
    m._engine.second_round_merged = merged
    m.render_precision = precision
    m._engine.profile(True)
    try:
        with torch.no_grad():
            out = m(to_device(inp, dev, cameras_on_host=True), z=[t.to(dev) for t in z])
        torch.cuda.synchronize()
        stages = [n for n, _ in m._engine.stage_times()]
    finally:
        m._engine.profile(False)
    assert m._engine.last_precision == precision
    return {k: out[k].detach().cpu() for k in ("rgb", "at_wt", "depth_ray")}, stages


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_whole_forward_merged_equals_split(precision):
    a, stages_a = _forward(precision, True)
    b_, stages_b = _forward(precision, False)
    assert "attend_2" in stages_a and "round2_logits" not in stages_a, stages_a
    assert "attend_2" in stages_b and "round2_logits" in stages_b, stages_b
    for k in ("rgb", "at_wt", "depth_ray"):
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b_[k]), f"{k}: max |diff| {(a[k] - b_[k]).abs().max().item():.3e}"
