"""tests/vit_backward_reference.py (the written-out backward the GPU suite of the transformer stage's backward is judged against) held, in
float64 on the CPU, to float64 autograd of vit_reference's forward at rounding level; the ctypes table of include/car_encoder_train.h held
to the header; the new entries' sizes and refusals, which need no device.  Nothing here is marked gpu."""
import ctypes
import os
import re

import pytest
import torch

import vit_backward_reference as BR
import vit_reference as VR
from parity_rule import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
ROUNDING = 2.0 ** -40                                                  # float64 against float64: a few hundred terms of 2^-53 each


def _close(got, want, bound, what):
    r = float(((got.double() - want.double()).abs() / bound.clamp_min(1e-300)).max())
    assert r <= ROUNDING, (what, r)


def _autograd(fn, inputs, cot):
    leaves = [t.double().requires_grad_(True) for t in inputs]
    (fn(*leaves) * cot.double()).sum().backward()
    return [t.grad for t in leaves]


@pytest.mark.parametrize("M,C", [(3, 64), (65, 128)])
def test_layernorm_backward_is_autograd_of_the_forward(M, C):
    x, g, b = VR.ln_input("gauss", M, C)
    dy = BR.ln_dy(M, C)
    (dx, Bx), (dg, Bg), (db, Bb) = BR.layernorm_backward(x, g, dy)
    ax, ag, ab = _autograd(lambda x_, g_, b_: VR.layernorm(x_, g_, b_)[0], (x, g, b), dy)
    _close(dx, ax, Bx, "dx"), _close(dg, ag, Bg, "dgamma"), _close(db, ab, Bb, "dbeta")
    # a constant row: xhat = 0, rstd = 1 / sqrt(eps) = 1000
    xc, g, b = VR.ln_input("const", M, C)
    (dx, Bx), _, _ = BR.layernorm_backward(xc, g, dy)
    a = dy.double() * g.double()
    assert torch.isfinite(dx).all() and torch.allclose(dx, 1000.0 * (a - a.mean(dim=1, keepdim=True)), rtol=1e-12, atol=0)


def test_gelu_backward_is_autograd_of_the_forward():
    u = VR.gelu_grid()[None, :]
    dy = torch.randn(u.shape, generator=gen(3))
    du, B = BR.gelu_backward(u, dy)
    (au,) = _autograd(lambda u_: VR.gelu(u_)[0], (u,), dy)
    # autograd differentiates x (1 + erf(x / sqrt 2)) / 2, whose 1 + erf cancels in the lower tail: ITS terms have magnitude 1, not Phi
    _close(du, au, dy.double().abs() * (1.0 + B), "du")
    d, _ = BR.gelu_grad(torch.tensor([0.0, -0.0, 40.0, -40.0]))
    assert d.tolist() == [0.5, 0.5, 1.0, 0.0]


@pytest.mark.parametrize("b,S,heads", [(2, 5, 2), (1, 1, 1), (1, 33, 1), (1, 66, 2)])
def test_attention_backward_is_autograd_of_the_forward(b, S, heads):
    qkv, dout = VR.mha_input("gauss", b, S, heads), BR.mha_dout(b, S, heads)
    dqkv, B = BR.attention_backward(qkv, dout, b, S, heads)
    (a,) = _autograd(lambda x: VR.attention(x, b, S, heads)[0], (qkv,), dout)
    _close(dqkv, a, B, "dqkv")
    dim = heads * VR.HEAD
    if S == 1:                                                          # one key: the softmax is constant, dv = dout
        assert float(dqkv[:, :2 * dim].abs().max()) <= 1e-12 and torch.equal(dqkv[:, 2 * dim:], dout.double())
    lse = BR.log_sum_exp(qkv, b, S, heads)
    assert lse.shape == (b, heads, S) and torch.isfinite(lse).all()
    # the integer set is exact in float32 where the GPU suite needs it to be: at S = 1
    qi, di = BR.mha_integers(1, 1, 1)
    d32, _ = BR.attention_backward(qi, di, 1, 1, 1, F32)
    assert not d32[:, :128].any() and torch.equal(d32[:, 128:], di)


@pytest.mark.parametrize("which", ["all", "tap1", "tap2"])
def test_stage_backward_is_autograd_of_the_stage(which):
    dim, depth, taps, b, S = 128, 3, (1, 2), 2, 10
    params = VR.seeded_stage(dim, depth)
    tok0, dtaps, dout, a_tok, a_params = BR.autograd_stage(dim, depth, taps, b, S, which)
    ops = {}
    (dtok, Bt), grads = BR.stage_backward(tok0, params, b, S, dim // VR.HEAD, taps, dtaps, dout, ops=ops)
    assert float(((dtok - a_tok).abs() / Bt).max()) <= 2.0 ** -36
    for i, ((g, B), a) in enumerate(zip(grads, a_params)):
        assert g.shape == params[i].shape
        assert float((g - a).abs().max()) <= 2.0 ** -36 * max(float(B), 1e-300), (i, float(B))
    assert sorted(ops) == [0, 1, 2] and [o[0] for o in ops[0]] == [10, 8, 4, 2]
    nonzero = [bool(g.any()) for g, _ in grads]
    if which == "tap1":                                                 # nothing behind block 1 sees the gradient
        assert not any(nonzero[24:]) and all(nonzero[:24])
    else:
        assert all(nonzero)


def test_the_float32_run_is_a_float32_run():
    qkv, dout = VR.mha_input("gauss", 1, 33, 1), BR.mha_dout(1, 33, 1)
    d32, _ = BR.attention_backward(qkv, dout, 1, 33, 1, F32)
    d64, B = BR.attention_backward(qkv, dout, 1, 33, 1)
    assert d32.dtype == F32 and B.dtype == F64
    r = float(((d32.double() - d64).abs() / B).max())
    assert 2.0 ** -30 < r < 2.0 ** -18


# ---- the C ABI's table, sizes and refusals (no device) ---------------------------------------------------------------------------------------
def test_encoder_train_signatures_mirror_their_header_type_by_type():
    import test_abi as T
    from cross_attention_renderer_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "car_encoder_train.h")).read(), flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    protos = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(car_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [p.strip() for p in " ".join(params.split()).split(",")]
        params = [] if params == ["void"] else ["*" if "*" in p else " ".join(w for w in p.split()[:-1] if w != "const") for p in params]
        protos[name] = (" ".join(ret.split()).replace(" *", "*"), params)
    assert len(protos) == 15 == len(_lib.ENCODER_TRAIN_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.MATCH_SIGNATURES) | set(_lib.ENCODER_SIGNATURES) | set(_lib.TRUNK_SIGNATURES) | set(_lib.DECODER_SIGNATURES)
    assert not set(protos) & others
    assert T._abi_disagreements(protos, _lib.ENCODER_TRAIN_SIGNATURES) == []
    hip_h = open(os.path.join(ROOT, "include", "car_hip.h")).read()
    assert hip_h.index('#include "car_decoder.h"') < hip_h.index('#include "car_encoder_train.h"') < hip_h.index("#ifdef __cplusplus\n}")
    assert "#define CAR_VERSION 300" in hip_h                                                  # additive entries: the number stays
    import __graft_entry__ as G
    assert G.UNITS["car_vit_backward.hip"] == [] == G.UNITS["car_vit.hip"]
    src = open(os.path.join(ROOT, "cross_attention_renderer_amd", "_lib.py")).read()
    assert '"car_encoder_train.h"' in src[src.index("def source_hash"):src.index("def _rebuild_stale")]
    assert "ENCODER_TRAIN_SIGNATURES" in src[src.index("def check_exports"):src.index("def check(")]
    assert "no entry here has a backward" not in " ".join(open(os.path.join(ROOT, "include", "car_encoder.h")).read().split())


def test_encoder_train_entries_are_exported_bound_and_refuse_without_a_device():
    import __graft_entry__ as G
    G.build()
    from cross_attention_renderer_amd import _lib
    lib, api = _lib.load(), _lib.api()
    for name, (res, _) in _lib.ENCODER_TRAIN_SIGNATURES.items():
        assert hasattr(lib, name), name
        assert (getattr(api, name).errcheck is _lib._errcheck) == (res is ctypes.c_int), name
    msg = lambda: lib.car_last_error().decode()
    for call in (lambda: api.car_mha_backward(None, 0, None, None, 0, None, 0, 1, 1, 1, None, 0, None, 0, None),
                 lambda: api.car_layernorm_backward(None, 0, None, 4, 1e-6, None, 0, None, 0, 1, 0, None, None, None, 0, None),
                 lambda: api.car_gelu_backward(None, 0, None, 0, 1, 4, None),
                 lambda: api.car_vit_blocks_backward(None, 1, 1, 64, None, 1, None, 0, None, None, 0, None, 0, None, 0, None)):
        with pytest.raises(_lib.CarError, match="null pointer"):
            call()
    # sizes.  The statistics: two floats a (scene, head, row).  One tile record of the backward: 7 forms x 4 K steps x 2 KB
    assert lib.car_mha_stats_floats(2, 33, 3) == 2 * 3 * 33 * 2
    one = lib.car_mha_backward_workspace_bytes(1, 32, 1)
    assert lib.car_mha_backward_workspace_bytes(1, 64, 1) - one == 7 * 4 * 2048
    for bad in ((1, 0, 1), (1, 1025, 1), (1, 5, 0), (1, 5, 17), (0, 5, 1)):
        for entry in (lib.car_mha_stats_floats, lib.car_mha_backward_workspace_bytes):
            assert entry(*bad) == 0 and "outside" in msg(), bad
    # what a block saves: 10 dim floats a row and the statistics, in pieces of whole 64 floats; the issue's figure at the training batch
    up = lambda n: (n + 63) // 64 * 64
    for b, S, dim, depth in ((1, 1, 64, 1), (3, 33, 192, 3), (12, 514, 768, 12)):
        rows, heads = b * S, dim // 64
        want = 4 * depth * (3 * up(rows * dim) + up(rows * 3 * dim) + up(rows * 4 * dim) + up(rows * heads * 2))
        assert lib.car_vit_saved_bytes(b, S, dim, depth) == want
    per_block = lib.car_vit_saved_bytes(12, 514, 768, 1)
    print(f"[size] saved per block at b = 12, S = 514, dim = 768: {per_block / 1e6:.1f} MB")
    assert 0.18e9 < per_block < 0.2e9
    assert lib.car_vit_saved_bytes(1, 33, 65, 1) == 0 and lib.car_vit_saved_bytes(1, 33, 64, 33) == 0 and lib.car_vit_saved_bytes(1, 0, 64, 1) == 0
    # the train pack starts with car_vit_pack's own layout; the gradient buffer is torch's shapes one after the other
    for dim, depth in ((64, 1), (192, 3), (768, 12)):
        fwd, total = lib.car_vit_packed_floats(dim, depth), lib.car_vit_packed_train_floats(dim, depth)
        assert lib.car_vit_packed_train_offset(dim, depth, 5) == fwd
        tr = [lib.car_vit_packed_train_offset(dim, depth, i) for i in range(5)]
        assert tr[0] == 0 and tr == sorted(tr) and total == fwd + depth * tr[4] + 4 * dim * dim
        shapes = [dim, dim, 3 * dim * dim, 3 * dim, dim * dim, dim, dim, dim, 4 * dim * dim, 4 * dim, 4 * dim * dim, dim]
        assert [lib.car_vit_grad_offset(dim, i) for i in range(13)] == [sum(shapes[:i]) for i in range(13)]
    assert lib.car_vit_packed_train_floats(65, 1) == 0 and lib.car_vit_packed_train_offset(64, 1, 6) == 0 and lib.car_vit_grad_offset(64, 13) == 0
    assert lib.car_layernorm_backward_workspace_bytes(65, 128) == 8 * (2 * 65 + 6 + 2 * 2 * 128)   # row statistics (whole 8 doubles), 2 slabs x 2 x C
    assert lib.car_layernorm_backward_workspace_bytes(1, 6) == 0 and lib.car_layernorm_backward_workspace_bytes(0, 64) == 0
    assert lib.car_vit_backward_workspace_bytes(1, 33, 65) == 0 and lib.car_vit_backward_workspace_bytes(1, 33, 64) > lib.car_vit_workspace_bytes(1, 33, 64)
