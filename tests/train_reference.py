"""The stages of the training forward (cross_attention_renderer_amd/staged.py with a ``Saved`` record) and of its backward
(training.py), restated in plain torch with the dtype a parameter — the checker of tests/test_train_stages_hip.py; this file itself is
checked by tests/test_train_reference.py.  No GPU, no ctypes, no product code: written from staged.py's comments and the kernels'
contracts in include/car_hip.h, on top of the one-kernel references (linear_reference, attention_reference, gather_reference).

One pair of functions per stage, named after it:

    decode / decode_adjoint                          phi.lin_in; per block x += lin_z(zrep), net = fc_0(relu(x)), x += fc_1(relu(net));
                                                     lin_out(relu(x)); rgb = out valid + (1 - valid)
    attention_rounds / attention_rounds_adjoint      ebar1 = sum_s w_s e_s, the depth read-out; z1 = latent_value(ebar1); hb = encode_latent(z1);
                                                     k1r = relu(Wr[:, 128:] g + br + Wr[:, :128] hb[ray]); key2 = query_repeat_embed_2(k1r);
                                                     logits <key, q> / 16; z = V z1 + latent_value(ebar2); zrep = V copies of z
    keys_and_queries / keys_and_queries_adjoint      k1 = relu(key_map(e)), key = key_map_2(k1), q1 = relu(query_embed(g)), q = query_embed_2(q1)
    e_concat2, e_concat3, e_single, e_plain / *_adjoint     the four ways of making e, their gathers through gather_reference

A value travels with the magnitude its rounding error scales with, as a pair (value in the run's dtype, bound in float64): the float64
value of the same expression with every operand replaced by its magnitude and every subtraction by an addition — the one-kernel bounds
of linear_reference (|x| |W|^T + |b|, |dY|^T |act(X)|), attention_reference.backward (Ba, Bl) and gather_reference (sum |w| |dout|)
composed along the stage.  A stage's input cotangent is taken as given: its bound is its magnitude; so is d z1 between the two
attention rounds (attention_rounds_adjoint and backward say why: carried further, the sums of magnitudes outgrow the values by many
orders of magnitude and stop being a scale any error could be large against).

An adjoint takes the SAVED tensors as given (a dict with staged.Saved's field names): ReLU masks are ``act > 0`` on the saved
activation (the kernels' rule ``!(act > 0) -> 0``: NaN and either zero give no gradient), softmax weights are the saved at_wt / at_wt2,
weight-gradient operands are the saved rows.  The record is the point of linearisation, so a pre-activation within rounding of zero
cannot put reference and device on different branches.

The linear layers and weight gradients go through an ``Arith``: float64 (the reference), float32 (the yardstick of the fp32-pipe
routes), or float32 with linear_reference.x3_linear / wgrad_bf16 on exactly the launches that take those routes (``takes_x3`` restates
engine.linear's rule, linear_reference.wgrad_dispatch car_linear_wgrad's), fed the engine's linear_x3_min_rows and wgrad_fp32.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

import attention_reference as AR
import gather_reference as GR
import linear_reference as LR

F32, F64 = torch.float32, torch.float64


def takes_x3(M: int, K: int, N: int, min_rows: int) -> bool:
    """engine.linear's choice of car_linear_x3 for a layer [N, K] over M rows (the row strides of every launch of the training path are
    multiples of 4 and its buffers 16-byte aligned): packed for it (N % 32 == 0, K >= 64) and at least linear_x3_min_rows rows."""
    return N % 32 == 0 and K >= 64 and M >= min_rows


class Arith:
    """The arithmetic of one run.  Arith(): float64 throughout.  Arith(F32): float32 throughout.  Arith(F32, x3_min_rows, wgrad_fp32):
    float32, with the split-fp16 emulation on the layers that take car_linear_x3 and the bf16 emulation on the weight gradients that take
    wgrad16_kernel — the arithmetic each launch of the default (or conservative) route is entitled to."""

    def __init__(self, dtype=F64, x3_min_rows: Optional[int] = None, wgrad_fp32: bool = True):
        self.dtype, self.x3_min_rows, self.wgrad_fp32 = dtype, x3_min_rows, wgrad_fp32

    def lin(self, x, W, b=None):
        """x W^T + b."""
        if self.x3_min_rows is not None and takes_x3(x.shape[0], W.shape[1], W.shape[0], self.x3_min_rows):
            return LR.x3_linear(x, W, b).to(self.dtype)
        dt = self.dtype
        return F.linear(x.to(dt), W.to(dt), None if b is None else b.to(dt))

    def wgrad(self, dy, x, relu: bool, bias: bool):
        """(dy^T act(x), column sums of dy or None)."""
        M, N, K = dy.shape[0], dy.shape[1], x.shape[1]
        if self.x3_min_rows is not None and LR.wgrad_dispatch(M, N, K, bias, LR.WGRAD_FP32 if self.wgrad_fp32 else 0) == "bf16":
            dW, db = LR.wgrad_bf16(dy.float(), x.float(), relu, torch.zeros(N, K), torch.zeros(N) if bias else None)
            return dW.to(self.dtype), None if db is None else db.to(self.dtype)
        dt = self.dtype
        xx = F.relu(x) if relu else x
        return dy.to(dt).T @ xx.to(dt), dy.to(dt).sum(0) if bias else None


REF = Arith()


def _abs(t):
    return t.detach().double().abs()


def given(t, dtype=None):
    """A tensor taken as given -> the pair (t, |t|), t in `dtype` when one is named; a pair passes as it is."""
    return t if isinstance(t, tuple) else (t if dtype is None else t.to(dtype), _abs(t))


def weight(par, name):
    w = par[name + ".weight"]
    return w.reshape(w.shape[0], -1)


def n_blocks(par) -> int:
    return sum(1 for k in par if k.startswith("phi.lin_z.") and k.endswith(".weight"))


def sizes(sv) -> dict:
    """b, V, R, P, n, S, bR, pts of a record."""
    b, R = sv["valid"].shape[:2]
    n, _, P = sv["pixel_val"].shape[:3]
    return dict(b=b, V=n // b, R=R, P=P, n=n, S=n * R * P, bR=b * R, pts=R * P)


def inv_q_of(poses, V):
    """[b V, 96] pose records -> inv_q [b, 3, 4]: floats 77:89 of every scene's first view."""
    return poses[::V, 77:89].reshape(-1, 3, 4)


# ---- pairs through the pieces ------------------------------------------------------------------------------------------------------------------
def _fwd(ar, x, W, b):
    """A forward layer on a pair."""
    v, B = x
    K = W.shape[1]
    Bo = B[:, :K] @ _abs(W).T
    return ar.lin(v[:, :K], W, b), Bo if b is None else Bo + _abs(b)


def _relu(x):
    return F.relu(x[0]), x[1]


def _add(x, y):
    return x[0] + y[0], x[1] + y[1]


def _dx(ar, dy, W, act=None):
    """The data gradient dy W of a layer y = x W^T; `act`: x = relu(act), so the gradient is +0 where !(act > 0)."""
    v, B = ar.lin(dy[0], W.t()), dy[1] @ _abs(W)
    if act is not None:
        keep = act > 0
        v, B = torch.where(keep, v, torch.zeros_like(v)), torch.where(keep, B, torch.zeros_like(B))
    return v, B


class Grads(dict):
    """name -> pair, both [N, K] (weights, as matrices) or [N] (biases); a name appears when something was added to it."""

    def __init__(self, par, dtype):
        super().__init__()
        self.par, self.dtype = par, dtype

    def add(self, name, v, B, col0=0):
        if name not in self:
            shape = weight(self.par, name[:-7]).shape if name.endswith(".weight") else self.par[name].shape
            self[name] = (torch.zeros(shape, dtype=self.dtype), torch.zeros(shape, dtype=F64))
        gv, gB = self[name]
        if v.dim() == 2:
            gv[:, col0:col0 + v.shape[1]] += v
            gB[:, col0:col0 + v.shape[1]] += B
        else:
            gv += v
            gB += B

    def shaped(self) -> Dict[str, tuple]:
        """The pairs in the parameters' own shapes."""
        return {k: (v.reshape(self.par[k].shape), B.reshape(self.par[k].shape)) for k, (v, B) in self.items()}


def _wg(ar, G: Grads, name, dy, x, relu=False, col0=0, K=None, bias=True):
    """car_linear_wgrad of layer `name`: dW[:, col0:col0 + K] += dy^T act(x[:, :K]), db += sum dy."""
    K = weight(G.par, name).shape[1] if K is None else K
    xx = x[:, :K]
    dW, db = ar.wgrad(dy[0], xx, relu, bias)
    G.add(name + ".weight", dW, dy[1].T @ _abs(F.relu(xx) if relu else xx), col0)
    if bias:
        G.add(name + ".bias", db, dy[1].sum(0))


# ---- decode --------------------------------------------------------------------------------------------------------------------------------------
def decode(par, phi_x, zrep, valid, ar: Arith = REF) -> dict:
    """staged._decode from phi_x [bR, >= 9 V], zrep [bR, V Dl], valid [b, R, 1] -> pairs: xas, nets (lists), dec_out, out [bR, 3] and
    rgb [b, R, 3] = out valid + (1 - valid)."""
    x = _fwd(ar, given(phi_x), weight(par, "phi.lin_in"), par["phi.lin_in.bias"])
    zr = given(zrep)
    xas, nets = [], []
    for i in range(n_blocks(par)):
        xa = _add(x, _fwd(ar, zr, weight(par, f"phi.lin_z.{i}"), par[f"phi.lin_z.{i}.bias"]))
        net = _fwd(ar, _relu(xa), weight(par, f"phi.blocks.{i}.fc_0"), par[f"phi.blocks.{i}.fc_0.bias"])
        x = _add(xa, _fwd(ar, _relu(net), weight(par, f"phi.blocks.{i}.fc_1"), par[f"phi.blocks.{i}.fc_1.bias"]))
        xas.append(xa)
        nets.append(net)
    out = _fwd(ar, _relu(x), weight(par, "phi.lin_out"), par["phi.lin_out.bias"])
    m = valid.reshape(-1, 1).to(out[0].dtype)
    b, R = valid.shape[:2]
    rgb = ((out[0][:, :3] * m + (1 - m)).reshape(b, R, 3), (out[1][:, :3] * m.double() + (1 - m.double())).reshape(b, R, 3))
    return dict(xas=xas, nets=nets, dec_out=x, out=out, rgb=rgb)


def decode_adjoint(sv, par, d_rgb, ar: Arith = REF, G: Optional[Grads] = None):
    """Adjoint of decode at the record: d_rgb [b, R, 3] (None: zeros) -> (d z [bR, Dl] pair — the V copies' cotangents summed —, G with
    every phi.* gradient)."""
    G = Grads(par, ar.dtype) if G is None else G
    dt = ar.dtype
    z = sizes(sv)
    V, bR = z["V"], z["bR"]
    Dl = sv["zrep"].shape[1] // V
    m = sv["valid"].reshape(bR, 1)
    d_rgb = torch.zeros(bR, 3) if d_rgb is None else d_rgb.reshape(bR, 3)
    Wo = weight(par, "phi.lin_out")
    d_out = (torch.zeros(bR, Wo.shape[0], dtype=dt), torch.zeros(bR, Wo.shape[0], dtype=F64))
    d_out[0][:, :3] = d_rgb.to(dt) * m.to(dt)
    d_out[1][:, :3] = _abs(d_rgb) * _abs(m)
    _wg(ar, G, "phi.lin_out", d_out, sv["dec_out"], relu=True)
    d_x = _dx(ar, d_out, Wo, act=sv["dec_out"])
    d_zrep = None
    for i in reversed(range(n_blocks(par))):
        xa, net = sv["xas"][i], sv["nets"][i]
        _wg(ar, G, f"phi.blocks.{i}.fc_1", d_x, net, relu=True)
        d_net = _dx(ar, d_x, weight(par, f"phi.blocks.{i}.fc_1"), act=net)
        _wg(ar, G, f"phi.blocks.{i}.fc_0", d_net, xa, relu=True)
        d_x = _add(d_x, _dx(ar, d_net, weight(par, f"phi.blocks.{i}.fc_0"), act=xa))
        _wg(ar, G, f"phi.lin_z.{i}", d_x, sv["zrep"])
        t = _dx(ar, d_x, weight(par, f"phi.lin_z.{i}"))
        d_zrep = t if d_zrep is None else _add(d_zrep, t)
    _wg(ar, G, "phi.lin_in", d_x, sv["phi_x"])
    d_z = (d_zrep[0][:, :Dl], d_zrep[1][:, :Dl])
    for v in range(1, V):
        d_z = _add(d_z, (d_zrep[0][:, v * Dl:(v + 1) * Dl], d_zrep[1][:, v * Dl:(v + 1) * Dl]))
    return d_z, G


# ---- attention rounds ----------------------------------------------------------------------------------------------------------------------------
def _rays(x, z):
    """[S, ...] sample rows -> [b, R, V P, ...]."""
    return AR.ray_major(x.reshape(z["n"], z["R"], z["P"], *x.shape[1:]), z["b"], z["V"])


def _samples(x, z):
    """[b, R, V P, ...] -> [S, ...] (the inverse of _rays)."""
    y = AR.view_major(x, z["b"], z["V"])
    return y.reshape(z["S"], *y.shape[3:])


def softmax_weights(key, q, z):
    """The ray softmax of <key, q> / 16 -> w [b V, R, P]."""
    return AR.view_major(torch.softmax(_rays((key * q).sum(-1) / 16.0, z), dim=-1), z["b"], z["V"])


def attend(w, e, z, dtype=F64):
    """sum_s w_s e_s per ray in `dtype`: w [b V, R, P] given, e a pair [S, Ce] -> pair [bR, Ce]."""
    wr = _rays(w.reshape(-1), z)
    ebar = (wr.to(dtype)[..., None] * _rays(e[0], z).to(dtype)).sum(2)
    B = (wr.detach().double()[..., None] * _rays(e[1], z)).sum(2)
    return ebar.reshape(z["bR"], -1), B.reshape(z["bR"], -1)


def depth_readout(w, pt, poses, z):
    """The first round's depth: clamp(m[:3] . sum_s w_s clamp(pt_s, +-100) + m[3], 0, 10), m the last row of inv_q -> (depth [b, R], zc)."""
    zc, _, _, _ = AR._depth_terms(_rays(w.reshape(-1), z).double(), pt, inv_q_of(poses, z["V"]), z["b"], z["V"])
    return zc.clamp(0.0, AR.DEPTH_MAX), zc


def ray_of_rows(z):
    """[S] int64: the ray (row of a [bR, .] tensor) of every sample row."""
    sc = torch.arange(z["n"]) // z["V"]
    return (sc[:, None, None] * z["R"] + torch.arange(z["R"])[None, :, None]).expand(z["n"], z["R"], z["P"]).reshape(-1)


def reduce_samples(d, z):
    """car_reduce_samples: d [S, C] -> [bR, C], the sum over the V P samples of a ray."""
    return _rays(d, z).sum(2).reshape(z["bR"], -1)


def attention_rounds(par, sv_in, repeat: bool, ar: Arith = REF, weights=None) -> dict:
    """staged._attention_rounds' training form from e [S, Ce], g [S, 16], q, key [S, 128], pt, poses, pixel_val and valid (sizes only).
    weights = (at_wt, at_wt2): the softmax weights taken as given (the record's: how the record's averages are tied to their own
    inputs); None: the softmax of the logits.  -> at_wt, at_wt2 (tensors), depth [b, R], and pairs ebar1, z1, hb, k1r, key2, ebar2, zrep."""
    z = sizes(sv_in)
    V = z["V"]
    e, g, q, key = given(sv_in["e"]), given(sv_in["g"]), sv_in["q"], sv_in["key"]
    Wv, bv = weight(par, "latent_value"), par["latent_value.bias"]
    at_wt = softmax_weights(key, q, z) if weights is None else weights[0]
    out = dict(at_wt=at_wt, at_wt2=None, depth=depth_readout(at_wt, sv_in["pt"], sv_in["poses"], z)[0])
    ebar1 = out["ebar1"] = attend(at_wt, e, z, ar.dtype)
    if repeat:
        Wr, br = weight(par, "query_repeat_embed"), par["query_repeat_embed.bias"]
        z1 = out["z1"] = _fwd(ar, ebar1, Wv, bv)
        hb = out["hb"] = _fwd(ar, z1, weight(par, "encode_latent"), par["encode_latent.bias"])
        uh = _fwd(ar, hb, Wr[:, :128], None)
        ug = _fwd(ar, g, Wr[:, 128:], br)
        rows = ray_of_rows(z)
        k1r = out["k1r"] = _relu(_add(ug, (uh[0][rows], uh[1][rows])))
        key2 = out["key2"] = _fwd(ar, k1r, weight(par, "query_repeat_embed_2"), par["query_repeat_embed_2.bias"])
        at_wt2 = out["at_wt2"] = softmax_weights(key2[0], q, z) if weights is None else weights[1]
        ebar2 = out["ebar2"] = attend(at_wt2, e, z, ar.dtype)
        zl = _add((float(V) * z1[0], float(V) * z1[1]), _fwd(ar, ebar2, Wv, bv))
    else:
        zl = _fwd(ar, ebar1, Wv, bv)
    out["zrep"] = (zl[0].repeat(1, V), zl[1].repeat(1, V))
    return out


def attend_adjoint(ar: Arith, w, e, dz, z, ddepth=None, pt=None, poses=None):
    """car_attend_backward in the run's dtype, `w` taken as given: a_s = <dz, e_s> + ddepth [0 < zc < 10] m[:3] . clamp(pt_s),
    dlogit_s = w_s (a_s - sum_t w_t a_t), dval_s = w_s dz; bounds as attention_reference.backward's with dz's bound in |dz|'s place.
    dz a pair [bR, D], ddepth [bR] or None -> (dlogit [S] pair, dval [S, D] pair)."""
    dt = ar.dtype
    b, R = z["b"], z["R"]
    D = e.shape[1]
    w64 = _rays(w.reshape(-1), z).double()
    wr, vr = w64.to(dt), _rays(e, z)
    dzv, dzB = dz[0].reshape(b, R, 1, D), dz[1].reshape(b, R, 1, D)
    a = (vr.to(dt) * dzv).sum(-1)
    Ba = (vr.double().abs() * dzB).sum(-1)
    if ddepth is not None:
        zc, _, mp, mp_abs = AR._depth_terms(w64, pt, inv_q_of(poses, z["V"]), b, z["V"])
        dd = torch.where((zc > 0.0) & (zc < AR.DEPTH_MAX), ddepth.reshape(b, R).double(), torch.zeros_like(zc))
        a = a + (dd[..., None] * mp).to(dt)
        Ba = Ba + _abs(ddepth).reshape(b, R, 1) * mp_abs
    dl = wr * (a - (wr * a).sum(-1, keepdim=True))
    Bl = w64 * (Ba + (w64 * Ba).sum(-1, keepdim=True))
    return (_samples(dl, z), _samples(Bl, z)), (_samples(wr[..., None] * dzv, z), _samples(w64[..., None] * dzB, z))


def _scaled(dlogit, x, scale=1.0 / 16.0):
    """car_scale_rows: scale dlogit[m] x[m, :]."""
    return dlogit[0][:, None] * x.to(dlogit[0].dtype) * scale, dlogit[1][:, None] * _abs(x) * scale


def attention_rounds_adjoint(sv, par, d_z, d_depth, repeat: bool, ar: Arith = REF, G: Optional[Grads] = None):
    """Adjoint of attention_rounds at the record: d_z [bR, Dl] (the cotangent of the latent z), d_depth [bR] or None ->
    (d e [S, Ce], d key [S, 128], d q [S, 128] pairs, G with latent_value and, with the second round, query_repeat_embed,
    query_repeat_embed_2 and encode_latent)."""
    G = Grads(par, ar.dtype) if G is None else G
    z = sizes(sv)
    V = z["V"]
    d_z = given(d_z, ar.dtype)
    Wv = weight(par, "latent_value")
    e = sv["e"]
    d_e = d_q = None
    if repeat:
        Wr = weight(par, "query_repeat_embed")
        _wg(ar, G, "latent_value", d_z, sv["ebar2"])
        dlogit, d_e = attend_adjoint(ar, sv["at_wt2"], e, _dx(ar, d_z, Wv), z)
        d_key2, d_q = _scaled(dlogit, sv["q"]), _scaled(dlogit, sv["key2"])
        _wg(ar, G, "query_repeat_embed_2", d_key2, sv["k1r"])
        d_k1r = _dx(ar, d_key2, weight(par, "query_repeat_embed_2"), act=sv["k1r"])
        _wg(ar, G, "query_repeat_embed", d_k1r, sv["g"], col0=128, K=16)
        d_uh = (reduce_samples(d_k1r[0], z), reduce_samples(d_k1r[1], z))
        _wg(ar, G, "query_repeat_embed", d_uh, sv["hb"], col0=0, K=128, bias=False)
        d_hb = _dx(ar, d_uh, Wr[:, :128])
        _wg(ar, G, "encode_latent", d_hb, sv["z1"])
        # d z1 = V d z + d hb W; the first round takes it as given, as a stage takes its input cotangent (backward() says why): carried
        # through the second round's softmax the bound of d z1 is some 10^5 times its value, and the first round's results would be
        # judged against a scale no error of theirs could reach
        d_z = given(_add((float(V) * d_z[0], float(V) * d_z[1]), _dx(ar, d_hb, weight(par, "encode_latent")))[0])
    _wg(ar, G, "latent_value", d_z, sv["ebar1"])
    dlogit, dval = attend_adjoint(ar, sv["at_wt"], e, _dx(ar, d_z, Wv), z, d_depth, sv["pt"], sv["poses"])
    d_e = dval if d_e is None else _add(d_e, dval)
    d_key, dq1 = _scaled(dlogit, sv["q"]), _scaled(dlogit, sv["key"])
    d_q = dq1 if d_q is None else _add(d_q, dq1)
    return d_e, d_key, d_q, G


# ---- keys and queries ----------------------------------------------------------------------------------------------------------------------------
def keys_and_queries(par, e, g, ar: Arith = REF) -> dict:
    """staged._keys_and_queries' five-launch form -> pairs k1, key, q1, q."""
    k1 = _relu(_fwd(ar, given(e), weight(par, "key_map"), par["key_map.bias"]))
    q1 = _relu(_fwd(ar, given(g), weight(par, "query_embed"), par["query_embed.bias"]))
    return dict(k1=k1, key=_fwd(ar, k1, weight(par, "key_map_2"), par["key_map_2.bias"]), q1=q1,
                q=_fwd(ar, q1, weight(par, "query_embed_2"), par["query_embed_2.bias"]))


def keys_and_queries_adjoint(sv, par, d_e, d_key, d_q, ar: Arith = REF, G: Optional[Grads] = None):
    """Adjoint of keys_and_queries at the record -> (d e with key_map's data gradient added, G with the four layers)."""
    G = Grads(par, ar.dtype) if G is None else G
    d_e, d_key, d_q = given(d_e, ar.dtype), given(d_key, ar.dtype), given(d_q, ar.dtype)
    _wg(ar, G, "key_map_2", d_key, sv["k1"])
    d_k1 = _dx(ar, d_key, weight(par, "key_map_2"), act=sv["k1"])
    _wg(ar, G, "key_map", d_k1, sv["e"])
    d_e = _add(d_e, _dx(ar, d_k1, weight(par, "key_map")))
    _wg(ar, G, "query_embed_2", d_q, sv["q1"])
    _wg(ar, G, "query_embed", _dx(ar, d_q, weight(par, "query_embed_2"), act=sv["q1"]), sv["g"])
    return d_e, G


# ---- the four ways of making e -------------------------------------------------------------------------------------------------------------------
def shapes_of(maps):
    return [tuple(t.shape[1:]) for t in maps]


def channels(maps) -> int:
    return sum(t.shape[3] for t in maps)


def _grid(t, n):
    return t.detach().reshape(n, -1, 2).float()


def _placed(val, rows, n_rows):
    """Gathered rows (a pair, in (map, point) order) at the rows of their placement; every other row zero."""
    rows = rows.reshape(-1)
    return tuple(torch.zeros(n_rows, t.shape[1], dtype=t.dtype).index_copy(0, rows, t) for t in val)


def _with_points(feat, ptcols):
    """features ‖ point channels (taken as given: the geometry is not differentiated)."""
    return torch.cat([feat[0], ptcols.to(feat[0].dtype)], 1), torch.cat([feat[1], _abs(ptcols)], 1)


def point_mlp(par, rows, ar: Arith = REF):
    """query_encode_latent -> relu -> query_encode_latent_2 over the rows (a pair [M, >= C + 3]) -> pairs h1 [M, C], enc [M, C / 2]."""
    h1 = _relu(_fwd(ar, rows, weight(par, "query_encode_latent"), par["query_encode_latent.bias"]))
    return h1, _fwd(ar, h1, weight(par, "query_encode_latent_2"), par["query_encode_latent_2.bias"])


def rows_concat2(maps, pixel_val, grid_other, ptcols, dtype=F64):
    """The input rows of the two-view point MLP [S V, C + 3]: row (sample (m, i)) V + slot holds, in slot m % V, map m's own features at
    pixel_val (border padding) and, in the other slot, the other view's features where this line's points land there (zeros padding:
    gathered from map m' at grid_other[m'] into the rows of m' 's partner), then the point channels."""
    n, pts = maps[0].shape[0], pixel_val[0].numel() // 2
    own = GR.gather_ref(maps, _grid(pixel_val, n), 0, dtype)
    oth = GR.gather_ref(maps, _grid(grid_other, n), 1, dtype)
    feat = _add(_placed(own, GR.rows_of(GR.OWN, 2, n, pts), n * pts * 2), _placed(oth, GR.rows_of(GR.OTHER2, 2, n, pts), n * pts * 2))
    return _with_points(feat, ptcols)


def e_concat2(par, rows, ar: Arith = REF) -> dict:
    """staged._e_concat2's training form from its input rows -> pairs h1, e [S, 2 (C / 2)] (the two slots' encodings side by side)."""
    h1, enc = point_mlp(par, given(rows), ar)
    return dict(h1=h1, e=tuple(t.reshape(t.shape[0] // 2, -1) for t in enc))


def rows_concat3(maps, pixel_val, cross, ptcols, b, dtype=F64):
    """The exchange rows [S 3, C + 3], row (sample, component k): k = 0 the view's own features at its own samples (border), k = 1, 2 of
    context c: view o's features at the grid of `cross` [(c, o, k, grid [b, pts, 2])] (zeros padding); then the point channels."""
    n, V = maps[0].shape[0], 3
    pts = pixel_val[0].numel() // 2
    C = channels(maps)
    own = GR.gather_ref(maps, _grid(pixel_val, n), 0, dtype)
    comp = [[None] * 3 for _ in range(V)]                       # [context][component] -> pair [b, pts, C]
    for c in range(V):
        comp[c][0] = tuple(t.reshape(b, V, pts, C)[:, c] for t in own)
    for c, o, k, grid in cross:
        got = GR.gather_ref([t.reshape(b, V, *t.shape[1:])[:, o] for t in maps], _grid(grid, b), 1, dtype)
        comp[c][k] = tuple(t.reshape(b, pts, C) for t in got)
    feat = tuple(torch.stack([torch.stack([comp[c][k][j] for k in range(3)], 2) for c in range(V)], 1).reshape(n * pts * 3, C) for j in (0, 1))
    return _with_points(feat, ptcols)


def e_concat3(par, rows, ar: Arith = REF) -> dict:
    """staged._encode_three_views' training form from the exchange rows -> pairs h1, e [S, 3 (C / 2)] with e[s, 3 ch + k] = enc[(s, k), ch]."""
    h1, enc = point_mlp(par, given(rows), ar)
    return dict(h1=h1, e=tuple(t.reshape(t.shape[0] // 3, 3, -1).permute(0, 2, 1).reshape(t.shape[0] // 3, -1) for t in enc))


def rows_single(maps, pixel_val, ptcols, dtype=F64):
    """[S, C + 6]: the own features (border padding, plain placement), then the six point channels."""
    return _with_points(GR.gather_ref(maps, _grid(pixel_val, maps[0].shape[0]), 0, dtype), ptcols)


def e_single(par, rows, ar: Arith = REF) -> dict:
    return dict(e=_fwd(ar, given(rows), weight(par, "update_val_merge"), par["update_val_merge.bias"]))


def e_plain(maps, pixel_val, dtype=F64) -> dict:
    """no_latent_concat: the gathered features are e."""
    return dict(e=GR.gather_ref(maps, _grid(pixel_val, maps[0].shape[0]), 0, dtype))


def scatter(ar: Arith, shapes, n, gathers, V, d_rows):
    """The gathers' adjoint through gather_reference: d_rows a pair [rows, >= C] -> [pair [n, H_l, W_l, C_l]] per level."""
    gathers = [(_grid(g, n), mode, place) for g, mode, place in gathers]
    (val,), _ = GR.scatter_runs(shapes, n, gathers, V, d_rows[0], 0, (ar.dtype,))
    _, bound = GR.scatter_runs(shapes, n, gathers, V, d_rows[1], 0, (F64,))
    return list(zip(val, bound))


def point_mlp_adjoint(sv, par, d_enc, need_dz: bool, ar: Arith, G: Grads):
    """query_encode_latent_2, then query_encode_latent; its data gradient over the C feature columns only, and only when asked."""
    C = weight(par, "query_encode_latent_2").shape[1]
    _wg(ar, G, "query_encode_latent_2", d_enc, sv["h1"])
    d_h1 = _dx(ar, d_enc, weight(par, "query_encode_latent_2"), act=sv["h1"])
    _wg(ar, G, "query_encode_latent", d_h1, sv["enc_rows"])
    return _dx(ar, d_h1, weight(par, "query_encode_latent")[:, :C]) if need_dz else None


def e_concat2_adjoint(sv, par, d_e, need_dz: bool, ar: Arith = REF, G: Optional[Grads] = None):
    """-> (the levels' gradients [pair [n, H, W, C_l]] channel-last, or None; G)."""
    G = Grads(par, ar.dtype) if G is None else G
    d_e = given(d_e, ar.dtype)
    z = sizes(sv)
    d_rows = point_mlp_adjoint(sv, par, tuple(t.reshape(z["S"] * 2, -1) for t in d_e), need_dz, ar, G)
    if d_rows is None:
        return None, G
    return scatter(ar, shapes_of(sv["maps"]), z["n"], [(sv["pixel_val"], 0, GR.OWN), (sv["grid_other"], 1, GR.OTHER2)], 2, d_rows), G


def e_concat3_adjoint(sv, par, d_e, need_dz: bool, ar: Arith = REF, G: Optional[Grads] = None):
    G = Grads(par, ar.dtype) if G is None else G
    d_e = given(d_e, ar.dtype)
    z = sizes(sv)
    b, V, S, pts = z["b"], 3, z["S"], z["pts"]
    d_rows = point_mlp_adjoint(sv, par, tuple(t.reshape(S, -1, 3).permute(0, 2, 1).reshape(S * 3, -1) for t in d_e), need_dz, ar, G)
    if d_rows is None:
        return None, G
    shapes = shapes_of(sv["maps"])
    C = channels(sv["maps"])
    rv = tuple(t.reshape(b, V, pts, 3, C) for t in d_rows)
    dmaps = scatter(ar, shapes, z["n"], [(sv["pixel_val"], 0, GR.PLAIN)], V, tuple(t[:, :, :, 0].reshape(S, C) for t in rv))
    dmaps = [tuple(t.clone() for t in lv) for lv in dmaps]
    for c, o, k, grid in sv["cross"]:
        part = scatter(ar, shapes, b, [(grid, 1, GR.PLAIN)], 1, tuple(t[:, c, :, k].reshape(b * pts, C) for t in rv))
        for full, p in zip(dmaps, part):
            for f, q in zip(full, p):
                f.view(b, V, *f.shape[1:])[:, o] += q
    return dmaps, G


def e_single_adjoint(sv, par, d_e, need_dz: bool, ar: Arith = REF, G: Optional[Grads] = None):
    G = Grads(par, ar.dtype) if G is None else G
    d_e = given(d_e, ar.dtype)
    _wg(ar, G, "update_val_merge", d_e, sv["enc_rows"])
    if not need_dz:
        return None, G
    z = sizes(sv)
    d_rows = _dx(ar, d_e, weight(par, "update_val_merge")[:, :channels(sv["maps"])])
    return scatter(ar, shapes_of(sv["maps"]), z["n"], [(sv["pixel_val"], 0, GR.PLAIN)], z["V"], d_rows), G


def e_plain_adjoint(sv, par, d_e, need_dz: bool, ar: Arith = REF, G: Optional[Grads] = None):
    G = Grads(par, ar.dtype) if G is None else G
    if not need_dz:
        return None, G
    z = sizes(sv)
    return scatter(ar, shapes_of(sv["maps"]), z["n"], [(sv["pixel_val"], 0, GR.PLAIN)], z["V"], given(d_e, ar.dtype)), G


E_ADJOINT = {"concat2": e_concat2_adjoint, "concat3": e_concat3_adjoint, "single": e_single_adjoint, "plain": e_plain_adjoint}


def level_grads(dmaps, asks) -> list:
    """Channel-last scatter results -> pairs [n, C, H, W]; None for a level that asked for none."""
    return [tuple(t.permute(0, 3, 1, 2) for t in lv) if ask else None for lv, ask in zip(dmaps, asks)]


# ---- the whole backward, the whole forward -------------------------------------------------------------------------------------------------------
def backward(record, params, d_rgb, d_depth, mode: str, need_dz, ar: Arith = REF):
    """The stage adjoints in the order of training._RenderTrain.backward.  need_dz: one flag, or one per pyramid level.
    Every stage takes the cotangent the previous one hands it as given, as it does on its own: a gradient's bound is composed along the
    stage that writes it and starts from the magnitude of that stage's input cotangent, not from d_rgb's.  (Carried through all four
    stages the sums of magnitudes outgrow the values by ten and more orders of magnitude, and no error would be large against them;
    what the earlier stages' rounding does to a later stage's result is in the yardstick, which runs the same chain.)
    -> ({parameter name: pair in the parameter's shape}, [pair [n, C, H, W] or None per level])."""
    sv, par = record, params
    repeat = sv.get("z1") is not None
    asks = list(need_dz) if isinstance(need_dz, (list, tuple)) else [bool(need_dz)] * len(sv["maps"])
    G = Grads(par, ar.dtype)
    d_z, _ = decode_adjoint(sv, par, d_rgb, ar, G)
    d_e, d_key, d_q, _ = attention_rounds_adjoint(sv, par, d_z[0], d_depth, repeat, ar, G)
    d_e, _ = keys_and_queries_adjoint(sv, par, d_e[0], d_key[0], d_q[0], ar, G)
    dmaps, _ = E_ADJOINT[mode](sv, par, d_e[0], any(asks), ar, G)
    return G.shaped(), [None] * len(asks) if dmaps is None else level_grads(dmaps, asks)


def forward(par, geom, maps, mode: str, repeat: bool, ar: Arith = REF) -> dict:
    """Every stage forward chained from the channel-last pyramid `maps`: geom holds what the geometry hands the stages (pixel_val, g, pt,
    poses, phi_x, valid, the point channels `ptcols` and, per mode, grid_other / cross).  -> a record with staged.Saved's field names
    (values, not pairs) plus rgb [b, R, 3] and depth [b, R]."""
    dt = ar.dtype
    rec = dict(geom, maps=maps, z1=None, hb=None, k1r=None, key2=None, at_wt2=None, ebar2=None, enc_rows=None, h1=None)
    b = geom["valid"].shape[0]
    if mode == "concat2":
        rows = rows_concat2(maps, geom["pixel_val"], geom["grid_other"], geom["ptcols"], dt)
        head = e_concat2(par, rows, ar)
    elif mode == "concat3":
        rows = rows_concat3(maps, geom["pixel_val"], geom["cross"], geom["ptcols"], b, dt)
        head = e_concat3(par, rows, ar)
    elif mode == "single":
        rows = rows_single(maps, geom["pixel_val"], geom["ptcols"], dt)
        head = e_single(par, rows, ar)
    else:
        rows, head = None, e_plain(maps, geom["pixel_val"], dt)
    if rows is not None:
        rec["enc_rows"] = rows[0]
    rec["h1"] = head["h1"][0] if "h1" in head else None
    rec["e"] = head["e"][0]
    rec["Ce"] = rec["e"].shape[1]
    kq = keys_and_queries(par, rec["e"], geom["g"], ar)
    rec.update({k: v[0] for k, v in kq.items()})
    at = attention_rounds(par, rec, repeat, ar)
    rec.update({k: (v[0] if isinstance(v, tuple) else v) for k, v in at.items()})
    dec = decode(par, geom["phi_x"], rec["zrep"], geom["valid"], ar)
    rec.update(xas=[t[0] for t in dec["xas"]], nets=[t[0] for t in dec["nets"]], dec_out=dec["dec_out"][0], rgb=dec["rgb"][0])
    return rec
