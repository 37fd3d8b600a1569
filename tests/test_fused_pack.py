"""Operand packing consumed by csrc/car_fused.hip and csrc/car_round2.hip.

CPU: evaluating a layer exactly the way the MFMA contracts the packed tiles (K step, tile, lane group, element) must reproduce
W x for the standard, bias-folded and chained K mappings (tests/pack_reference.py is the layout's reference statement).
GPU: the device packers of the C ABI (car_fused_pack / car_round2_pack and the per-layer entries car_linear_x3_pack, car_chain_pack,
car_conv3x3_pack, car_conv3x3_backward_pack, all through the kernels of csrc/car_pack.hip) must emit exactly those bytes."""
import ctypes

import pytest
import torch

import abi_harness as abi
import pack_reference as PR
from cross_attention_renderer_amd import synthetic as S
from cross_attention_renderer_amd.models import CrossAttentionRenderer


def _module(seed):
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, npoints=8, with_encoder=False).eval()
    S.perturb_parameters(m, seed=seed)
    return m


def _walk16(tiles, x_of):
    """tiles (ksteps, n_tiles, 2, 64, 8) fp16 halves as floats; x_of(step, lane group q, e) -> B value of that K slot.  Evaluates the
    layer the way v_mfma_f32_16x16x32_f16 contracts it: lane l = 16 q + i holds A[i][8 q + e] and B[8 q + e][.]."""
    ks, nt = tiles.shape[:2]
    y = torch.zeros(16 * nt, dtype=torch.float64)
    w = (tiles[:, :, 0].double() + tiles[:, :, 1].double())                   # hi + lo: (ks, nt, 64, 8)
    for m in range(ks):
        for q in range(4):
            for e in range(8):
                y += w[m, :, 16 * q:16 * q + 16, e].reshape(-1) * x_of(m, q, e)
    return y


def test_fused_blob_layout():
    """Standard, bias-folded and chained K mappings of the 16x16x32 tiles, every layer with its own power of two."""
    from cross_attention_renderer_amd import _lib
    m = _module(1)
    blob, bias, wpt = PR.pack_fused(m)
    lib = _lib.load()
    assert blob.numel() == lib.car_fused_blob_floats() and bias.numel() == lib.car_fused_bias_floats()
    T = 512
    down = {n: bias[672 + i].double().item() for i, n in enumerate(PR.LAYERS)}
    g = torch.Generator().manual_seed(0)
    halves = lambda a, b_, ks, nt: blob[a * T:b_ * T].view(torch.float16).reshape(ks, nt, 2, 64, 8).float()
    chained = lambda x, base=0: (lambda m_, q, e: x[base + 16 * (2 * m_ + e // 4) + 4 * q + e % 4])
    # W2: 18 K steps x 18 tiles, standard
    x = torch.randn(576, generator=g).double()
    y = _walk16(halves(0, 324, 18, 18), lambda m_, q, e: x[32 * m_ + 8 * q + e]) * down["W2"]
    want = m.query_encode_latent_2.weight.detach().reshape(288, 576).double() @ x
    assert (y - want).abs().max() < 1e-5
    # Q1: one K step, lane group 2 element 0 carries the constant 1 of the folded bias
    gq = torch.randn(16, generator=g).double()
    gin = lambda m_, q, e: gq[8 * q + e] if q < 2 else (1.0 if (q == 2 and e == 0) else 0.0)
    y = _walk16(halves(324, 332, 1, 8), gin) * down["Q1"]
    want = m.query_embed.weight.detach().reshape(128, 16).double() @ gq + m.query_embed.bias.detach().double()
    assert (y - want).abs().max() < 1e-5
    # M = Wk2^T Wq2: chained over a 128-wide accumulator set (8 source tiles, 4 K steps); with v, u, c it reproduces <key, qry> of the two
    # closing layers for any pair of hidden vectors (models.py:491, 529, 533)
    x, r = torch.randn(128, generator=g).double(), torch.randn(128, generator=g).double()
    wk2, bk2 = m.key_map_2.weight.detach().reshape(128, 128).double(), m.key_map_2.bias.detach().double()
    wq2, bq2 = m.query_embed_2.weight.detach().reshape(128, 128).double(), m.query_embed_2.bias.detach().double()
    y = _walk16(halves(332, 364, 4, 8), chained(x)) * down["M"]
    assert (y - wk2.T @ wq2 @ x).abs().max() < 1e-5
    folded = r @ (y + bias[288:416].double()) + bias[544:672].double() @ x + bias[678].double()
    assert abs(folded - (wk2 @ r + bk2) @ (wq2 @ x + bq2)) < 1e-4
    # K1: chained over [e_0 ; e_1], 9 K steps per source
    x = torch.randn(576, generator=g).double()
    y = sum(_walk16(halves(364 + 72 * sv, 364 + 72 * (sv + 1), 9, 8), chained(x, 288 * sv)) for sv in range(2)) * down["K1"]
    assert (y - m.key_map.weight.detach().reshape(128, 576).double() @ x).abs().max() < 1e-5
    # bias table order, the point / bias bound of h
    assert torch.equal(bias[:288], m.query_encode_latent_2.bias.detach()) and torch.equal(bias[416:544], m.key_map.bias.detach())
    w1 = m.query_encode_latent.weight.detach().reshape(576, 579)
    assert bias[677] >= (w1[:, 576:].abs().sum(1) + m.query_encode_latent.bias.detach().abs()).max() * (1 - 1e-6)


@pytest.mark.parametrize("scale", [1.0, 1e-4, 3e3])
def test_layer_scale_keeps_the_fp16_halves_normal(scale):
    """Whatever the magnitude of a layer's weights, its packed high halves sit below 2^14 and hi + lo reproduces W 2^shift to
    fp32 accuracy (absolute error below 2^-22 of the largest weight)."""
    m = _module(2)
    with torch.no_grad():
        m.query_encode_latent_2.weight.mul_(scale)
    W = m.query_encode_latent_2.weight.detach().reshape(288, 576)
    p = PR.pow2_scale(W.abs().max().item())
    assert 2 ** 13 <= W.abs().max().item() * p < 2 ** 14
    tiles = PR.pack_tiles16(W, None, 18, PR.std16_k(18), p).view(torch.float16).reshape(18, 18, 2, 64, 8).float()
    assert torch.isfinite(tiles).all() and tiles[:, :, 0].abs().max() < 2 ** 14
    rec = (tiles[:, :, 0] + tiles[:, :, 1]) / p                               # (K step, tile, lane, e)
    n_idx = 16 * torch.arange(18)[:, None] + (torch.arange(64) % 16)[None, :]
    for ks in (0, 7, 17):
        k_idx = 32 * ks + 8 * (torch.arange(64) // 16)[:, None] + torch.arange(8)[None, :]
        want = W[n_idx[:, :, None].expand(18, 64, 8), k_idx[None].expand(18, 64, 8)]
        assert (rec[ks] - want).abs().max() <= 2 ** -22 * W.abs().max()


def test_round2_packing_layout():
    """csrc/car_round2.hip: Wr2 in the accumulator ("chained") K order of the layer before it, then Wr1[:, 128:]; 32x32x16 tiles:
    lane l = 32 h + i holds A[i][8 h + e] and B[8 h + e][.] of a K step (chunk, group kg)."""
    m = _module(3)
    packed, bias = PR.pack_round2(m)
    from cross_attention_renderer_amd import _lib
    lib = _lib.load()
    assert packed.numel() == lib.car_round2_packed_floats() and bias.numel() == lib.car_round2_bias_floats()
    g = torch.Generator().manual_seed(1)
    w2 = packed[:16384].view(torch.float16).reshape(4, 4, 2, 2, 64, 8).double()      # (c, t, kg, hl, lane, e)
    w2 = w2[:, :, :, 0] + w2[:, :, :, 1]
    x = torch.randn(128, generator=g).double()
    y = torch.zeros(128, dtype=torch.float64)
    for c in range(4):
        for kg in range(2):
            for h in range(2):
                for e in range(8):
                    # B element e of lane half h in K step (c, kg) = accumulator register 8 kg + e of source tile c
                    k = 32 * c + (e & 3) + 8 * (2 * kg + (e >> 2)) + 4 * h
                    y += w2[c, :, kg, 32 * h:32 * h + 32, e].reshape(-1) * x[k]
    want = m.query_repeat_embed_2.weight.detach().reshape(128, 128).double() @ x
    assert (y * bias[257].double() - want).abs().max() < 1e-5
    w1 = packed[16384:].view(torch.float16).reshape(4, 2, 64, 8).double()              # (t, hl, lane, e)
    w1 = w1[:, 0] + w1[:, 1]
    gq = torch.randn(16, generator=g).double()
    y = torch.zeros(128, dtype=torch.float64)
    for h in range(2):
        for e in range(8):
            y += w1[:, 32 * h:32 * h + 32, e].reshape(-1) * gq[8 * h + e]
    want = m.query_repeat_embed.weight.detach().reshape(128, 144)[:, 128:].double() @ gq
    assert (y * bias[256].double() - want).abs().max() < 1e-5


def test_round2q_fold_reproduces_the_two_layers():
    """car_round2_logits_from_g's operands: M = Wr2^T Wq2 walked the way the 32x32x16 MFMA contracts the chained tiles, with v, u, c, gives
    <query_repeat_embed_2(y), query_embed_2(x)> for any pair of hidden vectors; the two 16 -> 128 layers sit behind it."""
    m = _module(5)
    packed, bias = PR.pack_round2q(m)
    from cross_attention_renderer_amd import _lib
    lib = _lib.load()
    assert packed.numel() == lib.car_round2q_packed_floats() and bias.numel() == lib.car_round2q_bias_floats()
    g = torch.Generator().manual_seed(2)
    wm = packed[:16384].view(torch.float16).reshape(4, 4, 2, 2, 64, 8).double()      # (c, t, kg, hl, lane, e)
    wm = wm[:, :, :, 0] + wm[:, :, :, 1]
    x, y = torch.randn(128, generator=g).double().abs(), torch.randn(128, generator=g).double().abs()
    t = torch.zeros(128, dtype=torch.float64)
    for c in range(4):
        for kg in range(2):
            for h in range(2):
                for e in range(8):
                    k = 32 * c + (e & 3) + 8 * (2 * kg + (e >> 2)) + 4 * h
                    t += wm[c, :, kg, 32 * h:32 * h + 32, e].reshape(-1) * x[k]
    t = t * bias[513].double() + bias[128:256].double()                                  # M x + v
    folded = y @ t + bias[384:512].double() @ x + bias[515].double()
    wr2, br2 = m.query_repeat_embed_2.weight.detach().reshape(128, 128).double(), m.query_repeat_embed_2.bias.detach().double()
    wq2, bq2 = m.query_embed_2.weight.detach().reshape(128, 128).double(), m.query_embed_2.bias.detach().double()
    assert abs(folded - (wr2 @ y + br2) @ (wq2 @ x + bq2)) < 1e-4
    gq = torch.randn(16, generator=g).double()
    for off, slot, W in ((16384, 512, m.query_repeat_embed.weight.detach().reshape(128, 144)[:, 128:]), (16384 + 2048, 514, m.query_embed.weight.detach().reshape(128, 16))):
        w1 = packed[off:off + 2048].view(torch.float16).reshape(4, 2, 64, 8).double()  # (t, hl, lane, e)
        w1 = w1[:, 0] + w1[:, 1]
        yy = torch.zeros(128, dtype=torch.float64)
        for h in range(2):
            for e in range(8):
                yy += w1[:, 32 * h:32 * h + 32, e].reshape(-1) * gq[8 * h + e]
        assert (yy * bias[slot].double() - W.double() @ gq).abs().max() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 2e-4, 5e3, 0.0])
def test_device_packers_emit_the_reference_bytes(scale):
    from cross_attention_renderer_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    m = _module(4)
    with torch.no_grad():
        if scale == 0.0:                       # an all-zero layer: the clamp of the power-of-two rule (2^43, not 2^113)
            m.query_encode_latent_2.weight.zero_()
        else:
            for p_ in (m.query_encode_latent_2.weight, m.key_map.weight, m.query_embed.bias, m.query_repeat_embed_2.weight):
                p_.mul_(scale)
    blob, bias, wpt = PR.pack_fused(m)
    r2w, r2b = PR.pack_round2(m)
    keep = []

    def d(t):
        t = t.detach().float().reshape(t.shape[0], -1).contiguous().to(dev) if t.dim() > 1 else t.detach().float().contiguous().to(dev)
        keep.append(t)
        return t.data_ptr()
    w = _lib.CarWeights()
    for n in _lib.WEIGHT_FIELDS[0]:
        mod = m
        for part in n.split("."):
            mod = getattr(mod, part)
        setattr(w, f"{n.replace('.', '_')}_w", d(mod.weight))
        setattr(w, f"{n.replace('.', '_')}_b", d(mod.bias))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dblob, dbias, dwpt = torch.empty_like(blob, device=dev), torch.empty_like(bias, device=dev), torch.empty(576 * 4, device=dev)
    rc = lib.car_fused_pack(ctypes.byref(w), dblob.data_ptr(), dbias.data_ptr(), dwpt.data_ptr(), st)
    assert rc == 0, lib.car_last_error()
    dr2w, dr2b = torch.empty_like(r2w, device=dev), torch.empty_like(r2b, device=dev)
    rc = lib.car_round2_pack(w.query_repeat_embed_w, w.query_repeat_embed_b, w.query_repeat_embed_2_w, w.query_repeat_embed_2_b,
                             dr2w.data_ptr(), dr2b.data_ptr(), st)
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dblob.cpu().view(torch.int32), blob.view(torch.int32))
    assert torch.equal(dbias.cpu(), bias)
    assert torch.equal(dwpt.cpu().view(576, 4), wpt)
    assert torch.equal(dr2w.cpu().view(torch.int32), r2w.view(torch.int32))
    assert torch.equal(dr2b.cpu(), r2b)
    # the folded layer and the two 16 -> 128 layers car_round2_logits_from_g reads
    r2qw, r2qb = PR.pack_round2q(m)
    assert r2qw.numel() == lib.car_round2q_packed_floats() and r2qb.numel() == lib.car_round2q_bias_floats()
    dqw, dqb = torch.empty_like(r2qw, device=dev), torch.empty_like(r2qb, device=dev)
    rc = lib.car_round2q_pack(w.query_repeat_embed_w, w.query_repeat_embed_b, w.query_repeat_embed_2_w, w.query_repeat_embed_2_b,
                              w.query_embed_w, w.query_embed_b, w.query_embed_2_w, w.query_embed_2_b, dqw.data_ptr(), dqb.data_ptr(), st)
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dqw.cpu().view(torch.int32), r2qw.view(torch.int32))
    assert torch.equal(dqb.cpu(), r2qb)
    # the fp16 precision's plan (car_plan_f16_build): compact blob | bias table | point table, each rounded up to 64 floats; the compact blob
    # holds exactly the hi halves of car_fused_pack's tiles, in the same order (508 tiles, every one written).  The offsets restate
    # car_render.hip's plan16_layout by hand (as tools/bench_fused.py does); the size query below checks the restatement
    up64 = lambda n: (n + 63) & ~63
    dims = _lib.CarDims()
    dims.b, dims.V, dims.R, dims.P, dims.H, dims.W, dims.n_levels, dims.repeat_attention = 1, 2, 64, 8, 64, 64, 3, 1
    for l, (c, h) in enumerate(((256, 16), (256, 32), (64, 64))):
        dims.level_c[l], dims.level_h[l], dims.level_w[l] = c, h, h
    n16 = lib.car_plan_f16_bytes(ctypes.byref(dims)) // 4
    o_bias = up64(508 * 256)
    o_wpt = o_bias + up64(bias.numel())
    assert n16 == o_wpt + up64(576 * 4), lib.car_last_error()
    p16 = torch.zeros(n16, device=dev)
    rc = lib.car_plan_f16_build(ctypes.byref(dims), ctypes.byref(w), p16.data_ptr(), st)
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    p16 = p16.cpu()
    hi16 = p16[:508 * 256].view(torch.int16).view(508, 512)
    assert torch.equal(hi16, dblob.cpu().view(torch.int16).view(508, 2, 512)[:, 0])
    assert torch.equal(p16[o_bias:o_bias + bias.numel()].view(torch.int32), dbias.cpu().view(torch.int32))
    assert torch.equal(p16[o_wpt:o_wpt + 576 * 4].view(torch.int32), dwpt.cpu().view(torch.int32))
    # car_fused_pack_rows (the first two point-MLP layers alone) into zeroed buffers: W2's 324 tiles, the point table, b2 and the scale slots
    # 0 (2^-shift of W2), 5 (the point / bias bound), 8 (2^shift of W2) as car_fused_pack leaves them; everything else it owns stays zero
    rblob, rbias, rwpt = torch.zeros_like(dblob), torch.zeros_like(dbias), torch.zeros_like(dwpt)
    rc = lib.car_fused_pack_rows(w.query_encode_latent_w, w.query_encode_latent_b, w.query_encode_latent_2_w, w.query_encode_latent_2_b,
                                 rblob.data_ptr(), rbias.data_ptr(), rwpt.data_ptr(), st)
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    want_blob = torch.zeros_like(blob).view(torch.int32)
    want_blob[:324 * 512] = dblob.cpu().view(torch.int32)[:324 * 512]
    assert torch.equal(rblob.cpu().view(torch.int32), want_blob)
    assert torch.equal(rwpt.cpu().view(torch.int32), dwpt.cpu().view(torch.int32))
    want_bias = torch.zeros_like(bias).view(torch.int32)
    for lo, hi in ((0, 288), (672 + 0, 672 + 1), (672 + 5, 672 + 6), (672 + 8, 672 + 9)):
        want_bias[lo:hi] = dbias.cpu().view(torch.int32)[lo:hi]
    assert torch.equal(rbias.cpu().view(torch.int32), want_bias)
    # car_kq_pack (the stage route's key / query chain): K2 (32 tiles) | Q1 (8) | Q2 (32) in the fused kernel's operand formats, K2 and Q2
    # chained over the accumulator order of the layer before, Q1 standard with its bias folded in at k = 16;
    # bias = bk2 | bq2 | 2^-shift of K2, Q1, Q2 (slots 0..2) and their 2^shift (slots 8..10, the packer's scratch), zeros between
    f = lambda t: t.detach().float().cpu().reshape(t.shape[0], -1)
    v = lambda t: t.detach().float().cpu()
    k2, q1, q2 = f(m.key_map_2.weight), f(m.query_embed.weight), f(m.query_embed_2.weight)
    pk2 = PR.pow2_scale(k2.abs().max().item())
    pq1 = PR.pow2_scale(max(q1.abs().max().item(), v(m.query_embed.bias).abs().max().item()))
    pq2 = PR.pow2_scale(q2.abs().max().item())
    tail = torch.cat([PR.pack_tiles16(k2, None, 8, PR.chained16_k(4), pk2).reshape(-1),
                      PR.pack_tiles16(q1, v(m.query_embed.bias), 8, PR.std16_k(1), pq1).reshape(-1),
                      PR.pack_tiles16(q2, None, 8, PR.chained16_k(4), pq2).reshape(-1)])
    scales = torch.zeros(16)
    scales[0:3] = torch.tensor([1.0 / pk2, 1.0 / pq1, 1.0 / pq2])
    scales[8:11] = torch.tensor([pk2, pq1, pq2])
    kqb = torch.cat([v(m.key_map_2.bias), v(m.query_embed_2.bias), scales])
    assert tail.numel() == lib.car_kq_tail_floats() and kqb.numel() == lib.car_kq_bias_floats()
    dtail, dkqb = torch.empty_like(tail, device=dev), torch.empty_like(kqb, device=dev)
    rc = lib.car_kq_pack(w.key_map_2_w, w.key_map_2_b, w.query_embed_w, w.query_embed_b, w.query_embed_2_w, w.query_embed_2_b,
                         dtail.data_ptr(), dkqb.data_ptr(), st)
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dtail.cpu().view(torch.int32), tail.view(torch.int32))
    assert torch.equal(dkqb.cpu().view(torch.int32), kqb.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 2e-4, 5e3, 0.0])
@pytest.mark.parametrize("K,N,ldw", [(64, 32, 64), (72, 48, 80), (576, 288, 579)])
def test_linear_x3_pack_emits_the_reference_bytes(K, N, ldw, scale):
    """car_linear_x3_pack: ceil(K / 32) x N / 16 standard tiles of the 16-wide format read out of a matrix with row stride ldw (K no
    multiple of 32: zeros behind it), then 2^shift, 2^-shift.  scale 0.0: an all-zero matrix, the clamp of the power-of-two rule."""
    from cross_attention_renderer_amd import _lib
    lib = _lib.load()
    W = torch.randn(N, ldw, generator=torch.Generator().manual_seed(K + N)) * scale
    p = PR.pow2_scale(W[:, :K].abs().max().item())
    ksteps = (K + 31) // 32
    want = PR.pack_tiles16(W[:, :K], None, N // 16, PR.std16_k(ksteps), p).reshape(-1)
    n = int(lib.car_linear_x3_packed_floats(K, N))
    assert n == want.numel() + 64
    dW, packed = W.to("cuda:0"), torch.full((n,), float("nan"), device="cuda:0")
    rc = lib.car_linear_x3_pack(dW.data_ptr(), ldw, K, N, packed.data_ptr(), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert torch.equal(abi.bits(packed[:want.numel()].cpu()), abi.bits(want))
    assert torch.equal(abi.bits(packed[want.numel():want.numel() + 2].cpu()), abi.bits(torch.tensor([p, 1.0 / p])))


@pytest.mark.gpu
@pytest.mark.parametrize("K,N,chained,twice", [(18, 128, 0, False), (128, 3, 1, False), (288, 128, 1, True)])
def test_chain_pack_emits_the_reference_bytes(K, N, chained, twice):
    """car_chain_pack: ceil(K / 32) x ceil(N / 32) tiles of the 32-wide format with two K groups, standard or chained K order, outputs
    >= N and inputs >= K zero; twice: W2 = the matrix's second K columns (row stride 2 K) added before the power of two, as lin_z is
    packed.  The layer's 2^shift / 2^-shift land in its slot of the 32 shared floats and nowhere else."""
    from cross_attention_renderer_amd import _lib
    lib = _lib.load()
    ldw = 2 * K if twice else K
    Wfull = torch.randn(N, ldw, generator=torch.Generator().manual_seed(K + N))
    W, W2 = Wfull[:, :K], (Wfull[:, K:] if twice else None)
    p = PR.pow2_scale((W + W2 if twice else W).abs().max().item())
    chunks, tiles, slot = (K + 31) // 32, (N + 31) // 32, 5
    want = PR.pack_tiles32(W, chunks, 2, bool(chained), p, tiles=tiles, W2=W2)
    assert want.numel() == int(lib.car_chain_packed_floats(K, N))
    dW = Wfull.to("cuda:0")
    packed = torch.full((want.numel(),), float("nan"), device="cuda:0")
    scales = torch.full((32,), float("nan"), device="cuda:0")
    rc = lib.car_chain_pack(dW.data_ptr(), ldw, dW.data_ptr() + 4 * K if twice else None, K, N, chained, packed.data_ptr(), scales.data_ptr(), slot,
                            abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert torch.equal(abi.bits(packed.cpu()), abi.bits(want))
    scales = scales.cpu()
    assert scales[slot].item() == p and scales[16 + slot].item() == 1.0 / p
    others = torch.ones(32, dtype=torch.bool)
    others[[slot, 16 + slot]] = False
    assert bool(torch.isnan(scales[others]).all())


@pytest.mark.gpu
def test_conv3x3_packs_emit_the_reference_bytes():
    """car_conv3x3_pack (K, N) = (64, 64): standard 16-wide tiles over k = tap * K + channel of torch's [N][K][3][3], 64 scale floats
    (2^shift, 2^-shift, the largest magnitude, zeros), the bias.  car_conv3x3_backward_pack (64, 128): the data gradient's matrix
    w'[k][tap * N + n] = w[n][k][8 - tap] (transposed, taps flipped) in the same tiles, then its 64 scale floats."""
    from cross_attention_renderer_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(7)

    def scale_floats(Wm):
        p = PR.pow2_scale(Wm.abs().max().item())
        s = torch.zeros(64)
        s[0], s[1], s[2] = p, 1.0 / p, Wm.abs().max()
        return p, s
    K, N = 64, 64
    w, b = torch.randn(N, K, 3, 3, generator=g) * 0.05, torch.randn(N, generator=g)
    Wm = w.permute(0, 2, 3, 1).reshape(N, 9 * K)
    p, s = scale_floats(Wm)
    want = torch.cat([PR.pack_tiles16(Wm, None, N // 16, PR.std16_k(9 * K // 32), p).reshape(-1), s, b])
    assert want.numel() == int(lib.car_conv3x3_packed_floats(K, N))
    dw, db, packed = w.to("cuda:0"), b.to("cuda:0"), torch.full((want.numel(),), float("nan"), device="cuda:0")
    rc = lib.car_conv3x3_pack(dw.data_ptr(), db.data_ptr(), K, N, packed.data_ptr(), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert torch.equal(abi.bits(packed.cpu()), abi.bits(want))
    K, N = 64, 128
    w = torch.randn(N, K, 3, 3, generator=g) * 0.05
    Wm = w.flip(2, 3).permute(1, 2, 3, 0).reshape(K, 9 * N)
    p, s = scale_floats(Wm)
    want = torch.cat([PR.pack_tiles16(Wm, None, K // 16, PR.std16_k(9 * N // 32), p).reshape(-1), s])
    assert want.numel() == int(lib.car_conv3x3_backward_packed_floats(K, N))
    dw, packed = w.to("cuda:0"), torch.full((want.numel(),), float("nan"), device="cuda:0")
    rc = lib.car_conv3x3_backward_pack(dw.data_ptr(), K, N, packed.data_ptr(), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert torch.equal(abi.bits(packed.cpu()), abi.bits(want))
