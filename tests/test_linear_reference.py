"""CPU checks of tests/linear_reference.py, the checker of tests/test_linear_hip.py: the float64 layer, chain and weight gradient against
torch.nn.functional.linear, torch modules and autograd; the split-fp16 and bf16 emulations exact where their operands are exactly
representable, and no longer exact when one of their three products is dropped; car_linear_pack's index formula against a loop written
from the kernel's comment; the restated launch rules on every shape the GPU file runs — each on the path its name says, a rule moved
by one block noticed; and every input set holds what it exists for."""
import pytest
import torch
import torch.nn.functional as F

import linear_reference as LR

F32, F64 = torch.float32, torch.float64
ULP64 = 2.0 ** -53
FLAG_SETS = [f for f in range(8)]                                     # RELU_IN | RELU_OUT | ACCUM in every combination


# ---- the float64 restatement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_float64_layer_is_torch_linear(flags):
    """layer() against F.linear in float64 with the flags applied from the header's sentence Y = act(act_in(X) W^T + bias (+ Y)): the two
    differ by the order of a K-term float64 sum at most, (K + 2) 2^-53 of the bound; padding columns of X never enter."""
    M, K, N = 37, 67, 21
    X, W, b, Y0 = LR.linear_set("gauss", M, K, N, 5)
    Xp = LR.padded(X, K + 5)
    y, B = LR.layer(Xp, W, b, Y0, flags)
    x = X.double().clamp_min(0) if flags & LR.RELU_IN else X.double()
    want = F.linear(x, W.double(), b.double())
    if flags & LR.ACCUM:
        want = want + Y0.double()
    if flags & LR.RELU_OUT:
        want = want.clamp_min(0)
    assert LR.ratio(y, want, B) <= (K + 2) * ULP64
    assert bool((B >= want.abs() * (1 - 1e-12)).all())
    # the bound itself: every term's magnitude once
    Bw = x.abs() @ W.double().abs().T + b.double().abs() + (Y0.double().abs() if flags & LR.ACCUM else 0)
    assert torch.allclose(B, Bw, rtol=1e-14, atol=0)
    y0, B0 = LR.layer(Xp, W, None, Y0, flags & ~LR.ACCUM)
    assert bool((B0 <= B).all())


@pytest.mark.parametrize("relu", [False, True])
def test_float64_wgrad_is_autograd(relu):
    """wgrad() against torch autograd through F.linear(act(X), W, b) in float64: (M + 2) 2^-53 of the bound."""
    M, N, K = 53, 19, 23
    dY, X, dW0, db0 = LR.wgrad_set("gauss", M, N, K, 3)
    W = torch.zeros(N, K, dtype=F64, requires_grad=True)
    b = torch.zeros(N, dtype=F64, requires_grad=True)
    x = X.double().clamp_min(0) if relu else X.double()
    F.linear(x, W, b).backward(dY.double())
    dW, db, BW, Bb = LR.wgrad(LR.padded(dY, N + 5), LR.padded(X, K + 1), relu, dW0, db0)
    assert LR.ratio(dW, dW0.double() + W.grad, BW) <= (M + 2) * ULP64
    assert LR.ratio(db, db0.double() + b.grad, Bb) <= (M + 2) * ULP64
    dW2, db2, _, Bb2 = LR.wgrad(dY, X, relu, dW0, None)
    assert db2 is None and Bb2 is None and torch.equal(dW2, dW)


def test_unfolded_chain_is_the_torch_modules():
    """kq_chain() against nn.Linear / nn.ReLU modules in float64, and its bounds: B_key of a row whose k1 is negative throughout is |bk2|."""
    M, Ce = 9, 100
    P = LR.kq_params(Ce, 11)
    e, g = LR.kq_rows(M, Ce, 12)

    def mod(W, b):
        m = torch.nn.Linear(W.shape[1], W.shape[0]).double()
        m.weight.data, m.bias.data = W.double(), b.double()
        return m
    key_map = torch.nn.Sequential(mod(P["Wk1"], P["bk1"]), torch.nn.ReLU(), mod(P["Wk2"], P["bk2"]))
    qry_map = torch.nn.Sequential(mod(P["Wq1"], P["bq1"]), torch.nn.ReLU(), mod(P["Wq2"], P["bq2"]))
    with torch.no_grad():
        key, qry = key_map(e.double()), qry_map(g.double())
    r = LR.kq_chain(LR.padded(e, Ce + 4), g, P)
    assert LR.ratio(r["key"], key, r["B_key"]) <= (Ce + 130) * ULP64 and LR.ratio(r["qry"], qry, r["B_qry"]) <= 150 * ULP64
    assert LR.ratio(r["logit"], (key * qry).sum(-1) / 16, r["B_logit"]) <= 4 * (Ce + 260) * ULP64
    assert bool((r["k1"][0] == 0).all()) and torch.equal(r["B_key"][0], P["bk2"].double().abs())
    assert torch.equal(r["key"][0], P["bk2"].double())
    assert bool((r["B_key"][1:] > P["bk2"].double().abs()).all())
    # the gate never removes an entry that is alive
    pre = F.linear(e.double(), P["Wk1"].double(), P["bk1"].double())
    full = r["B_k1"] @ P["Wk2"].double().abs().T + P["bk2"].double().abs()
    assert bool((r["B_key"] <= full).all()) and bool(((pre > 0).double() @ torch.ones(128, 1, dtype=F64) > 0)[1:].all())


# ---- the emulations -------------------------------------------------------------------------------------------------------------------------------
def test_fp16_toward_zero():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10, -1.0 - 2.0 ** -11 - 2.0 ** -20, 2049.0, -2049.0, 3.0 * 2.0 ** -20, 0.0, 16383.9])
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -10, -1.0, 2048.0, -2048.0, 3.0 * 2.0 ** -20, 0.0, 16376.0])
    assert torch.equal(LR.fp16_rtz(x), want)
    hi, lo = LR.split_x(x)
    assert bool(((hi + lo - x).abs() <= 2.0 ** -21 * x.abs()).all())     # csrc/car_split.h: |x - hi - lo| < 2^-21 |x|


def test_row_power_of_two_is_the_header_s():
    m = torch.tensor([1.0, 1.5, 2.0 ** -30, 2.0 ** -31, 1e-30, 2.0 ** 103, 2.0 ** 120, 8191.0])
    p = LR.row_pow2(m)
    assert torch.equal(p, torch.tensor([2.0 ** 13, 2.0 ** 13, 2.0 ** 43, 2.0 ** 43, 2.0 ** 43, 2.0 ** -90, 2.0 ** -90, 2.0]))
    import pack_reference as PR
    for v in (1.0, 0.3, 700.0, 1e-30, 2.0 ** -40):
        assert float(LR.row_pow2(torch.tensor([v]))) == PR.pow2_scale(v)


@pytest.mark.parametrize("wide", ["x", "w"])
def test_split_fp16_emulation_is_exact_on_the_integer_sets(wide):
    """On int_x / int_w every product and partial sum is an integer below 2^24, the wide operand needs its lo half and the narrow one does
    not: x3_linear returns the float64 layer exactly; with the lo half of the wide operand ignored it does not."""
    M, K, N = LR.X3_SET_SHAPE
    X, W, b, Y0 = LR.linear_set("int_" + wide, M, K, N)
    assert LR.x3_exact(X, W)
    for t in (X, W, b, Y0):
        assert torch.equal(t, t.round())
    y, B = LR.layer(X, W, b, Y0, LR.ACCUM)
    assert float(B.max()) < 2 ** 24
    assert torch.equal(LR.x3_linear(X, W, b) + Y0.double(), y)
    hi_only = lambda t: LR.fp16_rtz(t)
    assert not torch.equal(LR.x3_linear(hi_only(X), hi_only(W), b) + Y0.double(), y), "the lo halves carry signal"
    lo_of = LR.split_x(X * LR.row_pow2(X.abs().amax(1))[:, None])[1] if wide == "x" else LR.split_w(W * 2.0)[1]
    assert bool(lo_of.any())
    assert not LR.x3_exact(X + 4096 * X.sign() * (wide == "w"), W + 4096 * W.sign() * (wide == "x")), "both wide: a lo lo product would be lost"


def test_split_fp16_emulation_follows_the_running_row_scale():
    """A row that grows 2^20-fold from its first chunk to its second: the first chunk is split against its own maximum (22 bits of IT),
    not against the row's."""
    x = torch.zeros(1, 64)
    x[0, 0], x[0, 32] = 1.0 + 2.0 ** -20, 2.0 ** 20
    W = torch.zeros(1, 64)
    W[0, 0] = 1.0
    assert float(LR.x3_linear(x, W, None)) == 1.0 + 2.0 ** -20


@pytest.mark.parametrize("wide", ["dY", "X"])
def test_bf16_emulation_is_exact_on_the_integer_sets_and_needs_all_three_products(wide):
    """int_dY / int_X: integer operands, the narrow one of at most 8 significant bits (its lo is zero), the wide one with lo != 0;
    sum |terms| < 2^24.  wgrad_bf16 equals the float64 gradient exactly; without the product that carries the wide operand's lo half
    it does not, and without hi hi neither."""
    for case in ("bf16-partial-block", "bf16-whole-one-tile"):
        M, N, K, _, _, _ = LR.WGRAD_SHAPES[case]
        dY, X, dW0, db0 = LR.wgrad_set("int_" + wide, M, N, K)
        assert LR.bf16_exact(dY, X)
        (yh, yl), (xh, xl) = LR.bf16_split(dY), LR.bf16_split(X)
        assert bool(yl.any()) == (wide == "dY") and bool(xl.any()) == (wide == "X")
        dW, db, BW, Bb = LR.wgrad(dY, X, False, dW0, db0)
        assert float(BW.max()) < 2 ** 24 and float(Bb.max()) < 2 ** 24
        eW, eb = LR.wgrad_bf16(dY, X, False, dW0, db0)
        assert torch.equal(eW, dW) and torch.equal(eb, db)
        carrier = "lh" if wide == "dY" else "hl"
        for dropped in (carrier, "hh"):
            kept = tuple(p for p in ("hh", "hl", "lh") if p != dropped)
            wW, wb = LR.wgrad_bf16(dY, X, False, dW0, db0, products=kept)
            assert not torch.equal(wW, dW), f"dropping {dropped} went unnoticed"
        idle = "hl" if wide == "dY" else "lh"
        wW, _ = LR.wgrad_bf16(dY, X, False, dW0, db0, products=("hh", carrier))
        assert torch.equal(wW, dW), f"{idle} carries nothing in this set: the other integer set pins it"
        # with RELU_IN the negative entries of X leave: still exact
        dWr, dbr, _, _ = LR.wgrad(dY, X, True, dW0, db0)
        eWr, ebr = LR.wgrad_bf16(dY, X, True, dW0, db0)
        assert torch.equal(eWr, dWr) and torch.equal(ebr, dbr) and not torch.equal(dWr, dW)


def test_bf16_split_rounds_both_halves_to_nearest():
    x = torch.tensor([257.0, 383.0, 1.0 + 2.0 ** -8 + 2.0 ** -16, -65535.0, 3.0e-30])
    hi, lo = LR.bf16_split(x)
    assert torch.equal(hi[:2], torch.tensor([256.0, 384.0])) and torch.equal(lo[:2], torch.tensor([1.0, -1.0]))
    assert bool(((hi + lo - x).abs() <= 2.0 ** -16 * x.abs()).all())
    assert float(hi[3] + lo[3]) == -65535.0


# ---- car_linear_pack's layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", LR.PACK_SHAPES)
def test_packed_layout_is_the_operand_order(K, N):
    """The index formula against loops written from car_linear.hip's comment: per (chunk, tile) four blocks j4 of 64 lanes x float4; lane l
    of block j4 holds W[32 tile + l % 32][32 chunk + 16 (l / 32) + 4 j4 + 0..3]; column K is the bias, later columns and rows >= N zero.
    Every weight and every bias value appears exactly once; a bias column moved by one does not pass."""
    g = LR.pack_geom(K, N)
    W = torch.arange(1, N * (K + 3) + 1, dtype=F32).reshape(N, K + 3)       # ldw > K, every entry distinct and non-zero
    b = -torch.arange(1, N + 1, dtype=F32)
    got = LR.packed_layout(W, b, K, N).reshape(g["chunks"], g["tiles_alloc"], 4, 64, 4)

    def walk(bias_col):
        want = torch.zeros_like(got)
        for c in range(g["chunks"]):
            for t in range(g["tiles_alloc"]):
                for j4 in range(4):
                    for lane in range(64):
                        n = 32 * t + lane % 32
                        for e in range(4):
                            k = 32 * c + 16 * (lane // 32) + 4 * j4 + e
                            if n < N:
                                want[c, t, j4, lane, e] = b[n] if k == bias_col else (W[n, k] if k < K else 0.0)
        return want
    assert torch.equal(got, walk(K))
    assert not torch.equal(got, walk(K - 1)) and not torch.equal(got, walk(K + 1)), "a bias column moved by one went unnoticed"
    vals = got.reshape(-1)
    assert torch.equal(vals[vals > 0].sort().values, W[:, :K].reshape(-1).sort().values)
    assert torch.equal(vals[vals < 0].sort().values, b.sort().values)
    assert got.numel() == g["floats"] == g["chunks"] * g["tiles_alloc"] * 1024
    nob = LR.packed_layout(W, None, K, N)
    assert bool((nob >= 0).all()) and torch.equal(nob[nob > 0].sort().values, vals[vals > 0].sort().values)


# ---- launch rules -----------------------------------------------------------------------------------------------------------------------------------
def test_linear_shapes_reach_every_tile_instance():
    seen_nt, ragged_m, ragged_k = set(), set(), set()
    for M, K, N, extra in LR.LINEAR_SHAPES:
        L = LR.linear_launch(M, K, N)
        assert L["nt"] == LR.LINEAR_NT[N] and L["phantom"] == LR.LINEAR_PHANTOM.get(N, 0), (M, K, N, L)
        assert L["grid"] == ((M + 127) // 128, L["tiles_alloc"] // L["nt"]) and L["chunks"] == (K + 32) // 32
        seen_nt.add(L["nt"])
        if M % 128:
            ragged_m.add(L["nt"])
        if (K + 1) % 32 and K % 4:
            ragged_k.add(L["nt"])
    assert seen_nt == ragged_m == ragged_k == {1, 2, 4, 9}
    assert {s[0] for s in LR.LINEAR_SHAPES} == {1, 31, 33, 127, 128, 129, 257}
    assert {s[1] for s in LR.LINEAR_SHAPES} == {1, 15, 16, 31, 32, 33, 576, 579}
    assert {s[2] for s in LR.LINEAR_SHAPES} == {3, 5, 32, 64, 96, 130, 160, 288, 320}
    assert any(K == 576 and extra == 0 for _, K, _, extra in LR.LINEAR_SHAPES), "ldx == K: load_x clamps at the row's end"
    assert [LR.tiles_per_block(t) for t in (1, 2, 3, 4, 5, 8, 9, 10, 18)] == [1, 2, 4, 4, 4, 4, 9, 9, 9]
    assert LR.pack_geom(576, 320)["tiles_alloc"] == 18 and LR.pack_geom(31, 32)["chunks"] == 1 and LR.pack_geom(32, 64)["chunks"] == 2
    for M, K, N in LR.LINEAR_SET_SHAPES:
        assert LR.linear_launch(M, K, N)["grid"][0] > 1


def test_x3_shapes_reach_every_column_group_and_the_second_round():
    for M, K, N, extra in LR.X3_SHAPES:
        L = LR.x3_launch(M, K, N)
        assert (L["nt"], L["groups"]) == LR.X3_NT[N], (N, L)
        assert L["grid"] % (8 * L["groups"]) == 0 and L["grid"] // L["groups"] >= L["row_blocks"]
        # the block map reaches every (row block, group) exactly once
        ids = torch.arange(L["grid"])
        rblock, grp = (ids // 8 // L["groups"]) * 8 + ids % 8, (ids // 8) % L["groups"]
        live = rblock * 192 < M
        pairs = set(zip(rblock[live].tolist(), grp[live].tolist()))
        assert len(pairs) == int(live.sum()) == L["row_blocks"] * L["groups"] and int((~live).sum()) == L["idle_blocks"]
    assert {s[0] for s in LR.X3_SHAPES} == {1, 15, 16, 17, 191, 192, 193, 1537}
    assert {s[1] for s in LR.X3_SHAPES} == {1, 31, 32, 33, 100, 579}
    assert {s[2] for s in LR.X3_SHAPES} == {32, 64, 96, 128, 160, 256, 288, 576}
    assert {LR.X3_NT[n][0] for n in LR.X3_NT} == {2, 4, 8, 18}
    big = [LR.x3_launch(M, K, N) for M, K, N, _ in LR.X3_SHAPES if M == 1537]
    assert all(L["rounds"] == 2 and L["row_blocks"] == 9 and L["last_block_rows"] == 1 for L in big), "8 x 192 + 1 rows: the second round of row blocks"
    assert {L["groups"] for L in big} == {2, 3}
    assert all(LR.x3_launch(M, K, N)["rounds"] == 1 for M, K, N, _ in LR.X3_SHAPES if M <= 1536)
    assert {(M, Ce) for M, Ce, _ in LR.KQ_SHAPES} >= {(1, 96), (17, 100), (193, 288), (17, 576), (193, 864)}


def test_wgrad_shapes_take_the_paths_they_are_named_for():
    W = {n: LR.wgrad_launch(M, N, K, db, fl) for n, (M, N, K, db, relu, fl) in LR.WGRAD_SHAPES.items()}
    for n, L in W.items():
        assert n.startswith(L["kernel"]), (n, L)
        M = LR.WGRAD_SHAPES[n][0]
        assert (L["gz"] - 1) * L["slab"] < M <= L["gz"] * L["slab"] and L["gz"] <= 65535
        assert L["slab"] % (32 if L["kernel"] == "bf16" else 16) == 0 and (L["kernel"] == "bf16" or L["slab"] >= 64)
    S = LR.WGRAD_SHAPES
    # the fp32-pipe kernels: one block, a partial block, the four-block minimum slab and one row beyond it
    assert (W["tile22-one-row"]["last_slab_rows"], W["tile22-partial-block"]["last_block_rows"], W["tile22-one-block-K128"]["last_block_rows"]) == (1, 15, 16)
    assert W["tile35-K128-db"]["last_slab_blocks"] == 2 and W["tile35-K128-db"]["last_block_rows"] == 1
    assert W["tile35-N129"]["last_block_rows"] == 15 and W["tile35-N129"]["last_slab_blocks"] == 4
    assert W["tile35-bias-last-of-tile"]["gz"] == 1 and W["tile35-bias-last-of-tile"]["last_slab_rows"] == 64
    assert W["tile35-bias-alone"]["gz"] == 2 and W["tile35-bias-alone"]["last_slab_rows"] == 1
    assert {S[n][0] for n in S if n.startswith("tile") and S[n][0] < 2047} == {1, 15, 16, 17, 63, 64, 65}
    # K = 128 below 2048 rows: the bias column decides between the two tile kernels
    assert S["tile22-one-block-K128"][1:3] == S["tile35-K128-db"][1:3] == (128, 128) and not S["tile22-one-block-K128"][3] and S["tile35-K128-db"][3]
    # the bias column: last column of a 320-wide tile (gy stays 1), alone in a new one (gy = 2); tile-exact without it
    assert W["tile35-bias-last-of-tile"]["gy"] == 1 and W["tile35-bias-alone"]["gy"] == 2 and W["tile35-tile-exact"]["gy"] == 1
    assert W["bf16-bias-last-of-tile"]["gy"] == 1 and W["bf16-short-last-slab"]["gy"] == 2 and W["bf16-tile-exact"]["gy"] == 1
    assert W["tile35-tile-exact"]["gx"] == 2 and W["tile35-bias-alone"]["gx"] == 2 and W["bf16-tile-exact"]["gx"] == 1 and W["tile35-bias-last-of-tile"]["gx"] == 1
    assert {S[n][1] for n in S} >= {3, 128, 129, 192, 193, 384} and {S[n][2] for n in S} >= {16, 319, 320, 579}
    # either side of the dispatch, and the flag
    assert S["tile22-below-dispatch"][1:4] == S["bf16-at-dispatch"][1:4] == S["tile22-fp32-flag"][1:4]
    assert (S["tile22-below-dispatch"][0], S["bf16-at-dispatch"][0]) == (2047, 2048)
    assert S["bf16-short-last-slab"][:5] == S["tile35-fp32-flag"][:5]
    # the bf16 kernel's slabs
    assert W["bf16-at-dispatch"]["slab"] == 32 and W["bf16-at-dispatch"]["last_slab_rows"] == 32 and W["bf16-at-dispatch"]["whole_iterations"] == 0
    assert W["bf16-partial-block"]["last_block_rows"] == 1 and W["bf16-bias-last-of-tile"]["last_block_rows"] == 2
    assert W["bf16-short-last-slab"]["slab"] == 64 and W["bf16-short-last-slab"]["last_slab_rows"] == 32 and W["bf16-short-last-slab"]["whole_iterations"] == 0
    for n, tiles in (("bf16-whole-multi-tile", 4), ("bf16-whole-one-tile", 1)):
        assert W[n]["gx"] * W[n]["gy"] == tiles and W[n]["slab"] == 96 and W[n]["whole_iterations"] == 1
        assert 0 < W[n]["last_block_rows"] < 32 and W[n]["last_slab_rows"] < W[n]["slab"]
    assert S["bf16-whole-multi-tile"][4] and not S["bf16-whole-one-tile"][4], "a whole-block iteration with RELU_IN and without"
    # the fewest rows at which a one-tile layer runs a whole-block iteration: 256 slabs of more than 64 rows
    m0 = LR.smallest_whole_block_rows(128, 16, True)
    assert m0 == 16385 and LR.wgrad16_launch(m0, 128, 16, True)["whole_iterations"] == 1 and LR.wgrad16_launch(m0 - 1, 128, 16, True)["whole_iterations"] == 0
    m1 = LR.smallest_whole_block_rows(384, 579, True)
    assert m1 == 4097 and LR.wgrad16_launch(m1, 384, 579, True)["whole_iterations"] == 1 and LR.wgrad16_launch(m1 - 1, 384, 579, True)["whole_iterations"] == 0
    assert max(M * max(N, K) for M, N, K, *_ in S.values()) <= 25000 * 128


def test_the_slab_rules_against_a_walk_of_the_kernels_loops():
    """The closed forms against the kernels' loops walked literally (m_begin, m_end, the two for loops of wgrad16_kernel), and a slab rule
    that is one block off fails that walk."""
    def walk(M, slab, block, ahead):
        gz = (M + slab - 1) // slab
        per = []
        for z in range(gz):
            m, m_end, whole, blocks = z * slab, min(z * slab + slab, M), 0, 0
            while m + ahead * block <= m_end:
                whole, blocks, m = whole + 1, blocks + 1, m + block
            last = block
            while m < m_end:
                blocks, last, m = blocks + 1, min(block, m_end - m), m + block
            per.append((whole, blocks, last))
        return gz, per
    for n, (M, N, K, db, relu, fl) in LR.WGRAD_SHAPES.items():
        L = LR.wgrad_launch(M, N, K, db, fl)
        block, ahead = (32, 3) if L["kernel"] == "bf16" else (16, 1)
        gz, per = walk(M, L["slab"], block, ahead)
        assert gz == L["gz"] and per[-1] == (L["whole_iterations_last_slab"], L["last_slab_blocks"], L["last_block_rows"]), (n, per[-1], L)
        assert per[0][0] == L["whole_iterations"] and (gz == 1 or per[0][1] == L["blocks_per_slab"])
        if L["kernel"] == "bf16":
            wrong = walk(M, L["slab"] + 32, 32, 3)                      # the slab one block longer than the launcher's
            assert (wrong[0], wrong[1][-1], wrong[1][0][0]) != (gz, per[-1], per[0][0]), n


# ---- the input sets ---------------------------------------------------------------------------------------------------------------------------------
def test_padding_is_poison():
    p = LR.padded(torch.zeros(7, 5), 8)
    pad = p[:, 5:]
    assert not bool(torch.isfinite(pad).any()) and bool(torch.isnan(pad).any()) and bool((pad == LR.INF).any()) and bool((pad == -LR.INF).any())
    assert torch.equal(LR.padded(torch.ones(3, 4), 4), torch.ones(3, 4))


@pytest.mark.parametrize("M,K,N", LR.LINEAR_SET_SHAPES + (LR.X3_SET_SHAPE,))
def test_layer_value_sets_hold_what_they_are_named_for(M, K, N):
    for name in set(LR.LINEAR_SETS + LR.X3_SETS):
        X, W, b, Y0 = LR.linear_set(name, M, K, N)
        assert X.shape == (M, K) and W.shape == (N, K) and b.shape == (N,) and Y0.shape == (M, N)
        assert all(bool(torch.isfinite(t).all()) for t in (X, W, b, Y0))
    X = LR.linear_set("span", M, K, N)[0]
    s = X.abs().amax(1)
    assert float(s.min()) < 1e-5 and float(s.max()) > 1e3 and float(s.max() / s.min()) > 1e8
    X, W, b, _ = LR.linear_set("cancel", M, K, N)
    y, B = LR.layer(X, W, b, None, 0)
    assert bool((y.abs() <= 2.0 ** -9 * B).all()) and float(y.abs().max()) > 0 and not bool(b.any())
    assert torch.equal(W[:, 0:2 * (K // 2):2], W[:, 1:2 * (K // 2):2])
    for name, grow in (("grow", True), ("shrink", False)):
        X = LR.linear_set(name, M, K, N)[0]
        first, last = X[:, :8].abs().amax(1), X[:, -8:].abs().amax(1)
        r = (last / first) if grow else (first / last)
        assert float(r.median()) > 1e4
        if grow and K > 64:                                            # the running row scale moves at least twice in most rows
            cm = torch.stack([X[:, c:c + 32].abs().amax(1) for c in range(0, K, 32)], 1)
            moves = (LR.row_pow2(torch.cummax(cm, 1).values).log2().diff(dim=1) != 0).sum(1)
            assert float(moves.float().median()) >= 2
    X = LR.linear_set("lead0", M, K, N)[0]
    if K > 32:
        assert bool((X[1, :32] == 0).all()) and bool(X[1, 32:].any()) and bool(X[0, :32].any())
    X = LR.linear_set("zero_rows", M, K, N)[0]
    assert not bool(X[0::2].any()) and bool(X[1::2].any(dim=1).all())
    X = LR.linear_set("tiny_huge", M, K, N)[0]
    assert float(X[0].abs().max()) == 2.0 ** -40 and float(X[1].abs().max()) == 2.0 ** 40
    assert float(LR.row_pow2(X[0].abs().max().reshape(1))) == 2.0 ** 43, "below 2^-30 the row's power of two is the clamp"
    for name in ("int", "int_x", "int_w"):
        X, W, b, Y0 = LR.linear_set(name, M, K, N)
        assert all(torch.equal(t, t.round()) for t in (X, W, b, Y0))
        for flags in (0, LR.RELU_IN, LR.ACCUM):
            y64, B = LR.layer(X, W, b, Y0, flags)
            assert float(B.max()) < 2 ** 24
            y32, _ = LR.layer(X, W, b, Y0, flags, F32)
            assert torch.equal(y32.double(), y64), "float32 is exact on integers below 2^24"
        assert LR.x3_exact(X, W)
        assert torch.equal(LR.x3_linear(X, W, b), LR.layer(X, W, b, None, 0)[0])


@pytest.mark.parametrize("case", LR.WGRAD_SET_SHAPES)
def test_wgrad_value_sets_hold_what_they_are_named_for(case):
    M, N, K, db, relu, fl = LR.WGRAD_SHAPES[case]
    for name in LR.WGRAD_SETS:
        dY, X, dW0, db0 = LR.wgrad_set(name, M, N, K)
        assert dY.shape == (M, N) and X.shape == (M, K) and dW0.shape == (N, K) and db0.shape == (N,)
        assert all(bool(torch.isfinite(t).all()) for t in (dY, X, dW0, db0))
    dY, X, _, _ = LR.wgrad_set("rows12", M, N, K)
    sy, sx = dY.abs().amax(1), X[:, min(8, K):].abs().amax(1) if K > 8 else X.abs().amax(1)
    assert float(sy.max() / sy.min()) > 1e10 and bool((X[:, :min(8, K)] == 1).all())
    if K > 8:
        assert float(sx.max() / sx.min()) > 1e7
    dY, X, _, _ = LR.wgrad_set("const", M, N, K)
    assert bool((X[:, :min(8, K)] == 1).all()) and bool((dY[:, :min(4, N)] == 0.5).all())
    dW, _, BW, _ = LR.wgrad(dY, X, False, torch.zeros(N, K), None)
    assert float((dW[0, 0].abs() / BW[0, 0])) == 1.0, "a sum without cancellation"
    for name in ("int_dY", "int_X"):
        dY, X, dW0, db0 = LR.wgrad_set(name, M, N, K)
        assert all(torch.equal(t, t.round()) for t in (dY, X, dW0, db0)) and LR.bf16_exact(dY, X)
        assert int(dY.any(dim=1).sum()) <= 1024 and int(X.any(dim=1).sum()) <= 1024
        narrow = X if name == "int_dY" else dY
        assert float(narrow.abs().max()) <= 255
        for r in (False, True):
            dW, dbv, BW, Bb = LR.wgrad(dY, X, r, dW0, db0)
            assert float(BW.max()) < 2 ** 24 and float(Bb.max()) < 2 ** 24
            d32, b32, _, _ = LR.wgrad(dY, X, r, dW0, db0, F32)
            assert torch.equal(d32.double(), dW) and torch.equal(b32.double(), dbv)
            eW, eb = LR.wgrad_bf16(dY, X, r, dW0, db0)
            assert torch.equal(eW, dW) and torch.equal(eb, dbv)
        L = LR.wgrad_launch(M, N, K, True)
        if M > 1024:                                                   # live rows in the first slab, the last slab and between
            live = dY.any(dim=1).nonzero()[:, 0]
            assert int(live.min()) < L["slab"] and int(live.max()) >= (L["gz"] - 1) * L["slab"] and len(set((live // L["slab"]).tolist())) > L["gz"] // 2


@pytest.mark.parametrize("M,Ce,extra", LR.KQ_SHAPES)
def test_chain_rows_hold_what_they_are_named_for(M, Ce, extra):
    P = LR.kq_params(Ce, 20 + Ce)
    e, g = LR.kq_rows(M, Ce, 30 + M)
    assert not bool(e[0].any()) and not bool(g[M - 1].any()) and bool((P["bk1"] < 0).all())
    r = LR.kq_chain(e, g, P)
    assert bool((r["k1"][0] == 0).all()) and torch.equal(r["key"][0], P["bk2"].double()) and torch.equal(r["B_key"][0], P["bk2"].double().abs())
    q1_of_zero_g = F.relu(P["bq1"].double())
    assert torch.equal(r["q1"][M - 1], q1_of_zero_g) and bool(q1_of_zero_g.any())
    if M > 1:
        assert bool((r["k1"][1:] > 0).any(dim=1).all())
    assert bool((r["B_logit"] > 0).all()) and bool((r["B_qry"] >= P["bq2"].double().abs()).all())
