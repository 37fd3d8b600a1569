"""The pyramid gather and its two scatters through the C ABI against tests/gather_reference.py: car_gather_bilinear (csrc/car_gather.hip),
car_gather_bilinear_backward (the fp32-atomic scatter, csrc/car_backward.hip), car_gather_bilinear_backward_binned (csrc/car_scatter.hip),
and their refusals.

Tolerance, measured against the reference and never against the kernel: every element must satisfy |got - ref64| <= tol x bound with
bound = sum |w| |texel| (forward) or sum |w| |dout| over the texel's records (scatters), both on the taps of the float32 tier of the
reference; where the bound is 0 the value must be exactly 0.  tol = 8 x max(r32, 2^-22), r32 the worst ratio of the reference run in
float32 on the same inputs (the project's rule, tests/test_raychain_hip.py).  Every test prints ratio_kernel / tolerance as a ``[parity]``
line (profiles/gather_parity.md).  The integer set is exact in fp32 in any order and is compared bit for bit.

Every output lies inside a larger NaN-filled buffer and starts as NaN itself (the atomic scatter's maps as zero: it accumulates); row
padding of out / dout and the rows of dout no placement names hold NaN or inf: they must come back untouched, or never be read."""
import ctypes
import functools

import pytest
import torch

import abi_harness as abi
import gather_reference as GR
from abi_harness import CAR_E_ARG, INF, NAN, Guarded
from parity_rule import judge

pytestmark = pytest.mark.gpu


def _levels(shapes):
    return abi.ints([s[2] for s in shapes]), abi.ints([s[0] for s in shapes]), abi.ints([s[1] for s in shapes])


def _named_rows(n_maps, pts, V, places):
    return torch.cat([GR.rows_of(p, V, n_maps, pts).flatten() for p in places]).unique()


def _dout(values, ld, col_out, named):
    """values [rows, C] on the device inside rows of stride ld: padding columns hold inf, rows outside `named` NaN."""
    rows, C = values.shape
    d = Guarded((rows, ld), fill=INF)
    d.view[:, col_out:col_out + C] = NAN
    d.view[named.to(abi.dev()), col_out:col_out + C] = values.to(abi.dev())[named.to(abi.dev())]
    return d


def _judge(test, case, pairs, r32):
    """pairs: [(got, ref64, bound)] on one device, one per level; the worst of them is held to the float32 run's ratio r32 by
    gather_reference.ratio's reading of a bound and of a non-finite value."""
    judge(test, case, {"": (pairs, r32)}, ratio=GR.ratio)


# ---------------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_forward(lib, s, mode):
    shapes, n_maps, pts, place, V = s["shapes"], s["n_maps"], s["pts"], s["place"], s["V"]
    C = sum(c for _, _, c in shapes)
    rows, ld, col_out = GR.n_rows(place, V, n_maps, pts), s["ld"], s["col_out"]
    maps = [t.to(abi.dev()) for t in s["maps"]]
    grid = s["grid"].to(abi.dev())
    out = Guarded((rows, ld))
    cs, hs, ws = _levels(shapes)
    rc = lib.car_gather_bilinear(abi.ptrs(maps), cs, hs, ws, len(shapes), n_maps, abi.ptr(grid), pts, s["run"], mode, place, V, abi.ptr(out.view), ld, col_out,
                                 abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    named = GR.rows_of(place, V, n_maps, pts).flatten().to(abi.dev())
    got = out.view[named, col_out:col_out + C].clone()
    out.view[named, col_out:col_out + C] = NAN
    assert out.margins_untouched() and bool(torch.isnan(out.view).all()), "wrote outside the rows' windows"
    return got


def _forward_case(lib, test, case, s, mode):
    got = run_forward(lib, s, mode)
    ref, bound = GR.gather_ref(s["maps"], s["grid"], mode, device=abi.dev())
    f32, _ = GR.gather_ref(s["maps"], s["grid"], mode, torch.float32, device=abi.dev())
    _judge(test, case, [(got, ref, bound)], GR.ratio(f32, ref, bound))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", GR.FORWARD_SETS)
def test_forward_edge_sets(name, mode):
    """Four levels with a 512-channel one (wave tasks, two segments), (256, 64, 8) (wave tasks), (8, 12, 4) and (4,) (the per-float4 kernel);
    levels of 1 x 1, 1 x 7, 5 x 3 and 16 x 16; plain, own with V = 2 and 3, other2; run = 1, 4 over 37 rays, and a non-divisor."""
    _forward_case(abi.lib(), "forward", f"{name} mode={mode}", GR.edge_set(name), mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel", list(GR.FORWARD_STRIDE))
def test_forward_group_stride(kernel, mode):
    """2 200 000 rows, more groups of 32 than the grid's 65536 work groups, so that the group loop takes a second trip: in the wave-task
    kernel (one 8-channel level, 68 750 groups) and in the per-float4 kernel (one 12-channel level, 275 000 rays x 4 steps: 68 752 groups
    with a ragged last ray block)."""
    _forward_case(abi.lib(), "forward", f"group-stride {kernel} mode={mode}", GR.forward_stride_set(kernel), mode)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the scatters
# ---------------------------------------------------------------------------------------------------------------------------------------
def _gathers_of(s, mode=None):
    """[(grid on the CPU, mode, place)] of a set."""
    if "gathers" in s:
        return [(s["grid"], m, p) for m, p in s["gathers"]]
    if "grids" in s:
        return [(g, m, p) for g, m, p in zip(s["grids"], s["modes"], s.get("places", (GR.PLAIN,) * len(s["grids"])))]
    return [(s["grid"], s["mode"] if mode is None else mode, s["place"])]


@functools.lru_cache(maxsize=None)
def _scatter_reference(key, mode, on_device):
    """(ref64, bound, r32) of a set shared by the two scatters, computed once: on the CPU (the float32 run then adds in row order), or on the
    device for the sets too large for that."""
    s = _SETS[key]() if key in _SETS else GR.edge_set(key)
    dev = abi.dev() if on_device else torch.device("cpu")
    args = (s["shapes"], s["n_maps"], _gathers_of(s, mode), s["V"], s["dout"], 0)
    ref, bound, r32 = GR.scatter_ref_r32(*args, device=dev)
    return [r.to(abi.dev()) for r in ref], [b.to(abi.dev()) for b in bound], r32


_SETS = {"deep": GR.deep_set, "integer": GR.integer_set, "odd": GR.odd_set, "atomic-stride": GR.atomic_stride_set}


def _device_inputs(s, gathers):
    named = _named_rows(s["n_maps"], s["pts"], s["V"], [p for _, _, p in gathers])
    dout = _dout(s["dout"], s["ld"], s["col_out"], named)
    return dout, [g.to(abi.dev()) for g, _, _ in gathers]


def run_atomic(lib, s, gathers, dmaps=None):
    """One call per gather into zeroed (or the given) maps."""
    shapes, n_maps = s["shapes"], s["n_maps"]
    dout, grids = _device_inputs(s, gathers)
    dmaps = dmaps or [Guarded((n_maps, H, W, C), fill=0.0) for H, W, C in shapes]
    cs, hs, ws = _levels(shapes)
    for grid, (_, mode, place) in zip(grids, gathers):
        rc = lib.car_gather_bilinear_backward(abi.ptrs([d.view for d in dmaps]), cs, hs, ws, len(shapes), n_maps, abi.ptr(grid), s["pts"], mode, place, s["V"],
                                              abi.ptr(dout.view), s["ld"], s["col_out"], abi.stream())
        assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert all(d.margins_untouched() for d in dmaps), "wrote outside a map"
    return dmaps


def run_binned(lib, s, gathers, dmaps=None, misalign=0, short=0, work=None):
    """All gathers in one call into NaN-filled (or the given) maps.  work: (pointer, bytes) of the caller's own workspace."""
    shapes, n_maps = s["shapes"], s["n_maps"]
    dout, grids = _device_inputs(s, gathers)
    dmaps = dmaps or [Guarded((n_maps, H, W, C)) for H, W, C in shapes]
    cs, hs, ws = _levels(shapes)
    G = len(gathers)
    nbytes = lib.car_scatter_workspace_bytes(hs, ws, len(shapes), n_maps, s["pts"], G)
    assert nbytes > 0
    if work is None:
        work = torch.empty(nbytes + 16, dtype=torch.uint8, device=abi.dev())
        assert work.data_ptr() % 16 == 0
        work_ptr, work_bytes = ctypes.c_void_p(work.data_ptr() + misalign), nbytes - short
    else:
        work_ptr, work_bytes = work
    rc = lib.car_gather_bilinear_backward_binned(abi.ptrs([d.view for d in dmaps]), cs, hs, ws, len(shapes), n_maps, abi.ptrs(grids), abi.ints([m for _, m, _ in gathers]),
                                                 abi.ints([p for _, _, p in gathers]), G, s["pts"], s["V"], abi.ptr(dout.view), s["ld"], s["col_out"],
                                                 work_ptr, work_bytes, abi.stream())
    torch.cuda.synchronize()
    if misalign or short:
        return rc, dmaps
    assert rc == 0, lib.car_last_error()
    assert all(d.margins_untouched() for d in dmaps), "wrote outside a map"
    return dmaps


RUN = {"atomic": run_atomic, "binned": run_binned}


def _scatter_case(entry, case, key, mode=None, on_device=False):
    s = _SETS[key]() if key in _SETS else GR.edge_set(key)
    dmaps = RUN[entry](abi.lib(), s, _gathers_of(s, mode))
    ref, bound, r32 = _scatter_reference(key, mode, on_device)
    _judge(entry, case, [(d.view, r, b) for d, r, b in zip(dmaps, ref, bound)], r32)
    return s, dmaps, ref, bound, r32


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(GR.EDGE_SETS))
@pytest.mark.parametrize("entry", ["atomic", "binned"])
def test_scatter_edge_sets(entry, name, mode):
    """The forward's sets (every level size, channel set and placement; map 2 untouched with zeros padding) and levels of 12, 20 and 36
    channels (3, 5 and 9 float4s: the binned reduce's lanes loop)."""
    _scatter_case(entry, f"{name} mode={mode}", name, mode)


@pytest.mark.parametrize("entry", ["atomic", "binned"])
def test_scatter_deep_bins(entry):
    """Texels with exactly 0 .. 9 records (the reduce's four-at-a-time loop and its remainders), one with more than 50 000, a map without any."""
    _scatter_case(entry, "deep", "deep")


@pytest.mark.parametrize("entry", ["atomic", "binned"])
def test_scatter_integer_set_bit_for_bit(entry):
    """Every partial sum is exact in fp32 (tests/test_gather_reference.py asserts it): whatever the order of the additions, the result is the
    float64 reference to the last bit.  Two gathers (own border, other2 zeros) reading one dout."""
    s = GR.integer_set()
    dmaps = RUN[entry](abi.lib(), s, _gathers_of(s))
    ref, _, _ = _scatter_reference("integer", None, False)
    for l, (d, r) in enumerate(zip(dmaps, ref)):
        assert torch.equal(d.view.double(), r), (entry, l, int((d.view.double() != r).sum()))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("entry", ["atomic", "binned"])
def test_scatter_odd_size(entry, mode):
    """61 x 47 texels: (gx + 1) W - 1 rounds differently when the compiler fuses it, and a per-texel bound sees the weights move."""
    _scatter_case(entry, f"61x47 mode={mode}", "odd", mode)


@pytest.mark.parametrize("entry", ["atomic", "binned"])
def test_scatter_stride_set(entry):
    """16.9 M (point, channel) items: the atomic kernel's grid-stride loop loops (more than 65536 x 256 threads)."""
    _scatter_case(entry, "atomic-stride", "atomic-stride", 0, on_device=True)


def test_atomic_scatter_accumulates():
    """A second call into the first call's result: the sum of the two references."""
    s = GR.edge_set("wave3")
    lib = abi.lib()
    dmaps = run_atomic(lib, s, _gathers_of(s, 0))
    dmaps = run_atomic(lib, s, _gathers_of(s, 1), dmaps)
    (r0, b0, a), (r1, b1, b) = _scatter_reference("wave3", 0, False), _scatter_reference("wave3", 1, False)
    _judge("atomic", "accumulate wave3 mode=0 then 1", [(d.view, x + y, p + q) for d, x, y, p, q in zip(dmaps, r0, r1, b0, b1)], max(a, b))


def test_binned_scatter_overwrites():
    """A second call into the first call's result: the second reference alone."""
    s = GR.edge_set("wave3")
    lib = abi.lib()
    dmaps = run_binned(lib, s, _gathers_of(s, 0))
    dmaps = run_binned(lib, s, _gathers_of(s, 1), dmaps)
    ref, bound, r32 = _scatter_reference("wave3", 1, False)
    _judge("binned", "overwrite wave3 mode=0 then 1", [(d.view, r, b) for d, r, b in zip(dmaps, ref, bound)], r32)


@pytest.mark.parametrize("n_gathers", [1, 2, 4])
def test_binned_scatter_mixed_gathers(n_gathers):
    """One, two and four (kMaxGathers) gathers with their own grids, padding modes and placements reading one dout (GR.mixed_set)."""
    s = GR.mixed_set(n_gathers)
    gathers = _gathers_of(s)
    dmaps = run_binned(abi.lib(), s, gathers)
    args = (s["shapes"], s["n_maps"], gathers, s["V"], s["dout"], 0)
    ref, bound, r32 = GR.scatter_ref_r32(*args)
    _judge("binned", f"{n_gathers} gathers", [(d.view, r.to(abi.dev()), b.to(abi.dev())) for d, r, b in zip(dmaps, ref, bound)], r32)


def _big_binned_case(case, s):
    gathers = _gathers_of(s)
    dmaps = run_binned(abi.lib(), s, gathers)
    args = (s["shapes"], s["n_maps"], gathers, s["V"], s["dout"], 0)
    ref, bound, r32 = GR.scatter_ref_r32(*args, device=abi.dev())
    _judge("binned", case, [(d.view, r, b) for d, r, b in zip(dmaps, ref, bound)], r32)


@pytest.mark.parametrize("name", list(GR.SCAN_SETS))
def test_binned_scatter_scan_sets(name):
    """The three-kernel scan: n = 1024 (a whole number of scan blocks) and 1025 (the closing counter alone in the last block), and 1027 /
    3073 scan blocks (two / four block sums per thread of scan_blocks_kernel), records on the first and last counters of scan blocks and of
    threads' runs (tests/test_gather_reference.py asserts where they are).  Every texel of every map is compared."""
    _big_binned_case(f"scan {name}", GR.scan_set(name))


def test_binned_scatter_bin_stride():
    """Four plain gathers x 2 maps x 530 000 points x four levels = 16.96 M items: bin_kernel's grid-stride loop loops, in both passes."""
    _big_binned_case("bin-stride", GR.bin_stride_set())


def test_binned_scatter_fits_its_workspace_exactly():
    """Two levels of 5 x 3 and 4 x 4 texels, two maps, seven points, two gathers: a workspace of exactly car_scatter_workspace_bytes, NaN
    all around it, then one twice as large.  Neither call writes outside its workspace.  The order of a texel's additions is the order in
    which the binning pass's integer atomics landed (csrc/car_scatter.hip), so two runs of this entry need not give the same bits: each
    call is judged by this suite's rule instead."""
    n_maps, pts, shapes = 2, 7, ((5, 3, 4), (4, 4, 8))
    grids = [torch.rand(n_maps, pts, 2, generator=GR.gen(71 + j)) * 3 - 1.5 for j in range(2)]
    grids[0][:, 0], grids[1][:, 0] = torch.tensor([0.0, 0.0]), torch.tensor([-1.0, 1.0])
    s = {"shapes": shapes, "n_maps": n_maps, "pts": pts, "V": 1, "ld": 16, "col_out": 4, "grids": grids, "modes": (0, 1), "dout": GR._values((n_maps * pts, 12), 73)}
    gathers = _gathers_of(s)
    ref, bound, r32 = GR.scatter_ref_r32(shapes, n_maps, gathers, 1, s["dout"], 0)
    lib = abi.lib()

    def run(work, work_bytes):
        dmaps = run_binned(lib, s, gathers, work=(work.ptr, work_bytes))
        _judge("binned", f"exact workspace, {work_bytes} bytes", [(d.view, r.to(abi.dev()), b.to(abi.dev())) for d, r, b in zip(dmaps, ref, bound)], r32)
        return [d.get("dmaps") for d in dmaps]

    abi.exact_then_twice(lib.car_scatter_workspace_bytes(*_levels(shapes)[1:], len(shapes), n_maps, pts, 2), run, "car_gather_bilinear_backward_binned", same=False)


def test_binned_scatter_refuses_a_bad_workspace():
    s = GR.edge_set("quad1")
    lib = abi.lib()
    for kw in ({"short": 1}, {"misalign": 8}):
        rc, dmaps = run_binned(lib, s, _gathers_of(s, 0), **kw)
        assert rc == CAR_E_ARG and b"workspace" in lib.car_last_error(), kw
        assert all(bool(torch.isnan(d.full).all()) for d in dmaps), kw


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals: one argument wrong, every other one as an accepted call has it; nothing launches
# ---------------------------------------------------------------------------------------------------------------------------------------
_SHAPES = ((5, 3, 8), (4, 4, 4))
_BIG = ((1, 1, 4), (65536, 32768, 4))           # the second level alone holds 2^31 texels
_SUM = ((32768, 16384, 8), (32768, 16384, 4))   # 2^29 texels each: two maps of either stay below 2^31, the counters of both (2^31 + 1) do not


def _refusal_args(entry, **kw):
    """The accepted call's arguments as a dict, `kw` applied; buffers are tiny and NaN-filled."""
    shapes, null_map, null_grid = kw.pop("shapes", _SHAPES), kw.pop("null_map", None), kw.pop("null_grid", None)
    n_maps, pts, V, C = 2, 8, 2, sum(c for _, _, c in shapes)
    maps = [Guarded((2, 5, 3, 8)), Guarded((2, 4, 4, 4))]
    grid, out = torch.zeros(n_maps, pts, 2, device=abi.dev()), Guarded((n_maps * pts * V, C + 4))
    cs, hs, ws = _levels(shapes)
    a = {"maps": abi.ptrs([m.view for m in maps]), "c": cs, "h": hs, "w": ws, "n_levels": len(shapes), "n_maps": n_maps}
    if entry == "forward":
        a.update(grid=abi.ptr(grid), pts=pts, run=1, mode=0, place=GR.OWN, V=V, out=abi.ptr(out.view), ld=C + 4, col_out=4)
    elif entry == "atomic":
        a.update(grid=abi.ptr(grid), pts=pts, mode=0, place=GR.OWN, V=V, out=abi.ptr(out.view), ld=C + 4, col_out=4)
    else:
        work = torch.empty(1 << 16, dtype=torch.uint8, device=abi.dev())
        a.update(grids=abi.ptrs([grid, grid]), modes=abi.ints([0, 1]), places=abi.ints([GR.OWN, GR.OTHER2]), n_gathers=2, pts=pts, V=V, out=abi.ptr(out.view), ld=C + 4,
                 col_out=4, work=abi.ptr(work), nbytes=1 << 16)
    if null_map is not None:                                    # one element of the array of map pointers
        a["maps"][null_map] = None
    if null_grid is not None:
        a["grids"][null_grid] = None
    for k, v in kw.items():
        assert k in a, k
        a[k] = v
    return a, maps + [out], (grid,)


_ENTRY_FN = {"forward": "car_gather_bilinear", "atomic": "car_gather_bilinear_backward", "binned": "car_gather_bilinear_backward_binned"}
_COMMON = [("bad sizes", {"n_levels": 0}), ("bad sizes", {"n_levels": 5}), ("bad sizes", {"n_maps": 0}), ("bad sizes", {"pts": 0}),
           ("multiple of 4", {"c": abi.ints([8, 6])}), ("multiple of 4", {"h": abi.ints([5, 0])}), ("multiple of 4", {"w": abi.ints([0, 4])}),
           ("float4-aligned", {"ld": 18}), ("float4-aligned", {"col_out": 2}), ("float4-aligned", {"col_out": -4}), ("float4-aligned", {"col_out": 8}),
           ("multiple of 4", {"null_map": 1}), ("32-bit texel indices", {"shapes": _BIG})]
_SINGLE = [("null pointer", {"grid": None}), ("null pointer", {"out": None}), ("null pointer", {"maps": None}), ("mode must be", {"mode": 2}),
           ("bad placement", {"place": 3}), ("bad placement", {"place": GR.OTHER2, "V": 3}), ("bad placement", {"place": GR.OTHER2, "n_maps": 3})]
_BINNED = [("bad sizes", {"n_gathers": 0}), ("bad sizes", {"n_gathers": 5}), ("mode must be", {"modes": abi.ints([0, 2])}),
           ("bad placement", {"places": abi.ints([GR.OWN, 3])}), ("bad placement", {"V": 3}), ("bad placement", {"n_maps": 3}),
           ("mode must be", {"null_grid": 1}),
           # each term of the counter check alone: 32 pts records and 4 pts rows; one gather of one level with V = 8: 8 pts records, 16 pts
           # rows; two levels whose counters together pass 2^31
           ("32-bit counters", {"pts": 1 << 27}), ("32-bit counters", {"n_gathers": 1, "n_levels": 1, "V": 8, "places": abi.ints([GR.OWN]), "pts": 1 << 27}),
           ("32-bit counters", {"shapes": _SUM}), ("workspace", {"nbytes": 64})]
_REFUSALS = [(e, m, kw) for e in ("forward", "atomic") for m, kw in _COMMON + _SINGLE] + [("binned", m, kw) for m, kw in _COMMON + _BINNED]


@pytest.mark.parametrize("entry,message,kw", _REFUSALS, ids=[f"{e}-{m.split()[0]}-{'-'.join(kw)}-{i}" for i, (e, m, kw) in enumerate(_REFUSALS)])
def test_refusals(entry, message, kw):
    """CAR_E_ARG, the message of the CAR_REQUIRE that fired, and buffers that are still NaN."""
    lib = abi.lib()
    a, guarded, _keep = _refusal_args(entry, **dict(kw))
    rc = getattr(lib, _ENTRY_FN[entry])(*a.values(), abi.stream())
    torch.cuda.synchronize()
    assert rc == CAR_E_ARG, (entry, kw, rc)
    assert message.encode() in lib.car_last_error(), (entry, kw, lib.car_last_error())
    assert all(bool(torch.isnan(g.full).all()) for g in guarded), (entry, kw)


def test_binned_scatter_refuses_a_misaligned_dout():
    lib = abi.lib()
    a, guarded, _keep = _refusal_args("binned")
    a["out"] = ctypes.c_void_p(a["out"].value + 4)
    assert lib.car_gather_bilinear_backward_binned(*a.values(), abi.stream()) == CAR_E_ARG and b"float4-aligned" in lib.car_last_error()
    assert all(bool(torch.isnan(g.full).all()) for g in guarded)
