"""CPU checks of the C-ABI boundary: the library builds, loads and exports every symbol of include/car_hip.h,
argument validation returns error codes (never aborts), and the product package never touches the oracle."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from cross_attention_renderer_amd import _lib
    return _lib.load()


def test_every_declared_symbol_is_exported(lib):
    from cross_attention_renderer_amd import _lib
    header = open(os.path.join(ROOT, "include", "car_hip.h")).read()
    declared = set(re.findall(r"\b(car_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.car_version() == 300


def test_bad_arguments_return_codes_not_crashes(lib):
    from cross_attention_renderer_amd import _lib
    assert lib.car_linear(None, 4, None, 4, 4, None, 4, 1, 0, None) == -1
    assert b"null pointer" in lib.car_last_error()
    assert lib.car_ray_setup(None, None, 1, 2, 1, 8, 8, 4, 0, None, None, None, None, 0, None) == -1
    assert lib.car_linear_packed_floats(0, 4) == 0
    # K=579 (+1 bias column) -> 19 chunks of 32; N=576 -> 18 tiles; 1024 floats per (chunk, tile)
    assert lib.car_linear_packed_floats(579, 576) == 19 * 18 * 1024
    with pytest.raises(RuntimeError):
        _lib.check(-1, "probe")


def test_round5_entries_validate_their_arguments(lib):
    """The entries added in round 5 return codes (never abort) on null pointers and impossible shapes, and report their sizes without a GPU."""
    assert lib.car_fused_tile_steps() == 8
    assert lib.car_kq_tail_floats() == 72 * 512 and lib.car_kq_bias_floats() == 2 * 128 + 16
    assert lib.car_attend_parts(None, None, 8, 576, 1, 2, 8, 8, None, None, 576, 1, None, None, None, None, None) == -1
    assert b"null pointer" in lib.car_last_error()
    assert lib.car_fused_samples_parts(*([None] * 4), 521, 521, 5, *([None] * 4), 1, 2, 8, 8, 256, 256, 0, *([None] * 6), None) == -1
    assert lib.car_lattice_encode_linear(None, 37, 37, 5, None, None, None, None, 1, 16, None, None, 576, 288, None, 288, 0, None) == -1
    assert lib.car_fused_rows(None, 37, 37, 5, *([None] * 7), 1, 8, 8, 3, None, None) == -1
    assert lib.car_key_query_logits(None, 576, None, None, 576, None, None, None, 16, None, None, None) == -1
    assert lib.car_kq_pack(*([None] * 9)) == -1 and lib.car_fused_pack_rows(*([None] * 8)) == -1
    assert lib.car_exchange_rows(None, None, None, None, 1, 3, 8, 64, 64, None, None, None, None) == -1
    assert lib.car_linear_wgrad(None, 4, None, 4, 8, 4, 4, 16, None, 4, None, None) == -1


def test_round6_entries_validate_their_arguments(lib):
    """The entries added in round 6: sizes without a GPU, codes (never aborts) on null pointers."""
    # the folded 128 x 128 layer and two 128 x 16 layers as fp16 hi / lo tiles (64 + 8 + 8 KB); four vectors + scales, then 128 x 128 of scratch
    assert lib.car_round2q_packed_floats() == lib.car_round2_packed_floats() + 2048 and lib.car_round2q_bias_floats() == 4 * 128 + 8 + 128 * 128
    assert lib.car_fused_bias_floats() == 288 + 3 * 128 + 16 + 128 * 128                                # the table + the packer's scratch
    assert lib.car_round2_logits_from_g(None, None, None, None, 1, 2, 8, 8, None, None) == -1
    assert b"null pointer" in lib.car_last_error()
    assert lib.car_round2q_pack(*([None] * 11)) == -1
    assert lib.car_attend_parts(None, None, 4, 576, 1, 2, 8, 8, None, None, 576, 1, None, None, None, None, None) == -1


def test_round6_training_entries_validate_their_arguments(lib):
    """The backward entries added in round 6 (second session): the binned scatter's workspace size without a GPU, codes on bad arguments."""
    import ctypes
    hs, ws = (ctypes.c_int * 3)(256, 128, 64), (ctypes.c_int * 3)(256, 128, 64)
    texels = 256 * 256 + 128 * 128 + 64 * 64
    n_maps, pts, gathers = 24, 12288, 2
    n = n_maps * texels + 1
    blocks = (n + 1023) // 1024
    want = ((2 * n + blocks + 4) * 4 + 15) // 16 * 16 + gathers * n_maps * pts * 3 * 4 * 8       # counters | start | block sums, then 8-byte records
    assert lib.car_scatter_workspace_bytes(hs, ws, 3, n_maps, pts, gathers) == want
    assert lib.car_scatter_workspace_bytes(None, ws, 3, n_maps, pts, gathers) == 0 and lib.car_scatter_workspace_bytes(hs, ws, 5, n_maps, pts, gathers) == 0
    assert lib.car_gather_bilinear_backward_binned(None, None, hs, ws, 3, n_maps, None, None, None, gathers, pts, 2, None, 608, 0, None, 0, None) == -1
    assert b"null pointer" in lib.car_last_error()
    assert lib.car_linear_x3_masked(None, 4, None, None, 4, 32, None, 32, 8, 0, None, 32, None) == -1
    assert b"act" in lib.car_last_error()


_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "void": None, "const char*": ctypes.c_char_p}


def _header_prototypes():
    """{name: (return type, [parameter, ...])} of include/car_hip.h, comments and preprocessor lines stripped; a parameter is its scalar type's
    name, or "*" for a pointer of any kind."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "car_hip.h")).read(), flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    text = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", text, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(car_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [p.strip() for p in " ".join(params.split()).split(",")]
        params = [] if params == ["void"] else ["*" if "*" in p else " ".join(w for w in p.split()[:-1] if w != "const") for p in params]
        protos[name] = (" ".join(ret.split()).replace(" *", "*"), params)
    return protos


def _abi_disagreements(protos, table):
    """Where ``table`` (the layout of _lib.SIGNATURES) departs from the header's prototypes: names, return types, arity, every parameter."""
    out = [f"{n}: on one side only" for n in sorted(set(protos) ^ set(table))]
    for name in sorted(set(protos) & set(table)):
        (ret, params), (res, args) = protos[name], table[name]
        if ret not in _RETURNS or _RETURNS[ret] is not res:
            out.append(f"{name}: returns {ret}, the table says {res}")
        if len(params) != len(args):
            out.append(f"{name}: {len(params)} parameters, the table has {len(args)}")
            continue
        for i, (p, a) in enumerate(zip(params, args)):
            ok = (a in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(a, ctypes._Pointer)) if p == "*" else _SCALARS.get(p) is a
            if not ok:
                out.append(f"{name}: parameter {i} is {p}, the table says {a.__name__}")
    return out


def test_signatures_mirror_the_header_type_by_type():
    """Every prototype of the header against _lib.SIGNATURES: the return type, the arity, and each parameter's scalar kind or pointer-ness (a
    prototype that changes in the header alone would still link, load and run, with shifted arguments)."""
    from cross_attention_renderer_amd import _lib
    protos = _header_prototypes()
    assert len(protos) == 116 == len(_lib.SIGNATURES)
    assert _abi_disagreements(protos, _lib.SIGNATURES) == []


def test_the_header_comparison_catches_drift():
    from cross_attention_renderer_amd import _lib
    protos = _header_prototypes()
    res, args = _lib.SIGNATURES["car_linear"]
    assert ctypes.c_long in args
    narrowed = dict(_lib.SIGNATURES, car_linear=(res, [ctypes.c_int if a is ctypes.c_long else a for a in args]))
    assert _abi_disagreements(protos, narrowed) == ["car_linear: parameter 7 is long, the table says c_int"]
    res, args = _lib.SIGNATURES["car_attend"]
    assert _abi_disagreements(protos, dict(_lib.SIGNATURES, car_attend=(res, args[:-1]))) == ["car_attend: 20 parameters, the table has 19"]
    assert _abi_disagreements(protos, dict(_lib.SIGNATURES, car_version=(ctypes.c_size_t, []))) == [
        f"car_version: returns int, the table says {ctypes.c_size_t}"]
    swapped = dict(_lib.SIGNATURES, car_colormap=(ctypes.c_int, [ctypes.c_int if a is ctypes.c_float else a for a in _lib.SIGNATURES["car_colormap"][1]]))
    assert len(_abi_disagreements(protos, swapped)) == 1


def test_the_checked_handle_raises(lib):
    from cross_attention_renderer_amd import _lib
    with pytest.raises(_lib.CarError) as err:
        _lib.api().car_linear(None, 4, None, 4, 4, None, 4, 1, 0, None)
    e = err.value
    assert isinstance(e, RuntimeError) and e.code == -1 and e.entry == "car_linear" and "null pointer" in e.text
    assert str(e) == f"car_linear failed (-1): {e.text}"
    with pytest.raises(RuntimeError) as by_hand:
        _lib.check(-1, "car_linear")
    assert str(by_hand.value) == str(e)
    # the raw handle stays raw
    assert lib is _lib.load() and lib.car_linear(None, 4, None, 4, 4, None, 4, 1, 0, None) == -1


def test_value_and_size_entries_do_not_raise(lib):
    from cross_attention_renderer_amd import _lib
    api = _lib.api()
    assert api.car_fused_tile_steps() == 8
    assert api.car_linear_packed_floats(0, 4) == 0
    assert api.car_profile_count() == 0
    assert api.car_frames_table_slot(3, 5) == -1                      # "no table": a value, not a status
    for name in _lib.VALUE_ENTRIES:
        assert _lib.SIGNATURES[name][0] is ctypes.c_int, name
    for name, (res, _) in _lib.SIGNATURES.items():
        checked = getattr(api, name).errcheck is _lib._errcheck
        assert checked == (res is ctypes.c_int and name not in _lib.VALUE_ENTRIES), name
        assert getattr(lib, name).errcheck is not _lib._errcheck, name


def test_user_call_turns_a_refused_argument_into_value_error(lib):
    from cross_attention_renderer_amd import _lib
    assert lib.car_linear(None, 4, None, 4, 4, None, 4, 1, 0, None) == -1            # leaves the library's message
    text = lib.car_last_error().decode()
    with pytest.raises(ValueError) as err:
        _lib.user_call(_lib.check, -1, "probe")
    assert str(err.value) == text and "null pointer" in text
    with pytest.raises(_lib.CarError) as err:
        _lib.user_call(_lib.check, -2, "probe")
    assert err.value.code == -2 and err.value.entry == "probe"
    assert _lib.user_call(lambda a, b: a + b, 1, 2) == 3


def test_lds_step_down_rule(lib):
    """RenderEngine._ran with a stand-in entry: only CAR_E_LAUNCH with the "cannot reserve" text steps down (False, with a warning)."""
    import warnings
    from cross_attention_renderer_amd import _lib
    from cross_attention_renderer_amd.engine import RenderEngine

    def failing(code, text):
        def car_stand_in(*args):
            raise _lib.CarError(code, "car_stand_in", text)
        return car_stand_in
    with pytest.warns(UserWarning, match="car_stand_in: car_stand_in: cannot reserve 163840 bytes of LDS: taking the next kernel of the library"):
        assert RenderEngine._ran(failing(-2, "car_stand_in: cannot reserve 163840 bytes of LDS"), 1, 2) is False
    with pytest.warns(UserWarning, match="^car_other: .*cannot reserve"):
        assert RenderEngine._ran(failing(-2, "cannot reserve"), what="car_other") is False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(_lib.CarError):
            RenderEngine._ran(failing(-2, "an illegal memory access was encountered"))
        with pytest.raises(_lib.CarError):
            RenderEngine._ran(failing(-1, "cannot reserve"))
        seen = []
        assert RenderEngine._ran(lambda *a: seen.append(a) or 0, 3, None) is True and seen == [(3, None)]


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "cross_attention_renderer_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S), f"{f} mentions the oracle"


def test_forward_refuses_cpu_tensors():
    """No CPU fallback: the render path fails loudly off-device."""
    import torch
    from cross_attention_renderer_amd import synthetic as S
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    m = CrossAttentionRenderer(model="tiny", n_view=2, npoints=4).eval()
    inp = S.stereo_scene(16, b=1, uv=S.pixel_grid(16, 16)[:8].contiguous())
    z = S.feature_maps(1, 2, 16, channels=(16, 16), strides=(2, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(inp, z=z)


def test_module_state_dict_matches_reference_table():
    """Parameter names/shapes of SURVEY.md §8b (checked against the real reference in make_golden.py)."""
    from cross_attention_renderer_amd.models import renderer_param_shapes
    t = renderer_param_shapes("midas_vit", n_view=2)
    assert t["query_encode_latent.weight"] == (576, 579, 1, 1)
    assert t["query_encode_latent_2.weight"] == (288, 576, 1, 1)
    assert t["update_val_merge.weight"] == (288, 582, 1, 1)
    assert t["latent_value.weight"] == (288, 576, 1, 1)
    assert t["key_map.weight"] == (128, 576, 1, 1)
    assert t["query_repeat_embed.weight"] == (128, 144, 1, 1)
    assert t["latent_avg_repeat_query.weight"] == (128, 153, 1, 1)
    assert t["encode_latent.weight"] == (128, 288, 1)
    assert t["phi.lin_in.weight"] == (128, 18) and t["phi.lin_z.2.weight"] == (128, 576)
    assert t["conv_map.weight"] == (64, 3, 7, 7)
    assert sum(int(__import__("math").prod(s)) for s in t.values()) == 1457955



def test_one_call_abi_host_side(lib):
    """Host-only parts of the one-call forward (include/car_hip.h): sizes, argument validation, linspace."""
    import torch
    from cross_attention_renderer_amd import _lib
    d = _lib.CarDims()
    d.b, d.V, d.R, d.P, d.H, d.W, d.n_levels, d.repeat_attention = 1, 2, 8192, 64, 256, 256, 3, 1
    for l, (c, h) in enumerate(((256, 64), (256, 128), (64, 256))):
        d.level_c[l], d.level_h[l], d.level_w[l] = c, h, h
    S = 2 * 8192 * 64
    assert 4 * S * (576 + 128) > lib.car_workspace_bytes(ctypes.byref(d)) >= 4 * S * (576 + 16)      # e, g dominate; no 128-wide query rows
    assert lib.car_plan_bytes(ctypes.byref(d)) >= 4 * (lib.car_fused_blob_floats() + lib.car_round2_packed_floats())
    # the three levels (64, 128, 256 wide: factors 4, 2, 1) share the lattice u in [-5, 515] (pad = r_max + 1 = 5)
    lh, lw, pad = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.car_lattice_shape(ctypes.byref(d), ctypes.byref(lh), ctypes.byref(lw), ctypes.byref(pad)) == 0
    assert (lh.value, lw.value, pad.value) == (521, 521, 5)
    lattice = 2 * 2 * 521 * 521 * 576
    up64 = lambda n: (n + 63) // 64 * 64
    texels = 2 * (64 * 64 + 128 * 128 + 256 * 256)
    assert lib.car_gmeta_offset(ctypes.byref(d)) == up64(lattice)
    assert lib.car_gmaps_floats(ctypes.byref(d)) == up64(lattice) + 64 + texels * 576        # lattice, gmeta, the projected levels
    d.level_h[0] = 60                                                                       # 128 is no multiple of 60: no common lattice
    assert lib.car_gmaps_floats(ctypes.byref(d)) == 0 and b"lattice" in lib.car_last_error()
    d.level_h[0] = 64
    off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.car_workspace_find(ctypes.byref(d), b"e", ctypes.byref(off), ctypes.byref(cnt)) == 0 and cnt.value == S * 576
    assert lib.car_workspace_find(ctypes.byref(d), b"nope", ctypes.byref(off), ctypes.byref(cnt)) == -1
    assert lib.car_profile_count() == 0
    d.V = 3                                                                                 # not covered by the one-call entry
    assert lib.car_workspace_bytes(ctypes.byref(d)) == 0 and b"n_view = 2" in lib.car_last_error()
    assert lib.car_render_forward(ctypes.byref(d), None, None, None, None, 0, None) == -1
    # car_linspace: torch's scalar formula; torch's vectorised CPU kernel may differ in the last ulp for n >= 16
    for n in (2, 5, 8, 15, 16, 32, 64, 128):
        buf = (ctypes.c_float * n)()
        lib.car_linspace(0.0, 1.0, n, buf)
        got, want = torch.tensor(list(buf)), torch.linspace(0, 1, n)
        assert (got - want).abs().max() <= 6e-8, n
        if n < 8:
            assert torch.equal(got, want)


@pytest.mark.parametrize("levels, P, total", [(((256, 64), (256, 128), (64, 256)), 64, 5897472),
                                              (((560, 8), (12, 16), (4, 32)), 33, 5823232)])      # two levels off the split-fp16 path
def test_plan_bytes_are_the_sum_of_the_slices(lib, levels, P, total):
    """car_plan_bytes exactly: every slice of the plan rounded up to 64 floats, the per-ray chains' layers taken from raychain_reference's
    own statement of them (layer_specs, PLAN_SLOTS), not from the library's table."""
    import raychain_reference as RC
    from cross_attention_renderer_amd import _lib
    d = _lib.CarDims()
    d.b, d.V, d.R, d.P, d.H, d.W, d.n_levels, d.repeat_attention = 1, 2, 64, P, 256, 256, 3, 1
    for l, (c, h) in enumerate(levels):
        d.level_c[l], d.level_h[l], d.level_w[l] = c, h, h
    chain = {}
    for which in ("mid", "tail"):
        for slot, (_, _, _, k, n, _) in zip(RC.PLAN_SLOTS[which], RC.layer_specs(which)):
            assert chain.setdefault(slot, (k, n)) == (k, n)
    assert sorted(chain) == list(range(14))
    terms = [P, lib.car_fused_blob_floats(), lib.car_fused_bias_floats(), 576 * 4, lib.car_round2q_packed_floats(), lib.car_round2q_bias_floats()]
    terms += [lib.car_linear_packed_floats(c, 576) for c, _ in levels]
    terms += [lib.car_linear_x3_packed_floats(c, 576) for c, _ in levels if c % 4 == 0 and c >= 32]
    terms += [lib.car_chain_packed_floats(k, n) for k, n in chain.values()]
    terms += [32, 288 + 128, 288 + 128 + 9 * 128 + 32]
    want = 4 * sum((int(t) + 63) // 64 * 64 for t in terms)
    got = lib.car_plan_bytes(ctypes.byref(d))
    assert got == want, (got, want, lib.car_last_error())
    assert got == total
