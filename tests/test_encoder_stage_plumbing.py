"""CPU checks for the host plumbing that get_z's device stages share (encoder.py: refuse_off_device, pack_parameters, the route switches,
MultiViewDPTEncoder._cached / _workspace / drop_device_caches): the full texts of every refusal and every switch, and the rules of the
cached slots and the workspaces.  No GPU and no library: the refusals are reached with stand-ins that carry is_cuda, dtype and
requires_grad, the slots with a stand-in for engine._Cached, the workspaces with CPU tensors."""
import pytest
import torch

from cross_attention_renderer_amd import encoder as E
from cross_attention_renderer_amd.models import CrossAttentionRenderer

F32, F64 = torch.float32, torch.float64


class T:
    """What a refusal looks at."""

    def __init__(self, is_cuda=True, dtype=F32, requires_grad=False):
        self.is_cuda, self.dtype, self.requires_grad = is_cuda, dtype, requires_grad


def bare_encoder():
    """A MultiViewDPTEncoder without its 123 M parameters: the switches, the slots and nothing else."""
    enc = E.MultiViewDPTEncoder.__new__(E.MultiViewDPTEncoder)
    torch.nn.Module.__init__(enc)
    for slot in ("_vit_packed", "_trunk_packed", "_tokens_packed", "_decoder_packed"):
        setattr(enc, slot, None)
    for slot in ("_vit_work", "_trunk_work", "_decoder_work"):
        setattr(enc, slot, {})
    return enc


# ---- the refusals: the full texts, as the four sites stated them before they shared one function ---------------------------------------------
# switch, value at the site, its (CUDA, dtype, recording) texts; {} stands for the reported dtype
TEXTS = {
    ("trunk_route", "device"): (
        "trunk_route = 'device' needs the images and the encoder on a CUDA device; CPU tensors run on trunk_route = 'torch'",
        "trunk_route = 'device' computes in float32 (got {}); other dtypes run on trunk_route = 'torch'",
        "trunk_route = 'device' is inference only (its kernels have no backward): call it under torch.no_grad(), or "
        "keep trunk_route = 'torch' for a forward that autograd records"),
    ("vit_route", "device"): (
        "vit_route = 'device' needs the images and the encoder on a CUDA device; CPU tensors run on vit_route = 'torch'",
        "vit_route = 'device' computes in float32 (got {}); other dtypes run on vit_route = 'torch'",
        "vit_route = 'device' is inference only (its kernels have no backward): call it under torch.no_grad(), or "
        "keep vit_route = 'torch' for a forward that autograd records"),
    ("decoder_route", "device"): (
        "decoder_route = 'device' needs the images and the encoder on a CUDA device; CPU tensors run on decoder_route = 'torch'",
        "decoder_route = 'device' computes in float32 (got {}); other dtypes run on decoder_route = 'torch'",
        "decoder_route = 'device' is inference only (its kernels have no backward): call it under torch.no_grad(), or "
        "keep decoder_route = 'torch' for a forward that autograd records"),
    ("encoder_route", "device_full"): (
        "encoder_route = 'device_full' needs the images and the model on a CUDA device; CPU tensors run on encoder_route = 'torch'",
        "encoder_route = 'device_full' computes in float32 (got {}); other dtypes run on encoder_route = 'torch'",
        "encoder_route = 'device_full' is inference only (its kernels have no backward): call get_z under torch.no_grad(), or "
        "keep encoder_route = 'torch' for a forward that autograd records"),
}
VIT_TRAIN_TEXTS = (
    "vit_route = 'device_train' needs the images and the encoder on a CUDA device; CPU tensors run on vit_route = 'torch'",
    "vit_route = 'device_train' computes in float32 (got {}); other dtypes run on vit_route = 'torch'")


def refuse(switch, value, acts, params, recorded):
    """The call each site makes."""
    if switch == "encoder_route":                                           # this form looks only at what it was handed
        return CrossAttentionRenderer._refuse_off_device(None, acts[0], params)
    return E.refuse_off_device(switch, value, acts, params, recorded, **({"inference": "device"} if switch == "vit_route" else {}))


def message(*a):
    with pytest.raises(ValueError) as e:
        refuse(*a)
    return str(e.value)


@pytest.mark.parametrize("switch,value", list(TEXTS))
def test_each_refusal_gives_the_full_text(switch, value):
    cuda, dtype, recording = TEXTS[(switch, value)]
    n_acts = {"trunk_route": 2, "vit_route": 1, "decoder_route": 4, "encoder_route": 1}[switch]
    ok = lambda: [T() for _ in range(n_acts)]
    params = [T(), T()]
    with torch.enable_grad():
        refuse(switch, value, ok(), params, ok() + params)                  # nothing to refuse
        # CUDA: an activation or a parameter off the device
        assert message(switch, value, ok()[:-1] + [T(is_cuda=False)], params, []) == cuda
        assert message(switch, value, ok(), [T(), T(is_cuda=False)], []) == cuda
        # dtype: the FIRST activation's is the one reported, whichever tensor is off
        assert message(switch, value, [T(dtype=F64)] + ok()[1:], params, []) == dtype.format("torch.float64")
        assert message(switch, value, ok(), [T(), T(dtype=torch.float16)], []) == dtype.format("torch.float32")
        if n_acts > 1:
            assert message(switch, value, ok()[:-1] + [T(dtype=F64)], params, []) == dtype.format("torch.float32")
        # recording: any tensor of the recorded set, in grad mode only
        for i in range(n_acts + 2):
            acts, ps = ok(), [T(), T()]
            (acts + ps)[i].requires_grad = True
            assert message(switch, value, acts, ps, acts + ps) == recording
            with torch.no_grad():
                refuse(switch, value, acts, ps, acts + ps)
        # the order: CUDA, then dtype, then recording
        bad = T(is_cuda=False, dtype=F64, requires_grad=True)
        assert message(switch, value, [bad] + ok()[1:], params, [bad]) == cuda
        bad = T(dtype=F64, requires_grad=True)
        assert message(switch, value, [bad] + ok()[1:], params, [bad]) == dtype.format("torch.float64")


def test_the_recorded_set_is_its_own_argument():
    """The encoder's stages hand in x and ALL of the encoder's parameters, not the stage's own: a tensor outside acts and params refuses."""
    acts, params = [T()], [T()]
    with torch.enable_grad():
        assert message("decoder_route", "device", acts, params, iter([T(), T(requires_grad=True)])) == TEXTS[("decoder_route", "device")][2]
        E.refuse_off_device("decoder_route", "device", [T(requires_grad=True)], [T(requires_grad=True)], [T()])
        E.refuse_off_device("decoder_route", "device", [T(requires_grad=True)], [T(requires_grad=True)], None)


def test_vit_route_prints_its_current_value_and_names_the_inference_route():
    cuda, dtype = VIT_TRAIN_TEXTS
    assert message("vit_route", "device_train", [T(is_cuda=False)], [T()], None) == cuda
    assert message("vit_route", "device_train", [T()], [T(dtype=F64)], None) == dtype.format("torch.float32")
    with torch.enable_grad():
        # _blocks_recorded_on_device and recorded_elsewhere make the first two only
        E.refuse_off_device("vit_route", "device_train", [T(requires_grad=True)], [T(requires_grad=True)], None, inference="device")
        # the third names the route that is inference only, whatever the switch holds
        assert message("vit_route", "device_train", [T()], [T()], [T(requires_grad=True)]) == TEXTS[("vit_route", "device")][2]


# ---- the route switches -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch,values,text", [
    ("vit_route", ("torch", "device", "device_train"), "vit_route must be 'torch', 'device' or 'device_train' (got 'hip')"),
    ("trunk_route", ("torch", "device"), "trunk_route must be 'torch' or 'device' (got 'hip')"),
    ("decoder_route", ("torch", "device"), "decoder_route must be 'torch' or 'device' (got 'hip')")])
def test_each_switch_takes_its_values_and_refuses_another(switch, values, text):
    enc = bare_encoder()
    for v in values:
        setattr(enc, switch, v)
        assert getattr(enc, switch) == v
    with pytest.raises(ValueError) as e:
        setattr(enc, switch, "hip")
    assert str(e.value) == text and getattr(enc, switch) == values[-1]
    if switch != "vit_route":
        with pytest.raises(ValueError, match="got 'device_train'"):
            setattr(enc, switch, "device_train")
    assert E.MultiViewDPTEncoder.VIT_ROUTES == ("torch", "device") and E.MultiViewDPTEncoder.VIT_BLOCK_ROUTES == ("torch", "device", "device_train")
    other = bare_encoder()                                                  # the value is the instance's
    setattr(other, switch, "torch")
    assert getattr(enc, switch) == values[-1] and switch not in enc.state_dict()


# ---- the packer ---------------------------------------------------------------------------------------------------------------------------------
def test_pack_parameters_makes_the_copies_the_table_and_the_buffer():
    a = torch.nn.Parameter(torch.arange(6.0).reshape(2, 3))
    b = torch.arange(12.0).reshape(3, 4).t()                                # not contiguous
    seen = []
    packed = E.pack_parameters([a, b], "cpu", 18, lambda table, src, out: seen.append((table, src, out)))
    (table, src, out), = seen
    assert out is packed and packed.shape == (18,) and packed.dtype == F32 and packed.device.type == "cpu"
    assert len(table) == len(src) == 2 and [table[i] for i in range(2)] == [t.data_ptr() for t in src]
    assert all(t.is_contiguous() and not t.requires_grad for t in src)
    assert src[0].data_ptr() == a.data_ptr() and torch.equal(src[1], b) and src[1].data_ptr() != b.data_ptr()


# ---- the cached slots ---------------------------------------------------------------------------------------------------------------------------
class Cached:
    """engine._Cached's stand-in: says when to build."""
    made = 0

    def __init__(self):
        type(self).made += 1
        self.value, self.asked, self.dropped = None, [], 0

    def get(self, src, extra, build):
        self.asked.append((src, extra))
        if self.value is None:
            self.value = build()
        return self.value

    def drop(self):
        self.value, self.dropped = None, self.dropped + 1


def test_cached_slot_is_made_once_and_builds_when_the_cache_says_so(monkeypatch):
    from cross_attention_renderer_amd import engine
    monkeypatch.setattr(engine, "_Cached", Cached)
    Cached.made = 0
    enc, built = bare_encoder(), []
    src, extra = [torch.zeros(1)], ("cpu", 3)

    def build():
        built.append(1)
        return f"pack {len(built)}"
    assert enc._cached("_tokens_packed", src, extra, build) == "pack 1"
    slot = enc._tokens_packed
    assert isinstance(slot, Cached) and Cached.made == 1 and enc._vit_packed is None and enc._trunk_packed is None and enc._decoder_packed is None
    assert enc._cached("_tokens_packed", src, extra, build) == "pack 1" and enc._tokens_packed is slot and Cached.made == 1 and built == [1]
    assert len(slot.asked) == 2 and all(s is src and e is extra for s, e in slot.asked)      # passed through unchanged
    slot.drop()
    assert enc._cached("_tokens_packed", src, extra, build) == "pack 2" and enc._tokens_packed is slot and built == [1, 1]
    held = Cached()                                                         # a slot somebody filled is used as it is
    enc._vit_packed = held
    assert enc._cached("_vit_packed", src, (), build) == "pack 3" and enc._vit_packed is held and Cached.made == 2


# ---- the workspaces -----------------------------------------------------------------------------------------------------------------------------
def test_workspace_holds_one_entry_and_replaces_it_on_a_new_key():
    enc, asked = bare_encoder(), []

    def sizes(*n):
        def nbytes():
            asked.append(n)
            return n
        return nbytes
    work, twork = enc._workspace("_trunk_work", (2, 32, 32, "cpu"), "cpu", sizes(64, 16))
    assert work.shape == (16,) and twork.shape == (4,) and work.dtype == twork.dtype == F32
    again = enc._workspace("_trunk_work", (2, 32, 32, "cpu"), "cpu", sizes(8, 8))
    assert again[0] is work and again[1] is twork and asked == [(64, 16)]               # the same key: the same tensors, no size asked
    other, _ = enc._workspace("_trunk_work", (1, 32, 32, "cpu"), "cpu", sizes(32, 16))
    assert other is not work and other.shape == (8,) and list(enc._trunk_work) == [(1, 32, 32, "cpu")] and asked == [(64, 16), (32, 16)]
    assert enc._vit_work == {} and enc._decoder_work == {}

    class Lib:
        @staticmethod
        def car_vit_workspace_bytes(b, S, dim):
            asked.append(("vit", b, S, dim))
            return 4 * b * S * dim
    w = enc._vit_workspace(Lib, 2, 5, 64, "cpu")                            # _VitBlocksTrain's way in keeps its signature and its key
    assert isinstance(w, torch.Tensor) and w.shape == (2 * 5 * 64,) and list(enc._vit_work) == [(2, 5, "cpu")]
    assert enc._vit_workspace(Lib, 2, 5, 64, "cpu") is w and asked[2:] == [("vit", 2, 5, 64)]
    assert enc._vit_workspace(Lib, 2, 6, 64, "cpu") is not w and list(enc._vit_work) == [(2, 6, "cpu")]


# ---- drop_device_caches -------------------------------------------------------------------------------------------------------------------------
def test_drop_device_caches_reaches_every_slot():
    enc = bare_encoder()
    held = {slot: Cached() for slot in ("_vit_packed", "_trunk_packed", "_tokens_packed", "_decoder_packed")}
    for slot, c in held.items():
        c.value = slot
        setattr(enc, slot, c)
    for slot in ("_vit_work", "_trunk_work", "_decoder_work"):
        setattr(enc, slot, {"key": 1})
    enc.drop_device_caches()
    assert all(c.dropped == 1 and c.value is None and getattr(enc, slot) is c for slot, c in held.items())
    assert enc._vit_work == {} and enc._trunk_work == {} and enc._decoder_work == {}
    fresh = bare_encoder()                                                  # slots never used are None and stay None
    fresh.drop_device_caches()
    assert fresh._vit_packed is None and fresh._decoder_packed is None and fresh._trunk_work == {}
    assert set(E.MultiViewDPTEncoder._PACKED_SLOTS) == set(held) and set(E.MultiViewDPTEncoder._WORK_SLOTS) == {"_vit_work", "_trunk_work", "_decoder_work"}
