"""Host side of the render forward: what ``CrossAttentionRenderer.forward`` runs.

Every arithmetic step of the reference forward (models.py:206-621) is a HIP kernel of ``libcar_hip.so`` reached through the
C ABI (``include/car_hip.h``); PyTorch is used for device memory, the stream handle and the (reference-identical) 4x4 pose
algebra on the host.  There is no CPU or eager-PyTorch fallback: tensors must live on a ROCm device and the library must load.

Two routes, both dispatched by ``RenderEngine._render``; this module holds what they share (the caches and weight packing, the
plan and lattice builders, the budgets, the kernel wrappers):
  * the reference's default configuration (n_view = 2, three pyramid levels, 576 channels; epipolar sampling or ``no_sample``'s depth
    sampling, with or without the second attention round) goes through the
    ONE-CALL C ABI — ``car_plan_build`` once per set of weights, ``car_project_maps`` once per stereo pair,
    ``car_render_forward`` per batch of rays (csrc/car_render.hip over csrc/car_pack.hip and csrc/car_lattice.hip: weight packing, the
    lattice merge and the launch sequence are C++).  ``one_call.render`` only sizes the calls;
  * the other constructor variants (n_view 1 / 3, no_latent_concat, other widths) are sequenced stage by stage
    (``staged.forward``) — also the A/B partner of the first route in the tests.  The training forward (training.render_train)
    is the same function with a ``staged.Saved`` record: the literal stage forms, every activation its backward reads kept.

Stage map:
  a3 poses.pack_poses (host, torch.inverse like the reference)          a11-a13, a15, a17  car_linear (fp32 MFMA)
  a4-a6 car_ray_setup / car_sample_setup                                  a14-a16            car_attend
  a7/a10 car_gather_bilinear                                              a18                car_finalize
"""
from __future__ import annotations

import collections
import ctypes
from typing import Dict, List, Optional

import torch

from . import _lib
from .poses import pack_poses

Tensor = torch.Tensor

RELU_IN, RELU_OUT, ACCUM, NO_GLDS = 1, 2, 4, 8
WGRAD_FP32 = 16            # CAR_WGRAD_FP32 (include/car_hip.h)
PLACE_PLAIN, PLACE_OWN, PLACE_OTHER2 = 0, 1, 2


_ptr, _stream = _lib.ptr, _lib.stream


def _levels(maps: List[Tensor], rows: Optional[slice] = None):
    """Channel-last levels [n, H_l, W_l, C_l] as the C ABI takes them: (pointers, channels, heights, widths, number of levels);
    ``rows``: the pointers lead to that slice of every level's maps."""
    L = len(maps)
    return ((ctypes.c_void_p * L)(*[(t if rows is None else t[rows]).data_ptr() for t in maps]), (ctypes.c_int * L)(*[t.shape[3] for t in maps]),
            (ctypes.c_int * L)(*[t.shape[1] for t in maps]), (ctypes.c_int * L)(*[t.shape[2] for t in maps]), L)


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class PackedLinear:
    """A linear / 1x1-conv layer re-laid out for the MFMA kernel (``car_linear_pack``)."""

    def __init__(self, weight: Tensor, bias: Optional[Tensor], device, name: str = ""):
        self.name = name
        lib = _lib.api()
        w = weight.detach().reshape(weight.shape[0], -1).to(device=device, dtype=torch.float32).contiguous()
        self.N, self.K = int(w.shape[0]), int(w.shape[1])
        bdev = None if bias is None else bias.detach().to(device=device, dtype=torch.float32).contiguous()
        n = lib.car_linear_packed_floats(self.K, self.N)
        self.packed = torch.empty(n, device=device, dtype=torch.float32)
        lib.car_linear_pack(_ptr(w), self.K, _ptr(bdev), self.K, self.N, _ptr(self.packed), _stream())
        # the same layer for the split-fp16 kernel (car_linear_x3: 5x the fp32 pipe's ceiling): layers wide enough to matter, whose
        # outputs fill whole 32-channel tiles; the narrow ones (point embeddings, the 16-wide query input, rgb) stay on car_linear
        self.x3 = None
        if self.N % 32 == 0 and self.K >= 64:
            tiles = torch.empty(lib.car_linear_x3_packed_floats(self.K, self.N), device=device, dtype=torch.float32)
            lib.car_linear_x3_pack(_ptr(w), self.K, self.K, self.N, _ptr(tiles), _stream())
            self.x3 = (tiles, bdev)


def _mode(m) -> str:
    """How the staged forward makes the per-sample features e: "concat2" (two views, point MLP over own ‖ other features), "concat3"
    (the three-view exchange), "single" (one view, update_val_merge over features ‖ point channels), "plain" (no_latent_concat: the
    gathered features themselves)."""
    if m.no_latent_concat:
        return "plain"
    return {1: "single", 2: "concat2", 3: "concat3"}[m.n_view]


_Layers = collections.namedtuple("_Layers", "head attention round2 decoder blocks")


def _render_layers(m) -> _Layers:
    """The linear layers a module's render path reads, by part: ``head`` (what makes e, per _mode), ``attention``, ``round2`` (read with
    repeat_attention), ``decoder`` (its two ends, then block by block) and, again, the decoder's ``blocks`` as [(lin_z, fc_0, fc_1)]."""
    qel = ["query_encode_latent", "query_encode_latent_2"]
    blocks = [(f"phi.lin_z.{i}", f"phi.blocks.{i}.fc_0", f"phi.blocks.{i}.fc_1") for i in range(m.phi.n_blocks)]
    return _Layers(head={"concat2": qel, "concat3": qel, "single": ["update_val_merge"], "plain": []}[_mode(m)],
                   attention=["latent_value", "key_map", "key_map_2", "query_embed", "query_embed_2"],
                   round2=["query_repeat_embed", "query_repeat_embed_2", "encode_latent"],
                   decoder=["phi.lin_in", "phi.lin_out"] + [n for block in blocks for n in block], blocks=blocks)


class _Cached:
    """One object built on the device from source tensors and plain values, rebuilt when any of them changes.  The key is each source's
    data pointer, _version, shape, strides, dtype and device, plus the plain values.  The sources are held beside the value as storage
    aliases (``t.detach()``: ``p.data = new`` swaps a Parameter's storage under the same object), so no address in the key can be handed
    to another tensor — with a _version that may match — while the entry lives."""

    def __init__(self):
        self.key = self.src = self.value = None

    @staticmethod
    def key_of(src, extra=()) -> tuple:
        return tuple((t.data_ptr(), t._version, t.shape, t.stride(), t.dtype, t.device) for t in src) + tuple(extra)

    def holds(self, src, extra=()) -> bool:
        return self.value is not None and self.key == self.key_of(src, extra)

    def get(self, src, extra, build):
        key = self.key_of(src, extra)
        if self.value is None or key != self.key:
            self.drop()                # the old value goes before the builder allocates the new one (a lattice is 2.9 GB at c2)
            value = build()
            self.key, self.src, self.value = key, [t.detach() for t in src], value
        return self.value

    def put(self, src, extra, value) -> None:
        self.key, self.src, self.value = self.key_of(src, extra), [t.detach() for t in src], value

    def drop(self) -> None:
        self.key = self.src = self.value = None


class RenderEngine:
    """Per-module state of the HIP path: what it builds on the device once and reuses while its sources hold (_Cached) — packed layers,
    the channel-last pyramid and its lattice, pose records — and the switches of its routes."""

    def __init__(self, module):
        self.m = module
        self.lib = _lib.api()            # the checked handle: a negative status raises _lib.CarError
        # _weights, _channel_last, _projected_maps, _poses, _plan_for, _plan16_for, _pair_for, staged._exchange_lattice; _packed_layers by packer
        self._packed, self._pyramid, self._gmaps, self._pose = _Cached(), _Cached(), _Cached(), _Cached()
        self._plan, self._plan16, self._pairs, self._xlat = _Cached(), _Cached(), _Cached(), _Cached()
        self._layer_packs: Dict[str, _Cached] = collections.defaultdict(_Cached)
        self._steps: Dict[tuple, Tensor] = {}
        self.linear_flags = 0          # tests may set NO_GLDS for A/B
        self.linear_x3 = True          # stage entries: wide layers on the split-fp16 path (car_linear_x3); False = all on the fp32 pipe
        self.linear_x3_min_rows = 2048 # below this many rows a launch is latency bound either way (a training step has 2304 rays: 16.2 -> 15.8 ms)
        self.pose_records = None       # tests: (b*V, 96) CarPose records to use instead of the host pose algebra
        # "host": the reference's torch.inverse on the CPU wherever the cameras live (strict parity; cameras on the GPU cost one small
        # download per new pose); "device": car_pose_setup when the cameras are on the GPU (no host round trip, budgeted parity)
        # -> the module's ``pose_route`` attribute (scripts set it before the first forward creates the engine)
        self.last_pose_sync_ms = 0.0
        # first point-MLP layer as a gather over per-texel pre-projected maps (csrc/car_encode.hip) instead of a
        # K=579 GEMM per sample; False selects the literal gather -> GEMM pipeline (A/B and stage tests)
        self.project_maps = True
        # the one-call C ABI with the fused per-sample kernel (needs V == 2, three pyramid levels, C == 576); False keeps the
        # stage-by-stage pipeline of this module (A/B and stage tests)
        self.fuse_samples = True
        self.fuse_round2 = True        # staged route: round-2 per-sample layer + logits in one kernel (csrc/car_round2.hip)
        # one-call route: the first attention round folds the fused kernel's per-step-group partial sums (default); False = it streams
        # the rows of e as in rounds 1-4 (CAR_PHASE_ROWS_FIRST_ROUND: A/B measurements and tests)
        self.first_round_parts = True
        # one-call route: the second attention round in one launch (car_attend_round2, default wherever P % 32 == 0); False = logits and
        # attention as two launches (CAR_PHASE_SPLIT_SECOND_ROUND: A/B measurements and tests)
        self.second_round_merged = True
        self.wgrad_fp32 = False        # training: True keeps the wide layers' weight gradients on the fp32 matrix pipe (CAR_WGRAD_FP32) instead of bf16 x 3
        self.scatter_atomics = False   # training: True scatters the pyramid's gradient with fp32 atomics, one launch per gather (A/B and tests); False = taps binned by texel
        self.fuse_kq = True            # staged route: key / query chains and the first round's logits in one kernel (car_key_query_logits); False = five launches (A/B)
        # three-view exchange, first + second layer: "rows" = the fused per-sample kernel's source pass over the rows (car_fused_rows, default);
        # True = the gather-fed linear kernel (car_lattice_encode_linear); False = two launches (A/B partners)
        self.fuse_exchange = "rows"
        # sizing of the one-call route (tests shrink them to force several calls)
        self.max_workspace_bytes: Optional[int] = None     # None: 85 % of the free device memory
        self.max_level_bytes: Optional[int] = None         # tests: lattice bytes of one call (forces scene groups); None = no limit
        self.max_pair_bytes: Optional[int] = None          # tests: bytes of one lattice buffer (forces lattice groups, each projected on its own)
        self.last_pair_groups = 1      # number of lattice buffers (car_project_maps calls' scene groups) of the last forward
        self.last_calls = 0            # number of car_render_forward calls the last forward was split into
        self._pf = None                # prefetch(): announced stereo pairs (key -> channel-last pyramid + lattice), projected on a side stream
        self._pf_stream = None
        self.prefetch_side_stream = True   # False (A/B): prefetch() projects on the launch stream itself
        self.last_precision = None     # "fp32" / "fp16": the arithmetic of the last forward's fused per-sample kernel
        self._work: Optional[Tensor] = None

    @property
    def _maps(self) -> Optional[List[Tensor]]:
        """The cached channel-last pyramid of _channel_last (None: none)."""
        return self._pyramid.value

    @property
    def _pair(self) -> Optional[Tensor]:
        """The cached lattice buffer of _pair_for (None: none)."""
        return self._pairs.value

    @property
    def _plan_w(self):
        """struct CarWeights of the cached plan (the tensors its pointers lead to ride on it as ``keep``): what car_plan_f16_build reads."""
        return self._plan.value[1]

    @property
    def _pair_key(self):
        return self._pairs.key

    @_pair_key.setter
    def _pair_key(self, key) -> None:
        self._pairs.key = key          # None: the next _pair_for re-projects (bench.py times the pair set-up this way)

    @property
    def render_precision(self) -> str:
        """-> the module's ``render_precision`` ("fp32", the default, or the opt-in "fp16": DESIGN.md 4.11)."""
        p = getattr(self.m, "render_precision", "fp32")
        if p not in ("fp32", "fp16"):
            raise ValueError(f"render_precision must be 'fp32' or 'fp16' (got {p!r})")
        return p

    def _one_call_refusal(self, b: int, R: int, z: List[Tensor]) -> Optional[str]:
        """Why this forward cannot take the one-call route (None: it can).  The fp16 precision exists on that route only."""
        m = self.m
        if not (self.fuse_samples and self.project_maps):
            return "the engine's fuse_samples / project_maps switches select the stage route"
        if m.n_view != 2:
            return f"n_view = {m.n_view} (the one-call route renders two context views)"
        if m.no_latent_concat:
            return "no_latent_concat (the one-call route concatenates the two views' latents)"
        if len(z) != 3 or sum(t.shape[1] for t in z) != 576 or m.hidden_dim != 128 or m.phi.n_blocks != 3 or m.phi.d_hidden != 128:
            return "widths other than midas_vit's (three pyramid levels of 576 channels in all, hidden width 128, three decoder blocks)"
        if not self._common_lattice(z):
            return "a pyramid whose levels have no common lattice (each must be an integer factor coarser than the widest, same in both directions)"
        if not self._lattice_fits(b, R, z):
            return "a lattice beyond 2 GiB per view and padding mode (finest level wider than ~470 pixels)"
        return None

    @property
    def pose_route(self) -> str:
        return getattr(self.m, "pose_route", "host")

    @pose_route.setter
    def pose_route(self, route: str) -> None:
        if route not in ("host", "device"):
            raise ValueError("pose_route must be 'host' or 'device'")
        self.m.pose_route = route

    # ------------------------------------------------------------------ weights
    def _weights(self, device) -> Dict[str, PackedLinear]:
        m = self.m
        sd = dict(m.named_parameters())
        layers = _render_layers(m)
        qre, qre_2, encode_latent = layers.round2                    # query_repeat_embed is packed as its two halves below
        names = layers.head + layers.attention + [encode_latent, qre_2] + layers.decoder

        def build():
            pk = {n: PackedLinear(sd[n + ".weight"], sd[n + ".bias"], device, n) for n in names}
            if m.n_view == 3 and not m.no_latent_concat:
                # inference keeps e in component-major order [S, 3, C/2] (what query_encode_latent_2 writes) instead of the reference's channel-
                # major interleave e[s, 3 ch + k] (models.py:446): the layers that read e get their input columns permuted once instead
                for n in ("latent_value", "key_map"):
                    w = sd[n + ".weight"].reshape(sd[n + ".weight"].shape[0], -1)
                    pk[n + ".kmajor"] = PackedLinear(w.view(w.shape[0], -1, 3).permute(0, 2, 1).reshape(w.shape[0], -1), sd[n + ".bias"], device, n + ".kmajor")
            wr = sd["query_repeat_embed.weight"].reshape(128, -1)
            pk["query_repeat_embed.h"] = PackedLinear(wr[:, :128], None, device, "query_repeat_embed.h")           # z_embed half, per ray
            pk["query_repeat_embed.g"] = PackedLinear(wr[:, 128:], sd["query_repeat_embed.bias"], device, "query_repeat_embed.g")  # local_coords half
            return pk
        return self._packed.get([sd[n + k] for n in names + [qre] for k in (".weight", ".bias")], (str(device),), build)

    # ------------------------------------------------------------------ feature maps
    def _channel_last(self, z: List[Tensor]) -> List[Tensor]:
        """Channel-last copies of the pyramid, cached on the z tensors."""
        def build():
            pf = self._pf.pop(_Cached.key_of(z), None) if self._pf else None
            if pf is None:
                return [self._as_channel_last(t) for t in z]
            # this pyramid was announced by prefetch(): its channel-last copies and its lattice are (being) made on the side stream. The
            # launch stream waits for them here — at the latest possible point — and takes them over, the lattice with the plan it was
            # projected with (a plan rebuilt since then no longer matches it: _pair_for re-projects)
            torch.cuda.current_stream().wait_event(pf["done"])
            self._pairs.put([pf["plan"], *z], (0, pf["b"]), pf["pair"])
            return pf["maps"]
        return self._pyramid.get(z, (), build)

    @staticmethod
    def _as_channel_last(t: Tensor) -> Tensor:
        """[n, C, H, W] -> [n, H, W, C] rows for the kernels: a VIEW when the level already lies channel-last in memory (torch.channels_last:
        what an encoder run in that memory format returns, and what the training scripts allocate) — no copy; a channel-last copy
        otherwise (the reference's NCHW pyramid)."""
        tt = t.detach()
        if tt.dtype == torch.float32:
            v = tt.permute(0, 2, 3, 1)
            if v.is_contiguous():
                return v
        return tt.float().permute(0, 2, 3, 1).contiguous()

    def prefetch(self, z: List[Tensor]) -> bool:
        """Announces the NEXT stereo pair's pyramid while the current frame is still to be rendered (the eval loop knows its next batch:
        eval_realestate10k.py:142-161): the channel-last copies and car_project_maps of ``z`` run on a side stream, ordered behind
        everything queued so far (so behind the ``get_z`` that made ``z``) and beside the render that follows on the launch stream; the
        forward that later receives these very tensors waits for the side stream's event and finds its lattice ready.  Needs a plan (one
        forward with the current weights) and room for a second lattice; returns False — and does nothing — otherwise, or when ``z`` is the
        pyramid already in place.  Same kernels, same arguments, same results as the projection inside forward."""
        if self._plan.value is None or not z or z[0].device.type != "cuda":
            return False
        b = z[0].shape[0] // self.m.n_view
        if self._one_call_refusal(b, 48, z) is not None:
            return False
        if self._pyramid.holds(z) and self._pair is not None:
            return False
        if self._pf is None:
            self._pf = {}
        key = _Cached.key_of(z)
        if key in self._pf:
            return True
        dev = z[0].device
        d = self._dims(b, 48, z)
        if not self._plan.holds(*self._plan_sources(d, dev)):
            return False                                             # the plan in place was built for other dims or weights
        plan, _ = self._plan.value
        need = 4 * self.lib.car_gmaps_floats(ctypes.byref(d))
        if need == 0 or need > self._free_budget(dev) // 3:
            return False                                             # another lattice must leave the workspace its room
        with torch.cuda.device(dev):
            if self._pf_stream is None:
                self._pf_stream = torch.cuda.Stream(device=dev)
            main = torch.cuda.current_stream()
            side = self._pf_stream if self.prefetch_side_stream else main
            # the loop announces pair i + 1 BEFORE it renders pair i (announced one step earlier and not taken over yet): two announced pairs
            # may wait; an older one nobody came for is dropped — once the side stream is done with it (its buffers go back to the launch
            # stream's pool)
            while len(self._pf) >= 2:
                old = self._pf.pop(next(iter(self._pf)))
                main.wait_event(old["done"])
            # buffers come from the launch stream's pool; the side stream starts behind everything queued there so far (the allocator's
            # reuse of a freed block is ordered on the launch stream) and the tensors are handed back to it through the event
            maps = [torch.empty(t.shape[0], t.shape[2], t.shape[3], t.shape[1], device=dev, dtype=torch.float32) for t in z]
            pair = torch.empty(need // 4, device=dev, dtype=torch.float32)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                for dst, t in zip(maps, z):
                    dst.copy_(t.detach().permute(0, 2, 3, 1))
                self.lib.car_project_maps(ctypes.byref(d), _ptr(plan), _levels(maps)[0], _ptr(pair), ctypes.c_void_p(side.cuda_stream))
                done = torch.cuda.Event()
                done.record(side)
            # the entry holds everything the side stream reads (z, the plan) and writes until the launch stream has waited for ``done``
            self._pf[key] = {"src": list(z), "maps": maps, "pair": pair, "done": done, "plan": plan, "b": b}
        return True

    def drop_prefetched(self) -> None:
        """Forgets every announced pair (after the side stream is done with them)."""
        if self._pf:
            for old in self._pf.values():
                torch.cuda.current_stream().wait_event(old["done"])
        self._pf = None

    _PARAMETER_CACHES = ("_packed", "_gmaps", "_plan", "_plan16", "_pairs", "_xlat", "_layer_packs")

    def park_parameter_caches(self) -> dict:
        """Sets aside everything built from the module's parameters (packed layers, plans, projected levels, lattices) and starts from
        empty caches; returns what was set aside for ``restore_parameter_caches``.  The keys see an in-place update through the tensor's
        _version, and torch's fused optimizers (Adam(fused=True), training.make_adam) update parameters without advancing it: a render
        that must see the parameters as they are now — the validation pass between optimizer steps — cannot trust the keys
        (CrossAttentionRenderer.train parks on leaving train() mode and restores on returning, so the training loop's own caches are
        exactly what they would have been without the pass)."""
        parked = {n: getattr(self, n) for n in self._PARAMETER_CACHES}
        for n in self._PARAMETER_CACHES:
            setattr(self, n, collections.defaultdict(_Cached) if n == "_layer_packs" else _Cached())
        self.drop_prefetched()
        return parked

    def restore_parameter_caches(self, parked: dict) -> None:
        """Puts back what ``park_parameter_caches`` set aside; what was built in between is released."""
        self.drop_prefetched()
        for n in self._PARAMETER_CACHES:
            setattr(self, n, parked[n])

    def _projected_maps(self, maps: List[Tensor], device):
        """G_l = query_encode_latent.weight[:, ch_l] F_l per pyramid level (channel-last, C wide), plus the [C,4]
        table (W1[:, C:C+3], b1).  Recomputed only when the pyramid or the layer's parameters change."""
        m = self.m
        w1, b1 = m.query_encode_latent.weight, m.query_encode_latent.bias

        def build():
            C = w1.shape[0]
            w = w1.detach().reshape(C, -1).to(device=device, dtype=torch.float32)
            gm, off = [], 0
            for t in maps:
                n, Hl, Wl, Cl = t.shape
                layer = PackedLinear(w[:, off:off + Cl].contiguous(), None, device, "project_maps")
                g = torch.empty(n, Hl, Wl, C, device=device, dtype=torch.float32)
                self.linear(t, Cl, layer, g, C, n * Hl * Wl)
                gm.append(g)
                off += Cl
            return gm, torch.cat([w[:, off:off + 3], b1.detach().to(device=device, dtype=torch.float32)[:, None]], dim=1).contiguous()
        return self._gmaps.get([*maps, w1, b1], (str(device),), build)

    def gather_encode(self, gmaps: List[Tensor], wpt: Tensor, pixel_val: Tensor, grid_in: Tensor, ptenc: Tensor,
                      V: int, pts: int, out: Tensor, ld_out: int):
        ptrs, cs, hs, ws, L = _levels(gmaps)
        self.lib.car_gather_encode(ptrs, hs, ws, L, cs[0], _ptr(pixel_val), _ptr(grid_in), _ptr(ptenc), _ptr(wpt), gmaps[0].shape[0], V, pts,
                                   _ptr(out), ld_out, _stream())

    def _poses(self, inp, H: int, n: int, dev) -> Tensor:
        """Device pose records (``struct CarPose``) for this input (models.py:207-211, 285-286).

        ``pose_route == "host"`` (the default, the strict-parity route): the reference's own ``torch.inverse`` / ``matmul`` calls on
        the host CPU (poses.pack_poses) wherever the four camera tensors live.  Cameras that arrive on the GPU — the reference's
        scripts move the whole input dict there (render_realestate10k_traj.py:85) — are copied to the host first: ONE pinned
        download of the 4x4 matrices (a few hundred bytes; the stream is synchronised once, which the reference does on every
        call anyway, models.py:570), then one pinned upload of the records.  Cached on the identity/version of the four tensors, so a
        frame rendered in chunks pays once.  ``last_pose_sync_ms`` holds the host time of the last such round trip.
        ``pose_route == "device"`` (opt-in; ``--cameras device`` of the scripts): ``car_pose_setup`` on the device when the cameras
        are there — no host round trip, but fp64 Gauss-Jordan instead of LAPACK's fp32: the matrices differ in the last ulp, which
        the fp64 Pluecker intersection amplifies on the few samples whose pixel ray is nearly parallel to the query ray
         — as it does between two LAPACK builds."""
        if self.pose_records is not None:
            poses = self.pose_records.float().contiguous()
            if tuple(poses.shape) != (n, 96):
                raise ValueError(f"pose records must have shape ({n}, 96)")
            return poses.to(dev, non_blocking=True)
        if self.pose_route not in ("host", "device"):
            raise ValueError("RenderEngine.pose_route must be 'host' or 'device'")
        ts = (inp["context"]["cam2world"], inp["context"]["intrinsics"], inp["query"]["cam2world"], inp["query"]["intrinsics"])
        on_gpu = all(t.is_cuda for t in ts)
        if self.pose_route == "device" and on_gpu:
            b, V = ts[0].shape[:2]
            c2w, Kc, c2w_q, Kq = [t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in ts]
            poses = torch.empty(n, 96, device=dev, dtype=torch.float32)
            self.lib.car_pose_setup(_ptr(c2w), _ptr(c2w_q), _ptr(Kc), _ptr(Kq), b, V, H, _ptr(poses), _stream())
            return poses

        def build():
            src = inp
            if any(t.is_cuda for t in ts):
                import time
                t0 = time.perf_counter()
                src = self._cameras_to_host(ts)
                self.last_pose_sync_ms = (time.perf_counter() - t0) * 1e3
            # pinned staging: the 768-byte upload is queued behind the previous frame's kernels instead of waiting for them
            return pack_poses(src, H).pin_memory().to(dev, non_blocking=True)
        return self._pose.get(ts, (H, str(dev)), build)

    @staticmethod
    def _cameras_to_host(ts):
        """The four camera tensors as CPU tensors in the input dict's shape, through ONE device-to-host copy (tensors already on the
        host are passed through)."""
        gpu = [t for t in ts if t.is_cuda]
        flat = torch.cat([t.detach().reshape(-1).to(torch.float32) for t in gpu])
        host = torch.empty(flat.numel(), dtype=torch.float32, pin_memory=True)
        host.copy_(flat, non_blocking=True)
        torch.cuda.current_stream(flat.device).synchronize()
        out, off = [], 0
        for t in ts:
            if t.is_cuda:
                out.append(host[off:off + t.numel()].view(t.shape).clone())
                off += t.numel()
            else:
                out.append(t)
        return {"context": {"cam2world": out[0], "intrinsics": out[1]}, "query": {"cam2world": out[2], "intrinsics": out[3]}}

    def _linspace(self, a: float, b_: float, P: int, device) -> Tensor:
        k = (a, b_, P, str(device))
        if k not in self._steps:
            self._steps[k] = torch.linspace(a, b_, P).to(device)      # CPU linspace, like the reference's values
        return self._steps[k]

    def _packed_layers(self, packer: str, layers, sizes, device) -> List[Tensor]:
        """The weights ([N, K] rows) and biases of ``layers`` through ``packer``, a device-side packer of the C ABI, into zeroed buffers of
        ``sizes`` floats, re-packed when one of them changes."""
        ps = [getattr(self.m.get_submodule(n), k) for n in layers for k in ("weight", "bias")]

        def build():
            f = [t.detach().to(device=device, dtype=torch.float32).reshape(t.shape[0], -1).contiguous() for t in ps]
            out = [torch.zeros(n, device=device, dtype=torch.float32) for n in sizes]
            getattr(self.lib, packer)(*[_ptr(t) for t in f + out], _stream())
            return out
        return self._layer_packs[packer].get(ps, (str(device),), build)

    def _round2_weights(self, device):
        """query_repeat_embed[:, 128:] and query_repeat_embed_2 packed for csrc/car_round2.hip."""
        return self._packed_layers("car_round2_pack", ("query_repeat_embed", "query_repeat_embed_2"),
                                   (self.lib.car_round2_packed_floats(), self.lib.car_round2_bias_floats()), device)

    def _exchange_pack(self, device):
        """query_encode_latent (its point columns and bias) and query_encode_latent_2 packed for car_fused_rows."""
        return self._packed_layers("car_fused_pack_rows", ("query_encode_latent", "query_encode_latent_2"),
                                   (self.lib.car_fused_blob_floats(), self.lib.car_fused_bias_floats(), 576 * 4), device)

    def _kq_weights(self, device):
        """key_map_2, query_embed and query_embed_2 packed for the key / query chain kernel (car_key_query_logits)."""
        return self._packed_layers("car_kq_pack", ("key_map_2", "query_embed", "query_embed_2"),
                                   (self.lib.car_kq_tail_floats(), self.lib.car_kq_bias_floats()), device)

    # ------------------------------------------------------------------ plans, lattices and budgets (the one-call route; prefetch)
    def _dims(self, b: int, R: int, z: List[Tensor]) -> "_lib.CarDims":
        m = self.m
        d = _lib.CarDims()
        d.b, d.V, d.R, d.P, d.H, d.W = b, m.n_view, R, m.npoints, m.H, m.W
        d.n_levels = len(z)
        for l, t in enumerate(z):
            d.level_c[l], d.level_h[l], d.level_w[l] = t.shape[1], t.shape[2], t.shape[3]
        d.repeat_attention = int(m.repeat_attention)
        d.no_sample = int(m.no_sample)
        return d

    def _car_weights(self, device):
        """struct CarWeights: every layer the plans pack, weights as fp32 [N, K] rows and biases on the device.  The tensors its pointers
        lead to ride on it (``keep``), so they live as long as the struct."""
        sd = dict(self.m.named_parameters())
        keep: List[Tensor] = []

        def dev(name):
            t = sd[name].detach().to(device=device, dtype=torch.float32)
            t = t.reshape(t.shape[0], -1).contiguous() if t.dim() > 1 else t.contiguous()
            keep.append(t)
            return t.data_ptr()

        w = _lib.CarWeights()
        for n in _lib.WEIGHT_FIELDS[0]:
            setattr(w, f"{n.replace('.', '_')}_w", dev(n + ".weight"))
            setattr(w, f"{n.replace('.', '_')}_b", dev(n + ".bias"))
        for i, (lin_z, fc_0, fc_1) in enumerate(_render_layers(self.m).blocks[:3]):
            w.phi_lin_z_w[i], w.phi_lin_z_b[i] = dev(lin_z + ".weight"), dev(lin_z + ".bias")
            w.phi_fc_0_w[i], w.phi_fc_0_b[i] = dev(fc_0 + ".weight"), dev(fc_0 + ".bias")
            w.phi_fc_1_w[i], w.phi_fc_1_b[i] = dev(fc_1 + ".weight"), dev(fc_1 + ".bias")
        w.keep = keep
        return w

    def _plan_sources(self, d, device):
        """What a plan is built from: the parameters of every layer it packs, and the device and dims it packs them for."""
        sd = dict(self.m.named_parameters())
        names = list(_lib.WEIGHT_FIELDS[0]) + [n for block in _render_layers(self.m).blocks[:3] for n in block]
        return [sd[n + k] for n in names for k in (".weight", ".bias")], (str(device), d.P, tuple(d.level_c[:d.n_levels]))

    def _build_plan(self, what: str, d, device, w) -> Tensor:
        """car_<what>_build of the layers ``w`` (struct CarWeights) into a buffer of car_<what>_bytes: "plan" (every layer packed for the
        kernels) or "plan_f16" (the fused kernel's compact fp16 layers)."""
        nbytes = getattr(self.lib, f"car_{what}_bytes")(ctypes.byref(d))
        if nbytes == 0:
            _lib.check(-1, f"car_{what}_bytes")
        plan = torch.empty(nbytes // 4, device=device, dtype=torch.float32)
        getattr(self.lib, f"car_{what}_build")(ctypes.byref(d), ctypes.byref(w), _ptr(plan), _stream())
        return plan

    def _plan_for(self, d, device) -> Tensor:
        """car_plan_build: every layer packed for the kernels, once per set of parameter values.  Cached with the CarWeights it was built
        from (_plan_w)."""
        def build():
            w = self._car_weights(device)
            return self._build_plan("plan", d, device, w), w
        return self._plan.get(*self._plan_sources(d, device), build)[0]

    def _plan16_for(self, d, device) -> Tensor:
        """car_plan_f16_build: the fused kernel's compact fp16 layers, built from the same weights as the fp32 plan and cached on it (a change
        of the parameters rebuilds both).  Call after _plan_for."""
        plan, w = self._plan.value
        return self._plan16.get([plan], (), lambda: self._build_plan("plan_f16", d, device, w))

    def _pair_for(self, plan: Tensor, z: List[Tensor], device, s0: int, s1: int, R: int):
        """car_project_maps for scenes [s0, s1): the first point-MLP layer applied per texel of the pyramid and every level summed on the
        common lattice, once per stereo pair (and plan).  Returns (buffer, its car_dims).  One buffer is cached: the whole batch
        normally; when the lattices of all scenes do not fit the device memory (one_call.render) the last group's."""
        maps = self._channel_last(z)
        V = self.m.n_view
        d = self._dims(s1 - s0, R, z)

        def build():
            pair = torch.empty(self.lib.car_gmaps_floats(ctypes.byref(d)), device=device, dtype=torch.float32)
            ptrs = _levels(maps, slice(s0 * V, s1 * V))[0]
            self.lib.car_project_maps(ctypes.byref(d), _ptr(plan), ptrs, _ptr(pair), _stream())
            return pair
        return self._pairs.get([plan, *z], (s0, s1), build), d

    @staticmethod
    def _common_lattice(z: List[Tensor]) -> bool:
        """The fused kernel gathers every level from their common lattice (car_lattice_shape): each must be an integer factor coarser
        than the widest one, the same factor in both directions.  Other pyramids take the stage route."""
        sizes = [(t.shape[2], t.shape[3]) for t in z]
        hm, wm = max(h for h, _ in sizes), max(w for _, w in sizes)
        return all(hm % h == 0 and wm % w == 0 and hm // h == wm // w for h, w in sizes)

    def _lattice_shape(self, d) -> tuple:
        """(lat_h, lat_w, lat_pad) of the common lattice of d's pyramid (car_lattice_shape)."""
        lh, lw, lpad = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self.lib.car_lattice_shape(ctypes.byref(d), ctypes.byref(lh), ctypes.byref(lw), ctypes.byref(lpad))
        return lh.value, lw.value, lpad.value

    def _lattice_fits(self, b: int, R: int, z: List[Tensor]) -> bool:
        """car_fused_samples addresses the lattice of one (view, padding mode) with 32-bit byte offsets below 2 GiB (a finest level
        up to ~470 pixels wide at 576 channels); wider pyramids take the stage route, which has no such limit."""
        lh, lw, _ = self._lattice_shape(self._dims(b, R, z))
        return lh * lw * 576 * 4 < 2**31

    def _free_budget(self, device) -> int:
        """85 % of what this engine could allocate now: free device memory, the caching allocator's idle blocks, and its own workspace
        (which every caller either re-uses in place or releases before it allocates against this figure)."""
        free, _ = torch.cuda.mem_get_info(device)
        cached = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
        mine = self._work.numel() * 4 if self._work is not None else 0
        return int(0.85 * (free + cached + mine))

    def _workspace_budget(self, device) -> int:
        return int(self.max_workspace_bytes) if self.max_workspace_bytes is not None else self._free_budget(device)

    def _rays_in(self, inp, b: int, R: int):
        """a3: the pose records, the query pixels [b, R, 2] and the P sample steps of a forward."""
        m = self.m
        dev = inp["query"]["uv"].device
        poses = self._poses(inp, m.H, b * m.n_view, dev)
        uv = inp["query"]["uv"].detach().reshape(b, R, 2).float().contiguous()
        steps = self._linspace(0.1, 10.0, m.npoints, dev) if m.no_sample else self._linspace(0.0, 1.0, m.npoints, dev)
        return poses, uv, steps

    @staticmethod
    def _outputs(inp, z: List[Tensor], t: Dict[str, Tensor], debug: bool) -> Dict[str, Tensor]:
        """The forward's output dict (models.py:570-621) from the seven tensors both routes write (``t``, keyed by output name)."""
        return {"rgb": t["rgb"], "valid_mask": t["valid_mask"], "depth_ray": t["depth_ray"], "at_wt": t["at_wt"], "at_wts": [t["at_wt"]],
                "at_wt_max": t["at_wt_max"].long(), "coords": t["coords"], "uv": inp["query"]["uv"],
                # the reference returns pixel_val on the CPU (models.py:570), forcing a device sync on every call; here it stays on the
                # device unless debug is set
                "pixel_val": t["pixel_val"].cpu() if debug else t["pixel_val"], "z": z}

    # ------------------------------------------------------------------ stage timing (csrc/car_render.hip)
    def profile(self, on: bool) -> None:
        """Brackets every stage of the one-call route with HIP events on the launch stream (no synchronisation)."""
        self.lib.car_profile_enable(1 if on else 0)

    def stage_times(self) -> List[tuple]:
        """[(stage name, milliseconds)] of everything recorded since profile(True) / the last call; synchronises on the events."""
        lib = self.lib
        rows = []
        for i in range(lib.car_profile_count()):
            name, ms = ctypes.c_char_p(), ctypes.c_float()
            lib.car_profile_read(i, ctypes.byref(name), ctypes.byref(ms))
            rows.append((name.value.decode(), ms.value))
        lib.car_profile_reset()
        return rows

    # ------------------------------------------------------------------ kernels
    @staticmethod
    def _ran(entry, *args, what: str = "") -> bool:
        """Calls ``entry`` of the checked handle.  False when the device refused the kernel's LDS reservation (CAR_E_LAUNCH with the "cannot
        reserve" text: a part with less than gfx950's 160 KB per compute unit) — the ONE condition under which a route steps down to the next
        HIP kernel of the same library.  Anything else (an argument error, a sticky fault of an earlier launch) raises: it must not silently
        change the arithmetic."""
        try:
            entry(*args)
            return True
        except _lib.CarError as e:
            if e.code != _lib.CAR_E_LAUNCH or "cannot reserve" not in e.text:
                raise
            import warnings
            warnings.warn(f"{what or e.entry}: {e.text}: taking the next kernel of the library")
            return False

    def linear(self, x: Tensor, ldx: int, layer: PackedLinear, y: Tensor, ldy: int, M: int, flags: int = 0, mask=None):
        """``mask = (act, lda)``: the result is zeroed where ``act <= 0`` (the backward of a ReLU in front of the layer whose data gradient this
        is) — in the split-fp16 kernel's store (car_linear_x3_masked), or by car_relu_mask behind the fp32-pipe kernel."""
        # linear_flags (the NO_GLDS A/B knob of car_linear) selects the fp32-pipe kernel for every layer: the split-fp16 kernel has no such
        # variant, and an A/B run must not change arithmetic on some layers only
        if (self.linear_x3 and not self.linear_flags and layer.x3 is not None and ldx % 4 == 0 and ldy % 4 == 0 and x.data_ptr() % 16 == 0
                and y.data_ptr() % 16 == 0 and M >= self.linear_x3_min_rows):
            tiles, bias = layer.x3
            args = (_ptr(x), ldx, _ptr(tiles), _ptr(bias), layer.K, layer.N, _ptr(y), ldy, M, flags)
            if mask is not None and mask[1] % 4 == 0 and mask[0].data_ptr() % 16 == 0:
                if self._ran(self.lib.car_linear_x3_masked, *args, _ptr(mask[0]), mask[1], _stream(), what="car_linear_x3"):
                    return                                 # the mask was applied in the kernel's store
            elif self._ran(self.lib.car_linear_x3, *args, _stream()):
                if mask is not None:
                    self.lib.car_relu_mask(_ptr(y), ldy, _ptr(mask[0]), mask[1], M, layer.N, _stream())
                return
            # the split-fp16 kernel's 72 KB weight double buffer was refused: the same layer on the fp32 matrix pipe from here on — another
            # HIP kernel of the same library, never a host path
            self.linear_x3 = False
        self.lib.car_linear(_ptr(x), ldx, _ptr(layer.packed), layer.K, layer.N, _ptr(y), ldy, M, flags | self.linear_flags, _stream())
        if mask is not None:
            self.lib.car_relu_mask(_ptr(y), ldy, _ptr(mask[0]), mask[1], M, layer.N, _stream())

    def gather(self, maps: List[Tensor], grid: Tensor, pts: int, mode: int, place: int, V: int, out: Tensor,
               ld_out: int, col_out: int, run: int = 1):
        ptrs, cs, hs, ws, L = _levels(maps)
        self.lib.car_gather_bilinear(ptrs, cs, hs, ws, L, maps[0].shape[0], _ptr(grid), pts, run, mode, place, V, _ptr(out), ld_out, col_out, _stream())

    # ------------------------------------------------------------------ the forward pass
    @torch.no_grad()
    def render(self, inp, z: List[Tensor], debug: bool = False) -> Dict[str, Tensor]:
        dev = inp["query"]["uv"].device
        if dev.type != "cuda":
            raise RuntimeError("CrossAttentionRenderer.forward runs on the HIP engine only: move the model, the input "
                               "dict and z to a ROCm device (there is no CPU fallback)")
        # kernels are launched on the current device's current stream: make the tensors' device current for the call
        with torch.cuda.device(dev):
            return self._render(inp, z, debug)

    def _render(self, inp, z: List[Tensor], debug: bool) -> Dict[str, Tensor]:
        m = self.m
        b, V = inp["context"]["rgb"].shape[:2]
        n_qry, R = inp["query"]["uv"].shape[1:3]
        if n_qry != 1:
            raise ValueError("forward supports one query view per scene (reference models.py:213, 619)")
        if V != m.n_view:
            raise ValueError(f"input has {V} context views, module was built with n_view={m.n_view}")
        why = self._one_call_refusal(b, R, z)
        if why is None:
            return one_call.render(self, inp, z, b, R, debug)
        if self.render_precision == "fp16":
            raise ValueError(f"render_precision='fp16' exists on the one-call route only, and this forward cannot take it: {why}. "
                             "Set render_precision='fp32' for this configuration.")
        self.last_precision = "fp32"
        return staged.forward(self, inp, z, debug)


from . import one_call, staged  # noqa: E402  (the routes of _render; both import this module's names, so they come last)
