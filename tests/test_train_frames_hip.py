"""The device pixel chain of the training reader (csrc/car_frames.hip) and the loader that drives it (dataio.TrainLoader).

Everything is exact: the kernels do the integer arithmetic of dataio.resize_linear_u8 on tables the host made, so every comparison
here is array_equal / torch.equal against the host chain.  Outputs are placed inside larger buffers whose margins hold a sentinel
that must survive.  The argument refusals are decided on the host before anything is launched: those tests need no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lpips_restatement as LR
import train_scene

from cross_attention_renderer_amd import dataio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "experiment_scripts", "train_realestate10k.py")
SIDE = 256
MARGIN = 4096                       # elements of sentinel in front of and behind every output
F_SENTINEL, B_SENTINEL = -7.5, 0xAB


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from cross_attention_renderer_amd import _lib
    return _lib.load()


def _rec(**kw):
    r = np.zeros(1, dataio.FRAME_REC)
    base = dict(src_off=0, src_h=256, src_w=455, src_pitch=455 * 3, x0=99, y0=0, rw=256, rh=256, dst_w=256, dst_h=256, win_x0=0, win_w=256)
    for k, v in {**base, **kw}.items():
        r[k] = v
    return r


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


# ---- the boundary: sizes, slots, refusals (host only) -----------------------------------------------------------------------------------

def test_tables_and_slots(lib):
    assert lib.car_frames_table_ints() == 34 * 512 * 4 + 256
    assert [lib.car_frames_table_slot(256 - 2 * p, 256) for p in range(32)] == list(range(32))
    assert lib.car_frames_table_slot(360, 256) == 32 and lib.car_frames_table_slot(640, 455) == 33
    for n_src, n_dst in ((192, 256), (255, 256), (258, 256), (256, 255), (640, 256), (360, 455), (0, 0)):
        assert lib.car_frames_table_slot(n_src, n_dst) == -1
    t = dataio.frame_tables()
    assert t.dtype == np.int32 and t.shape == (lib.car_frames_table_ints(),)
    slot = t[7 * 2048:8 * 2048].reshape(512, 4)                  # 242 -> 256
    i0, i1, w0, w1 = dataio._linear_coefs(256, 242)
    assert np.array_equal(slot[:256], np.stack([i0, i1, w0, w1], axis=-1)) and not slot[256:].any()
    assert slot[:256, :2].max() == 241 and np.abs(slot[:256, 2] + slot[:256, 3] - 2048).max() <= 1
    assert np.array_equal(t[-256:].view(np.float32), np.arange(256, dtype=np.uint8).astype(np.float32) / 127.5 - 1)
    assert dataio.FRAME_REC.itemsize == 80


def test_bad_arguments_return_codes_and_launch_nothing(lib):
    """Every refusal comes from the host-side validation, before any launch: the 'device' pointers here are never read."""
    src = np.zeros(360 * 640 * 3, np.uint8)                      # room for a raw frame; the stored 256 x 455 one is its first bytes
    std_bytes = 256 * 455 * 3
    tables, out = np.zeros(lib.car_frames_table_ints() + 4, np.int32), np.zeros(SIDE * SIDE * 3 + 8, np.float32)
    tab, dst = (_ptr(tables) + 15) // 16 * 16, (_ptr(out) + 15) // 16 * 16
    idx = np.arange(1024, dtype=np.int32)
    n_out = SIDE * SIDE * 3

    def f32(rec, src_bytes=std_bytes, recs_host=True, idx_arr=idx, dst_elems=n_out, n=1, src_ptr=_ptr(src), tables_ptr=tab, dst_ptr=dst):
        return lib.car_frames_resize_f32(src_ptr, src_bytes, _ptr(rec) if recs_host else None, _ptr(rec), n, None if idx_arr is None else _ptr(idx_arr),
                                         None if idx_arr is None else _ptr(idx_arr), 0 if idx_arr is None else len(idx_arr), tables_ptr, dst_ptr, dst_elems, None)

    def refused(code, word):
        assert code == -1 and word.encode() in lib.car_last_error(), lib.car_last_error()

    refused(f32(_rec(), src_ptr=None), "null pointer")
    refused(f32(_rec(), recs_host=False), "null pointer")
    refused(f32(_rec(), tables_ptr=None), "null pointer")
    refused(f32(_rec(), dst_ptr=None), "null pointer")
    refused(lib.car_frames_resize_u8(None, 0, None, None, 1, None, None, 0, None), "null pointer")
    refused(f32(_rec(), n=0), "n_images")
    refused(f32(_rec(), dst_ptr=dst + 4), "aligned")
    refused(f32(_rec(x0=200)), "outside its")                    # 200 + 256 > 455
    refused(f32(_rec(y0=1)), "outside its")
    refused(f32(_rec(x0=-1)), "outside its")
    refused(f32(_rec(rw=0)), "outside its")
    refused(f32(_rec(), src_bytes=std_bytes - 1), "outside src")
    refused(f32(_rec(src_off=1)), "outside src")
    refused(f32(_rec(src_pitch=455 * 3 - 1)), "pitch")
    refused(f32(_rec(dst_w=255, win_w=252)), "no table")          # a destination size with no table
    refused(f32(_rec(rw=255)), "no table")
    refused(f32(_rec(rh=192)), "no table")
    refused(f32(_rec(dst_h=455)), "no table")
    refused(f32(_rec(win_x0=4)), "written columns")
    refused(f32(_rec(win_w=254)), "written columns")
    refused(f32(_rec(flip=2)), "flip")
    refused(f32(_rec(reserved=1)), "reserved")
    refused(f32(_rec(dst_off=2)), "dst_off")
    refused(f32(_rec(dst_off=4)), "outside dst")
    refused(f32(_rec(), dst_elems=n_out - 1), "outside dst")
    refused(f32(_rec(n_idx=1024), idx_arr=None), "null pointer")
    refused(f32(_rec(n_idx=1025)), "outside the list")
    refused(f32(_rec(n_idx=8, idx_off=1020)), "outside the list")
    refused(f32(_rec(n_idx=1024), dst_elems=3 * 1024 - 1), "outside dst")
    for bad in (65536, 1 << 20, -1):
        wrong = idx.copy()
        wrong[1000] = bad
        refused(f32(_rec(n_idx=1024), idx_arr=wrong), "pixel index")
    # a small written window bounds the indices too (256 rows x 4 columns = 1024 pixels: 1024 is the first one outside)
    refused(f32(_rec(win_w=4, n_idx=4), idx_arr=np.array([0, 1, 2, 1024], np.int32)), "pixel index")
    # the second record is checked like the first
    two = np.concatenate([_rec(), _rec(dst_off=n_out, x0=300)])
    refused(f32(two, n=2, dst_elems=2 * n_out), "image 1")
    # stage A's instance: the same validation, no index list
    raw = _rec(src_h=360, src_w=640, src_pitch=1920, x0=0, rw=640, rh=360, dst_w=455, win_x0=99, n_idx=0)
    u8 = lambda rec, src_bytes=360 * 1920, dst_elems=n_out: lib.car_frames_resize_u8(_ptr(src), src_bytes, _ptr(rec), _ptr(rec), 1, tab, dst, dst_elems, None)
    refused(u8(raw, src_bytes=src.nbytes - 1), "outside src")
    refused(u8(_rec(src_h=360, src_w=640, src_pitch=1920, x0=0, rw=640, rh=360, dst_w=455, win_x0=200)), "written columns")
    refused(u8(_rec(src_h=360, src_w=640, src_pitch=1920, x0=0, rw=640, rh=360, dst_w=455, win_x0=99, n_idx=4)), "null pointer")
    # the written range may share an allocation with src (the loader's stage A does), never a byte: blocks read while others write
    both = np.zeros(src.nbytes + n_out + 16, np.uint8)
    p0 = (_ptr(both) + 15) // 16 * 16
    inside = lambda dst_ptr, src_bytes=src.nbytes: lib.car_frames_resize_u8(p0, src_bytes, _ptr(raw), _ptr(raw), 1, tab, dst_ptr, n_out, None)
    refused(inside(p0), "overlaps")
    refused(inside(p0 + src.nbytes - 16), "overlaps")             # the last 16 bytes of src
    refused(inside(p0 + src.nbytes, src_bytes=src.nbytes + 1), "overlaps")
    refused(lib.car_frames_resize_u8(p0 + n_out - 16, src.nbytes, _ptr(raw), _ptr(raw), 1, tab, p0, n_out, None), "overlaps")   # dst in front, its end inside
    refused(f32(_rec(), src_ptr=dst + 4 * n_out - 16), "overlaps")  # float elements: the range is 4 x dst_elems bytes


def test_library_exports_the_new_symbols(lib):
    from cross_attention_renderer_amd import _lib
    header = open(os.path.join(ROOT, "include", "car_hip.h")).read()
    for name in ("car_frames_table_ints", "car_frames_table_slot", "car_frames_resize_u8", "car_frames_resize_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"{name}(" in header
    assert lib.car_version() == 300
    import __graft_entry__ as ge
    assert "car_frames.hip" in ge.UNITS


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def _chain(lib, frames, records, pixels=None, stages="ab"):
    """Runs the device chain on `frames` as the loader lays a batch out, every output inside sentinel margins.  Returns (windows,
    outputs): stage A's uint8 256 x 256 windows of the 360-line frames, stage B's float32 output per frame (None without stage B)."""
    dev = torch.device("cuda:0")
    pixels = pixels if pixels is not None else [None] * len(frames)
    offs, at = [], 0
    for f in frames:
        offs.append(at)
        at = dataio._align(at + f.nbytes)
    n_a = sum(r["resize360"] for r in records)
    upload, scratch = at, n_a * SIDE * SIDE * 3
    recs_a, recs_b, idx = dataio.stage_records([f.shape for f in frames], records, pixels, offs, upload)
    host = np.full(upload + scratch + MARGIN, B_SENTINEL, np.uint8)
    for f, o in zip(frames, offs):
        host[o:o + f.nbytes] = f.reshape(-1)
    buf = torch.from_numpy(host).to(dev)
    tables = torch.from_numpy(dataio.frame_tables()).to(dev)
    from cross_attention_renderer_amd import _lib
    windows = []
    if n_a:
        ra = torch.from_numpy(recs_a.view(np.uint8)).to(dev)
        _lib.check(lib.car_frames_resize_u8(buf.data_ptr(), upload, _ptr(recs_a), ra.data_ptr(), n_a, tables.data_ptr(), buf.data_ptr() + upload, scratch, None))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[:upload], host[:upload]), "stage A wrote into the frames in front of its output"
        assert (got[upload + scratch:] == B_SENTINEL).all(), "stage A wrote behind its output"
        windows = [got[upload + k * SIDE * SIDE * 3:upload + (k + 1) * SIDE * SIDE * 3].reshape(SIDE, SIDE, 3) for k in range(n_a)]
    if "b" not in stages:
        return windows, None
    sizes = [SIDE * SIDE * 3 if p is None else 3 * len(p) for p in pixels]
    n_out = int(recs_b["dst_off"][-1]) + dataio._align(sizes[-1], 4)
    out = torch.full((MARGIN + n_out + MARGIN,), F_SENTINEL, dtype=torch.float32, device=dev)
    rb, ib = torch.from_numpy(recs_b.view(np.uint8)).to(dev), torch.from_numpy(np.concatenate([idx, np.zeros(4, np.int32)])).to(dev)
    _lib.check(lib.car_frames_resize_f32(buf.data_ptr(), upload + scratch, _ptr(recs_b), rb.data_ptr(), len(frames), _ptr(idx) if len(idx) else None,
                                         ib.data_ptr() if len(idx) else None, len(idx), tables.data_ptr(), out.data_ptr() + 4 * MARGIN, n_out, None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:MARGIN] == F_SENTINEL).all() and (got[MARGIN + n_out:] == F_SENTINEL).all(), "stage B wrote outside its output"
    got = got[MARGIN:MARGIN + n_out]
    outputs, written = [], np.zeros(n_out, bool)
    for r, p, n in zip(recs_b, pixels, sizes):
        o = int(r["dst_off"])
        outputs.append(got[o:o + n].reshape((SIDE, SIDE, 3) if p is None else (-1, 3)))
        written[o:o + n] = True
    assert (got[~written] == F_SENTINEL).all(), "stage B wrote into the padding between two images' outputs"
    assert np.array_equal(buf.cpu().numpy()[:upload], host[:upload])
    return windows, outputs


def _frames(shape, n, seed):
    rng = np.random.RandomState(seed)
    out = [rng.randint(0, 256, size=shape + (3,)).astype(np.uint8) for _ in range(n)]
    return out + [np.full(shape + (3,), v, np.uint8) for v in (0, 255, 128)] + [train_scene.frame(shape, 11)]


def _record(resize360, augment=False, flip=False, py=0, px=0):
    return {"resize360": resize360, "augment": augment, "flip": flip, "py": py, "px": px, "out_hw": (SIDE, SIDE)}


@pytest.mark.gpu
def test_stage_a_equals_the_host_resize_and_crop(lib):
    frames = _frames((360, 640), 3, seed=1)
    windows, _ = _chain(lib, frames, [_record(True)] * len(frames), stages="a")
    assert len(windows) == len(frames)
    for f, w in zip(frames, windows):
        want = dataio.square_crop_img(dataio.resize_linear_u8(f, 455, 256))
        assert want.shape == (256, 256, 3) and w.dtype == np.uint8 and np.array_equal(w, want)
    assert (windows[3] == 0).all() and (windows[4] == 255).all() and (windows[5] == 128).all()


@pytest.mark.gpu
@pytest.mark.parametrize("flip", (False, True))
def test_stage_b_equals_the_host_chain_for_every_crop(lib, flip):
    """Every py in 0 .. 31 with px = 0, 1, py-dependent and 31, on random stored frames, constants and the scene's sawtooth."""
    frames = _frames((256, 455), 2, seed=2 + flip)
    cases = [(py, px) for py in range(32) for px in sorted({0, 1, (7 * py + 3) % 32, 31})]
    use, records = [], []
    for k, (py, px) in enumerate(cases):
        use.append(frames[k % len(frames)])
        records.append(_record(False, True, flip, py, px))
    _, outputs = _chain(lib, use, records)
    for f, r, got in zip(use, records, outputs):
        want = dataio.frame_pixels(f, r)
        assert got.dtype == np.float32 and np.array_equal(got, want), (r["py"], r["px"], flip)


@pytest.mark.gpu
def test_stage_b_without_augmentation_is_the_conversion_alone(lib):
    frames = _frames((256, 455), 2, seed=4)
    _, outputs = _chain(lib, frames, [_record(False)] * len(frames))
    for f, got in zip(frames, outputs):
        assert np.array_equal(got, f[:, 99:355].astype(np.float32) / 127.5 - 1)
    assert (outputs[2] == -1).all() and (outputs[3] == 1).all()
    # an augmented record that neither crops nor resizes: the flip alone
    _, outputs = _chain(lib, frames[:2], [_record(False, True, True)] * 2)
    for f, got in zip(frames, outputs):
        assert np.array_equal(got, f[:, 99:355][:, ::-1].astype(np.float32) / 127.5 - 1)


@pytest.mark.gpu
def test_both_stages_chained_on_raw_frames(lib):
    frames = _frames((360, 640), 2, seed=5)
    records = [_record(True, True, k % 2 == 1, (5 * k) % 32, (11 * k + 2) % 32) for k in range(len(frames))]
    records[0] = _record(True)                                   # raw and not augmented: stage A, then the conversion
    windows, outputs = _chain(lib, frames, records)
    for f, r, w, got in zip(frames, records, windows, outputs):
        assert np.array_equal(w, dataio.square_crop_img(dataio.resize_linear_u8(f, 455, 256)))
        assert np.array_equal(got, dataio.frame_pixels(f, r))
    # stored and raw frames in one launch
    mixed = [frames[0], _frames((256, 455), 1, seed=6)[0], frames[1]]
    recs = [_record(True, True, True, 3, 0), _record(False, True, False, 0, 30), _record(True, True, False, 31, 31)]
    _, outputs = _chain(lib, mixed, recs)
    for f, r, got in zip(mixed, recs, outputs):
        assert np.array_equal(got, dataio.frame_pixels(f, r))


@pytest.mark.gpu
def test_sparse_form_equals_indexing_the_full_result(lib):
    rng = np.random.RandomState(7)
    stored, raw = _frames((256, 455), 2, seed=8), _frames((360, 640), 1, seed=9)
    frames = [stored[0], stored[1], raw[0], stored[5], stored[0], raw[0]]
    records = [_record(False, True, True, 9, 20), _record(False), _record(True, True, False, 31, 1), _record(False, True, False, 0, 0),
               _record(False, True, True, 17, 0), _record(True)]
    patch = ((100 + np.arange(32))[:, None] * 256 + 223 + np.arange(32)[None]).reshape(-1)          # the last patch column the reader draws
    pixels = [rng.permutation(65536)[:1024], patch, rng.permutation(65536)[:192], np.array([0, 65535, 255, 65280, 32896, 1, 2]),     # 7: a ragged tail
              rng.permutation(65536)[:190], None]
    _, outputs = _chain(lib, frames, records, pixels)
    for f, r, p, got in zip(frames, records, pixels, outputs):
        full = dataio.frame_pixels(f, r)
        want = full if p is None else full.reshape(-1, 3)[p]
        assert got.shape == want.shape and np.array_equal(got, want), (r, None if p is None else len(p))


CASES = [(v, a, l) for v in (1, 2, 3) for a in (True, False) for l in (True, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("views,augment,lpips", CASES)
def test_device_batches_equal_the_host_collated_ones(views, augment, lpips):
    """Three scenes per batch: the stored 256 x 455 one, the raw 360-line one, and whatever the short scene's retry draws."""
    ds = dataio.RealEstate10k(train_scene.img_root(), train_scene.pose_root(), num_ctxt_views=views, num_query_views=1, query_sparsity=192,
                              augment=augment, lpips=lpips)
    dev = torch.device("cuda:0")
    seed = 10 * views + 2 * augment + lpips
    host = dataio.TrainLoader(ds, batch_size=3, seed=seed, num_workers=8)
    device = dataio.TrainLoader(ds, batch_size=3, seed=seed, num_workers=8, device=dev, cameras="gpu" if views == 2 else "host")
    for epoch in range(2):
        hb, db = list(host), list(device)
        assert len(hb) == len(db) == 1
        (h_inp, h_gt), (d_inp, d_gt) = hb[0], db[0]
        raw = sum(r["resize360"] for i in host.batch_indices(epoch)[0] for r in device._plan(epoch, i)["records"])
        assert raw >= 1 + views, "the batch must hold the raw 360-line scene"
        assert d_gt is d_inp["query"] or all(d_gt[k] is d_inp["query"][k] for k in d_gt)
        for part in ("query", "context"):
            assert list(h_inp[part]) == list(d_inp[part])
            for k, want in h_inp[part].items():
                got = d_inp[part][k]
                on_host = k in ("cam2world", "intrinsics") and views != 2
                assert got.device.type == ("cpu" if on_host else "cuda"), (part, k)
                assert got.dtype == want.dtype and got.shape == want.shape and got.is_contiguous() and torch.equal(got.cpu(), want), (part, k, epoch)
        R = 1024 if lpips else 192
        assert d_inp["query"]["rgb"].shape == (3, 1, R, 3) and d_inp["context"]["rgb"].shape == (3, views, 256, 256, 3)
        assert d_inp["query"]["mask"].dtype == (torch.int64 if lpips else torch.float64)


@pytest.mark.gpu
def test_device_loader_keeps_up_over_several_batches_and_full_frames():
    """query_sparsity=None (whole query frames, dense on the device) and more batches than staging buffers: every buffer is reused."""
    ds = dataio.RealEstate10k(train_scene.img_root(), train_scene.pose_root(), num_ctxt_views=2, num_query_views=1, query_sparsity=None, augment=True)
    dev = torch.device("cuda:0")
    host = dataio.TrainLoader(ds, batch_size=1, seed=3, num_workers=4)
    device = dataio.TrainLoader(ds, batch_size=1, seed=3, num_workers=4, device=dev, prefetch=1)
    n = 0
    for _ in range(2):
        for (h_inp, _), (d_inp, _) in zip(host, device):
            for part in h_inp:
                for k, want in h_inp[part].items():
                    assert torch.equal(d_inp[part][k].cpu(), want), (part, k)
            assert d_inp["query"]["rgb"].shape == (1, 1, 65536, 3)
            n += 1
    assert n == 6


def _train(tmp_path, *extra):
    return subprocess.run([sys.executable, TRAIN, "--experiment_name", "t", "--views", "2", "--data_root", train_scene.img_root(), "--pose_root",
                           train_scene.pose_root(), "--batch_size", "2", "--max_steps", "3", "--steps_til_summary", "1", "--num_workers", "4",
                           "--logging_root", str(tmp_path), *extra], capture_output=True, text=True, timeout=1500)


def _check_run(out, tmp_path, rays):
    assert out.returncode == 0, out.stdout + out.stderr
    assert any(l.startswith("data: RealEstate10K reader on ") for l in out.stdout.splitlines()), out.stdout
    lines = [l for l in out.stdout.splitlines() if l.startswith("step ")]
    assert len(lines) == 3 and all(f"2 scenes x {rays} rays" in l for l in lines), out.stdout
    losses = [float(l.split("loss")[1].split()[0]) for l in lines]
    assert all(np.isfinite(x) and x > 0 for x in losses), losses
    ckpt = torch.load(tmp_path / "t" / "checkpoints" / "model_final.pth", map_location="cpu")
    assert set(ckpt) == {"model", "optimizer"} and any(k.startswith("encoder.") for k in ckpt["model"])
    return lines


@pytest.mark.gpu
def test_train_script_runs_on_the_reader(tmp_path):
    _check_run(_train(tmp_path), tmp_path, 192)


@pytest.mark.gpu
def test_train_script_runs_on_the_reader_with_lpips_and_depth(tmp_path):
    vgg, lin = LR.state_dicts(*LR.seeded_weights(0), "split")
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin.pth")
    lines = _check_run(_train(tmp_path, "--lpips", "--depth", "--lpips_weights", str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth")), tmp_path, 1024)
    terms = [float(l.split("lpips")[1].split()[0]) for l in lines]
    assert all(np.isfinite(t) and t >= 0 for t in terms), terms                # 0 when every scene of a step drew random pixels (mask 0)
