"""Writes the summary fixture (build container only): what the REFERENCE's ``summaries.img_summaries`` (summaries.py:15-141) makes of the
seeded inputs of tests/summary_cases.py, as tests/golden/summary_expected.npz.  torchvision is not installed here, so the reference runs
with a stand-in ``torchvision.utils.make_grid`` that RECORDS its argument and returns the restatement's grid (tests/summary_restatement.py;
the timm_stub.py precedent): the fixture pins what the reference's own code hands to make_grid — the painted epipolar panel, the
jet-coloured depth, the clamped predictions — and its scalars, not make_grid itself.  matplotlib is the real package.
Run:  python tests/golden/make_summary_golden.py"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402
import summary_cases  # noqa: E402
import summary_restatement as R  # noqa: E402


class Recorder:
    """The writer and the make_grid stand-in: tags in call order, make_grid's arguments channel-last, scalars as float64."""

    def __init__(self):
        self.tags, self.grid_inputs, self.scalars, self.images = [], [], {}, {}

    def make_grid(self, tensor, scale_each=False, normalize=False, **kw):
        assert normalize and not kw, "the reference calls make_grid(x, scale_each=..., normalize=True) only"
        x = tensor.detach().cpu().numpy().transpose(0, 2, 3, 1).copy()
        self.grid_inputs.append(x)
        return torch.from_numpy(R.make_grid(x, scale_each=scale_each))

    def add_image(self, tag, img, step):
        self.tags.append(tag)
        self.images[tag] = self.grid_inputs[-1]

    def add_scalar(self, tag, value, step):
        self.tags.append(tag)
        self.scalars[tag] = float(value)


def main():
    import matplotlib
    assert not isinstance(matplotlib, ref_import._Anything), "the fixture needs the real matplotlib"
    ref_import.load_reference()                                       # geometry / utils behind the usual stand-ins
    sys.path.insert(0, ref_import.REFERENCE_ROOT)
    try:
        ref = importlib.import_module("summaries")
    finally:
        sys.path.remove(ref_import.REFERENCE_ROOT)
    out = {}
    for name, (B, V, H, W) in summary_cases.CASES.items():
        model_input, model_output = summary_cases.build(name)
        rec = Recorder()
        ref.torchvision = types.SimpleNamespace(utils=types.SimpleNamespace(make_grid=rec.make_grid))
        with contextlib.redirect_stdout(io.StringIO()):               # the reference's two prints
            ref.img_summaries(None, model_input, None, {}, model_output, rec, 0, prefix="val_", img_shape=(H, W), n_view=V)
        out[f"{name}.checksum"] = summary_cases.checksum(*summary_cases.build(name))
        out[f"{name}.tags"] = np.array(rec.tags)
        out[f"{name}.epipolar_line"] = rec.images["val_epipolar_line"]
        out[f"{name}.depth_images"] = rec.images["val_depth_images"]
        out[f"{name}.predictions"] = rec.images["val_predictions"]
        for tag, v in rec.scalars.items():
            out[f"{name}.{tag[4:]}"] = np.float64(v)
    np.savez_compressed(summary_cases.FIXTURE, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(summary_cases.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
