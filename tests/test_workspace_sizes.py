"""The sizes a caller allocates by are public: every size and offset entry of the library returns, over a fixed grid of shapes, what it
returned before the workspace layouts moved onto csrc/car_workspace.h (tests/golden/workspace_sizes.json, written by
tools/dump_workspace_sizes.py from that library).  CPU only: no entry here touches a device."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")


@pytest.fixture(scope="module")
def dump():
    spec = importlib.util.spec_from_file_location("dump_workspace_sizes", os.path.join(ROOT, "tools", "dump_workspace_sizes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tables(dump):
    from cross_attention_renderer_amd import _lib
    _lib.load()                                                        # a stale library is rebuilt or refused here, not asked
    with open(GOLDEN) as fh:
        return json.load(fh), dump.rows(dump.bind(_lib.LIB_PATH))


def test_every_row_equals_the_recorded_one(tables):
    want, got = tables
    assert [(r["entry"], r["args"]) for r in got] == [(r["entry"], r["args"]) for r in want], "the grid changed: the table must be dumped from the same grid"
    bad = [(g["entry"], g["args"], g["value"], w["value"]) for g, w in zip(got, want) if g["value"] != w["value"]]
    assert not bad, f"{len(bad)} sizes / offsets changed (entry, args, now, recorded): {bad[:8]}"


def test_the_grid_covers_every_size_entry(dump, tables):
    """Every entry that returns a size_t, and car_workspace_find: an accepted shape that gives a size, and a refusal (0 or (size_t)-1)
    wherever the entry takes a shape at all."""
    want, _ = tables
    by_entry = {}
    for r in want:
        by_entry.setdefault(r["entry"], []).append(r)
    assert sorted(by_entry) == sorted(dump.size_entries())
    for name, rs in by_entry.items():
        values = [r["value"] if name != "car_workspace_find" else r["value"][0] + 1 for r in rs]
        assert any(0 < v < 2 ** 64 - 1 for v in values), name
        if rs[0]["args"]:
            assert len(rs) >= 4, name
            assert name in dump.NEVER_REFUSES or any(v in (0, 2 ** 64 - 1) for v in values), name
