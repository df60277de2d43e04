"""Kernel selection is pinned: the library's selection entry points (pure host code, no GPU) answer the sweep of
tools/conv_routes.py exactly as tests/golden/conv_routes.json records — the kernel instance of every forward, data
gradient and weight gradient, the statistics row counts, the fused / eval decisions and the workspace sizes, under the
default policy, under ym_conv_set_select_batch(64) and (by digest) under every other setter value.  Zero mismatches:
a refactor of the selection code must leave this file alone; a change that means to move a call regenerates it
(python tools/conv_routes.py --write) and shows the moved rows in its diff."""
import importlib.util
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def routes():
    spec = importlib.util.spec_from_file_location("conv_routes", ROOT / "tools" / "conv_routes.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.sweep(), mod.load(mod.GOLDEN)


def test_conv_routes_match_golden(routes):
    mod, got, want = routes
    got = json.loads(json.dumps(got))
    diff = mod.first_difference(got, want)
    assert diff is None, diff
    assert got == {k: want[k] for k in got}


def test_conv_routes_cover_every_algo(routes):
    """The default table exercises every forward kernel family (algo 0..4) at least 5 times, the eval decision both
    ways and the K-split workspace."""
    _, got, _ = routes
    rows = got["default"]["rows"]
    for algo in range(5):
        assert sum(r[6] == algo for r in rows) >= 5, algo
    assert sum(r[10] == 1 for r in rows) >= 5 and sum(r[10] == 0 for r in rows) >= 5
    assert sum(r[11] > 0 for r in rows) >= 5
    assert len(set(got["sha256"].values())) > len(got["sha256"]) // 2      # the setters do move the tables
