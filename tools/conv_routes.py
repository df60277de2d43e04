"""Kernel-selection tables of libyolomi's convolutions, computed on the host (no GPU needed).

Every selection entry point (ym_conv_kernel, ym_conv_algo, ym_conv_fwd_stat_rows, ym_conv_fwd_bn_fused,
ym_conv_fwd_eval_ok, the workspace sizes, ym_bn_bwd_fold_ok) is pure host code.  This tool asks them about a fixed
sweep of descriptors under the default policy, under ym_conv_set_select_batch(64) and under every setter of
include/yolomi_experimental.h at its non-default values, one at a time (plus a few combinations whose effect shows
only together).  Where the forward takes the direct kernel the statistics row count follows the device (CUs x
occupancy), so it is recorded as null.  tests/golden/conv_routes.json records the
answers (full tables for the first two settings, packed; a SHA-256 of the table for the others);
tests/test_conv_routes_cpu.py recomputes them, so a change to the selection code that moves any call to another
kernel, row count or workspace size fails there.

    python tools/conv_routes.py --check            # compare the built library with the golden file
    python tools/conv_routes.py --show             # the golden file's tables, readable
    python tools/conv_routes.py --write            # regenerate it (only when a selection change is intended)
    YOLOMI_LIB=/path/to/libyolomi.so python tools/conv_routes.py --write    # ... from another build
"""
from __future__ import annotations

import argparse
import base64
import ctypes
import hashlib
import itertools
import json
import lzma
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "conv_routes.json"
for _p in (str(ROOT), str(ROOT / "yolo-scratch_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# the case lists of tests/test_gpu_conv.py (n, h, w, cin, cout, k, stride, pad, x extra channels, y extra channels,
# out_f32) and tests/test_gpu_eval_conv.py, frozen here: the golden file is keyed on this sweep, not on the tests
_CONV_TESTS = [
    # SHAPES (fp32 output, contiguous)
    (2, 9, 11, 64, 96, 3, 2, 1, 0, 0, 1), (2, 8, 8, 32, 64, 3, 1, 1, 0, 0, 1), (1, 7, 5, 48, 40, 1, 2, 0, 0, 0, 1),
    (2, 13, 13, 128, 136, 3, 2, 1, 0, 0, 1), (1, 6, 6, 16, 24, 1, 1, 0, 0, 0, 1), (3, 20, 20, 256, 128, 3, 2, 1, 0, 0, 1),
    (1, 5, 7, 520, 264, 3, 1, 1, 0, 0, 1), (2, 9, 9, 256, 136, 1, 1, 0, 0, 0, 1), (2, 33, 17, 64, 64, 3, 1, 1, 0, 0, 1),
    (2, 32, 32, 64, 128, 3, 1, 1, 0, 0, 1), (5, 20, 20, 96, 64, 3, 1, 1, 0, 0, 1), (1, 40, 40, 128, 136, 3, 1, 1, 0, 0, 1),
    (16, 64, 64, 32, 128, 3, 1, 1, 0, 0, 1), (3, 24, 10, 72, 80, 3, 1, 1, 0, 0, 1), (2, 40, 40, 128, 72, 3, 2, 1, 0, 0, 1),
    (1, 20, 20, 64, 64, 3, 1, 1, 0, 0, 1), (3, 64, 72, 64, 64, 3, 1, 1, 0, 0, 1), (2, 9, 7, 64, 32, 3, 1, 1, 0, 0, 1),
    (1, 10, 10, 8, 16, 3, 1, 1, 0, 0, 1), (2, 11, 11, 16, 32, 3, 2, 1, 0, 0, 1),
    # PIPE, HPIPE, HALO_VIEWS (fp16 output through channel-slice views)
    (16, 64, 64, 128, 128, 3, 1, 1, 0, 0, 2), (18, 61, 63, 128, 192, 3, 1, 1, 64, 8, 2),
    (16, 64, 64, 64, 128, 3, 1, 1, 0, 64, 2), (16, 128, 128, 64, 128, 3, 2, 1, 0, 0, 2),
    (70, 63, 61, 128, 128, 3, 2, 1, 0, 0, 2), (16, 64, 64, 256, 128, 1, 1, 0, 128, 0, 2),
    (12, 80, 80, 64, 64, 3, 1, 1, 0, 0, 2),
    (2, 16, 16, 128, 128, 3, 1, 1, 0, 0, 2), (1, 32, 48, 128, 128, 3, 1, 1, 64, 0, 2),
    (2, 16, 32, 128, 192, 3, 1, 1, 0, 8, 2), (3, 32, 32, 256, 128, 3, 1, 1, 0, 0, 2),
    (2, 48, 16, 192, 256, 3, 1, 1, 32, 64, 2), (9, 80, 80, 128, 128, 3, 1, 1, 0, 0, 2),
    (2, 16, 16, 64, 64, 3, 1, 1, 0, 0, 2), (3, 32, 48, 64, 64, 3, 1, 1, 64, 32, 2), (9, 80, 80, 64, 64, 3, 1, 1, 0, 0, 2),
    (1, 16, 16, 64, 64, 3, 1, 1, 0, 0, 2), (1, 32, 32, 128, 128, 3, 1, 1, 64, 0, 2),
    (2, 20, 20, 128, 128, 3, 1, 1, 0, 128, 2), (3, 40, 40, 64, 64, 3, 1, 1, 32, 32, 2),
    (2, 16, 16, 256, 128, 3, 1, 1, 0, 0, 2), (4, 80, 80, 64, 64, 3, 1, 1, 0, 0, 2),
    # DIRECT
    (2, 17, 19, 32, 64, 3, 2, 1, 0, 0, 2), (3, 33, 21, 32, 32, 3, 1, 1, 32, 16, 2), (2, 15, 13, 64, 64, 1, 1, 0, 0, 64, 2),
    (2, 11, 23, 96, 128, 1, 1, 0, 32, 0, 2), (1, 19, 9, 64, 64, 1, 1, 0, 0, 0, 2), (2, 21, 16, 32, 64, 3, 2, 1, 32, 0, 2),
    (10, 320, 320, 32, 64, 3, 2, 1, 0, 0, 2),
    # FOLD
    (16, 64, 64, 128, 128, 3, 1, 1, 0, 0, 2), (16, 64, 64, 256, 192, 1, 1, 0, 0, 0, 2),
    (16, 128, 128, 64, 128, 3, 1, 1, 0, 0, 2), (2, 20, 20, 128, 128, 3, 1, 1, 0, 0, 2), (3, 20, 20, 64, 64, 3, 1, 1, 0, 0, 2),
    (2, 20, 20, 256, 128, 1, 1, 0, 0, 0, 2), (24, 80, 80, 64, 64, 3, 1, 1, 0, 0, 2),
]
_EVAL_TESTS = [     # n, h, w, cin, cout, k, stride (output a slice of a cout + 24 channel buffer)
    (1, 20, 20, 128, 128, 3, 1), (2, 20, 20, 72, 64, 3, 1), (1, 10, 10, 256, 128, 3, 1), (1, 20, 20, 512, 256, 1, 1),
    (2, 40, 40, 128, 128, 3, 2), (2, 13, 11, 64, 96, 3, 2), (1, 80, 80, 64, 64, 1, 1), (1, 160, 160, 32, 32, 3, 1),
    (2, 20, 20, 64, 40, 1, 1), (1, 20, 20, 136, 64, 3, 1), (1, 10, 10, 1024, 64, 1, 1), (2, 40, 40, 48, 16, 3, 1),
    (1, 20, 20, 256, 24, 3, 1), (4, 128, 128, 64, 64, 1, 1), (4, 128, 128, 128, 128, 3, 1),
    (8, 160, 160, 64, 64, 3, 1), (1, 20, 20, 64, 32, 1, 1), (1, 20, 20, 256, 256, 3, 2), (1, 80, 80, 128, 64, 3, 1),
    (16, 80, 80, 128, 64, 3, 1),
]

# setters of include/yolomi_experimental.h: (name, the values swept one at a time).  Enumerated policies get every
# legal explicit value, thresholds a few on either side of their default.
SETTERS = [
    ("ym_conv_set_select_batch", (8,)),                 # 64 has a full table of its own
    ("ym_conv_set_halo", (0, 1, 2, 3)),
    ("ym_conv_set_pipe", (0, 1, 2, 3)),
    ("ym_conv_set_direct", (0, 1, 2, 3)),
    ("ym_conv_set_hpipe", (0, 1, 2)),
    ("ym_wgrad_set_target", (128, 512)),
    ("ym_conv_set_fold", (0, 1)),
    ("ym_conv_set_eval_cfg", (0, 2)),
    ("ym_conv_set_eval_narrow", (0,)),
    ("ym_conv_set_eval_split", (0, 16, 256)),
    ("ym_conv_set_eval_split_nk", (4, 27)),
    ("ym_conv_set_eval_pipe", (0,)),
    ("ym_conv_set_eval_route", (1, 2, 3)),
    ("ym_conv_set_eval_gemm_tiles", (4, 64)),
    ("ym_bn_set_bwd_fold", (0, 1, 2)),
]
# a few settings whose effect shows only together (the narrow tile's K-stage depth under eval cfg 0, the GEMM route of
# small halo layers, the inference threshold of the direct kernel at a pinned batch)
COMBOS = [
    (("ym_conv_set_eval_cfg", 0), ("ym_conv_set_eval_narrow", 0)),
    (("ym_conv_set_eval_route", 3), ("ym_conv_set_eval_gemm_tiles", 64), ("ym_conv_set_halo", 1)),
    (("ym_conv_set_select_batch", 64), ("ym_conv_set_direct", 3), ("ym_conv_set_hpipe", 2)),
]
_ALL_SETTERS = [n for n, _ in SETTERS]
BN_FOLD_M = (400, 1600, 25600, 25601, 102400, 102401)
BN_FOLD_C = (64, 96, 128, 2048)


def descriptors():
    """The sweep: tuples (n, h, w, cin, cout, k, stride, pad, x_ld, y_ld, out_f32, accumulate)."""
    out = []

    def add(n, hw, cin, cout, k, s, xe=0, ye=0, out_f32=2, acc=0):
        out.append((n, hw, hw, cin, cout, k, s, k // 2, cin + xe, cout + ye, out_f32, acc))

    for n, hw, cin, cout, k, s in itertools.product((1, 8, 64), (20, 40, 80, 160, 320), (32, 64, 128, 256),
                                                    (32, 64, 96, 128, 256), (1, 3), (1, 2)):
        add(n, hw, cin, cout, k, s)
    for n, h, w, cin, cout, k, s, p, xe, ye, of in _CONV_TESTS:
        out.append((n, h, w, cin, cout, k, s, p, cin + xe, cout + ye, of, 0))
    for n, h, w, cin, cout, k, s in _EVAL_TESTS:
        out.append((n, h, w, cin, cout, k, s, k // 2, cin, cout + 24, 2, 0))
    # a few channel-slice views, bf16 / fp32 outputs and accumulating calls
    small = list(itertools.product((1, 64), (20, 80, 160), (64,), (64, 128), (1, 3), (1, 2)))
    for n, hw, cin, cout, k, s in small:
        add(n, hw, cin, cout, k, s, xe=8, ye=24)
    for of in (0, 1):
        for n, hw, cin, cout, k, s in small:
            add(n, hw, cin, cout, k, s, out_f32=of)
    for n, hw, cin, cout, k, s in small:
        add(n, hw, cin, cout, k, s, out_f32=0, acc=1)
    return out


def _conv_desc(t):
    from yolomi._lib import ConvDesc
    n, h, w, cin, cout, k, s, p, x_ld, y_ld, of, acc = t
    d = ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.k, d.stride, d.pad = n, h, w, cin, cout, k, s, p
    d.oh, d.ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    d.x_bs, d.x_ld, d.y_bs, d.y_ld = h * w * x_ld, x_ld, d.oh * d.ow * y_ld, y_ld
    d.out_f32, d.accumulate = of, acc
    return d


def table(L, descs):
    """One setting's answers: a row per descriptor and the ym_bn_bwd_fold_ok grid."""
    name = ctypes.create_string_buffer(96)
    rows = []
    for d in descs:
        r = ctypes.byref(d)
        row = []
        for direction in (0, 1, 2):
            row.append(L.ym_conv_kernel(r, direction, name, 96))
            row.append(name.value.decode())
        a0 = L.ym_conv_algo(r, 0)
        rows_ = L.ym_conv_fwd_stat_rows(r)
        # the direct kernel's grid (its statistics rows) follows the device's CU count and occupancy
        row += [a0, L.ym_conv_algo(r, 1), None if a0 == 3 else rows_, L.ym_conv_fwd_bn_fused(r),
                L.ym_conv_fwd_eval_ok(r), L.ym_conv_fwd_eval_workspace_size(r), L.ym_conv_wgrad_workspace_size(r)]
        rows.append(row)
    bn = [L.ym_bn_bwd_fold_ok(m, c) for m in BN_FOLD_M for c in BN_FOLD_C]
    return {"rows": rows, "bn_bwd_fold_ok": bn}


def _digest(t):
    return hashlib.sha256(json.dumps(t, separators=(",", ":")).encode()).hexdigest()


def sweep(L=None):
    """Every setting's table: {"descs", "default", "select_batch_64", "sha256": {"<setter>=<value>": digest}}.
    The setters are put at their defaults first and left as they were found."""
    if L is None:
        from yolomi._lib import lib
        L = lib()
    tuples = descriptors()
    descs = [_conv_desc(t) for t in tuples]
    # select_batch's default is 0, every other setter restores its default on -1
    saved = [(n, getattr(L, n)(0 if n == "ym_conv_set_select_batch" else -1)) for n in _ALL_SETTERS]
    try:
        out = {"descs": [list(t) for t in tuples], "default": table(L, descs)}
        prev = L.ym_conv_set_select_batch(64)
        try:
            out["select_batch_64"] = table(L, descs)
        finally:
            L.ym_conv_set_select_batch(prev)
        out["sha256"] = {}
        settings = [((setter, v),) for setter, values in SETTERS for v in values] + COMBOS
        for setting in settings:
            prev = [(setter, getattr(L, setter)(v)) for setter, v in setting]
            try:
                out["sha256"][" ".join(f"{setter}={v}" for setter, v in setting)] = _digest(table(L, descs))
            finally:
                for setter, v in prev:
                    getattr(L, setter)(v)
        assert _digest(table(L, descs)) == _digest(out["default"]), "a setter was not restored"
    finally:
        for n, v in saved:
            getattr(L, n)(v)
    return out


COLUMNS = ("fwd kernel id", "fwd kernel", "dgrad kernel id", "dgrad kernel", "wgrad kernel id", "wgrad kernel",
           "fwd algo", "dgrad algo", "fwd stat rows", "fwd bn fused", "eval ok", "eval workspace", "wgrad workspace")


def first_difference(got, want):
    """None, or a sentence naming the first entry of a sweep that differs from the golden one."""
    if got["descs"] != want["descs"]:
        return "the descriptor sweep itself differs from the golden file's"
    for key in ("default", "select_batch_64"):
        for t, g, w in zip(got["descs"], got[key]["rows"], want[key]["rows"]):
            if g != w:
                col = next(c for c, a, b in zip(COLUMNS, g, w) if a != b)
                return (f"{key}: descriptor (n,h,w,cin,cout,k,stride,pad,x_ld,y_ld,out_f32,accumulate)={tuple(t)}: "
                        f"{col}: got {g[COLUMNS.index(col)]!r}, golden {w[COLUMNS.index(col)]!r}")
        if got[key]["bn_bwd_fold_ok"] != want[key]["bn_bwd_fold_ok"]:
            return f"{key}: ym_bn_bwd_fold_ok grid: got {got[key]['bn_bwd_fold_ok']}, golden {want[key]['bn_bwd_fold_ok']}"
    if sorted(got["sha256"]) != sorted(want["sha256"]):
        return "the swept settings differ from the golden file's"
    for k in got["sha256"]:
        if got["sha256"][k] != want["sha256"][k]:
            return f"setting {k}: table digest differs from the golden file's"
    return None


_FULL = ("descs", "default", "select_batch_64")


def dump(s, path):
    """The digests in the clear; the descriptors and the two full tables (some 3000 machine-made rows) as
    base64(xz(JSON)) — --show prints them."""
    blob = base64.b64encode(lzma.compress(json.dumps({k: s[k] for k in _FULL}, separators=(",", ":")).encode(), preset=9)).decode()
    doc = {"columns": COLUMNS, "sha256": s["sha256"], "tables_xz_base64": [blob[i:i + 112] for i in range(0, len(blob), 112)]}
    Path(path).write_text(json.dumps(doc, indent=0, sort_keys=True) + "\n")


def load(path):
    """The golden file in sweep()'s form."""
    doc = json.loads(Path(path).read_text())
    out = json.loads(lzma.decompress(base64.b64decode("".join(doc["tables_xz_base64"]))))
    out["sha256"] = doc["sha256"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--check", action="store_true", help="compare the library's answers with the golden file")
    g.add_argument("--write", action="store_true", help="write the golden file from the library's answers")
    g.add_argument("--show", action="store_true", help="print the golden file's tables, a descriptor and its row per line")
    ap.add_argument("--golden", default=str(GOLDEN))
    a = ap.parse_args()
    if a.show:
        want = load(a.golden)
        for key in _FULL[1:]:
            print(key, "ym_bn_bwd_fold_ok", want[key]["bn_bwd_fold_ok"])
            for t, r in zip(want["descs"], want[key]["rows"]):
                print(key, t, r)
        return 0
    s = sweep()
    algos = {}
    for r in s["default"]["rows"]:
        algos[r[6]] = algos.get(r[6], 0) + 1
    print(f"{len(s['descs'])} descriptors, {2 + len(s['sha256'])} settings; default forward algos {dict(sorted(algos.items()))}")
    if a.write:
        dump(s, a.golden)
        print(f"wrote {a.golden}")
        return 0
    diff = first_difference(json.loads(json.dumps(s)), load(a.golden))
    print(diff or "identical to the golden file")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
