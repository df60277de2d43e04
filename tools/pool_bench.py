"""Timing of ym_sppf_fwd / ym_sppf_bwd over batch sizes and map shapes and of ym_upsample2_fwd / _bwd at the s@640
bs64 head shapes, each launch alone on an idle GPU (HIP events around 10 launches; median and minimum of 30).
YOLOMI_LIB picks the library, so two builds compare as two processes (profiles/pool/kernels.txt).
usage: [YOLOMI_LIB=/path/to/libyolomi.so] python tools/pool_bench.py OUT.json"""
import json
import os
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "yolo-scratch_amd")]
import torch
from yolomi._lib import call, stream_ptr


def timeit(fn, reps=30, inner=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1000 / inner)
    ts.sort()
    return round(ts[len(ts) // 2], 1), round(ts[0], 1)


out = {}
st = stream_ptr()
for (B, H, W, C) in [(64, 20, 20, 256), (1, 20, 20, 256), (2, 20, 20, 256), (4, 20, 20, 256), (8, 20, 20, 256),
                     (16, 20, 20, 256), (8, 40, 40, 512), (64, 10, 10, 128)]:
    M = B * H * W
    x = (torch.randint(-8, 8, (M, C)).float() / 4).cuda()
    code = torch.zeros(3, M, C, dtype=torch.uint8, device="cuda")
    ybuf = torch.zeros(B, H, W, 4 * C, dtype=torch.float16, device="cuda")
    gbuf = torch.randn(B, H, W, 4 * C, device="cuda").bfloat16()
    dx32 = torch.empty(M, C, device="cuda")
    bs, ld = H * W * 4 * C, 4 * C
    sl = lambda t, j: t.data_ptr() + 2 * j * C
    f = lambda: call("ym_sppf_fwd", x.data_ptr(), code.data_ptr(), sl(ybuf, 1), sl(ybuf, 2), sl(ybuf, 3), bs, ld,
                     None, B, H, W, C, st)
    b = lambda: call("ym_sppf_bwd", code.data_ptr(), sl(gbuf, 1), sl(gbuf, 2), sl(gbuf, 3), bs, ld, gbuf.data_ptr(), bs,
                     ld, 0, dx32.data_ptr(), B, H, W, C, st)
    out[f"sppf_fwd {B}x{H}x{W}x{C}"] = timeit(f)
    out[f"sppf_bwd {B}x{H}x{W}x{C}"] = timeit(b)
for (n, h, w, c, xc, yc) in [(64, 20, 20, 512, 512, 768), (64, 40, 40, 256, 256, 384)]:
    xb = torch.randn(n, h, w, xc, device="cuda").bfloat16()
    yb = torch.randn(n, 2 * h, 2 * w, yc, device="cuda").bfloat16()
    f = lambda: call("ym_upsample2_fwd", xb.data_ptr(), h * w * xc, xc, yb.data_ptr(), 4 * h * w * yc, yc, n, h, w, c, st)
    b = lambda: call("ym_upsample2_bwd", yb.data_ptr(), 4 * h * w * yc, yc, xb.data_ptr(), h * w * xc, xc, n, h, w, c, 0, st)
    b1 = lambda: call("ym_upsample2_bwd", yb.data_ptr(), 4 * h * w * yc, yc, xb.data_ptr(), h * w * xc, xc, n, h, w, c, 1, st)
    out[f"up_fwd {n}x{h}x{w}x{c}"] = timeit(f)
    out[f"up_bwd {n}x{h}x{w}x{c}"] = timeit(b)
    xb.zero_()
    out[f"up_bwd_acc {n}x{h}x{w}x{c}"] = timeit(b1)
print(os.environ.get("YOLOMI_LIB", "tree"), "us (median, min)")
for k, v in out.items():
    print(f"  {k:32s} {v[0]:8.1f} {v[1]:8.1f}")
json.dump(out, open(sys.argv[1], "w"), indent=1)
