"""A/B of the 4-bit projection paths per (N, K) of Llama-3.2-1B's and Llama-3-8B's projections and row count M, in one
process, the arms alternating round by round (median of the rounds), HIP events around `iters` calls:
  (a) glb_w4_gemm on the 4-bit image                   (quant.W4Linear's fused path)
  (b) glb_w4_dequantize into a scratch + F.linear      (its other path)
  (c) F.linear on the 16-bit weight                    (an unquantised model)
Every call takes the next of a ring of weight buffers that together exceed the 256 MB Infinity Cache, so weights come from
HBM.  Then glb_w4_quantize / glb_w4_dequantize on their own, as fractions of 8 TB/s on the bytes they move, and the time to
quantise a Llama-3-8B-shaped model.  What quant.MIN_ROWS_FUSED and glb_w4_gemm_max_rows() are read from.

    python tools/w4_gemm_ab.py [--rounds 5] [--iters 20] [--rows 1,2,4,...] [--dtype bfloat16]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genlm_backend_amd  # noqa: E402,F401
from genlm_backend_amd.engine import HipEngine  # noqa: E402
from genlm_backend_amd.quant import CODEBOOKS  # noqa: E402

SHAPES = [("1B q/o", 2048, 2048), ("1B k/v", 512, 2048), ("1B gate/up", 8192, 2048), ("1B down", 2048, 8192),
          ("8B q/o", 4096, 4096), ("8B k/v", 1024, 4096), ("8B gate/up", 14336, 4096), ("8B down", 4096, 14336)]
LLAMA_8B = {(4096, 4096): 2, (1024, 4096): 2, (14336, 4096): 2, (4096, 14336): 1}  # matrices per layer, 32 layers
RING_BYTES = 320 << 20
PEAK = 8e12


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


class Ring:
    def __init__(self, items):
        self.items, self.i = items, 0

    def next(self):
        self.i = (self.i + 1) % len(self.items)
        return self.items[self.i]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", default="1,2,4,8,16,32,64,128,256,512,1024")
    ap.add_argument("--dtype", default="bfloat16")
    args = ap.parse_args()
    dtype = getattr(torch, args.dtype)
    eng = HipEngine("cuda:0")
    cb = CODEBOOKS["nf4"]
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = [int(r) for r in args.rows.split(",")]
    print(f"# {torch.cuda.get_device_name(0)}; {args.dtype}; rounds {args.rounds} x {args.iters} calls, median us per call; "
          f"glb_w4_gemm_max_rows() = {eng.w4_gemm_max_rows()}; weight rings of {RING_BYTES >> 20} MB")
    print(f"{'shape':11s} {'N':>6s} {'K':>6s} {'M':>5s} {'(a) fused':>10s} {'(b) deq+lin':>11s} {'(c) 16-bit':>10s} {'a/b':>6s} {'a/c':>6s} "
          f"{'(a) of 8TB/s':>12s}")
    quant_us = {}
    for name, n, k in SHAPES:
        img_bytes = eng.w4_bytes(n, k)
        w0 = torch.randn(n, k, device="cuda", generator=g, dtype=torch.float32).mul_(0.02).to(dtype)
        n_img = max(2, -(-RING_BYTES // img_bytes))
        imgs = Ring([eng.w4_quantize(w0, cb) for _ in range(n_img)])
        n_w = max(2, -(-RING_BYTES // (2 * n * k)))
        ws = Ring([w0.clone() for _ in range(n_w)])
        scratch = torch.empty(n, k, device="cuda", dtype=dtype)
        bias = None
        for m in rows:
            x = torch.randn(m, k, device="cuda", generator=g, dtype=torch.float32).to(dtype)
            out = torch.empty(m, n, device="cuda", dtype=dtype)

            def fused():
                return eng.w4_gemm(x, imgs.next(), n, cb, bias, out=out)

            def deq():
                eng.w4_dequantize(imgs.next(), n, k, cb, out=scratch)
                return torch.nn.functional.linear(x, scratch, bias)

            def lib():
                return torch.nn.functional.linear(x, ws.next(), bias)

            has_fused = fused() is not None
            deq(), lib()
            torch.cuda.synchronize()
            ta, tb, tc = [], [], []
            for _ in range(args.rounds):
                if has_fused:
                    ta.append(_time(fused, args.iters))
                tb.append(_time(deq, args.iters))
                tc.append(_time(lib, args.iters))
            mb, mc = statistics.median(tb), statistics.median(tc)
            if has_fused:
                ma = statistics.median(ta)
                print(f"{name:11s} {n:6d} {k:6d} {m:5d} {ma:10.1f} {mb:11.1f} {mc:10.1f} {ma / mb:6.2f} {ma / mc:6.2f} "
                      f"{img_bytes / (ma * 1e-6) / PEAK:12.3f}", flush=True)
            else:
                print(f"{name:11s} {n:6d} {k:6d} {m:5d} {'-':>10s} {mb:11.1f} {mc:10.1f} {'-':>6s} {'-':>6s} {'-':>12s}", flush=True)
        # the format kernels on their own (the source / destination ring defeats the cache as above)
        img = imgs.items[0]
        tq = statistics.median(_time(lambda: eng.w4_quantize(ws.next(), cb, out=img), args.iters) for _ in range(args.rounds))
        td = statistics.median(_time(lambda: eng.w4_dequantize(imgs.next(), n, k, cb, out=scratch), args.iters)
                               for _ in range(args.rounds))
        moved = 2 * n * k + img_bytes
        quant_us[(n, k)] = tq
        print(f"# {name}: glb_w4_quantize {tq:.1f} us = {moved / (tq * 1e-6) / PEAK:.3f} of 8 TB/s on {moved} bytes; "
              f"glb_w4_dequantize {td:.1f} us = {moved / (td * 1e-6) / PEAK:.3f}", flush=True)
        del imgs, ws, scratch
        torch.cuda.empty_cache()
    total = 32 * sum(cnt * quant_us[s] for s, cnt in LLAMA_8B.items())
    print(f"# quantising a Llama-3-8B-shaped model's 224 projections ({args.dtype} source): {total / 1e3:.1f} ms of kernel time")


if __name__ == "__main__":
    main()
