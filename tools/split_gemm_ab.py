"""A/B of the split-bf16 GEMM (glb_gemm_f32_split) against torch.addmm, per GPT-2 projection shape and row count, in one
process, the two arms alternating round by round (median of the rounds).  c_fc is timed with its tanh GELU: a separate
GELU kernel after addmm, the epilogue in the split GEMM.  What fuse.SPLIT_GEMM_MIN_ROWS is read from.

    python tools/split_gemm_ab.py [--rounds 7] [--iters 20] [--rows 512,1024,...]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genlm_backend_amd  # noqa: E402,F401
from genlm_backend_amd.engine import HipEngine  # noqa: E402

SHAPES = [("attn.c_attn", 2304, 768, False), ("attn.c_proj", 768, 768, False), ("mlp.c_fc", 3072, 768, True),
          ("mlp.c_proj", 768, 3072, False)]


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", default="256,512,1024,1536,2048,3072,4096,6144,9216,11520,14336,18432")
    args = ap.parse_args()
    eng = HipEngine("cuda:0")
    g = torch.Generator(device="cuda").manual_seed(0)
    print(f"# {torch.cuda.get_device_name(0)}; rounds {args.rounds} x {args.iters} calls, median per call")
    print(f"{'shape':12s} {'M':>6s} {'library us':>11s} {'split us':>9s} {'lib TF':>7s} {'split TF':>9s} {'split/lib':>9s}")
    for name, n, k, gelu in SHAPES:
        w = torch.randn(k, n, device="cuda", generator=g) * 0.02
        bias = torch.randn(n, device="cuda", generator=g) * 0.05
        img = eng.gemm_split_weights(w)
        for m in (int(r) for r in args.rows.split(",")):
            x = torch.randn(m, k, device="cuda", generator=g)
            out = torch.empty(m, n, device="cuda")

            def lib():
                y = torch.addmm(bias, x, w)
                return torch.nn.functional.gelu(y, approximate="tanh") if gelu else y

            def split():
                return eng.gemm_split(x, img, n, bias, gelu=gelu, out=out)

            lib(), split()
            torch.cuda.synchronize()
            tl, ts = [], []
            for _ in range(args.rounds):
                tl.append(_time(lib, args.iters))
                ts.append(_time(split, args.iters))
            ml, ms = statistics.median(tl), statistics.median(ts)
            fl = 2.0 * m * n * k
            print(f"{name:12s} {m:6d} {ml:11.1f} {ms:9.1f} {fl / ml / 1e6:7.1f} {fl / ms / 1e6:9.1f} {ms / ml:9.3f}",
                  flush=True)


if __name__ == "__main__":
    main()
