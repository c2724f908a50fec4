"""A/B of the split-bf16 GEMM (glb_gemm_f32_split) against torch.addmm, per GPT-2 projection shape and row count, in one
process, the two arms alternating round by round (median of the rounds).  c_fc is timed with its tanh GELU: a separate
GELU kernel after addmm, the epilogue in the split GEMM.  What fuse.SPLIT_GEMM_MIN_ROWS is read from.

    python tools/split_gemm_ab.py [--rounds 7] [--iters 20] [--rows 512,1024,...]

With --form the two arms are the kernel's two tile forms (glb_gemm_f32_split_form: 128 x 128 and 64 x 64) instead, at the
row counts the packed `sis` step feeds, and a `# crossover` line per shape names the first row count from which the large
form wins (by the medians) at every larger measured one - what glb_gemm_split_pick's thresholds are read from.

    python tools/split_gemm_ab.py --form [--rounds 7] [--iters 20] [--rows 1024,2176,...]
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


FORM_ROWS = "1024,2176,3200,4224,5248,6272,7296,8320,9344,12288,16384"


def _spread(ts):
    """median (min ... max) of the rounds"""
    return f"{statistics.median(ts):8.1f} ({min(ts):7.1f} ...{max(ts):7.1f})"


def forms(eng, args, g):
    from genlm_backend_amd import _lib

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# {torch.cuda.get_device_name(0)}, {cus} CUs; rounds {args.rounds} x {args.iters} calls, the forms alternating; "
          "us per call: median (min ... max)")
    print(f"{'shape':12s} {'n':>5s} {'k':>5s} {'M':>6s} {'tiles/CU':>8s} {'large us':>28s} {'small us':>28s} {'small/large':>11s} "
          f"{'picked':>6s}")
    for name, n, k, gelu in SHAPES:
        w = torch.randn(k, n, device="cuda", generator=g) * 0.02
        bias = torch.randn(n, device="cuda", generator=g) * 0.05
        img = eng.gemm_split_weights(w)
        rows = [int(r) for r in (args.rows or FORM_ROWS).split(",")]
        large_wins = []
        for m in rows:
            x = torch.randn(m, k, device="cuda", generator=g)
            out = torch.empty(m, n, device="cuda")
            arms = [lambda f=f: eng.gemm_split(x, img, n, bias, gelu=gelu, out=out, form=f)
                    for f in (_lib.GEMM_FORM_LARGE, _lib.GEMM_FORM_SMALL)]
            for fn in arms:
                fn()
            torch.cuda.synchronize()
            tl, ts = [], []
            for _ in range(args.rounds):
                tl.append(_time(arms[0], args.iters))
                ts.append(_time(arms[1], args.iters))
            ml, ms = statistics.median(tl), statistics.median(ts)
            large_wins.append(ml <= ms)
            picked = "small" if eng.gemm_split_pick(m, n, k) == _lib.GEMM_FORM_SMALL else "large"
            tiles = -(-m // 128) * (n // 128) / cus
            print(f"{name:12s} {n:5d} {k:5d} {m:6d} {tiles:8.3f} {_spread(tl)} {_spread(ts)} {ms / ml:11.3f} {picked:>6s}",
                  flush=True)
        first = len(rows)
        while first > 0 and large_wins[first - 1]:
            first -= 1
        print(f"# crossover {name} n {n} k {k} M {rows[first] if first < len(rows) else 'none'}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", default=None)
    ap.add_argument("--form", action="store_true", help="time the kernel's two tile forms against each other")
    args = ap.parse_args()
    eng = HipEngine("cuda:0")
    g = torch.Generator(device="cuda").manual_seed(0)
    if args.form:
        return forms(eng, args, g)
    args.rows = args.rows or "256,512,1024,1536,2048,3072,4096,6144,9216,11520,14336,18432"
    print(f"# {torch.cuda.get_device_name(0)}; rounds {args.rounds} x {args.iters} calls, median (min ... max) per call")
    print(f"{'shape':12s} {'M':>6s} {'library us':>28s} {'split us':>28s} {'lib TF':>7s} {'split TF':>9s} {'split/lib':>9s}")
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
            print(f"{name:12s} {m:6d} {_spread(tl)} {_spread(ts)} {fl / ml / 1e6:7.1f} {fl / ms / 1e6:9.1f} {ms / ml:9.3f}",
                  flush=True)


if __name__ == "__main__":
    main()
