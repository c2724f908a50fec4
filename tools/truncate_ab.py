#!/usr/bin/env python
"""A/B timing of top-k / top-p / min-p truncation, HIP events, alternating runs in one process:

  HipEngine.truncate_rows (the keep set as bit rows, one launch) against
    topk_rows            HipEngine.topk_rows with k = 64 at the same shape - a kernel that reads the row once
    sort_composition     what a PyTorch sampler does: torch.sort, softmax, cumsum, the three filters in sequence, a scatter of
                         the kept flags back to token order (a bool [n, V]: it is not even packed into bits)
  on [1024, 50257] float32 and [512, 128256] bfloat16 logits, Gaussian rows (2 N(0, 1)) and the benchmark's "peaked" rows (one
  token holds 0.9 of the mass over a Zipf(1.1) tail in random order), with top-k alone (50), top-p alone (0.9) and all three
  (50, 0.9, min-p 0.02).

    python tools/truncate_ab.py [--rounds 3] [--json out.json]
Prints one JSON line per case: the median, fastest and slowest round in microseconds, the ratios of truncate_rows's median to
both baselines', the floor - the logits once at 8 TB/s - and the tokens a row keeps."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genlm_backend_amd  # noqa: E402,F401
from genlm_backend_amd.engine import HipEngine  # noqa: E402

PEAK = 8e12  # bytes / s
OPTIONS = {"top_k": dict(top_k=50), "top_p": dict(top_p=0.9), "all_three": dict(top_k=50, top_p=0.9, min_p=0.02)}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(arms, rounds, iters):
    """{name: (median, fastest, slowest) microseconds} of `rounds` alternating timings of every arm (one warm-up each first)."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            got[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def peaked_rows(n, V, g, dev, p_top=0.9, zipf=1.1):
    """bench.py's real-shaped rows without its masks: one token holds p_top, the others fall off as rank^-zipf, random order."""
    rank = torch.argsort(torch.rand((n, V), device=dev, generator=g), dim=1) + 1
    x = -zipf * torch.log(rank.to(torch.float32))
    tail = float((torch.arange(2, V + 1, dtype=torch.float64) ** -zipf).sum())
    x[rank == 1] = float(np.log(p_top / (1.0 - p_top) * tail))
    return x


def sort_composition(x, top_k=0, top_p=1.0, min_p=0.0):
    """bool [n, V] kept, by sort + softmax + cumsum + scatter (ties at a boundary fall as the sort orders them)."""
    s, idx = torch.sort(x.float(), dim=1, descending=True)
    keep = torch.ones_like(s, dtype=torch.bool)
    if top_k:
        keep[:, top_k:] = False
        s = s.masked_fill(~keep, float("-inf"))
    if top_p < 1.0:
        pr = torch.softmax(s, dim=1)
        before = pr.cumsum(dim=1) - pr
        keep &= before < top_p
        s = s.masked_fill(~keep, float("-inf"))
    if min_p > 0.0:
        keep &= s >= s[:, :1] + float(np.log(min_p))
    return torch.zeros_like(keep).scatter_(1, idx, keep)


def cases(eng, rounds):
    dev = eng.device
    out = []
    for n, V, dtype in ((1024, 50257, torch.float32), (512, 128256, torch.bfloat16)):
        g = torch.Generator(device=dev).manual_seed(1)
        rows = {"gaussian": (2 * torch.randn((n, V), device=dev, generator=g)).to(dtype), "peaked": peaked_rows(n, V, g, dev).to(dtype)}
        floor = n * V * rows["gaussian"].element_size() / PEAK * 1e6
        for kind, x in rows.items():
            for oname, opts in OPTIONS.items():
                arms = {
                    "truncate_rows": lambda: eng.truncate_rows(x, **opts),
                    "topk_rows_k64": lambda: eng.topk_rows(x, 64, want=("logp",)),
                    "sort_composition": lambda: sort_composition(x, **opts),
                }
                got = alternate(arms, rounds, 5)
                kept = eng.truncate_rows(x, want=("kept",), **opts)["kept"].float()
                same = int((sort_composition(x, **opts).sum(dim=1) == kept).sum())
                line = {"rows": n, "vocab": V, "dtype": str(dtype).split(".")[-1], "logits": kind, "options": oname, "floor_us": round(floor, 1),
                        "kept_mean": round(float(kept.mean()), 1), "kept_max": int(kept.max()), "rows_with_the_composition_s_count": same}
                for name, (med, lo, hi) in got.items():
                    line[name + "_us"] = [round(med, 1), round(lo, 1), round(hi, 1)]
                line["truncate_over_topk"] = round(got["truncate_rows"][0] / got["topk_rows_k64"][0], 2)
                line["sort_over_truncate"] = round(got["sort_composition"][0] / got["truncate_rows"][0], 2)
                out.append(line)
                print(json.dumps(line), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json")
    a = ap.parse_args()
    res = cases(HipEngine(torch.device("cuda:0")), a.rounds)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
