#!/usr/bin/env python
"""A/B timing of the k most probable tokens per row, HIP events, alternating runs in one process:

  rows    HipEngine.topk_rows against what the library offered before it - log_softmax_rows, then torch.topk (under bit masks:
          a masked_fill with a boolean [n, V] mask made outside the clock in between) - on [1024, 50257] float32 and
          [512, 128256] bfloat16 logits, k = 8 and 64, without a mask and with a bit mask per row; and topk_rows on rows
          sorted ascending, where every element displaces one
  beam    one DeviceBeam step at width 16 over 64 prompts of GPT-2-small (random init) and one DeviceSIS step of 1024 particles

    python tools/ab_topk.py [--what rows|beam|all] [--rounds 3] [--json out.json]
Prints one JSON line per case: the median, fastest and slowest round in microseconds, and for topk_rows the floor - the
logits once at 8 TB/s - and the fraction of it reached."""
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


def rows_cases(eng, rounds):
    dev = eng.device
    out = []
    for n, V, dtype in ((1024, 50257, torch.float32), (512, 128256, torch.bfloat16)):
        g = torch.Generator(device=dev).manual_seed(1)
        x = (2 * torch.randn((n, V), device=dev, generator=g)).to(dtype)
        asc = torch.sort(x.float(), dim=1).values.to(dtype)
        bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, (V + 31) // 32), device=dev, generator=g, dtype=torch.int32)
        j = torch.arange(V, device=dev)
        forbid = ((bits[:, (j >> 5)] >> (j & 31)) & 1) == 0  # bool [n, V], made outside the clock
        nbytes = n * V * x.element_size()
        floor = nbytes / PEAK * 1e6
        for k in (8, 64):
            arms = {
                "topk_rows": lambda: eng.topk_rows(x, k, want=("logp",)),
                "log_softmax_topk": lambda: torch.topk(eng.log_softmax_rows(x), k, dim=1),
                "topk_rows_bits": lambda: eng.topk_rows(x, k, mask_kind=1, mask=bits, want=("logp", "logp_masked", "logZ")),
                "log_softmax_fill_topk": lambda: torch.topk(eng.log_softmax_rows(x).masked_fill_(forbid, float("-inf")), k, dim=1),
                "topk_rows_ascending": lambda: eng.topk_rows(asc, k, want=("logp",)),
            }
            for name, (med, lo, hi) in alternate(arms, rounds, 5).items():
                ours = name.startswith("topk_rows")
                out.append({"case": name, "rows": n, "vocab": V, "dtype": str(dtype).split(".")[-1], "k": k, "us": round(med, 1),
                            "fastest_us": round(lo, 1), "slowest_us": round(hi, 1), "floor_us": round(floor, 1) if ours else None,
                            "frac_of_floor": round(floor / med, 3) if ours else None})
    return out


def beam_cases(eng, rounds):
    from transformers import GPT2Config

    from genlm_backend_amd.beam import DeviceBeam
    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.sis import DeviceSIS

    dev = eng.device
    llm = AsyncAmdLM.from_config(GPT2Config(), None, device=dev, seed=0, engine=eng, batch_size=64, timeout=0.02)
    rs = np.random.default_rng(0)
    prompts = rs.integers(1, 50000, (64, 8)).tolist()
    beam = DeviceBeam(llm, 16, prompts, 12, 50256)
    sis = DeviceSIS(llm, 1024, prompts[0], 12, 50256, seed=0)

    def steps(obj):
        """microseconds of steps 2 .. 7 of a fresh run (step 0 holds one context a prompt)"""
        obj.reset()
        obj.step()
        obj.step()
        torch.cuda.synchronize()
        return timed(obj.step, 6)

    steps(beam), steps(sis)
    got = {"beam_step_w16_x64": [], "sis_step_1024": []}
    for _ in range(rounds):
        got["beam_step_w16_x64"].append(steps(beam))
        got["sis_step_1024"].append(steps(sis))
    return [{"case": k, "us": round(statistics.median(v), 1), "fastest_us": round(min(v), 1), "slowest_us": round(max(v), 1)}
            for k, v in got.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all", choices=("rows", "beam", "all"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json")
    a = ap.parse_args()
    eng = HipEngine(torch.device("cuda:0"))
    res = []
    if a.what in ("rows", "all"):
        res += rows_cases(eng, a.rounds)
    if a.what in ("beam", "all"):
        res += beam_cases(eng, a.rounds)
    for r in res:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
