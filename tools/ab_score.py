#!/usr/bin/env python
"""A/B timing of scoring given tokens, HIP events, medians of alternating runs in one process:

  rows      HipEngine.score_rows against what the library offered before it - log_softmax_rows, then a gather of the target
            column - on [10240, 50257] float32 and [5120, 128256] bfloat16 logits, with and without bit masks
  sequences batch_sequence_logprobs_device for 1024 GPT-2-small sequences of 10 tokens against ten
            batch_next_token_logprobs_sync calls, one per prefix

    python tools/ab_score.py [--what rows|sequences|all] [--rounds 3] [--json out.json]
Prints one JSON line per case: microseconds, and for score_rows the fraction of 8 TB/s on its algorithmic bytes (the logits
once, the mask words once)."""
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
    """{name: median microseconds} of `rounds` alternating timings of every arm (one warm-up each first)."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            got[k].append(timed(fn, iters))
    return {k: statistics.median(v) for k, v in got.items()}


def rows_cases(eng, rounds):
    dev = eng.device
    out = []
    for n, V, dtype in ((10240, 50257, torch.float32), (5120, 128256, torch.bfloat16)):
        g = torch.Generator(device=dev).manual_seed(1)
        x = (2 * torch.randn((n, V), device=dev, generator=g)).to(dtype)
        tok = torch.randint(0, V, (n,), device=dev, generator=g, dtype=torch.int32)
        bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (64, (V + 31) // 32), device=dev, generator=g, dtype=torch.int32)
        ids = torch.randint(0, 64, (n,), device=dev, generator=g, dtype=torch.int32)
        idx = tok.long()[:, None]
        arms = {
            "score_rows": lambda: eng.score_rows(x, tok, want=("logp",)),
            "score_rows_bits": lambda: eng.score_rows(x, tok, mask_kind=1, mask=bits, row_mask_id=ids, want=("logp", "logZ", "logp_masked")),
            "log_softmax_gather": lambda: eng.log_softmax_rows(x).gather(1, idx),
        }
        us = alternate(arms, rounds, 5)
        nbytes = n * V * x.element_size()
        for k, v in us.items():
            extra = n * bits.shape[1] * 4 if k == "score_rows_bits" else 0
            out.append({"case": k, "rows": n, "vocab": V, "dtype": str(dtype).split(".")[-1], "us": round(v, 1),
                        "frac_of_8TBs": round((nbytes + extra) / (v * 1e-6) / PEAK, 3) if k.startswith("score") else None})
    return out


def sequence_cases(eng, rounds):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM

    dev = eng.device
    llm = AsyncAmdLM.from_config(GPT2Config(), None, device=dev, seed=0, engine=eng, batch_size=64, timeout=0.02)
    N, P, T = 1024, 8, 10
    rs = np.random.default_rng(0)
    prompt = rs.integers(1, 50000, P).tolist()
    conts = rs.integers(1, 50000, (N, T)).tolist()
    tokens = torch.tensor([prompt + c for c in conts], dtype=torch.int32, device=dev)
    lengths = torch.full((N,), P + T, dtype=torch.int32, device=dev)
    plen = torch.full((N,), P, dtype=torch.int32, device=dev)

    def old():
        for t in range(T):
            llm.clear_cache()
            llm.batch_next_token_logprobs_sync([prompt + c[:t] for c in conts])

    arms = {"batch_sequence_logprobs_device": lambda: llm.batch_sequence_logprobs_device(tokens, lengths, plen),
            "ten_next_token_logprobs_calls": old}
    us = alternate(arms, rounds, 1)
    return [{"case": k, "sequences": N, "tokens": T, "us": round(v, 1)} for k, v in us.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all", choices=("rows", "sequences", "all"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json")
    a = ap.parse_args()
    eng = HipEngine(torch.device("cuda:0"))
    res = []
    if a.what in ("rows", "all"):
        res += rows_cases(eng, a.rounds)
    if a.what in ("sequences", "all"):
        res += sequence_cases(eng, a.rounds)
    for r in res:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
