"""A/B of glb_packed_attention_tile / DeviceSIS(share_prompt_rows="tile"), in one process, the arms alternating
round by round; median (min .. max).

Kernel: U = 1024 contexts behind one prompt of P = 48 / 128 / 512 rows with tails of t = 1 / 4 / 16 tokens, row-packed (P + U t
rows, the row map made once outside the timed calls), against glb_batch_attention_tile on the right-padded batch of the same
contexts ([U, P + t], causal, no mask: what encode_ragged hands it).  Then 8 prompts of 128 rows, the contexts behind them
grouped by prompt (a block of 64 queries names one prompt: one shared walk) and interleaved (a block names all 8: eight
walks) - equal rows, equal visible pairs: what the repeated prefix walk costs.  q / k / v are strided views of one projection
tensor, taken from a ring of such tensors larger than the 256 MB Infinity Cache; HIP events around `--iters` calls.

Step: DeviceSIS on GPT-2 small float32 (random weights), 1024 particles behind one prompt of 48 / 128 / 256 tokens, 8 steps:
share_prompt_rows="tile" against True (past 32 keys: encode_ragged); wall clock around runs that end in a synchronise.

    python tools/attn_packed_ab.py [--rounds 5] [--iters 10] [--step-rounds 3] [--no-step] [--no-kernel]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genlm_backend_amd  # noqa: E402,F401
from genlm_backend_amd.engine import HipEngine  # noqa: E402
from genlm_backend_amd.kv import packed_plan  # noqa: E402

RING_BYTES = 320 << 20
SHAPES = (("gpt2 12/12 x64 fp32", 12, 12, 64, torch.float32), ("1B 32/8 x64 bf16", 32, 8, 64, torch.bfloat16))
U = 1024


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def _ring(rows, W, dtype, g):
    n_buf = max(2, -(-RING_BYTES // (rows * W * (4 if dtype == torch.float32 else 2))))
    ring, state = [torch.randn((rows, W), device="cuda", generator=g).to(dtype) for _ in range(n_buf)], {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % n_buf
        return ring[state["i"]]

    return nxt


def _rounds(arms, rounds, iters):
    for fn in arms.values():
        fn()  # (warm-up: code objects)
    us = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            us[k].append(_time(fn, iters))
    return ({k: statistics.median(v) for k, v in us.items()},
            {k: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})" for k, v in us.items()})


def kernel_ab(eng, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(0)
    print(f"# glb_packed_attention_tile (row-packed) vs glb_batch_attention_tile (right-padded, causal), {U} contexts; us, median "
          f"(min .. max) of {rounds} alternating rounds x {iters} calls; TFLOP/s on the visible (query, key) pairs of each form")
    print(f"{'shape':22s} {'prompts':>9s} {'t':>3s} {'rows':>7s} {'packed':>30s} {'padded':>30s} {'p/p':>6s} {'TF/s pk':>8s} {'TF/s pad':>8s}")
    for name, H, Hkv, Dh, dtype in SHAPES:
        W, scale = (H + 2 * Hkv) * Dh, Dh ** -0.5

        def views(p, lead):  # q | k | v of a projection [*lead, W]
            return (p[..., :H * Dh].view(*lead, H, Dh), p[..., H * Dh:(H + Hkv) * Dh].view(*lead, Hkv, Dh),
                    p[..., (H + Hkv) * Dh:].view(*lead, Hkv, Dh))

        def packed_arm(group_lens, grp, t):
            seg, _, _, _ = packed_plan(group_lens, grp, [group_lens[g_] + t for g_ in grp])
            M = sum(group_lens) + U * t
            row_map = eng.packed_row_map(torch.from_numpy(seg).cuda(), M, max(group_lens) + t)
            nxt, out = _ring(M, W, dtype, g), torch.empty((M, H, Dh), dtype=dtype, device="cuda")
            pairs = sum(p * (p + 1) // 2 for p in group_lens) + sum(t * group_lens[g_] + t * (t + 1) // 2 for g_ in grp)
            return (lambda: eng.packed_attention_tile(*views(nxt(), (M,)), row_map, scale, out=out)), M, pairs

        for P in (48, 128, 512):
            for t in (1, 4, 16):
                L = P + t
                pk, M, pairs = packed_arm([P], [0] * U, t)
                nxt = _ring(U * L, W, dtype, g)
                pad = lambda: eng.batch_attention_tile(*(x.transpose(1, 2) for x in views(nxt().view(U, L, W), (U, L))), None, scale)
                med, cell = _rounds({"packed": pk, "padded": pad}, rounds, iters)
                print(f"{name:22s} {'1 x ' + str(P):>9s} {t:3d} {M:7d} {cell['packed']:>30s} {cell['padded']:>30s} "
                      f"{med['packed'] / med['padded']:6.3f} {4 * pairs * H * Dh / med['packed'] / 1e6:8.1f} "
                      f"{4 * U * (L * (L + 1) // 2) * H * Dh / med['padded'] / 1e6:8.1f}")
                del pk, pad, nxt
                torch.cuda.empty_cache()
        for t in (1, 4, 16):  # 8 prompts of 128: one shared walk a block against eight
            arms = {"grouped": packed_arm([128] * 8, [u * 8 // U for u in range(U)], t),
                    "interleaved": packed_arm([128] * 8, [u % 8 for u in range(U)], t)}
            med, cell = _rounds({k: v[0] for k, v in arms.items()}, rounds, iters)
            M, pairs = arms["grouped"][1:]
            print(f"{name:22s} {'8 x 128':>9s} {t:3d} {M:7d} grouped {cell['grouped']}   interleaved {cell['interleaved']}   "
                  f"i/g {med['interleaved'] / med['grouped']:.3f}   TF/s grouped {4 * pairs * H * Dh / med['grouped'] / 1e6:.1f}")
            del arms
            torch.cuda.empty_cache()


def step_ab(eng, rounds, n=1024, steps=8):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.sis import DeviceSIS

    cfg = GPT2Config()
    llm = AsyncAmdLM.from_config(cfg, None, device="cuda:0", dtype=torch.float32, seed=1234, engine=eng, batch_size=n)
    V = cfg.vocab_size
    g = torch.Generator(device="cuda").manual_seed(4321)
    valid = torch.where(torch.rand(V, device="cuda", generator=g) < 1 / 3, float("-inf"), 0.0)
    valid[cfg.eos_token_id] = float("-inf")  # (no particle finishes: the population stays whole for all the steps)
    eos1 = torch.full((V,), float("-inf"), device="cuda")
    eos1[cfg.eos_token_id] = 0.0
    llm.register_masks(torch.stack([valid, eos1]))
    print(f"# DeviceSIS, gpt2-small shape fp32 (random init), {n} particles, one prompt, {steps} steps; ms per step, median (min .. max) of "
          f"{rounds} alternating runs after one warm-up run an arm")
    for P in (48, 128, 256):
        prompt = [int(x) for x in np.random.default_rng(P).integers(1000, 30000, P)]
        ms, packed = {"tile": [], "True": []}, {}
        for rd in range(rounds + 1):
            for k, mode in (("tile", "tile"), ("True", True)):
                sis = DeviceSIS(llm, n, prompt, steps + 2, cfg.eos_token_id, seed=1234, share_prompt_rows=mode)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    sis.step()
                torch.cuda.synchronize()
                if rd:
                    ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
                packed[k] = sis.packed_steps
        cells = "   ".join(f"{k!r} {statistics.median(v):8.2f} ({min(v):.2f} .. {max(v):.2f}) [{packed[k]} packed steps]" for k, v in ms.items())
        print(f"  prompt {P:4d}: {cells}   tile / True {statistics.median(ms['tile']) / statistics.median(ms['True']):.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    a = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}")
    eng = HipEngine("cuda:0")
    if not a.no_kernel:
        kernel_ab(eng, a.rounds, a.iters)
    if not a.no_step:
        step_ab(eng, a.step_rounds)
