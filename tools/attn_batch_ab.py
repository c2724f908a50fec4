"""A/B of glb_batch_attention_tile / AsyncAmdLM(long_attention=True), in one process, the arms alternating
round by round; median (min .. max).

Kernel: the kernel against what the fall-through runs - scaled_dot_product_attention on the same views - on a padded
batch of 32 rows of L = 128, 512, 2048 tokens (q_len = k_len = L), three head shapes, two masks: causal (null for the kernel,
is_causal without a mask for SDPA: what a batch without padding hands either) and right padding to lengths uniform in
L / 2 .. L (the [32, 1, L, L] bool mask for both).  q / k / v are strided views of one projection tensor, taken from a ring of
such tensors larger than the 256 MB Infinity Cache; HIP events around `--iters` calls.

Step: 64 contexts of 512 tokens (no padding: no mask), then of 256 .. 512 tokens (right padding: the bool mask), through
`batch_next_token_logprobs_sync` and, split in halves into prompt and continuation, through `batch_sequence_logprobs_sync`;
GPT-2 small float32 and the Llama-3.2-1B shape bfloat16 (random weights), flag on against flag off; wall clock around calls
that end in a synchronise.

    python tools/attn_batch_ab.py [--rounds 5] [--iters 10] [--no-step] [--no-kernel]
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
from genlm_backend_amd.llm import AsyncAmdLM  # noqa: E402

RING_BYTES = 320 << 20
SHAPES = (("gpt2 12/12 x64 fp32", 12, 12, 64, torch.float32), ("1B 32/8 x64 bf16", 32, 8, 64, torch.bfloat16),
          ("8B 32/8 x128 bf16", 32, 8, 128, torch.bfloat16))


class Tok:
    pad_token_id = None
    eos_token_id = 0


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def kernel_ab(eng, rounds, iters, n=32):
    g = torch.Generator(device="cuda").manual_seed(0)
    print(f"# glb_batch_attention_tile vs SDPA (causal: is_causal, no mask; padded: the same bool mask); {n} rows, q_len = k_len = L; "
          f"us, median (min .. max) of {rounds} alternating rounds x {iters} calls; TFLOP/s on the visible (query, key) pairs")
    print(f"{'shape':22s} {'L':>5s} {'mask':>7s} {'kernel':>30s} {'sdpa':>30s} {'k/s':>6s} {'TFLOP/s':>8s} {'max |diff|':>10s}")
    for name, H, Hkv, Dh, dtype in SHAPES:
        for L in (128, 512, 2048):
            W = (H + 2 * Hkv) * Dh
            n_buf = max(2, -(-RING_BYTES // (n * L * W * (4 if dtype == torch.float32 else 2))))
            ring = [torch.randn((n, L, W), device="cuda", generator=g).to(dtype) for _ in range(n_buf)]
            lens = torch.randint(L // 2, L + 1, (n,), device="cuda", generator=g)
            ar = torch.arange(L, device="cuda")
            tril = (ar[None, :] <= ar[:, None])[None, None]
            pad = tril & (ar[None, None, None, :] < lens[:, None, None, None]) & (ar[None, None, :, None] < lens[:, None, None, None])
            state = {"i": 0}

            def qkv():
                state["i"] = (state["i"] + 1) % n_buf
                p = ring[state["i"]]
                return (p[..., :H * Dh].view(n, L, H, Dh).transpose(1, 2), p[..., H * Dh:(H + Hkv) * Dh].view(n, L, Hkv, Dh).transpose(1, 2),
                        p[..., (H + Hkv) * Dh:].view(n, L, Hkv, Dh).transpose(1, 2))

            for mname, k_mask, s_mask, pairs in (("causal", None, tril, n * L * (L + 1) // 2),
                                                 ("padded", pad, pad, int(pad.sum().item()))):
                arms = {"kernel": lambda: eng.batch_attention_tile(*qkv(), k_mask, Dh ** -0.5),
                        "sdpa": lambda: torch.nn.functional.scaled_dot_product_attention(
                            *qkv(), attn_mask=None if k_mask is None else s_mask, is_causal=k_mask is None, enable_gqa=H != Hkv)}
                state["i"] = 0
                a = arms["kernel"]().float()
                state["i"] = 0
                b = arms["sdpa"]().transpose(1, 2).float()
                seen = s_mask.expand(n, 1, L, L).any(-1)[:, 0]
                diff = (a - b)[seen].abs().max().item()  # (padding queries: zeros here, SDPA's mean of V or NaN there)
                us = {k: [] for k in arms}
                for _ in range(rounds):
                    for k, fn in arms.items():
                        us[k].append(_time(fn, iters))
                cell = {k: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})" for k, v in us.items()}
                ka, sa = statistics.median(us["kernel"]), statistics.median(us["sdpa"])
                print(f"{name:22s} {L:5d} {mname:>7s} {cell['kernel']:>30s} {cell['sdpa']:>30s} {ka / sa:6.2f} "
                      f"{4 * pairs * H * Dh / (ka * 1e-6) / 1e12:8.1f} {diff:10.2e}")
            del ring
            torch.cuda.empty_cache()


def step_ab(rounds, ragged, n=64, L=512):
    from transformers import GPT2Config, GPT2LMHeadModel, LlamaConfig, LlamaForCausalLM

    def models():
        torch.manual_seed(0)
        yield "gpt2-small fp32", GPT2LMHeadModel(GPT2Config()).eval().cuda()
        cfg = LlamaConfig(vocab_size=128256, hidden_size=2048, intermediate_size=8192, num_hidden_layers=16, num_attention_heads=32,
                          num_key_value_heads=8, head_dim=64, max_position_embeddings=2048, tie_word_embeddings=True)
        yield "llama-3.2-1B shape bf16", LlamaForCausalLM(cfg).eval().to(torch.bfloat16).cuda()

    for name, model in models():
        V = model.config.vocab_size
        llms = {k: AsyncAmdLM(model, None, batch_size=n, long_attention=flag) for k, flag in (("flag off", False), ("flag on", True))}
        for m in llms.values():
            m.tokenizer = Tok()
        rnd = np.random.default_rng(0)
        ms = {(k, w): [] for k in llms for w in ("next", "score")}
        for rd in range(rounds + 1):  # (round 0 warms every arm up)
            seqs = [rnd.integers(1, V, int(rnd.integers(L // 2, L + 1)) if ragged else L).tolist() for _ in range(n)]
            for k, m in llms.items():
                for w, call in (("next", lambda: m.batch_next_token_logprobs_sync(seqs)),
                                ("score", lambda: m.batch_sequence_logprobs_sync([s[:len(s) // 2] for s in seqs], [s[len(s) // 2:] for s in seqs]))):
                    m.clear_cache()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    if rd:
                        ms[k, w].append((time.perf_counter() - t0) * 1e3)
        print(f"## {name}, {n} contexts of {f'{L // 2} .. {L}' if ragged else L} tokens, {rounds} alternating rounds (ms per call: median, min .. max)")
        for w, what in (("next", "batch_next_token_logprobs_sync"), ("score", "batch_sequence_logprobs_sync")):
            cells = "   ".join(f"{k} {statistics.median(ms[k, w]):8.2f} ({min(ms[k, w]):.2f} .. {max(ms[k, w]):.2f})" for k in llms)
            print(f"  {what:32s} {cells}   on/off {statistics.median(ms['flag on', w]) / statistics.median(ms['flag off', w]):.3f}")
        for m in llms.values():
            m.close()
        del llms, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    a = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}")
    if not a.no_kernel:
        kernel_ab(HipEngine("cuda:0"), a.rounds, a.iters)
    if not a.no_step:
        step_ab(a.rounds, ragged=False)
        step_ab(a.rounds, ragged=True)
