"""A/B of auto_kv_chunk, in one process, the arms alternating round by round (median of the rounds).

Step cost: every context grows by `--grow` (4) tokens per call from a 16-token prompt - GPT-2 small float32 with 1024
contexts, the Llama-3.2-1B shape bfloat16 with 512 (random weights: the cost does not depend on them) - through
  (a) auto_kv_chunk=1: the rows find no context's first L - 1 tokens, every call re-encodes (the parent's behaviour),
  (b) auto_kv_chunk=8: every context is fed its four new tokens over its row,
  (c) no rows.
ms per call (wall clock around `batch_next_token_step_sync`, which ends in a D2H copy) and the rows of each kind.

Kernel: glb_slab_attention_chunk against SDPA with the explicit mask on the gathered slabs, T in {2, 4, 8, 16}, the two
models' head shapes, 1024 rows of 64 positions holding 24 + T tokens afterwards; a ring of slab sets larger than the 256 MB
Infinity Cache, so the K / V come from HBM; the fraction of 8 TB/s is on the bytes the kernel must move (the prefix's K / V
once per KV head, the new K / V read and written, q and the output).

    python tools/kv_chunk_ab.py [--rounds 5] [--calls 4] [--no-step] [--no-kernel]
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

PEAK = 8e12
RING_BYTES = 320 << 20


class Tok:
    pad_token_id = None
    eos_token_id = 0


def models():
    from transformers import GPT2Config, GPT2LMHeadModel, LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    yield "gpt2-small fp32", 1024, GPT2LMHeadModel(GPT2Config()).eval().cuda()
    cfg = LlamaConfig(vocab_size=128256, hidden_size=2048, intermediate_size=8192, num_hidden_layers=16, num_attention_heads=32,
                      num_key_value_heads=8, head_dim=64, max_position_embeddings=2048, tie_word_embeddings=True)
    yield "llama-3.2-1B shape bf16", 512, LlamaForCausalLM(cfg).eval().to(torch.bfloat16).cuda()


def step_ab(rounds, calls, grow):
    for name, n, model in models():
        V = model.config.vocab_size
        cap = 16 + grow * (calls + 1) + 8
        arms = {"chunk=1": dict(auto_kv_rows=n + n // 4, auto_kv_cap=cap), "chunk=8": dict(auto_kv_rows=n + n // 4, auto_kv_cap=cap, auto_kv_chunk=8),
                "no rows": {}}
        ms = {k: [] for k in arms}
        kinds = {}
        llms = {}
        for k, kw in arms.items():
            llms[k] = AsyncAmdLM(model, None, batch_size=n, **kw)
            llms[k].tokenizer = Tok()
        rnd = np.random.default_rng(0)
        for rd in range(rounds + 1):  # (round 0 warms every arm up: allocator, library set-up)
            seqs = [rnd.integers(1, V, 16 + grow * (calls + 1)).tolist() for _ in range(n)]
            for k, m in llms.items():
                m.clear_cache()
                m.set_rng("philox", rd)
                m.batch_next_token_step_sync([s[:16] for s in seqs], [0] * n)  # the prompts
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for c in range(1, calls + 1):
                    m.batch_next_token_step_sync([s[:16 + grow * c] for s in seqs], [0] * n)
                torch.cuda.synchronize()
                if rd:
                    ms[k].append((time.perf_counter() - t0) * 1e3 / calls)
                if m._auto_kv is not None:
                    kinds[k] = dict(m._auto_kv.stats)
        print(f"## {name}, {n} contexts, +{grow} tokens per call, {rounds} rounds x {calls} calls (median, min .. max ms per call)")
        for k in arms:
            st = kinds.get(k, {})
            print(f"  {k:8s} {statistics.median(ms[k]):8.2f} ms  ({min(ms[k]):.2f} .. {max(ms[k]):.2f})   "
                  + " ".join(f"{q}={st[q]}" for q in ("one_token_rows", "chunk_rows", "chunk_tokens", "encoded_rows", "copied_rows") if q in st))
        for m in llms.values():
            m.close()
        del llms, model
        torch.cuda.empty_cache()


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def kernel_ab(eng, rounds, iters):
    n, cap, keep = 1024, 64, 24
    g = torch.Generator(device="cuda").manual_seed(0)
    print(f"# glb_slab_attention_chunk vs SDPA + explicit mask; {n} rows, cap {cap}, {keep} cached positions; median us of "
          f"{rounds} rounds x {iters} calls")
    print(f"{'shape':22s} {'T':>3s} {'kernel':>9s} {'sdpa':>9s} {'k/s':>6s} {'of 8TB/s':>9s}")
    for name, H, Hkv, Dh, dtype in (("gpt2 12/12 x64 fp32", 12, 12, 64, torch.float32), ("1B 32/8 x64 bf16", 32, 8, 64, torch.bfloat16)):
        es = 4 if dtype == torch.float32 else 2
        per = 2 * n * Hkv * cap * Dh * es
        n_buf = max(2, -(-RING_BYTES // per))
        slabs = [(torch.randn((n, Hkv, cap, Dh), device="cuda", generator=g).to(dtype), torch.randn((n, Hkv, cap, Dh), device="cuda", generator=g).to(dtype))
                 for _ in range(n_buf)]
        pos = torch.full((n,), keep, dtype=torch.int32, device="cuda")
        for T in (2, 4, 8, 16):
            nn = torch.full((n,), T, dtype=torch.int32, device="cuda")
            proj = torch.randn((n, T, (H + 2 * Hkv) * Dh), device="cuda", generator=g).to(dtype)
            q = proj[..., :H * Dh].view(n, T, H, Dh).transpose(1, 2)
            kn = proj[..., H * Dh:(H + Hkv) * Dh].view(n, T, Hkv, Dh).transpose(1, 2)
            vn = proj[..., (H + Hkv) * Dh:].view(n, T, Hkv, Dh).transpose(1, 2)
            ar = torch.arange(cap, device="cuda")
            mask = (ar[None, None, None, :] <= (keep + torch.arange(T, device="cuda"))[None, None, :, None]).expand(n, 1, T, cap)
            state = {"i": 0}

            def native():
                state["i"] = (state["i"] + 1) % n_buf
                ks, vs = slabs[state["i"]]
                eng.slab_attention_chunk(q, kn, vn, ks, vs, pos, nn, Dh ** -0.5)

            def sdpa():  # what the fall-through does per layer: append the new K / V, dense attention under the mask
                state["i"] = (state["i"] + 1) % n_buf
                ks, vs = slabs[state["i"]]
                ks[:, :, keep:keep + T] = kn
                vs[:, :, keep:keep + T] = vn
                torch.nn.functional.scaled_dot_product_attention(q, ks, vs, attn_mask=mask, enable_gqa=H != Hkv)

            ta, tb = [], []
            native(), sdpa()
            for _ in range(rounds):
                ta.append(_time(native, iters))
                tb.append(_time(sdpa, iters))
            a, b = statistics.median(ta), statistics.median(tb)
            moved = n * (2 * Hkv * keep * Dh + 2 * 2 * Hkv * T * Dh + 2 * H * T * Dh) * es
            print(f"{name:22s} {T:3d} {a:9.1f} {b:9.1f} {a / b:6.2f} {moved / (a * 1e-6) / PEAK:9.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--grow", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    a = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}")
    if not a.no_kernel:
        kernel_ab(HipEngine("cuda:0"), a.rounds, a.iters)
    if not a.no_step:
        step_ab(a.rounds, a.calls, a.grow)
