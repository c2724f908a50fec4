"""A/B of glb_lora_rows, in one process, the arms alternating round by round (median of the rounds), HIP
events around `iters` calls:
  (a) HipEngine.lora_rows: two launches, in place on Y
  (b) the PyTorch composition: per adapter index_select of its rows, two F.linear, index_add_ into Y
over the projection shapes of GPT-2 small (float32) and Llama-3.2-1B (bfloat16), M = 512, 1024, 9216, r = 16 and 64, with
1, 2 and 4 adapters in the batch (every row has an adapter, dealt in blocks).  Every call takes the next of a ring of X / Y
buffers that together exceed the 256 MB Infinity Cache, so they come from HBM; the fraction of 8 TB/s is on the call's
algorithmic bytes (X once, Y twice).  Then the step cost (`--steps`): one `batch_next_token_step_sync` over a population
without `lora_names`, with `lora_names` half base / half one adapter, and the two switched passes that give the same numbers
through merging (set_lora, step, clear_lora, step), three alternating runs each.

    python tools/lora_rows_ab.py [--rounds 5] [--iters 10] [--no-kernel] [--steps]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genlm_backend_amd  # noqa: E402,F401
from genlm_backend_amd.engine import HipEngine  # noqa: E402

SHAPES = [("gpt2 c_attn", 2304, 768, torch.float32), ("gpt2 c_proj", 768, 768, torch.float32),
          ("gpt2 c_fc", 3072, 768, torch.float32), ("gpt2 mlp.c_proj", 768, 3072, torch.float32),
          ("1B q/o", 2048, 2048, torch.bfloat16), ("1B k/v", 512, 2048, torch.bfloat16),
          ("1B gate/up", 8192, 2048, torch.bfloat16), ("1B down", 2048, 8192, torch.bfloat16)]
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


def kernel_ab(eng, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(0)
    print(f"# {torch.cuda.get_device_name(0)}; rounds {rounds} x {iters} calls, median us per call; X / Y rings of "
          f"{RING_BYTES >> 20} MB")
    print(f"{'shape':16s} {'N':>5s} {'K':>5s} {'M':>5s} {'r':>3s} {'ad':>2s} {'(a) kernel':>10s} {'(b) torch':>10s} {'a/b':>6s} "
          f"{'(a) of 8TB/s':>12s}")
    for name, n, k, dtype in SHAPES:
        es = 4 if dtype == torch.float32 else 2
        for m in (512, 1024, 9216):
            per = m * (k + n) * es
            n_buf = max(2, min(64, -(-RING_BYTES // per)))
            xs = [torch.randn(m, k, device="cuda", generator=g).to(dtype) for _ in range(n_buf)]
            ys = [torch.randn(m, n, device="cuda", generator=g).to(dtype) for _ in range(n_buf)]
            for r in (16, 64):
                ads = [((torch.randn(r, k, device="cuda", generator=g) * 0.02).to(dtype),
                        (torch.randn(n, r, device="cuda", generator=g) * 0.02).to(dtype)) for _ in range(4)]
                table = eng.lora_rows_table([[dict(a=a, b=b, scale=2.0)] for a, b in ads])
                for n_ad in (1, 2, 4):
                    slots = (torch.arange(m, device="cuda") * n_ad // m).to(torch.int32)
                    rows = [(slots == s).nonzero().flatten() for s in range(n_ad)]
                    state = {"i": 0}

                    def native():
                        state["i"] = (state["i"] + 1) % n_buf
                        eng.lora_rows(xs[state["i"]], ys[state["i"]], slots, table, 0)

                    def composed():
                        state["i"] = (state["i"] + 1) % n_buf
                        x, y = xs[state["i"]], ys[state["i"]]
                        for s in range(n_ad):
                            a, b = ads[s]
                            d = F.linear(F.linear(x.index_select(0, rows[s]), a), b)
                            y.index_add_(0, rows[s], d, alpha=2.0)

                    native(), composed()
                    torch.cuda.synchronize()
                    ta, tb = [], []
                    for _ in range(rounds):
                        ta.append(_time(native, iters))
                        tb.append(_time(composed, iters))
                    ma, mb = statistics.median(ta), statistics.median(tb)
                    moved = m * (k + 2 * n) * es
                    print(f"{name:16s} {n:5d} {k:5d} {m:5d} {r:3d} {n_ad:2d} {ma:10.1f} {mb:10.1f} {ma / mb:6.2f} "
                          f"{moved / (ma * 1e-6) / PEAK:12.3f}", flush=True)
            del xs, ys
            torch.cuda.empty_cache()


def _write_adapter(d, model, targets, r, dtype, seed):
    """A peft-format LoRA adapter of rank r and scale 2 on `targets`, in directory d (loaded through add_new_lora, so the
    tool measures the shipped path)."""
    from safetensors.torch import save_file

    g = torch.Generator().manual_seed(seed)
    tensors = {}
    for p in targets:
        mod = model.get_submodule(p)
        conv = type(mod).__name__ == "Conv1D"
        k_in, n_out = (mod.weight.shape[0], mod.weight.shape[1]) if conv else (mod.weight.shape[1], mod.weight.shape[0])
        tensors[f"base_model.model.{p}.lora_A.weight"] = (torch.randn(r, k_in, generator=g) * 0.02).to(dtype)
        tensors[f"base_model.model.{p}.lora_B.weight"] = (torch.randn(n_out, r, generator=g) * 0.02).to(dtype)
    save_file(tensors, os.path.join(d, "adapter_model.safetensors"))
    cfg = dict(peft_type="LORA", r=r, lora_alpha=2.0 * r, target_modules=sorted({p.split(".")[-1] for p in targets}),
               fan_in_fan_out=type(model.get_submodule(targets[0])).__name__ == "Conv1D", use_rslora=False, rank_pattern={},
               alpha_pattern={}, lora_dropout=0.0, bias="none", modules_to_save=None, use_dora=False)
    with open(os.path.join(d, "adapter_config.json"), "w") as f:
        json.dump(cfg, f)


def step_cost(eng):
    from transformers import GPT2Config, LlamaConfig

    from genlm_backend_amd.llm import AsyncAmdLM

    cases = [
        ("GPT-2 small fp32, 1024 contexts", GPT2Config(), torch.float32, 1024,
         lambda L: [f"transformer.h.{i}.{m}" for i in range(L) for m in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")],
         12),
        ("Llama-3.2-1B shape bf16, 512 contexts",
         LlamaConfig(vocab_size=128256, hidden_size=2048, intermediate_size=8192, num_hidden_layers=16, num_attention_heads=32,
                     num_key_value_heads=8, head_dim=64, max_position_embeddings=2048, tie_word_embeddings=True),
         torch.bfloat16, 512,
         lambda L: [f"model.layers.{i}.{m}" for i in range(L) for m in (
             "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
             "mlp.down_proj")], 16),
    ]
    for title, cfg, dtype, n, targets, layers in cases:
        llm = AsyncAmdLM.from_config(cfg, None, device="cuda:0", dtype=dtype, seed=0, engine=eng)
        with tempfile.TemporaryDirectory() as d:
            _write_adapter(d, llm.model, targets(layers), 16, dtype, 1)
            llm.add_new_lora(d, "a")
        rs = np.random.default_rng(0)
        vocab = cfg.vocab_size
        ctxs = [[int(t) for t in rs.integers(3, vocab, 32)] for _ in range(n)]
        names = [None] * (n // 2) + ["a"] * (n - n // 2)

        def plain():
            llm.batch_next_token_step_sync(ctxs)

        def mixed():
            llm.batch_next_token_step_sync(ctxs, lora_names=names)

        def switched():
            llm.set_lora(lora_name="a")
            llm.batch_next_token_step_sync(ctxs)
            llm.clear_lora()
            llm.batch_next_token_step_sync(ctxs)

        arms = (("no lora_names", plain), ("lora_names half / half", mixed), ("set_lora, step, clear_lora, step", switched))
        for _, fn in arms:
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k, _ in arms}
        for _ in range(3):
            for k, fn in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"# {title}, 32 tokens each, r = 16 on every projection: " + "; ".join(
            f"{k} {med[k]:.1f} ms {[round(t, 1) for t in times[k]]}" for k, _ in arms))
        print(f"#   mixed / plain = {med[arms[1][0]] / med[arms[0][0]]:.2f}, mixed / switched = "
              f"{med[arms[1][0]] / med[arms[2][0]]:.2f}", flush=True)
        del llm
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--steps", action="store_true")
    args = ap.parse_args()
    eng = HipEngine("cuda:0")
    if not args.no_kernel:
        kernel_ab(eng, args.rounds, args.iters)
    if args.steps:
        step_cost(eng)


if __name__ == "__main__":
    main()
