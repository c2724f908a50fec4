"""4-bit weights end to end: `batch_sample_sync` of 1, 8 and 64 sequences and a 1024-particle DeviceSIS run with per-particle
KV, on a random-init model of Llama-3.2-1B's (and, with --shapes 1b,8b, Llama-3-8B's) shape, quantised against unquantised in
one process; device memory of both.  One JSON line per case.

    python tools/quant_bench.py [--shapes 1b] [--tokens 16] [--particles 1024] [--out profiles/r09/quant_bench.jsonl]
"""
import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genlm_backend_amd  # noqa: E402,F401
from genlm_backend_amd.llm import AsyncAmdLM  # noqa: E402

SHAPES = {
    "1b": dict(vocab_size=128256, hidden_size=2048, intermediate_size=8192, num_hidden_layers=16, num_attention_heads=32,
               num_key_value_heads=8, head_dim=64, max_position_embeddings=2048, tie_word_embeddings=True),
    "8b": dict(vocab_size=128256, hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32,
               num_key_value_heads=8, head_dim=128, max_position_embeddings=2048, tie_word_embeddings=False),
}


def _timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    from transformers import LlamaConfig

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1b")
    ap.add_argument("--tokens", type=int, default=16)
    ap.add_argument("--particles", type=int, default=1024)
    ap.add_argument("--quant-type", default="nf4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for shape in args.shapes.split(","):
        cfg = LlamaConfig(bos_token_id=1, eos_token_id=2, **SHAPES[shape])
        for quantised in (False, True):
            gc.collect()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            opts = {"load_in_4bit": True, "bnb_4bit_quant_type": args.quant_type} if quantised else None
            t0 = time.perf_counter()
            llm = AsyncAmdLM.from_config(cfg, None, dtype=torch.bfloat16, seed=0, bitsandbytes_opts=opts)
            torch.cuda.synchronize()
            common = dict(shape=shape, quantised=quantised, quant_type=args.quant_type if quantised else None,
                          model_bytes=torch.cuda.memory_allocated() - base, build_s=round(time.perf_counter() - t0, 2),
                          device=torch.cuda.get_device_name(0))
            if quantised:
                common.update(w4_bytes=llm.quantization["bytes"], w4_bytes_before=llm.quantization["bytes_before"])
            for nseq in (1, 8, 64):
                prompts = [[5 + i, 6, 7, 8] for i in range(nseq)]
                dt = _timed(lambda: llm.batch_sample_sync(prompts, max_tokens=args.tokens, eos_token_ids=[], seed=1))
                lines.append(dict(common, case="batch_sample", sequences=nseq, tokens=args.tokens,
                                  ms_per_token=round(dt * 1e3 / args.tokens, 3)))
                print(json.dumps(lines[-1]), flush=True)
            from genlm_backend_amd.sis import DeviceSIS

            masks = torch.zeros((2, cfg.vocab_size), dtype=torch.float32, device="cuda")
            masks[1, ::2] = float("-inf")
            llm.register_masks(masks)

            def run():
                sis = DeviceSIS(llm, args.particles, [5, 6, 7, 8], args.tokens, 2, seed=1234, use_particle_kv=True)
                for _ in range(args.tokens):
                    sis.step()

            dt = _timed(run, reps=2)
            lines.append(dict(common, case="device_sis", particles=args.particles, tokens=args.tokens,
                              ms_per_step=round(dt * 1e3 / args.tokens, 3)))
            print(json.dumps(lines[-1]), flush=True)
            del llm
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
