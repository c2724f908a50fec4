"""A/B of KV rows in e4m3, in one process, the arms alternating round by round; median (min .. max) of the rounds.

Kernel: glb_slab_attention_fp8 against glb_slab_attention at 64, 256 and 1024 held positions - 1024 rows of GPT-2 heads in
float32, 512 rows of 32/8 x 64 and 32/8 x 128 bfloat16 heads; rings of slab sets larger than the 256 MB Infinity Cache, so the
rows' K / V come from HBM.

Step: a DeviceSIS step (use_particle_kv, share_kv=False, the forward replayed from its graph) with kv_dtype="fp8_e4m3" and
without at the same prompts - GPT-2 small float32 with 1024 particles, the Llama-3.2-1B shape bfloat16 with 512 (random
weights: the cost does not depend on them) - and the KV bytes of both.  An arm that does not fit in memory is reported as that.

Accuracy: the largest |delta log p| of next-token log-probabilities, e4m3 rows against the model's own, over the steps of a run
of the small synthetic GPT-2 (random weights).

    python tools/kv_fp8_ab.py [--rounds 5] [--iters 10] [--tokens 12] [--no-step] [--no-kernel]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genlm_backend_amd  # noqa: E402,F401
from genlm_backend_amd.engine import HipEngine  # noqa: E402
from genlm_backend_amd.llm import AsyncAmdLM  # noqa: E402
from genlm_backend_amd.sis import DeviceSIS  # noqa: E402

RING_BYTES = 320 << 20
HELD = (64, 256, 1024)


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


def _cell(v):
    return f"{statistics.median(v):8.1f} ({min(v):.1f} .. {max(v):.1f})"


def kernel_ab(eng, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda dtype, *shape: torch.randn(shape, device="cuda", generator=g).to(dtype)
    print(f"# glb_slab_attention_fp8 vs glb_slab_attention; us, median (min .. max) of {rounds} alternating rounds x {iters} calls")
    for name, n, H, Hkv, Dh, dtype in (("gpt2 12/12 x64 fp32", 1024, 12, 12, 64, torch.float32), ("1B 32/8 x64 bf16", 512, 32, 8, 64, torch.bfloat16),
                                       ("8B 32/8 x128 bf16", 512, 32, 8, 128, torch.bfloat16)):
        proj = rnd(dtype, n, 1, (H + 2 * Hkv) * Dh)
        q = proj[..., :H * Dh].view(n, 1, H, Dh).transpose(1, 2)
        kn = proj[..., H * Dh:(H + Hkv) * Dh].view(n, 1, Hkv, Dh).transpose(1, 2)
        vn = proj[..., (H + Hkv) * Dh:].view(n, 1, Hkv, Dh).transpose(1, 2)
        for P in HELD:
            cap = P + 8
            pos = torch.full((n,), P, dtype=torch.int32, device="cuda")
            per = 2 * n * Hkv * cap * Dh
            wide = [(rnd(dtype, n, Hkv, cap, Dh), rnd(dtype, n, Hkv, cap, Dh)) for _ in range(max(2, -(-RING_BYTES // (per * proj.element_size()))))]
            codes = lambda: torch.randint(0, 0x78, (n, Hkv, cap, Dh), device="cuda", generator=g, dtype=torch.uint8).view(torch.float8_e4m3fn)
            scales = lambda: torch.rand((n, Hkv, cap), device="cuda", generator=g) / 100 + 1e-3
            narrow = [(codes(), codes(), scales(), scales()) for _ in range(max(2, -(-RING_BYTES // per)))]
            state = {"i": 0}

            def nxt(r):
                state["i"] += 1
                return r[state["i"] % len(r)]

            arms = {"rows": lambda: eng.slab_attention(q, kn, vn, *nxt(wide), pos, Dh ** -0.5),
                    "fp8": lambda: eng.slab_attention_fp8(q, kn, vn, *nxt(narrow), pos, Dh ** -0.5)}
            us = {k: [] for k in arms}
            for fn in arms.values():
                fn()
            for _ in range(rounds):
                for k, fn in arms.items():
                    us[k].append(_time(fn, iters))
            base = statistics.median(us["rows"])
            print(f"{name:20s} held {P:5d}: " + "  ".join(f"{k} {_cell(v)} x{statistics.median(v) / base:.2f}" for k, v in us.items()))
            del wide, narrow
            torch.cuda.empty_cache()


def models():
    from transformers import GPT2Config, GPT2LMHeadModel, LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    yield "gpt2-small fp32", 1024, GPT2LMHeadModel(GPT2Config(n_positions=2048)).eval().cuda()
    cfg = LlamaConfig(vocab_size=128256, hidden_size=2048, intermediate_size=8192, num_hidden_layers=16, num_attention_heads=32,
                      num_key_value_heads=8, head_dim=64, max_position_embeddings=2048, tie_word_embeddings=True)
    yield "llama-3.2-1B shape bf16", 512, LlamaForCausalLM(cfg).eval().to(torch.bfloat16).cuda()


def step_ab(rounds, tokens):
    for name, n, model in models():
        llm = AsyncAmdLM(model, None, batch_size=n)
        llm.tokenizer = Tok()
        print(f"## {name}, {n} particles, steps 4 .. {tokens} of a run (graph replays); ms per step, median (min .. max) of {rounds} alternating rounds")
        for P in HELD:
            prompt = torch.randint(1, 1000, (P,), generator=torch.Generator().manual_seed(P)).tolist()
            arms, ms = {}, {}
            for label, kvd in (("rows in the model's type", None), ("rows in e4m3", "fp8_e4m3")):
                try:
                    arms[label] = DeviceSIS(llm, n, prompt, tokens, eos_id=-1, seed=0, use_particle_kv=True, share_kv=False, kv_dtype=kvd)
                    arms[label].step()  # (allocates the rows)
                    ms[label] = []
                except torch.cuda.OutOfMemoryError:
                    arms.pop(label, None)
                    torch.cuda.empty_cache()
                    print(f"  prompt {P:5d}: {label}: does not fit in memory")
            for rd in range(rounds + 1):  # (round 0 warms every arm up and captures its graph)
                for label, sis in arms.items():
                    sis.reset()
                    for _ in range(4):
                        sis.step()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(4, tokens):
                        sis.step()
                    torch.cuda.synchronize()
                    if rd:
                        ms[label].append((time.perf_counter() - t0) * 1e3 / (tokens - 4))
            print(f"  prompt {P:5d}: " + "  ".join(f"{k}: {_cell(v)} ms, KV {arms[k].pkv.nbytes() / 2**30:.2f} GiB" for k, v in ms.items()))
            del arms
            torch.cuda.empty_cache()
        llm.close()
        del llm, model
        torch.cuda.empty_cache()


def accuracy(eng):
    from transformers import GPT2Config, GPT2LMHeadModel

    from genlm_backend_amd.kv import SlabForward, SlabKV, encode_ragged, ragged

    torch.manual_seed(3)
    V, n, P, steps = 200, 8, 21, 40
    model = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=96, n_embd=128, n_layer=2, n_head=2)).eval().cuda()
    llm = AsyncAmdLM(model, None, batch_size=64, engine=eng)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(1, V, (P,), generator=g).tolist() for _ in range(n)]
    batch = tuple(torch.from_numpy(a).cuda() for a in ragged(prompts))
    ar = torch.arange(n, dtype=torch.int32, device="cuda")
    layers = encode_ragged(llm, batch, ar, n, P, keep_kv=True).kv_layers()
    fwd = []
    for kvd in ("fp8_e4m3", None):
        pkv = SlabKV(eng, n, P + steps, len(layers), kv_dtype=kvd)
        pkv.fill_rows(layers, ar, batch[2])
        fwd.append(SlabForward(pkv, llm._body, graph=False))
    worst = 0.0
    for t in range(steps):
        ids = torch.randint(1, V, (n, 1), generator=g).cuda()
        pos = torch.full((n,), P + t, dtype=torch.int32, device="cuda")
        lp = [torch.log_softmax(llm._lm_head(f(ids, pos)).float(), -1) for f in fwd]
        worst = max(worst, (lp[0] - lp[1]).abs().max().item())
    print(f"# synthetic GPT-2 (2 layers, 2 heads x 64, float32, random weights), {n} rows, {steps} tokens behind {P}: max |delta log p| = {worst:.3e}")
    llm.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tokens", type=int, default=12)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    a = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}")
    eng = HipEngine("cuda:0")
    accuracy(eng)
    if not a.no_kernel:
        kernel_ab(eng, a.rounds, a.iters)
    if not a.no_step:
        step_ab(a.rounds, a.tokens)
