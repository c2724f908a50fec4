"""LoRA merge and SIS steps under an adapter, one JSON line per case.

    python tools/lora_bench.py [--reps 20] [--only merge|sis]

merge cases: glb_lora_merge of a whole adapter in one call (HipEngine.lora_merge) - device time by HIP events over `reps`
calls after two warm-up calls - against torch's `(W.float() + s * (B.float() @ A.float())).to(W.dtype)` per matrix in the
same process; `frac_8TBs` = the merge's bytes (W read, out written, A and B read) / time / 8 TB/s.
  gpt2-fp32-r16       GPT-2 small, the four Conv1D shapes of its 12 layers, fp32, r = 16
  llama1b-bf16-r16/64 Llama-3.2-1B shape, all seven projections of its 16 layers, bf16, r = 16 and 64
  llama8b-bf16-r16    Llama-3-8B shape, all seven projections of its 32 layers, bf16, r = 16 (made on the device)
sis cases: bench.py's sis / sis-llama step (SisBenchWorkload: 1024 x GPT-2 small fp32 / 512 x Llama-3.2-1B bf16, 10-token
loops) without and with an active adapter on every projection (r = 16), alternating, wall time per step.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import genlm_backend_amd  # noqa: E402,F401
from genlm_backend_amd.engine import HipEngine  # noqa: E402

DEV = "cuda:0"
HBM = 8e12


def _shapes(name):
    """(n_out, k_in, transposed) of one layer's targeted matrices, and the number of layers."""
    if name == "gpt2":
        return [(2304, 768, True), (768, 768, True), (3072, 768, True), (768, 3072, True)], 12
    if name == "llama1b":
        d, f, kv = 2048, 8192, 512
        return [(d, d, False), (kv, d, False), (kv, d, False), (d, d, False), (f, d, False), (f, d, False), (d, f, False)], 16
    d, f, kv = 4096, 14336, 1024
    return [(d, d, False), (kv, d, False), (kv, d, False), (d, d, False), (f, d, False), (f, d, False), (d, f, False)], 32


def _time(fn, reps):
    for _ in range(2):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us


def merge_case(eng, name, dtype, r, reps):
    shapes, layers = _shapes(name)
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    jobs, nbytes = [], 0
    es = torch.tensor([], dtype=dtype).element_size()
    for _ in range(layers):
        for n_out, k_in, tr in shapes:
            wshape = (k_in, n_out) if tr else (n_out, k_in)
            w = (torch.randn(wshape, device=DEV, generator=g, dtype=torch.float32) * 0.02).to(dtype)
            a = (torch.randn((r, k_in), device=DEV, generator=g, dtype=torch.float32) * 0.02).to(dtype)
            b = (torch.randn((n_out, r), device=DEV, generator=g, dtype=torch.float32) * 0.02).to(dtype)
            jobs.append(dict(w=w, a=a, b=b, scale=2.0, transposed=tr, out=torch.empty_like(w)))
            nbytes += 2 * w.numel() * es + (a.numel() + b.numel()) * es
    t_glb = _time(lambda: eng.lora_merge(jobs), reps)

    def torch_merge():
        for j in jobs:
            d = j["b"].float() @ j["a"].float()
            j["out"].copy_((j["w"].float() + j["scale"] * (d.T if j["transposed"] else d)).to(dtype))

    t_torch = _time(torch_merge, max(2, reps // 4))
    out = dict(case=f"{name}-{'fp32' if dtype == torch.float32 else 'bf16'}-r{r}", matrices=len(jobs),
               merge_us=round(t_glb, 1), bytes=nbytes, frac_8TBs=round(nbytes / (t_glb * 1e-6) / HBM, 3),
               torch_us=round(t_torch, 1), speedup_vs_torch=round(t_torch / t_glb, 2))
    del jobs
    torch.cuda.empty_cache()
    return out


def _write_adapter(d, model, r):
    from safetensors.torch import save_file

    tensors, targets = {}, []
    g = torch.Generator().manual_seed(1)
    for name, mod in model.named_modules():
        kind = type(mod).__name__
        if kind == "Conv1D" or (kind == "Linear" and "lm_head" not in name):
            k_in, n_out = (mod.weight.shape[0], mod.weight.shape[1]) if kind == "Conv1D" else (mod.weight.shape[1],
                                                                                               mod.weight.shape[0])
            tensors[f"base_model.model.{name}.lora_A.weight"] = (torch.randn(r, k_in, generator=g) * 0.01).to(mod.weight.dtype)
            tensors[f"base_model.model.{name}.lora_B.weight"] = (torch.randn(n_out, r, generator=g) * 0.01).to(mod.weight.dtype)
            targets.append(name.split(".")[-1])
    save_file(tensors, os.path.join(d, "adapter_model.safetensors"))
    with open(os.path.join(d, "adapter_config.json"), "w") as f:
        json.dump(dict(peft_type="LORA", r=r, lora_alpha=2 * r, target_modules=sorted(set(targets)), bias="none"), f)
    return len(tensors) // 2


def sis_case(eng, model, n_particles, rounds=3, steps=10):
    from genlm_backend_amd.sis import DeviceSIS, SisBenchWorkload

    wl = SisBenchWorkload(eng, torch.device(DEV), 0, 1, None, n_particles=n_particles, model=model)
    llm = wl.llm
    with tempfile.TemporaryDirectory() as d:
        n_mod = _write_adapter(d, llm.model, 16)
        llm.add_new_lora(d, "bench")
    prompt, eos = wl.sis._ctx0[0, :8].tolist(), wl.sis.eos_id

    def loop():
        sis = DeviceSIS(llm, n_particles, prompt, wl.max_tokens, eos, seed=1234)
        sis.step()  # (untimed: a fresh population's first step)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps - 1):
            sis.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (steps - 1)

    t0 = time.perf_counter()
    llm.set_lora(lora_name="bench")
    torch.cuda.synchronize()
    set_ms = (time.perf_counter() - t0) * 1e3
    loop()
    llm.clear_lora()
    loop()
    times = {"base": [], "lora": []}
    for _ in range(rounds):
        llm.clear_lora()
        times["base"].append(loop())
        llm.set_lora(lora_name="bench")
        times["lora"].append(loop())
    return dict(case=f"sis-{model}", particles=n_particles, adapter_modules=n_mod, rank=16,
                step_ms_base=[round(t, 3) for t in times["base"]], step_ms_lora=[round(t, 3) for t in times["lora"]],
                ratio=round(float(np.mean(times["lora"]) / np.mean(times["base"])), 3), set_lora_ms=round(set_ms, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("merge", "sis"), default=None)
    args = ap.parse_args()
    eng = HipEngine(DEV)
    if args.only in (None, "merge"):
        for name, dtype, r in (("gpt2", torch.float32, 16), ("llama1b", torch.bfloat16, 16), ("llama1b", torch.bfloat16, 64),
                               ("llama8b", torch.bfloat16, 16)):
            print(json.dumps(merge_case(eng, name, dtype, r, args.reps)), flush=True)
    if args.only in (None, "sis"):
        print(json.dumps(sis_case(eng, "gpt2", 1024)), flush=True)
        print(json.dumps(sis_case(eng, "llama-3.2-1b", 512)), flush=True)


if __name__ == "__main__":
    main()
