"""Host trace of the backend's evaluation paths on the CPU: which engine methods, which transformer-body calls and which
host read-backs a fixed, seeded scenario issues, in order.  Two commits whose traces are byte-identical launch the same
work from the host and read the same things back at the same places (what a host-side refactor must keep).

    python tools/host_trace.py > trace.txt

CPU only: the HIP engine is replaced by the test doubles under tests/ (CpuOracleEngine with the chunk and LoRA-rows
methods), the model is the 2-layer GPT-2 the CPU LoRA tests build.  Logged, one line each:

    eng  <method>(<arguments>)      every public engine method; tensors as dtype[shape], Python scalars by value
    body input_ids=[U, L] kw=[...] use_cache=<bool>
                                    every call of the transformer body; kw: the keyword arguments that carry a value (an
                                    argument handed over as None is the call that leaves it out)
    d2h  <cpu|item|tolist> dtype[shape]
                                    every Tensor.cpu / .item / .tolist, whoever calls it
"""
import asyncio
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = []


def log(line):
    OUT.append(line)


def _desc(x):
    if isinstance(x, torch.Tensor):
        return f"{str(x.dtype).replace('torch.', '')}{list(x.shape)}"
    if isinstance(x, np.ndarray):
        return f"np.{x.dtype}{list(x.shape)}"
    if isinstance(x, (list, tuple)):
        return "[" + ", ".join(_desc(e) for e in x) + "]"
    if isinstance(x, dict):
        return "{" + ", ".join(f"{k}: {_desc(v)}" for k, v in x.items()) + "}"
    if x is None or isinstance(x, (bool, int, float, str, np.integer, np.floating)):
        return repr(x if not isinstance(x, (np.integer, np.floating)) else x.item())
    if isinstance(x, torch.dtype):
        return str(x).replace("torch.", "")
    return f"<{type(x).__name__}>"


def trace_engine(engine):
    """Every public method of `engine` logs its call (methods it calls on itself included)."""
    for name in dir(engine):
        fn = getattr(engine, name)
        if name.startswith("_") or not callable(fn):
            continue

        def wrapped(*a, _fn=fn, _name=name, **k):
            args = [_desc(v) for v in a] + [f"{key}={_desc(v)}" for key, v in k.items()]
            log(f"eng  {_name}({', '.join(args)})")
            return _fn(*a, **k)

        setattr(engine, name, wrapped)
    return engine


def _body_hook(_mod, args, kwargs):
    kw = sorted(k for k, v in kwargs.items() if v is not None and k not in ("input_ids", "use_cache"))
    log(f"body input_ids={list(kwargs['input_ids'].shape)} kw={kw} use_cache={bool(kwargs.get('use_cache'))}")


def trace_body(llm):
    body = llm._net.base_model
    if _body_hook not in body._forward_pre_hooks.values():  # (shadows of one model share its hook tables)
        body.register_forward_pre_hook(_body_hook, with_kwargs=True)


def trace_readbacks():
    for name in ("cpu", "item", "tolist"):
        orig = getattr(torch.Tensor, name)

        def wrapped(self, *a, _orig=orig, _name=name, **k):
            log(f"d2h  {_name} {_desc(self)}")
            return _orig(self, *a, **k)

        setattr(torch.Tensor, name, wrapped)


def make_engine():
    from tests.kv_chunk_engine import ChunkCpuEngine
    from tests.lora_rows_engine import LoraRowsOracleEngine

    class TraceEngine(ChunkCpuEngine, LoraRowsOracleEngine):
        pass

    return trace_engine(TraceEngine())


def make_llm(model, masks, **kw):
    from genlm_backend_amd.llm import AsyncAmdLM
    from tests.test_lora_cpu import Tok

    llm = AsyncAmdLM(model, None, batch_size=64, timeout=0.02, engine=make_engine(), **kw)
    llm.tokenizer = Tok()
    llm.register_masks(masks)
    llm.set_rng("philox", 7)
    trace_body(llm)
    return llm


CTXS = [[3, 1, 4, 1, 5], [9, 2, 6, 5, 3, 5], [8, 9], [7], [3, 1, 4, 1, 5], [3, 1, 4, 1, 5, 9, 2]]
PRE = [3, 1, 4]


def scenario():
    from genlm_backend_amd.sis import DeviceSIS
    from tests.test_lora_cpu import GPT2_TARGETS, V, _gpt2, write_adapter

    model = _gpt2()
    rs = np.random.default_rng(3)
    masks = np.where(rs.random((2, V)) < 0.5, 0.0, -np.inf).astype(np.float32)
    masks[1, 1:] = -np.inf
    masks[:, 0] = 0.0
    masks = torch.from_numpy(masks)
    mids = [i % 2 for i in range(len(CTXS))]

    async def many(fn, items):
        return await asyncio.gather(*[fn(*it) for it in items])

    log("== queued next_token_logprobs")
    llm = make_llm(model, masks)
    asyncio.run(many(llm.next_token_logprobs, [(c,) for c in CTXS]))
    log("== queued next_token_logprobs behind a cache_kv prefix")
    llm.clear_cache()
    llm.cache_kv(PRE)
    asyncio.run(many(llm.next_token_logprobs, [(c,) for c in CTXS]))
    log("== queued next_token_step behind a cache_kv prefix")
    asyncio.run(many(llm.next_token_step, list(zip(CTXS, mids))))
    log("== queued next_token_step")
    llm.clear_cache()
    asyncio.run(many(llm.next_token_step, list(zip(CTXS, mids))))
    log("== batch_next_token_step_sync")
    llm.batch_next_token_step_sync(CTXS, mids)
    llm.batch_next_token_step_sync(CTXS)
    log("== batch_next_token_step_sync with cached prefixes")
    llm.cache_kv(PRE)
    llm.cache_kv([9, 2])
    llm.batch_next_token_step_sync(CTXS, mids)
    log("== batch_next_token_logprobs_sync")
    llm.clear_cache()
    llm.batch_next_token_logprobs_sync(CTXS)
    llm.batch_next_token_logprobs_sync([c + [5] for c in CTXS] + [[11, 12]])

    for chunk in (1, 4):
        log(f"== batch_next_token_step_sync with auto_kv_rows, auto_kv_chunk={chunk}")
        llm = make_llm(model, masks, auto_kv_rows=8, auto_kv_cap=24, auto_kv_chunk=chunk)
        ctxs = [list(c) for c in CTXS]
        for step in range(4):
            llm.batch_next_token_step_sync(ctxs, mids)
            grow = 1 if step % 2 == 0 else 3  # (three new tokens: a chunk forward with auto_kv_chunk=4, re-encoded without)
            ctxs = [c + [(5 * i + step + j) % V for j in range(grow)] for i, c in enumerate(ctxs)]
        log("== batch_next_token_logprobs_sync with auto_kv_rows: every position of the contexts (re-encoded)")
        llm.batch_next_token_logprobs_sync(ctxs)
        # (the shorter prefixes are in the trie now: a context one token longer wants the row after its last token only)
        log("== the same contexts grown by one token, batched")
        llm.batch_next_token_logprobs_sync([c + [7] for c in ctxs])
        log("== grown by one more token, queued: the auto-KV last-row path (match_rows / match_prefix_rows, no log-prob of an earlier position)")
        asyncio.run(many(llm.next_token_logprobs, [(c + [7, 8],) for c in ctxs]))

    log("== lora_names")
    with tempfile.TemporaryDirectory() as tmp:
        write_adapter(os.path.join(tmp, "a"), model, GPT2_TARGETS, fan_in_fan_out=True, seed=1, rank_pattern={"c_fc": 6})
        write_adapter(os.path.join(tmp, "b"), model, GPT2_TARGETS[1:6], r=3, alpha=9.0, fan_in_fan_out=True, seed=7, rslora=True)
        llm = make_llm(model, masks)
        llm.add_new_lora(os.path.join(tmp, "a"), "a")
        llm.add_new_lora(os.path.join(tmp, "b"), "b")
        names = [None, "a", "b", "a", None, "b"]
        llm.batch_next_token_step_sync(CTXS, mids, lora_names=names)
        llm.batch_next_token_logprobs_sync(CTXS, lora_names=names)

    prompts = [[3, 1, 4, 1]] * 5 + [[9, 2, 6, 5]] * 3
    modes = {"no KV": {}, "prefix KV": dict(use_prefix_kv=True),
             "private KV rows": dict(use_particle_kv=True, share_kv=False),
             "shared KV rows": dict(use_particle_kv=True, share_kv=True)}
    for name, kw in modes.items():
        log(f"== DeviceSIS, {name}")
        llm = make_llm(model, masks)
        sis = DeviceSIS(llm, len(prompts), prompts, max_tokens=6, eos_id=0, seed=5, **kw)
        for _ in range(3):
            sis.step()

    N = len(prompts)
    log("== DeviceSIS with particle_masks: first seen (raw), seen again (prepared), one row updated (that row prepared again)")
    llm = make_llm(model, masks)
    bits = llm.engine.mask_to_bits(masks)[0]
    sis = DeviceSIS(llm, N, prompts, max_tokens=6, eos_id=0, seed=5, particle_masks=torch.cat([bits[:1].expand(N, -1), bits[1:2]]).contiguous())
    sis.step()
    sis.step()
    sis.update_particle_masks(torch.tensor([1], dtype=torch.int32), bits[1:2])
    sis.step()
    log("== DeviceSIS with registered float masks")
    soft = masks.clone()
    soft[0, 0] = -0.5  # (a finite weight: the table stays float)
    llm = make_llm(model, soft)
    sis = DeviceSIS(llm, N, prompts, max_tokens=6, eos_id=0, seed=5)
    for _ in range(3):
        sis.step()
    log("== batch_next_token_step_sync: mask ids per logits row, per context (contexts 0 and 4 are equal, their ids are not), parity draws")
    llm = make_llm(model, masks)
    llm.batch_next_token_step_sync(CTXS, [0, 1, 0, 1, 0, 1])
    llm.batch_next_token_step_sync(CTXS, [0, 1, 0, 1, 1, 1])
    llm.set_rng("torch", 3)
    llm.batch_next_token_step_sync(CTXS, [0, 1, 0, 1, 1, 1])


if __name__ == "__main__":
    torch.manual_seed(0)
    trace_readbacks()
    with torch.no_grad():
        scenario()
    sys.stdout.write("\n".join(OUT) + "\n")
