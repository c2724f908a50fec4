"""A/B of the evicting mask bank against the claim path of §17, in one process, the arms alternating round by
round (medians), bit banks at V = 50257:
  fits     a `mask_rows` call of 1024 particles in 1024 distinct states, every row present: an evicting bank of 1026 rows
           over a 2048-state ring (touch, the selection's early exit, the fill's exit, ids) against the claim path's unwarmed
           call with nothing new (claim, the fill's exit, commit, ids) over a bank that holds every state
  thrash   64 and 1024 evictions a call (the bank full, the call's states all new) against 64 and 1024 first-time fills of
           the claim path from an empty bank
  --sis    DeviceSIS, 1024 particles, gpt2-small shape, shared KV rows, a counting automaton of 2048 states: a 10-step loop
           over an evicting bank of 1026 rows against the same loop over a bank that holds everything, three alternating runs

    python tools/dfa_evict_ab.py [--rounds 5] [--sis]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genlm_backend_amd  # noqa: E402,F401
from dfa_ab import _event_us, vocabulary  # noqa: E402
from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint  # noqa: E402
from genlm_backend_amd.engine import HipEngine  # noqa: E402

S, N, V = 2048, 1024, 50257


def ring(counting=False):
    """S states, every byte moves to the next, every state accepts; `counting`: the last state has no way on."""
    d = np.repeat(((np.arange(S, dtype=np.int32) + 1) % S)[:, None], 256, axis=1)
    if counting:
        d[-1] = -1
    return ByteDFA(d, np.ones(S, np.bool_), 0)


def pair(eng, dfa, vocab, eos_id=0, skip=()):
    full = DeviceConstraint(eng, dfa, vocab, eos_id=eos_id, skip_ids=skip)
    small = DeviceConstraint(eng, dfa, vocab, eos_id=eos_id, skip_ids=skip, mask_bank_bytes=(N + 2) * ((V + 31) // 32) * 4,
                             on_full="evict")
    assert full.capacity == S + 2 and small.capacity == N + 2 and small._evicting
    return full, small


def kernels(eng, rounds):
    med = statistics.median
    vocab = vocabulary(V)
    full, small = pair(eng, ring(), vocab)
    dev = eng.device
    st = torch.arange(N, dtype=torch.int32, device=dev)
    print(f"# {torch.cuda.get_device_name(0)}; V = {V}, bit rows; median of {rounds} rounds, us (events round the Python call)")
    # (a) the working set fits: nothing to fill in either arm
    small.mask_rows(st), full.mask_rows(st)
    t_small, t_full = [], []
    for _ in range(rounds):
        t_small.append(_event_us(lambda: small.mask_rows(st)))
        t_full.append(_event_us(lambda: full.mask_rows(st)))
    assert small.stats() == {"rows_in_use": N + 2, "fills": N, "evictions": 0}
    print(f"fits    1024 states, all rows present: evicting bank {med(t_small):7.1f}   claim path, nothing new {med(t_full):7.1f}   "
          f"difference {med(t_small) - med(t_full):+.1f}")
    # (b) thrash: k evictions a call against k first-time fills
    for k in (64, N):
        t_small, t_full, base = [], [], N
        new = torch.arange(k, dtype=torch.int32, device=dev)
        for _ in range(rounds):
            small._reset_bank()
            small.mask_rows(st)  # the bank full, every row last requested here
            before = small.stats()["evictions"]
            nxt = (base + new) % S
            torch.cuda.synchronize()
            t_small.append(_event_us(lambda: small.mask_rows(nxt)))
            assert small.stats()["evictions"] - before == k
            full._reset_bank()
            torch.cuda.synchronize()
            t_full.append(_event_us(lambda: full.mask_rows(new)))
        small.check(), full.check()
        print(f"thrash  {k:4d} new states: {k:4d} evictions and fills {med(t_small):8.1f}   claim path, {k:4d} first fills {med(t_full):8.1f}   "
              f"difference {med(t_small) - med(t_full):+.1f}", flush=True)


def sis_ab(eng):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.sis import DeviceSIS

    T = 10
    llm = AsyncAmdLM.from_config(GPT2Config(), None, device="cuda:0", dtype=torch.float32, seed=1234, engine=eng, batch_size=N)
    vocab = vocabulary(V)
    vocab[50256] = b"<eos>"
    full, small = pair(eng, ring(counting=True), vocab, eos_id=50256, skip=(50256,))
    prompt = list(range(100, 108))
    arms = {"evicting bank, 1026 rows": DeviceSIS(llm, N, prompt, T, 50256, seed=1, use_particle_kv=True, constraint=small),
            "bank of all 2050 rows": DeviceSIS(llm, N, prompt, T, 50256, seed=1, use_particle_kv=True, constraint=full)}

    def loop(s):
        s.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(T):
            s.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / T

    for s in arms.values():
        loop(s), loop(s)
    times = {k: [] for k in arms}
    for _ in range(3):
        for k, s in arms.items():
            times[k].append(loop(s))
    for k, v in times.items():
        print(f"# {k}: median {statistics.median(v):.3f} ms a step, runs {[round(t, 3) for t in v]}")
    a, b = (statistics.median(v) for v in times.values())
    spread = max(times["bank of all 2050 rows"]) - min(times["bank of all 2050 rows"])
    small.check(), full.check()
    print(f"# difference {1e3 * (a - b):+.1f} us a step; run-to-run spread of the full-bank arm {1e3 * spread:.1f} us; "
          f"the evicting bank over all runs: {small.stats()}; the full bank: {full.stats()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sis", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    eng = HipEngine("cuda:0")
    if not args.no_kernels:
        kernels(eng, args.rounds)
    if args.sis:
        sis_ab(eng)


if __name__ == "__main__":
    main()
