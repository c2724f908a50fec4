"""A/B of the device-made DFA token masks, in one process, the arms alternating round by round (medians):
  kernels   glb_dfa_claim_rows + glb_dfa_fill_masks + glb_dfa_mask_ids for 1, 64 and 1024 NEW states (and the same four
            launches again with nothing new: the claim finds every row, the fill exits) at V = 50257 and 128256, under a permissive automaton (every byte string is accepted: every token walks to its last byte) and a
            restrictive one ([0-9]+: most tokens die at their first byte); beside them what users do today - the masks of
            the same states made on the host in NumPy (all tokens side by side, one byte position at a time) and the H2D
            copy of the [N, W] bit rows
  --sis     DeviceSIS, 1024 particles, gpt2-small shape, shared KV rows: a 10-step loop with a warmed constraint against the
            same loop with `particle_masks` holding the same bits and standing still, three alternating runs

    python tools/dfa_ab.py [--rounds 5] [--sis]
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
from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint  # noqa: E402
from genlm_backend_amd.engine import HipEngine  # noqa: E402


def vocabulary(V, seed=0):
    """Byte strings shaped like a BPE vocabulary's: the 256 bytes, then words of 2 .. 12 letters, digits and spaces."""
    rng = np.random.default_rng(seed)
    chars = np.frombuffer(b" etaoinshrdlucmfw0123456789", np.uint8)
    lens = rng.integers(2, 13, V - 256)
    return [bytes([b]) for b in range(256)] + [bytes(rng.choice(chars, int(n))) for n in lens]


def automaton(kind, S):
    """S states in a ring: permissive - every byte moves on, every state accepts; restrictive - only digits do."""
    d = np.full((S, 256), -1, np.int32)
    nxt = (np.arange(S, dtype=np.int32) + 1) % S
    if kind == "permissive":
        d[:] = nxt[:, None]
    else:
        d[:, 48:58] = nxt[:, None]
    return ByteDFA(d, np.ones(S, np.bool_), 0)


def host_masks(dfa, vocab, states):
    """Today's path, vectorised as far as NumPy goes: [len(states), ceil(V / 32)] uint32."""
    V = len(vocab)
    lens = np.array([len(t) for t in vocab])
    pad = np.zeros((V, int(lens.max())), np.int64)
    for i, t in enumerate(vocab):
        pad[i, :len(t)] = list(t)
    out = np.zeros((len(states), (V + 31) // 32), np.uint32)
    delta = dfa.delta.astype(np.int64)
    for k, s in enumerate(states):
        cur = np.full(V, s, np.int64)
        for j in range(pad.shape[1]):
            on = (j < lens) & (cur >= 0)
            cur = np.where(on, delta[np.maximum(cur, 0), pad[:, j]], cur)
        ok = (cur >= 0) & dfa.live[np.maximum(cur, 0)]
        bits = np.zeros(out.shape[1] * 32, np.uint8)
        bits[:V] = ok
        out[k] = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    return out


def _event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def kernels(eng, rounds):
    print(f"# {torch.cuda.get_device_name(0)}; median of {rounds} rounds, us; every device round starts from an empty bank")
    print(f"{'V':>7s} {'automaton':>11s} {'new':>5s} {'claim+fill+ids':>15s} {'nothing new':>11s} {'host masks':>11s} {'H2D [N,W]':>10s}")
    for V in (50257, 128256):
        vocab = vocabulary(V)
        for kind in ("permissive", "restrictive"):
            dfa = automaton(kind, 1024)
            c = DeviceConstraint(eng, dfa, vocab, eos_id=0, skip_ids=())
            for n_new in (1, 64, 1024):
                st = torch.arange(n_new, dtype=torch.int32, device=eng.device)
                host_states = list(range(min(n_new, 8)))  # (the host walk is linear in the states: 8 are timed, scaled)
                t_dev, t_ids, t_host, t_h2d = [], [], [], []
                pinned = torch.zeros((n_new, c.words), dtype=torch.int32).pin_memory()
                dst = torch.empty((n_new, c.words), dtype=torch.int32, device=eng.device)
                for _ in range(rounds):
                    c._reset_bank()
                    torch.cuda.synchronize()
                    t_dev.append(_event_us(lambda: c.mask_rows(st)))
                    t_ids.append(_event_us(lambda: c.mask_rows(st)))  # nothing new: the claim finds every row, the fill exits
                    t0 = time.perf_counter()
                    host_masks(dfa, vocab, host_states)
                    t_host.append((time.perf_counter() - t0) * 1e6 * n_new / len(host_states))
                    t_h2d.append(_event_us(lambda: dst.copy_(pinned, non_blocking=True)))
                c.check()
                med = statistics.median
                print(f"{V:7d} {kind:>11s} {n_new:5d} {med(t_dev):15.1f} {med(t_ids):11.1f} {med(t_host):11.0f} {med(t_h2d):10.1f}",
                      flush=True)


def sis_ab(eng):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.sis import DeviceSIS

    N, T, V = 1024, 10, 50257
    llm = AsyncAmdLM.from_config(GPT2Config(), None, device="cuda:0", dtype=torch.float32, seed=1234, engine=eng, batch_size=N)
    vocab = vocabulary(V)
    vocab[50256] = b"<eos>"
    dfa = automaton("permissive", 64)
    c = DeviceConstraint(eng, dfa, vocab, eos_id=50256, skip_ids=(50256,))
    assert c.warm()
    prompt = list(range(100, 108))
    # the parent commit's arm: the same bits per particle, standing still (the permissive ring gives every state one mask)
    row = c.bank[c.mask_rows(c.states0(1)).long()]
    pm = torch.cat([row.expand(N, -1), c.bank[1:2]]).contiguous()
    arms = {"constraint (warmed)": DeviceSIS(llm, N, prompt, T, 50256, seed=1, use_particle_kv=True, constraint=c),
            "particle_masks standing still": DeviceSIS(llm, N, prompt, T, 50256, seed=1, use_particle_kv=True, particle_masks=pm)}

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
    spread = max(times["particle_masks standing still"]) - min(times["particle_masks standing still"])
    s = arms["constraint (warmed)"]
    s.reset()
    for _ in range(3):
        s.step()
    # the two launches a warmed step adds, on a population three tokens in: the ids, and the advance over the newest token
    # (from the state before it: recomputed over the suffix without it)
    ln_was = (s.lengths - 1).clamp_min(0)
    before = c.advance(None, s.contexts, s.prompt_len, torch.maximum(ln_was, s.prompt_len))
    ids_us = statistics.median(_event_us(lambda: c.mask_rows(s.states)) for _ in range(9))
    adv_us = statistics.median(_event_us(lambda: c.advance(before, s.contexts, torch.maximum(ln_was, s.prompt_len), s.lengths))
                               for _ in range(9))
    print(f"# difference {1e3 * (a - b):.1f} us a step; run-to-run spread of the particle_masks arm {1e3 * spread:.1f} us; "
          f"the constraint's own launches (events round the Python call): mask ids {ids_us:.1f} us, advance over one token {adv_us:.1f} us")


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
