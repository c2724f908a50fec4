"""A/B of `constraints.LazyConstraint` against the existing path - `determinize`, then `DeviceConstraint` over
the automaton - arms alternating in one process, HIP events, median [min .. max]:
  step     one steady-state step at 1024 particles, `advance` of one token and `mask_rows`, no new set and every row in the
           bank: the lazy constraint's ten launches (six and four) against the five of `DeviceConstraint`, on the same tokens
  fill     the row of one new state: glb_lazy_serve with the bank started over, lane form and (W == 1: forced) wave form,
           against glb_dfa_claim_rows + glb_dfa_fill_masks + glb_dfa_mask_ids for one state
  first    from the pattern to the first mask, wall clock: the lazy constructor and one `mask_rows` against `determinize`,
           the `DeviceConstraint` constructor and one `mask_rows`
Workloads, V = 50257: (a|b)*a(a|b){11} (4096 states, W = 1) and an alternation of words of tests/dfa_min_ref.lexicon_trie.

    python tools/lazy_ab.py [--rounds 5] [--out profiles/rNN/lazy_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dfa_ab import _event_us, vocabulary  # noqa: E402  (imports the package too)
from genlm_backend_amd.constraints import ByteNFA, DeviceConstraint, LazyConstraint, determinize  # noqa: E402
from genlm_backend_amd.engine import HipEngine  # noqa: E402
from tests import dfa_min_ref as M  # noqa: E402

N, V = 1024, 50257


def _spread(xs):
    return f"{statistics.median(xs):9.1f} [{min(xs):.1f} .. {max(xs):.1f}]"


def workload(eng, name, pattern, letters, spread, rounds, say):
    vocab = vocabulary(V)
    vocab[256:256 + len(letters)] = letters  # (tokens the pattern reads beside the single bytes)
    eos, dev = V - 1, eng.device
    nfa = ByteNFA.from_regex(pattern)
    first_lazy, first_eager = [], []
    for _ in range(rounds):  # from the pattern to the first mask
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lazy = LazyConstraint(eng, nfa, vocab, eos, skip_ids=(eos,))
        lazy.mask_rows(lazy.states0(N))
        torch.cuda.synchronize()
        first_lazy.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        dfa = determinize(eng, nfa)[0]
        eager = DeviceConstraint(eng, dfa, vocab, eos, skip_ids=(eos,))
        eager.mask_rows(eager.states0(N))
        torch.cuda.synchronize()
        first_eager.append((time.perf_counter() - t0) * 1e3)
    # a population spread over the automaton: `spread` steps of tokens the pattern reads, then one step repeated (no new set)
    rng = np.random.default_rng(1)
    reads = [t for t in range(V - 1) if vocab[t] and set(vocab[t]) <= set(b"".join(letters))][:64]
    tok = torch.from_numpy(rng.choice(np.array(reads, np.int32), (N, spread + 1)).astype(np.int32)).to(dev)
    sl, se = lazy.states0(N), eager.states0(N)
    at = lambda t: (torch.full((N,), t, dtype=torch.int32, device=dev), torch.full((N,), t + 1, dtype=torch.int32, device=dev))
    for t in range(spread):
        sl, se = lazy.advance(sl, tok, *at(t)), eager.advance(se, tok, *at(t))
        lazy.mask_rows(sl), eager.mask_rows(se)
    assert torch.equal(sl < 0, se < 0)
    frm, to = at(spread)
    outl, oute = torch.empty_like(sl), torch.empty_like(se)
    step_l = lambda: lazy.mask_rows(lazy.advance(sl, tok, frm, to, out=outl))
    step_e = lambda: eager.mask_rows(eager.advance(se, tok, frm, to, out=oute))
    step_l(), step_e()
    known = lazy.n_states
    lazy_us, eager_us = [], []
    for _ in range(rounds):
        torch.cuda.synchronize()
        lazy_us.append(_event_us(step_l))
        eager_us.append(_event_us(step_e))
    assert lazy.n_states == known
    lazy.check(), eager.check()
    # the row of one new state: the bank started over, one state asked for
    one_l, one_e = sl[sl >= 0][:1].contiguous(), se[se >= 0][:1].contiguous()
    fills = {arm: [] for arm in (["lane", "wave (forced)"] if lazy.W == 1 else ["wave"]) + ["glb_dfa_fill_masks"]}
    for _ in range(rounds):
        for arm in fills:
            if arm == "glb_dfa_fill_masks":
                eager._reset_bank()
                torch.cuda.synchronize()
                fills[arm].append(_event_us(lambda: eager.mask_rows(one_e)))
            else:
                lazy.force_wave = arm == "wave (forced)"
                lazy._counters.zero_(), lazy._row_of_state.fill_(-1)
                lazy._counters[0] = 2
                torch.cuda.synchronize()
                fills[arm].append(_event_us(lambda: lazy.mask_rows(one_l)))
    lazy.force_wave = False
    say(f"{name}: {len(lazy.bit_state)} important states (W = {lazy.W}), {dfa.n_states} DFA states; {int((sl >= 0).sum())} of {N} particles alive, {known} sets numbered")
    say(f"    step us       lazy {_spread(lazy_us)}   DeviceConstraint {_spread(eager_us)}   ratio {statistics.median(lazy_us) / statistics.median(eager_us):.2f}x")
    for arm, xs in fills.items():
        say(f"    fill us       {arm:20s} {_spread(xs)}")
    say(f"    first mask ms lazy {_spread(first_lazy)}   determinize + DeviceConstraint {_spread(first_eager)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = HipEngine("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# {torch.cuda.get_device_name(0)}; median [min .. max] of {args.rounds} rounds, the arms alternating in one process; V = {V}, {N} particles")
    workload(eng, "(a|b)*a(a|b){11}", rb"(a|b)*a(a|b){11}", [b"ab", b"ba", b"aab", b"bb", b"abab"], 12, args.rounds, say)
    words = list(dict.fromkeys(M.lexicon_trie()))
    n = len(words)
    while sum(len(w) for w in words[:n]) + 1 > 4096:
        n -= 1
    workload(eng, f"an alternation of {n} of the lexicon's words", b"|".join(words[:n]), words[:200], 2, args.rounds, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
