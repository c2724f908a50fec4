"""A/B of `constraints.determinize` on the device, arms alternating in one process, medians and spread:
  search   the closure's sweeps and the rounds alone: HIP events round `_nfa_search`, which is the two batch loops and nothing
           else (glb_nfa_closure and glb_nfa_subset_round in batches of 64 launches, the status words read between them); the
           automaton is uploaded and the block's buffers allocated once, outside the window
  whole    `determinize(...)`: the host's arrays (CSRs, byte groups), the upload, the search, liveness, every table down to
           the host; wall clock
  host     where the automaton comes from a pattern, `_regex_dfa` (what `ByteDFA.from_regex` runs without a device); else the
           restatement tests/nfa_det_ref.py; one run, wall clock
Workloads: (a|b)*a(a|b){k} at k = 11 and 15 (2^(k+1) states); an alternation of words of tests/dfa_min_ref.lexicon_trie written
as a pattern (as many of the 1000 as stay within 4096 important states); the trie, a separator and the trie again, `concat`.

    python tools/nfa_det_ab.py [--rounds 5]
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
from dfa_ab import _event_us  # noqa: E402  (imports the package too)
from genlm_backend_amd.constraints import ByteDFA, ByteNFA, _regex_dfa, determinize  # noqa: E402
from genlm_backend_amd.constraints.tables import _nfa_arrays, _nfa_block, _nfa_search  # noqa: E402
from genlm_backend_amd.engine import HipEngine  # noqa: E402
from tests import dfa_min_ref as M  # noqa: E402
from tests import nfa_det_ref as N  # noqa: E402  (the restatement: the host arm of what no pattern gives)


def _spread(xs):
    return f"{statistics.median(xs):10.2f} [{min(xs):.2f} .. {max(xs):.2f}]"


def workload(eng, name, nfa, pattern, max_states, rounds):
    dfa, sets, states = determinize(eng, nfa, max_states)  # warm-up of the device path
    arrays = _nfa_arrays(nfa)
    p, buf = _nfa_block(eng, arrays, int(min(max_states, 1 << min(len(states), 30))))
    stats = _nfa_search(eng, p, buf["status"])
    search_ms, whole_ms = [], []
    for _ in range(rounds):
        torch.cuda.synchronize()
        search_ms.append(_event_us(lambda: _nfa_search(eng, p, buf["status"])) / 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        determinize(eng, nfa, max_states)
        torch.cuda.synchronize()
        whole_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    if pattern is not None:
        d, acc = _regex_dfa(pattern, max_states)
        host_ms, arm = (time.perf_counter() - t0) * 1e3, "_regex_dfa"
        d, acc, _ = N.renumber(d, acc, 0)
    else:
        want = N.determinize(nfa)
        host_ms, arm = (time.perf_counter() - t0) * 1e3, "restatement"
        d, acc = want["delta"], want["accepting"]
    assert np.array_equal(d, dfa.delta) and np.array_equal(acc, dfa.accepting)
    print(f"{name}: {nfa.n_states} NFA states, {len(states)} important ({sets.shape[1]} words a set), {arrays['n_groups']} byte groups: "
          f"{stats['sweeps']} sweeps, {stats['rounds']} rounds of {p.chunk} states at most, {dfa.n_states} states")
    print(f"    search ms {_spread(search_ms)}   whole ms {_spread(whole_ms)}   host ({arm}) ms {host_ms:10.2f} (1 run)")
    print(f"    host / whole {host_ms / statistics.median(whole_ms):.2f}x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    eng = HipEngine("cuda:0")
    print(f"# {torch.cuda.get_device_name(0)}; median [min .. max] of {args.rounds} rounds, the arms alternating in one process; host: one run")
    for k in (11, 15):
        pattern = b"(a|b)*a(a|b){%d}" % k
        workload(eng, pattern.decode(), ByteNFA.from_regex(pattern), pattern, 1 << 17, args.rounds)
    words = list(dict.fromkeys(M.lexicon_trie()))
    n = len(words)
    while sum(len(w) for w in words[:n]) + 1 > 4096:  # (a Thompson automaton has an important state a byte, and the last)
        n -= 1
    pattern = b"|".join(words[:n])
    workload(eng, f"an alternation of {n} of the lexicon's {len(words)} words", ByteNFA.from_regex(pattern), pattern, 1 << 16, args.rounds)
    trie = ByteDFA.from_strings(words)
    workload(eng, f"concat(trie of {trie.n_states} states, ' ', the trie)", ByteNFA.concat([trie, ByteDFA.from_regex(rb" "), trie]), None, 1 << 16,
             args.rounds)


if __name__ == "__main__":
    main()
