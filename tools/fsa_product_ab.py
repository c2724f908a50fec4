"""A/B of `constraints.product` on the device, arms alternating in one process, medians and spread:
  search   the rounds and the liveness sweeps alone: HIP events round `DeviceTables._product_search`, which is the two batch
           loops and nothing else (glb_fsa_product_round and glb_fsa_live in batches of 64 launches, the status words read
           between them); the operands are uploaded and the block's buffers allocated once, outside the window
  whole    `product(...)`: both operands up, the search, the trim (glb_dfa_quotient), every table down to the host; wall clock
  host     the NumPy restatement tests/fsa_product_ref.py on the same host (its queue search is a Python loop a state), wall
           clock; `--host-rounds` runs of it (it is the slow arm)
Two workloads: a lexicon trie of about 10^5 states (§20's, §21's) "and" the README's number pattern widened to letters, and a
seeded random pair of 10^3 states each with one arc in ten.  Also: rounds, sweeps, states before and after the trim, states
after `minimize`, and the bytes a second the search moves counted at the expansion's algorithmic 3 KB a pair state (two delta
rows read, one written) over the WHOLE search - all six launches of every round and the sweeps.  The expansion kernel alone
is a run of its own: `--once` makes each workload's product a single time, for
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/fsa_product_ab.py --once
whose kernel statistics give fsa_expand_kernel's total time; 3 KB x the pair states of both workloads over it is its rate.

    python tools/fsa_product_ab.py [--rounds 5] [--host-rounds 1] [--once]
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
from genlm_backend_amd.constraints import ByteDFA, DeviceTables, minimize, product  # noqa: E402
from genlm_backend_amd.engine import HipEngine  # noqa: E402
from tests import fsa_product_ref as F  # noqa: E402  (the NumPy restatement: the host arm)
from tests import wfsa_push_ref as P  # noqa: E402


def random_sparse(S, seed, keep=0.1):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, S, (S, 256)).astype(np.int32)
    d[rng.random((S, 256)) >= keep] = -1
    acc = rng.random(S) < 0.2
    acc[0] = True
    return ByteDFA(d, acc, 0)


def _spread(xs):
    return f"{statistics.median(xs):10.2f} [{min(xs):.2f} .. {max(xs):.2f}]"


def workload(eng, name, a, b, op, max_states, rounds, host_rounds, once):
    cap = int(min(max_states, (a.n_states + 1) * (b.n_states + 1)))
    both, pairs = product(eng, a, b, op, max_states)  # warm-up of every arm's device path
    if once:
        print(f"{name}: {a.n_states} x {b.n_states} states, op={op!r}: one product, {both.n_states} states after the trim", flush=True)
        return
    ta, tb = DeviceTables.upload(eng, a), DeviceTables.upload(eng, b)
    p, buf = ta._product_block(tb, op, cap)
    stats = ta._product_search(p, buf["status"])
    search_ms, whole_ms, host_ms = [], [], []
    for r in range(rounds):
        torch.cuda.synchronize()
        search_ms.append(_event_us(lambda: ta._product_search(p, buf["status"])) / 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        product(eng, a, b, op, max_states)
        torch.cuda.synchronize()
        whole_ms.append((time.perf_counter() - t0) * 1e3)
        if r < host_rounds:
            t0 = time.perf_counter()
            want = F.product(a, b, op)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(want["delta"], both.delta) and np.array_equal(want["pairs"], pairs)
    small = minimize(eng, both)[0]
    gbs = 3072 * stats["states"] / (statistics.median(search_ms) * 1e-3) / 1e9
    print(f"{name}: {a.n_states} x {b.n_states} states, op={op!r}: {stats['rounds']} rounds, {stats['sweeps']} sweeps, "
          f"{stats['states']} states before the trim, {both.n_states} after, {small.n_states} minimised")
    print(f"    search ms {_spread(search_ms)}   whole ms {_spread(whole_ms)}   host ms {_spread(host_ms)} ({len(host_ms)} run(s))")
    print(f"    host / whole {statistics.median(host_ms) / statistics.median(whole_ms):.1f}x   3 KB a pair state over the whole search: "
          f"{gbs:.2f} GB/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--once", action="store_true", help="each workload's product a single time, nothing timed: for a profiler")
    args = ap.parse_args()
    eng = HipEngine("cuda:0")
    print(f"# {torch.cuda.get_device_name(0)}; median [min .. max] of {args.rounds} rounds, the arms alternating in one process")
    d, acc, start, _, _ = P.trie(n_strings=24000, max_len=10, seed=1)
    t0 = time.perf_counter()
    trie = ByteDFA(d, acc, start)
    print(f"# (the trie's host `ByteDFA`, its `_live` loop included: {(time.perf_counter() - t0) * 1e3:.0f} ms, paid once, in no arm)")
    number = ByteDFA.from_regex(rb"-?(0|[1-9][0-9a-z]*)(\.[0-9a-z]+)?")
    workload(eng, "lexicon trie and number pattern", trie, number, "and", 1 << 18, args.rounds, args.host_rounds, args.once)
    workload(eng, "random pair", random_sparse(1000, 0), random_sparse(1000, 1), "and", 1 << 21, args.rounds, args.host_rounds, args.once)


if __name__ == "__main__":
    main()
