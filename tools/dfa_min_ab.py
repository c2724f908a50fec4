"""A/B of minimisation on the device, arms alternating in one process, HIP events, medians:
  cost     `constraints.minimize` on the device (glb_dfa_refine in batches with the status read between them, the class array
           down, the ids up, glb_dfa_quotient, the quotient down) against the NumPy restatement tests/dfa_min_ref.py on the host
           (its refinement alone: `np.unique(axis=0)` over the signatures).  §20's three automata: S = 64 and 4096 (random) and
           a lexicon trie of about 10^5 states; states in and out, rounds, microseconds a round from one call of exactly that
           many.  The restatement is timed at full size where a run takes under a minute, else on a smaller trie of the same kind of at
           most `--host-states` states, and the last column says which.
  bank     the trie under a float bank (V = 50257): `warm()` and the bank's bytes, minimised against not.

    python tools/dfa_min_ab.py [--rounds 5] [--no-bank] [--bank-gib 8]
"""
import argparse
import ctypes as C
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
from dfa_push_ab import random_automaton  # noqa: E402
from genlm_backend_amd import _lib  # noqa: E402
from genlm_backend_amd.constraints import ByteDFA, ByteWFSA, DeviceConstraint, _kept, minimize  # noqa: E402
from genlm_backend_amd.engine import HipEngine  # noqa: E402
from tests import dfa_min_ref as M  # noqa: E402  (the NumPy restatement: the host arm)
from tests import wfsa_push_ref as P  # noqa: E402


def host_refine(dfa):
    keep = dfa.live & dfa.reachable
    keep[dfa.start] = True
    t0 = time.perf_counter()
    cls, rounds = M.refine(dfa.delta, keep, dfa.accepting.astype(np.int64))
    return (time.perf_counter() - t0) * 1e3, len(np.unique(cls[cls >= 0])), rounds


def cost(eng, rounds, host_limit_states):
    print(f"# {torch.cuda.get_device_name(0)}; median of {rounds} rounds; device: events round constraints.minimize (uploads, status "
          "reads, class array down, ids up, quotient down included); host: the restatement's refinement alone, wall clock")
    print(f"{'automaton':>14s} {'S in':>7s} {'S out':>7s} {'rounds':>6s} {'device us':>10s} {'us/round':>9s} {'quotient us':>11s} "
          f"{'host ms':>10s} {'host S':>7s}")
    cases = [("random", random_automaton(64)), ("random", random_automaton(4096))]
    d, acc, start, _, _ = P.trie(n_strings=24000, max_len=10, seed=1)
    cases.append(("lexicon trie", (d, acc, start)))
    for name, (d, acc, start) in cases:
        dfa = ByteDFA(d, acc, start)
        S = dfa.n_states
        small, state_map = minimize(eng, dfa)
        # one call of exactly the rounds it takes, nothing read in between; then the quotient alone
        keep = _kept(dfa)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
        delta_d, keep_d, fin_d, acc_d = up(dfa.delta), up(keep.astype(np.uint8)), up(acc.astype(np.int32)), up(acc.astype(np.uint8))
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=eng.device)
        slots = 1 << max(1, (2 * S - 1).bit_length())
        cls, scratch, table = i32(S), i32(S), torch.empty(slots * 12 // 8, dtype=torch.int64, device=eng.device)
        status = torch.zeros(_lib.DFA_MIN_STATUS, dtype=torch.int32, device=eng.device)
        p = _lib.DfaMinArgs()
        p.struct_size, p.n_states = C.sizeof(_lib.DfaMinArgs), S
        p.delta, p.keep, p.final_bits = delta_d.data_ptr(), keep_d.data_ptr(), fin_d.data_ptr()
        p.cls, p.scratch, p.table, p.table_slots, p.status = cls.data_ptr(), scratch.data_ptr(), table.data_ptr(), slots, status.data_ptr()
        p.restart = 1
        eng.dfa_call("glb_dfa_refine", _rounds(p, 4096))
        n_rounds = int(status[0].item())
        new_id, rep = M.new_ids(cls.cpu().numpy())
        assert np.array_equal(new_id, state_map) and len(rep) == small.n_states and status[1:3].tolist() == [1, 0]
        both = up(np.concatenate([new_id, rep]))
        delta_out, acc_out = i32(len(rep) * 256), torch.empty(len(rep), dtype=torch.uint8, device=eng.device)
        p.new_id, p.rep, p.n_new = both.data_ptr(), both.data_ptr() + 4 * S, len(rep)
        p.accepting, p.delta_out, p.accepting_out = acc_d.data_ptr(), delta_out.data_ptr(), acc_out.data_ptr()
        dev_us, round_us, quot_us = [], [], []
        for _ in range(rounds):
            torch.cuda.synchronize()
            dev_us.append(_event_us(lambda: minimize(eng, dfa)))
            round_us.append(_event_us(lambda: eng.dfa_call("glb_dfa_refine", _rounds(p, n_rounds))) / n_rounds)
            quot_us.append(_event_us(lambda: eng.dfa_call("glb_dfa_quotient", p)))
        assert status[:3].tolist() == [n_rounds, 1, 0]
        host = dfa
        if S > host_limit_states:  # the restatement on a smaller trie of the same kind
            n = 24000
            while host.n_states > host_limit_states:
                n //= 2
                hd, hacc, hstart, _, _ = P.trie(n_strings=n, max_len=10, seed=1)
                host = ByteDFA(hd, hacc, hstart)
        host_ms, host_out, host_rounds = host_refine(host)
        if host is dfa:
            assert (host_out, host_rounds) == (small.n_states, n_rounds)
        print(f"{name:>14s} {S:7d} {small.n_states:7d} {n_rounds:6d} {statistics.median(dev_us):10.1f} {statistics.median(round_us):9.2f} "
              f"{statistics.median(quot_us):11.1f} {host_ms:10.1f} {host.n_states:7d}", flush=True)
        del delta_d, cls, scratch, table, delta_out
        torch.cuda.empty_cache()


def _rounds(p, n):
    p.rounds = n
    return p


def bank(eng, rounds, gib):
    V = 50257
    vocab = vocabulary(V)
    vocab[50256] = b"<eos>"
    d, acc, start, _, _ = P.trie(n_strings=24000, max_len=10, seed=1)
    arc, fin = np.where(d >= 0, 0.0, -np.inf).astype(np.float32), np.where(acc, 0.0, -np.inf).astype(np.float32)
    wf = ByteWFSA(d, arc, fin, start)
    print(f"# the lexicon trie ({wf.n_states} states, zero weights) under a float bank, V = {V}, mask_bank_bytes = {gib} GiB")
    for minimise in (False, True):
        t0 = time.perf_counter()
        c = DeviceConstraint(eng, wf, vocab, eos_id=50256, skip_ids=(50256,), mask_bank_bytes=gib << 30, on_full="evict", minimize=minimise)
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3
        held = c.dfa.n_states + 2 <= c.capacity
        warm_us = []
        for _ in range(rounds if held else 0):
            c._reset_bank()
            torch.cuda.synchronize()
            warm_us.append(_event_us(c.warm))
        c.check()
        print(f"# minimize={minimise}: {c.dfa.n_states} states, bank {c.capacity} rows = {c.bank.numel() * 4 / 2 ** 20:.1f} MiB, "
              f"holds every state: {held}, warm() {statistics.median(warm_us) / 1e3 if warm_us else float('nan'):.2f} ms, "
              f"constructor {build_ms:.0f} ms, stats {c.minimize_stats()}", flush=True)
        del c
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-bank", action="store_true")
    ap.add_argument("--bank-gib", type=int, default=8, help="mask_bank_bytes of the float bank, GiB")
    ap.add_argument("--host-states", type=int, default=200000, help="the largest automaton the NumPy restatement is timed on")
    args = ap.parse_args()
    eng = HipEngine("cuda:0")
    cost(eng, args.rounds, args.host_states)
    if not args.no_bank:
        bank(eng, args.rounds, args.bank_gib)


if __name__ == "__main__":
    main()
