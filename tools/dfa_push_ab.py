"""A/B of weight pushing, arms alternating in one process, HIP events, medians:
  cost     backward weights + pushed tables made on the device (what DeviceConstraint(push="log") runs: glb_dfa_backward in
           batches with the status read between them, then glb_dfa_push_weights) against the NumPy restatement on the host plus
           the upload of the pushed tables - what a user had before.  S = 64 and 4096 (random automata, substochastic weights)
           and a lexicon trie of about 10^5 states; sweep counts, and microseconds a sweep from one call of exactly that many.
  --sis    DeviceSIS, 1024 particles, gpt2-small shape, shared KV rows, a `from_weighted_strings` lexicon: the time of a warmed
           step pushed against unpushed, and the effective sample size after every step of both runs.

    python tools/dfa_push_ab.py [--rounds 5] [--sis] [--no-cost]
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
from genlm_backend_amd import _lib  # noqa: E402
from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint  # noqa: E402
from genlm_backend_amd.engine import HipEngine  # noqa: E402
from tests import wfsa_push_ref as P  # noqa: E402  (the NumPy restatement: the host arm)


def random_automaton(S, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, S, (S, 256)).astype(np.int32)
    d[rng.random((S, 256)) < 0.3] = -1
    acc = rng.random(S) < 0.2
    acc[0] = True
    return d, acc, 0


def cost(eng, rounds):
    print(f"# {torch.cuda.get_device_name(0)}; median of {rounds} rounds; device: events round DeviceConstraint's own pushing "
          "(its status reads included); host: NumPy float32 sweeps + push + upload of the two tables, wall clock")
    print(f"{'automaton':>14s} {'S':>7s} {'sweeps':>6s} {'device us':>10s} {'us/sweep':>9s} {'push us':>8s} {'host ms':>9s} {'host/device':>11s}")
    byte_vocab = [bytes([b]) for b in range(256)] + [b"<eos>"]
    cases = [("random", random_automaton(64)), ("random", random_automaton(4096))]
    d, acc, start, _, _ = P.trie(n_strings=24000, max_len=10, seed=1)
    cases.append(("lexicon trie", (d, acc, start)))
    for name, (d, acc, start) in cases:
        arc, fin = P.substochastic_weights(d, acc, 7)
        wf = ByteWFSA(d, arc, fin, start)
        c = DeviceConstraint(eng, wf, byte_vocab, 256, skip_ids=(256,), mask_bank_bytes=4 << 20)
        own = (c._arc_logw, c._final_logw)
        c.push = "log"
        dev_us, host_ms, sweep_us, push_us = [], [], [], []

        def device():
            c._arc_logw, c._final_logw = own
            c._push_weights(P.TOL, 4096)

        device()
        sweeps = c.push_stats()["sweeps"]
        # one call of exactly `sweeps` launches, nothing read in between; then the push alone
        S = wf.n_states
        f32 = lambda n: torch.empty(n, dtype=torch.float32, device=eng.device)
        beta, scratch, arc_out, final_out = f32(S), f32(S), f32(S * 256), f32(S)
        status = torch.zeros(_lib.DFA_PUSH_STATUS, dtype=torch.int32, device=eng.device)
        p = _lib.DfaPushArgs()
        p.struct_size, p.n_states, p.start, p.semiring = C.sizeof(_lib.DfaPushArgs), S, start, _lib.DFA_PUSH_LOG
        p.delta, p.arc_logw, p.final_logw = c._delta.data_ptr(), own[0].data_ptr(), own[1].data_ptr()
        p.beta, p.scratch, p.arc_out, p.final_out = beta.data_ptr(), scratch.data_ptr(), arc_out.data_ptr(), final_out.data_ptr()
        p.status, p.sweeps, p.restart, p.tol = status.data_ptr(), sweeps, 1, P.TOL
        for _ in range(rounds):
            torch.cuda.synchronize()
            dev_us.append(_event_us(device))
            t0 = time.perf_counter()
            b, _, ok = P.backward(d, arc, fin, P.LOG)
            a, f = P.push(d, arc, fin, b)
            up = [torch.from_numpy(x).to(eng.device) for x in (a, f, b)]
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            del up
            sweep_us.append(_event_us(lambda: eng.dfa_call("glb_dfa_backward", p)) / sweeps)
            push_us.append(_event_us(lambda: eng.dfa_call("glb_dfa_push_weights", p)))
        assert ok and status[:3].tolist() == [sweeps, 1, 0]
        dv, hs = statistics.median(dev_us), statistics.median(host_ms)
        print(f"{name:>14s} {S:7d} {sweeps:6d} {dv:10.1f} {statistics.median(sweep_us):9.2f} {statistics.median(push_us):8.1f} "
              f"{hs:9.2f} {hs * 1e3 / dv:11.1f}", flush=True)
        del c, own, beta, scratch, arc_out, final_out
        torch.cuda.empty_cache()


def lexicon(n=300, seed=3):
    """{bytes: log-weight}: seeded words of 3 .. 8 letters, Zipf weights normalised to one."""
    rng = np.random.default_rng(seed)
    chars = np.frombuffer(b"etaoinshr", np.uint8)
    words = set()
    while len(words) < n:
        words.add(bytes(rng.choice(chars, int(rng.integers(3, 9)))))
    words = sorted(words)
    rng.shuffle(words)
    w = 1.0 / np.arange(1, n + 1)
    return {s: float(np.log(x)) for s, x in zip(words, w / w.sum())}


def sis_ab(eng, rounds):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.sis import DeviceSIS

    N, T, V = 1024, 10, 50257
    llm = AsyncAmdLM.from_config(GPT2Config(), None, device="cuda:0", dtype=torch.float32, seed=1234, engine=eng, batch_size=N)
    vocab = vocabulary(V)
    vocab[50256] = b"<eos>"
    wf = ByteWFSA.from_weighted_strings(lexicon())
    cons = {"pushed": DeviceConstraint(eng, wf, vocab, eos_id=50256, skip_ids=(50256,), mask_bank_bytes=2 << 30, push="log"),
            "unpushed": DeviceConstraint(eng, wf, vocab, eos_id=50256, skip_ids=(50256,), mask_bank_bytes=2 << 30)}
    print(f"# lexicon of {len(lexicon())} strings, {wf.n_states} states; pushing took {cons['pushed'].push_stats()['sweeps']} sweeps, "
          f"start_logw {cons['pushed'].start_logw:.6f}")
    prompt = list(range(100, 108))
    arms = {}
    for k, c in cons.items():
        assert c.warm()
        arms[k] = DeviceSIS(llm, N, prompt, T, 50256, seed=1, use_particle_kv=True, constraint=c)

    def loop(s, ess=None):
        s.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(T):
            s.step()
            if ess is not None:
                w = s.log_weights.double()
                ess.append(float(torch.exp(2 * torch.logsumexp(w, 0) - torch.logsumexp(2 * w, 0)).item()))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / T

    for s in arms.values():
        loop(s), loop(s)
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, s in arms.items():
            times[k].append(loop(s))
    for k, v in times.items():
        print(f"# {k}: median {statistics.median(v):.3f} ms a step, runs {[round(t, 3) for t in v]}, spread {1e3 * (max(v) - min(v)):.1f} us")
    a, b = (statistics.median(v) for v in times.values())
    print(f"# pushed - unpushed: {1e3 * (a - b):.1f} us a step")
    for k, s in arms.items():
        ess = []
        loop(s, ess)
        alive = int(torch.isfinite(s.log_weights).sum().item())
        print(f"# {k}: effective sample size of {N} after each step: {[round(e, 1) for e in ess]}; particles with a finite weight "
              f"at the end: {alive}")
    for c in cons.values():
        c.check()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sis", action="store_true")
    ap.add_argument("--no-cost", action="store_true")
    args = ap.parse_args()
    eng = HipEngine("cuda:0")
    if not args.no_cost:
        cost(eng, args.rounds)
    if args.sis:
        sis_ab(eng, args.rounds)


if __name__ == "__main__":
    main()
