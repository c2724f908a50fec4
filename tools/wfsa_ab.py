"""A/B of the device-made token log-weight rows of a weighted byte automaton against the bit masks of the
same automaton (§17), in one process, the arms alternating round by round (medians):
  kernels   glb_dfa_claim_rows + glb_dfa_fill_weights + glb_dfa_mask_ids for 1, 64 and 1024 NEW states at V = 50257 and
            128256, under a permissive automaton (every token walks to its last byte) and a restrictive one ([0-9]+: most
            tokens die at their first byte); beside it the same three calls with glb_dfa_fill_masks, and the ratio.  The float
            rows are 32 times the bytes of the bit rows.
  --sis     DeviceSIS, 1024 particles, gpt2-small shape, shared KV rows: a 10-step loop under a warmed weighted constraint
            against the same loop under the warmed boolean constraint of the same automaton

    python tools/wfsa_ab.py [--rounds 5] [--sis] [--no-kernels]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfa_ab import _event_us, automaton, vocabulary  # noqa: E402  (imports the package too)
from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint  # noqa: E402
from genlm_backend_amd.engine import HipEngine  # noqa: E402


def weighted(dfa, seed=0):
    """`dfa` with seeded arc weights in [-4, 0] and final weights in [-2, 0]."""
    rng = np.random.default_rng(seed)
    arc = np.where(dfa.delta >= 0, -4.0 * rng.random(dfa.delta.shape), -np.inf).astype(np.float32)
    fin = np.where(dfa.accepting, -2.0 * rng.random(dfa.n_states), -np.inf).astype(np.float32)
    return ByteWFSA(dfa.delta, arc, fin, dfa.start)


def kernels(eng, rounds):
    print(f"# {torch.cuda.get_device_name(0)}; median of {rounds} rounds, us; every round starts from an empty bank; "
          "claim + fill + ids, events round the Python call")
    print(f"{'V':>7s} {'automaton':>11s} {'new':>5s} {'weights':>9s} {'bits':>9s} {'ratio':>6s} {'MB written':>10s} {'GB/s':>7s}")
    for V in (50257, 128256):
        vocab = vocabulary(V)
        for kind in ("permissive", "restrictive"):
            dfa = automaton(kind, 1024)
            arms = {"weights": DeviceConstraint(eng, weighted(dfa), vocab, eos_id=0, skip_ids=(), mask_bank_bytes=1 << 30),
                    "bits": DeviceConstraint(eng, dfa, vocab, eos_id=0, skip_ids=())}
            assert arms["weights"].capacity == arms["bits"].capacity == 1026
            for n_new in (1, 64, 1024):
                st = torch.arange(n_new, dtype=torch.int32, device=eng.device)
                times = {k: [] for k in arms}
                for _ in range(rounds):
                    for k, c in arms.items():
                        c._reset_bank()
                        torch.cuda.synchronize()
                        times[k].append(_event_us(lambda: c.mask_rows(st)))
                for c in arms.values():
                    c.check()
                w, b = (statistics.median(times[k]) for k in ("weights", "bits"))
                mb = n_new * V * 4 / 1e6
                print(f"{V:7d} {kind:>11s} {n_new:5d} {w:9.1f} {b:9.1f} {w / b:6.2f} {mb:10.1f} {mb * 1e-3 / (w * 1e-6):7.0f}", flush=True)
            del arms
            torch.cuda.empty_cache()


def sis_ab(eng, rounds):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.sis import DeviceSIS

    N, T, V = 1024, 10, 50257
    llm = AsyncAmdLM.from_config(GPT2Config(), None, device="cuda:0", dtype=torch.float32, seed=1234, engine=eng, batch_size=N)
    vocab = vocabulary(V)
    vocab[50256] = b"<eos>"
    dfa = automaton("permissive", 64)
    cons = {"weighted constraint (warmed)": DeviceConstraint(eng, weighted(dfa), vocab, eos_id=50256, skip_ids=(50256,)),
            "boolean constraint (warmed)": DeviceConstraint(eng, dfa, vocab, eos_id=50256, skip_ids=(50256,))}
    prompt = list(range(100, 108))
    arms = {}
    for k, c in cons.items():
        assert c.warm()
        arms[k] = DeviceSIS(llm, N, prompt, T, 50256, seed=1, use_particle_kv=True, constraint=c)

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
    for _ in range(rounds):
        for k, s in arms.items():
            times[k].append(loop(s))
    for k, v in times.items():
        print(f"# {k}: median {statistics.median(v):.3f} ms a step, runs {[round(t, 3) for t in v]}")
    a, b = (statistics.median(v) for v in times.values())
    spread = {k: max(v) - min(v) for k, v in times.items()}
    for c in cons.values():
        c.check()
    print(f"# difference {1e3 * (a - b):.1f} us a step; run-to-run spread: weighted arm {1e3 * spread['weighted constraint (warmed)']:.1f} us, "
          f"boolean arm {1e3 * spread['boolean constraint (warmed)']:.1f} us; raw steps over all loops: "
          + ", ".join(f"{k.split()[0]} {s.constraint_raw_steps}" for k, s in arms.items()))


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
        sis_ab(eng, args.rounds)


if __name__ == "__main__":
    main()
