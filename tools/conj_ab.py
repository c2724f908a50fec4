"""A/B of `constraints.ConstraintProduct`, arms alternating in one process, HIP events, median [min .. max]:
  (a) step   one steady-state step at 1024 particles, `advance` of one token and `mask_rows`, nothing new and every row in the
             bank, of `ConstraintProduct([DeviceConstraint(a), DeviceConstraint(b)])` against `DeviceConstraint(product(a, b))`
             and against the two parts stepped alone: the same language two ways, so the difference is the combinator's
             machinery
  (b) fill   the row of one new state with the product's bank started over (the parts' rows are there): glb_conj_serve
             against glb_dfa_claim_rows + glb_dfa_fill_masks + glb_dfa_mask_ids, for a bit bank and - one part a `ByteWFSA` -
             a float bank against glb_dfa_fill_weights
  (c) json   `BytePDA.json()` at max_depth = 32 with a `from_regex` pattern: the steady-state step and the fill of one row
V = 50257, 1024 particles.  The masks are compared bit for bit before anything is timed.

    python tools/conj_ab.py [--rounds 5] [--out profiles/rNN/conj_ab.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dfa_ab import _event_us, vocabulary  # noqa: E402  (imports the package too)
from pda_ab import _at, _spread, _texts  # noqa: E402
from genlm_backend_amd.constraints import (ByteDFA, BytePDA, ByteWFSA, ConstraintProduct, DeviceConstraint, PDAConstraint,  # noqa: E402
                                           product)
from genlm_backend_amd.engine import HipEngine  # noqa: E402

N, V = 1024, 50257


def _restart(c):
    """The bank of `c` started over: no state has a row (the tuples and ids stay)."""
    if isinstance(c, DeviceConstraint):
        c._reset_bank()
    else:
        c._counters.zero_(), c._row_of_state.fill_(-1)
        c._counters[0] = 2


def regular(eng, rounds, say):
    vocab = vocabulary(V)
    letters = [b"ab", b"ba", b"aab", b"bb", b"abab"]
    vocab[256:256 + len(letters)] = letters
    eos, dev = V - 1, eng.device
    a, b = ByteDFA.from_regex(rb"(a|b)*abb(a|b)*"), ByteDFA.from_regex(rb"(a|b)*a(a|b){7}")
    new = lambda d: DeviceConstraint(eng, d, vocab, eos, skip_ids=(eos,))
    whole = product(eng, a, b, "and")[0]
    wb = ByteWFSA(b.delta, np.where(b.delta >= 0, -0.5, -np.inf).astype(np.float32), np.where(b.accepting, -1.0, -np.inf).astype(np.float32), b.start)
    arms = {"ConstraintProduct": ConstraintProduct(eng, [new(a), new(b)]), "DeviceConstraint(product)": new(whole), "part a alone": new(a),
            "part b alone": new(b), "ConstraintProduct, float": ConstraintProduct(eng, [new(a), new(wb)]), "DeviceConstraint(wfsa b)": new(wb)}
    rng = np.random.default_rng(1)
    reads = [t for t in range(V - 1) if vocab[t] and set(vocab[t]) <= set(b"ab")][:64]
    spread = 12
    tok = torch.from_numpy(rng.choice(np.array(reads, np.int32), (N, spread + 1)).astype(np.int32)).to(dev)
    st = {k: c.states0(N) for k, c in arms.items()}
    for t in range(spread):
        for k, c in arms.items():
            st[k] = c.advance(st[k], tok, *_at(dev, t))
            c.mask_rows(st[k])
    frm, to = _at(dev, spread)
    out = {k: torch.empty_like(s) for k, s in st.items()}
    step = {k: (lambda k=k, c=c: c.mask_rows(c.advance(st[k], tok, frm, to, out=out[k]))) for k, c in arms.items()}
    rows = {k: fn() for k, fn in step.items()}
    conj, auto = arms["ConstraintProduct"], arms["DeviceConstraint(product)"]
    assert torch.equal(st["ConstraintProduct"] < 0, st["DeviceConstraint(product)"] < 0)  # the same masks, bit for bit
    assert torch.equal(conj.bank[rows["ConstraintProduct"].long(), :conj.words], auto.bank[rows["DeviceConstraint(product)"].long(), :auto.words])
    both = arms["part a alone"].bank[rows["part a alone"].long(), :conj.words] & arms["part b alone"].bank[rows["part b alone"].long(), :conj.words]
    assert torch.equal(conj.bank[rows["ConstraintProduct"].long(), :conj.words], both)
    known = conj.n_states
    us = {k: [] for k in arms}
    for _ in range(rounds):
        torch.cuda.synchronize()
        for k, fn in step.items():
            us[k].append(_event_us(fn))
    assert conj.n_states == known
    one = {k: s[s >= 0][:1].contiguous() for k, s in st.items()}
    fills = {k: [] for k in arms}
    for _ in range(rounds):
        for k, c in arms.items():
            _restart(c)
            torch.cuda.synchronize()
            fills[k].append(_event_us(lambda: c.mask_rows(one[k])))
    for c in arms.values():
        c.check()
    say(f"(a|b)*abb(a|b)* and (a|b)*a(a|b){{7}}: {a.n_states} and {b.n_states} states, the product automaton {whole.n_states}; "
        f"{int((st['ConstraintProduct'] >= 0).sum())} of {N} particles alive, {known} tuples numbered")
    base = statistics.median(us["DeviceConstraint(product)"])
    for k in arms:
        say(f"    (a) step us   {k:26s} {_spread(us[k])}   {statistics.median(us[k]) / base:.2f}x DeviceConstraint(product)")
    for k, against in (("ConstraintProduct", "DeviceConstraint(product)"), ("ConstraintProduct, float", "DeviceConstraint(wfsa b)")):
        say(f"    (b) fill us   {k:26s} {_spread(fills[k])}   {statistics.median(fills[k]) / statistics.median(fills[against]):.2f}x {against}: "
            f"{_spread(fills[against])}")


def nested(eng, rounds, say):
    vocab = vocabulary(V)
    eos, dev, steps = V - 1, eng.device, 48
    grammar = PDAConstraint(eng, BytePDA.json(), vocab, eos, skip_ids=(eos,), max_depth=32)
    alone = PDAConstraint(eng, BytePDA.json(), vocab, eos, skip_ids=(eos,), max_depth=32)
    only = DeviceConstraint(eng, ByteDFA.from_regex(rb'[\[\]{}":, 0-9a-z]*'), vocab, eos, skip_ids=(eos,))
    arms = {"ConstraintProduct": ConstraintProduct(eng, [grammar, only]), "PDAConstraint alone": alone}
    tok = torch.from_numpy(_texts(N, steps + 1)).to(dev)  # (a single byte is the token of its own value)
    st = {k: c.states0(N) for k, c in arms.items()}
    for t in range(steps):
        for k, c in arms.items():
            st[k] = c.advance(st[k], tok, *_at(dev, t))
            c.mask_rows(st[k])
    frm, to = _at(dev, steps)
    out = {k: torch.empty_like(s) for k, s in st.items()}
    step = {k: (lambda k=k, c=c: c.mask_rows(c.advance(st[k], tok, frm, to, out=out[k]))) for k, c in arms.items()}
    for fn in step.values():
        fn()
    known = arms["ConstraintProduct"].n_states
    us, fills = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(rounds):
        torch.cuda.synchronize()
        for k, fn in step.items():
            us[k].append(_event_us(fn))
    assert arms["ConstraintProduct"].n_states == known
    one = {k: s[s >= 0][-1:].contiguous() for k, s in st.items()}
    for _ in range(rounds):
        for k, c in arms.items():
            _restart(c)
            torch.cuda.synchronize()
            fills[k].append(_event_us(lambda: c.mask_rows(one[k])))
    for c in arms.values():
        c.check()
    say(f"BytePDA.json() at max_depth = 32 with [][{{}}\":, 0-9a-z]*: a 48-step run of {N} particles numbers {known} tuples "
        f"({alone.n_states} configurations alone); {int((st['ConstraintProduct'] >= 0).sum())} particles alive")
    for k in arms:
        say(f"    (c) step us   {k:26s} {_spread(us[k])}")
    for k in arms:
        say(f"    (c) fill us   {k:26s} {_spread(fills[k])}")


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
    regular(eng, args.rounds, say)
    nested(eng, args.rounds, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
