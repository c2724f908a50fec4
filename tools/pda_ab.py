"""A/B of `constraints.PDAConstraint`, arms alternating in one process, HIP events, median [min .. max]:
  (a) step   one steady-state step at 1024 particles, `advance` of one token and `mask_rows`, nothing new and every row in the
             bank, of `PDAConstraint(BytePDA.from_dfa(d))` against `DeviceConstraint(d)` and `LazyConstraint(d)` for the same d,
             (a|b)*a(a|b){11} determinised: the same language three ways, so the difference is the machinery
  (b) fill   the row of one new state with the bank started over: glb_pda_serve against glb_lazy_serve and against
             glb_dfa_claim_rows + glb_dfa_fill_masks + glb_dfa_mask_ids
  (c) json   `BytePDA.json()` at max_depth = 32: the steady-state step and the fill of one row, and how many configurations a
             48-step run over seeded JSON texts numbers
V = 50257, 1024 particles.

    python tools/pda_ab.py [--rounds 5] [--out profiles/rNN/pda_ab.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dfa_ab import _event_us, vocabulary  # noqa: E402  (imports the package too)
from genlm_backend_amd.constraints import ByteDFA, BytePDA, DeviceConstraint, LazyConstraint, PDAConstraint  # noqa: E402
from genlm_backend_amd.engine import HipEngine  # noqa: E402

N, V = 1024, 50257


def _spread(xs):
    return f"{statistics.median(xs):9.1f} [{min(xs):.1f} .. {max(xs):.1f}]"


def _at(dev, t):
    return torch.full((N,), t, dtype=torch.int32, device=dev), torch.full((N,), t + 1, dtype=torch.int32, device=dev)


def _restart(c):
    """The bank of `c` started over: no state has a row (the configurations, sets and ids stay)."""
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
    d = ByteDFA.from_regex(rb"(a|b)*a(a|b){11}")
    arms = {"PDAConstraint": PDAConstraint(eng, BytePDA.from_dfa(d), vocab, eos, skip_ids=(eos,), max_depth=1),
            "LazyConstraint": LazyConstraint(eng, d, vocab, eos, skip_ids=(eos,)),
            "DeviceConstraint": DeviceConstraint(eng, d, vocab, eos, skip_ids=(eos,))}
    rng = np.random.default_rng(1)
    reads = [t for t in range(V - 1) if vocab[t] and set(vocab[t]) <= set(b"ab")][:64]
    spread = 12
    tok = torch.from_numpy(rng.choice(np.array(reads, np.int32), (N, spread + 1)).astype(np.int32)).to(dev)
    st = {k: c.states0(N) for k, c in arms.items()}
    for t in range(spread):
        for k, c in arms.items():
            st[k] = c.advance(st[k], tok, *_at(dev, t))
            c.mask_rows(st[k])
    assert all(torch.equal(st[k] < 0, st["DeviceConstraint"] < 0) for k in arms)
    frm, to = _at(dev, spread)
    out = {k: torch.empty_like(s) for k, s in st.items()}
    step = {k: (lambda k=k, c=c: c.mask_rows(c.advance(st[k], tok, frm, to, out=out[k]))) for k, c in arms.items()}
    rows = {k: fn() for k, fn in step.items()}
    for k, c in arms.items():  # the same masks, bit for bit
        assert torch.equal(c.bank[rows[k].long(), :c.words], arms["DeviceConstraint"].bank[rows["DeviceConstraint"].long(), :c.words])
    known = arms["PDAConstraint"].n_states
    us = {k: [] for k in arms}
    for _ in range(rounds):
        torch.cuda.synchronize()
        for k, fn in step.items():
            us[k].append(_event_us(fn))
    assert arms["PDAConstraint"].n_states == known
    one = {k: s[s >= 0][:1].contiguous() for k, s in st.items()}
    fills = {k: [] for k in arms}
    for _ in range(rounds):
        for k, c in arms.items():
            _restart(c)
            torch.cuda.synchronize()
            fills[k].append(_event_us(lambda: c.mask_rows(one[k])))
    for c in arms.values():
        c.check()
    say(f"(a|b)*a(a|b){{11}}: {d.n_states} DFA states; {int((st['PDAConstraint'] >= 0).sum())} of {N} particles alive, {known} configurations "
        f"numbered, {arms['LazyConstraint'].n_states} sets")
    base = statistics.median(us["DeviceConstraint"])
    for k in arms:
        say(f"    (a) step us   {k:18s} {_spread(us[k])}   {statistics.median(us[k]) / base:.2f}x DeviceConstraint")
    base = statistics.median(fills["DeviceConstraint"])
    for k in arms:
        say(f"    (b) fill us   {k:18s} {_spread(fills[k])}   {statistics.median(fills[k]) / base:.2f}x glb_dfa_fill_masks")


def _texts(n, steps):
    """n seeded JSON texts, cut or padded with blanks to `steps` bytes where that leaves them alive: nested values, a byte a token."""
    rng = np.random.default_rng(2)

    def value(depth):
        kind = int(rng.integers(0, 10 if depth else 6))
        if kind < 2:
            return int(rng.integers(0, 1000))
        if kind < 4:
            return "".join(chr(int(c)) for c in rng.integers(97, 123, int(rng.integers(0, 6))))
        if kind < 6:
            return [None, True, False][int(rng.integers(0, 3))]
        if kind < 8:
            return [value(depth - 1) for _ in range(int(rng.integers(1, 4)))]
        return {chr(int(c)): value(depth - 1) for c in rng.integers(97, 123, int(rng.integers(1, 3)))}

    out = np.full((n, steps), 32, np.int32)
    for i in range(n):
        s = json.dumps([value(int(rng.integers(1, 6))) for _ in range(8)]).encode()[:steps]
        out[i, :len(s)] = list(s)
    return out


def nested(eng, rounds, say):
    vocab = vocabulary(V)
    eos, dev, steps = V - 1, eng.device, 48
    c = PDAConstraint(eng, BytePDA.json(), vocab, eos, skip_ids=(eos,), max_depth=32)
    tok = torch.from_numpy(_texts(N, steps + 1)).to(dev)  # (a single byte is the token of its own value)
    s = c.states0(N)
    for t in range(steps):
        s = c.advance(s, tok, *_at(dev, t))
        c.mask_rows(s)
    frm, to = _at(dev, steps)
    out = torch.empty_like(s)
    fn = lambda: c.mask_rows(c.advance(s, tok, frm, to, out=out))
    fn()
    known = c.n_states
    us, fills = [], []
    for _ in range(rounds):
        torch.cuda.synchronize()
        us.append(_event_us(fn))
    assert c.n_states == known
    deep = s[s >= 0]
    one = deep[-1:].contiguous()
    for _ in range(rounds):
        _restart(c)
        torch.cuda.synchronize()
        fills.append(_event_us(lambda: c.mask_rows(one)))
    c.check()
    configs = c.configs()
    say(f"BytePDA.json(), max_depth = 32 (W = {c.W}), {c.pda.n_states} states: a 48-step run of {N} particles over seeded JSON texts numbers "
        f"{known} configurations, the deepest stack {max(len(k) for _, k in configs)}; {int((s >= 0).sum())} particles alive")
    say(f"    (c) step us   PDAConstraint      {_spread(us)}")
    say(f"    (c) fill us   PDAConstraint      {_spread(fills)}   (the row of a stack of {len(configs[int(one[0])][1])})")


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
