"""Time the constrained draw-and-advance of one byte step at V = 50257, without a model: glb_bytelm_step against
the same step composed from the calls there were before it.

    python tools/bytelm_step_ab.py [--out profiles/r33/bytelm_step_ab.txt]

For n x width = 16 x 16 and 64 x 16, on the state `tools/bytelm_ab.py` builds (synthetic bfloat16 rows, candidates at random
inner nodes of a synthetic 50257-token trie) after its children / masses / extend / children / masses - what both paths
share.  Timed, between stream events, as medians over `--iters` steps after a warm-up, the two paths taking turns step by
step and the beam's state put back outside the events:
  (a) composed: bytelm_next (rows), a mask from delta[state] and live, the masked row renormalised by log_softmax,
      torch.multinomial, bytelm_next(byte=), the state gather and the weight update - COMPOSED_OPS lists what is enqueued;
  (b) bytelm_step: one launch (and the allocation of its two outputs)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bytelm_ab import vocab  # noqa: E402

COMPOSED_OPS = ["glb_bytelm_next (rows)", "delta[state]", "clamp", "live[target]", "target >= 0", "and", "accepting[state]", "cat",
                "where (mask)", "logsumexp", "subtract", "exp", "compare", "where (rows without mass)", "multinomial", "to int32", "glb_bytelm_next (byte)", "gather target",
                "where (EOS: -1)", "log_weight +="]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import genlm_backend_amd  # noqa: F401
    from genlm_backend_amd.bytelm import byte_trie, byte_trie_arrays
    from genlm_backend_amd.constraints import ByteDFA
    from genlm_backend_amd.constraints.tables import DeviceTables
    from genlm_backend_amd.engine import HipEngine

    eng = HipEngine("cuda:0")
    dev, V, width = eng.device, 50257, 16
    trie = byte_trie(vocab(V), [0], engine=eng)
    host = byte_trie_arrays(trie)
    tdev = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in host.items()}
    inner = np.array([n for n, kids in enumerate(trie.children) if kids], np.int32)
    tables = DeviceTables.upload(eng, ByteDFA.from_regex(rb"([a-z]+ )*[a-z]+"))
    live = tables.live.bool()
    lines = [f"constrained draw and advance at V = {V}, width {width}, bfloat16 rows, {args.iters} steps (median, us); "
             f"device: {torch.cuda.get_device_name(0)}"]
    for n in (16, 64):
        N = n * width
        rng = np.random.default_rng(n)
        store = (torch.randn((N, V), device=dev) * 3).to(torch.bfloat16)
        lse = eng.row_lse(store, vocab=V)
        node = torch.from_numpy(inner[rng.integers(0, len(inner), N)]).to(dev)
        alive = torch.ones(N, dtype=torch.int32, device=dev)
        u = torch.from_numpy((-8 * rng.random(N)).astype(np.float32)).to(dev)
        sel = eng.bytelm_children(tdev, node, alive, width)
        o = eng.bytelm_extend(tdev, node, u, u.clone(), alive, sel, trie.masses_from_logits(store, lse=lse, nodes=sel), width)
        sel2 = eng.bytelm_children(tdev, o["node"], o["alive"], width)
        mass2 = trie.masses_from_logits(store, lse=lse, nodes=sel2)
        keep = {k: o[k].clone() for k in ("node", "w", "alive")}
        state0 = torch.full((n,), tables.start, dtype=torch.int32, device=dev)
        st = dict(state=state0.clone(), ended=torch.zeros(n, dtype=torch.int32, device=dev), lw=torch.zeros(n, device=dev),
                  logp=torch.zeros(n, device=dev))
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        ninf, ones = torch.full((n, 257), float("-inf"), device=dev), torch.ones((n, 257), device=dev)

        def restore():
            for k in keep:
                o[k].copy_(keep[k])
            st["state"].copy_(state0)
            st["ended"].zero_()
            st["lw"].zero_()

        def composed():
            row, _ = eng.bytelm_next(tdev, o["node"], o["u"], o["w"], o["alive"], sel2, mass2, width)
            s = st["state"].long()
            to = tables.delta[s]
            ok = live[to.clamp_min(0).long()] & (to >= 0)
            allow = torch.cat([ok, tables.accepting[s].bool()[:, None]], dim=1)
            lc = torch.where(allow, row, ninf)
            logZc = torch.logsumexp(lc, dim=1, keepdim=True)
            p = torch.where(logZc > float("-inf"), (lc - logZc).exp(), ones)  # (a row without mass still needs something to draw from)
            byte = torch.multinomial(p, 1, generator=gen)
            b32 = byte[:, 0].to(torch.int32)
            eng.bytelm_next(tdev, o["node"], o["u"], o["w"], o["alive"], sel2, mass2, width, byte=b32, logp=st["logp"])
            nxt = torch.gather(to, 1, byte.clamp_max(255))[:, 0]
            st["state"] = torch.where(b32 == 256, torch.full_like(nxt, -1), nxt)
            st["lw"] += logZc[:, 0]

        def fused():
            eng.bytelm_step(tdev, o["node"], o["u"], o["w"], o["alive"], sel2, mass2, width, tables, st["state"], st["ended"], st["lw"],
                            st["logp"], seed=1, offset=0)

        times = {"a": [], "b": []}
        for i in range(args.iters + 10):
            for name, fn in (("a", composed), ("b", fused)) if i % 2 == 0 else (("b", fused), ("a", composed)):
                restore()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                times[name].append((e0, e1))
        torch.cuda.synchronize()
        med = {k: float(np.median([a.elapsed_time(b) for a, b in v[10:]])) * 1e3 for k, v in times.items()}
        lines.append(f"n x width = {n} x {width}: (a) composed {med['a']:.0f} us, {len(COMPOSED_OPS)} device operations | "
                     f"(b) glb_bytelm_step {med['b']:.0f} us, 1 launch | (a) / (b) = {med['a'] / med['b']:.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
