"""Time one byte step of the byte-level beam's device side at V = 50257, without a model.

    python tools/bytelm_ab.py [--out profiles/r32/bytelm_ab.txt]

For n x width = 16 x 16 and 64 x 16: synthetic bfloat16 logits rows stand in for the store, the candidates stand at random
inner nodes of a synthetic 50257-token trie.  A step here is what `ByteBeam` launches per byte apart from the forward:
children, masses, extend, children, masses, next.  Reported, as medians of CUDA-event times over `--iters` steps after a warm-up:
the whole step, the three new kernels alone, the two `masses_from_logits` calls alone, and the same selection and
normalisation composed in PyTorch on the same masses (`gather` / `topk` / `logsumexp`)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def vocab(V, seed=0):
    rng = np.random.default_rng(seed)
    out, seen = [b"<eos>"] + [bytes([b]) for b in range(256)], set()
    alphabet = np.frombuffer(b"etaoinshrdlu ", np.uint8)
    while len(out) < V:
        wd = bytes(rng.choice(alphabet, int(rng.integers(2, 9))))
        if wd not in seen:
            seen.add(wd)
            out.append(wd)
    return out


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import genlm_backend_amd  # noqa: F401
    from genlm_backend_amd.bytelm import byte_trie, byte_trie_arrays
    from genlm_backend_amd.engine import HipEngine

    eng = HipEngine("cuda:0")
    dev, V, width = eng.device, 50257, 16
    trie = byte_trie(vocab(V), [0], engine=eng)
    host = byte_trie_arrays(trie)
    tdev = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in host.items()}
    inner = np.array([n for n, kids in enumerate(trie.children) if kids], np.int32)
    lines = [f"byte step at V = {V}, width {width}, bfloat16 rows, {args.iters} steps (median, us); device: {torch.cuda.get_device_name(0)}"]
    for n in (16, 64):
        N = n * width
        rng = np.random.default_rng(n)
        store = (torch.randn((N, V), device=dev) * 3).to(torch.bfloat16)
        lse = eng.row_lse(store, vocab=V)
        node = torch.from_numpy(inner[rng.integers(0, len(inner), N)]).to(dev)
        alive = torch.ones(N, dtype=torch.int32, device=dev)
        u = torch.from_numpy((-8 * rng.random(N)).astype(np.float32)).to(dev)
        w = u.clone()
        st = {}

        def masses(s):
            return trie.masses_from_logits(store, lse=lse, nodes=s)

        def step():
            st["sel"] = eng.bytelm_children(tdev, node, alive, width)
            st["mass"] = masses(st["sel"])
            st["out"] = o = eng.bytelm_extend(tdev, node, u, w, alive, st["sel"], st["mass"], width)
            st["sel2"] = eng.bytelm_children(tdev, o["node"], o["alive"], width)
            st["mass2"] = masses(st["sel2"])
            st["row"] = eng.bytelm_next(tdev, o["node"], o["u"], o["w"], o["alive"], st["sel2"], st["mass2"], width)

        step()

        def kernels():
            eng.bytelm_children(tdev, node, alive, width)
            o = eng.bytelm_extend(tdev, node, u, w, alive, st["sel"], st["mass"], width)
            eng.bytelm_children(tdev, o["node"], o["alive"], width)
            eng.bytelm_next(tdev, o["node"], o["u"], o["w"], o["alive"], st["sel2"], st["mass2"], width)

        def two_masses():
            masses(st["sel"])
            masses(st["sel2"])

        def in_torch():  # the same selection and normalisation on the same masses
            m, o = st["mass"], st["out"]
            offers = (u[:, None] + m[:, 256:].clamp_min(1e-45).log()).masked_fill(st["sel"][:, 256:] < 0, float("-inf"))
            cand = torch.cat([w.view(n, width), offers.view(n, width * 4)], dim=1)
            top = cand.topk(width, dim=1)
            parent = torch.where(top.indices < width, top.indices, (top.indices - width) // 4)
            torch.gather(node.view(n, width), 1, parent)
            m2 = st["mass2"].view(n, width, 260)
            lw = o["u"].view(n, width, 1) + m2[:, :, :256].clamp_min(1e-45).log()
            num = torch.logsumexp(lw, dim=1)
            return num - torch.logsumexp(num, dim=1, keepdim=True)

        t_step, t_k, t_m, t_t = timed(step, args.iters), timed(kernels, args.iters), timed(two_masses, args.iters), timed(in_torch, args.iters)
        lines.append(f"n x width = {n} x {width}: step {t_step:.0f} | children + extend + children + next {t_k:.0f} ({100 * t_k / t_step:.0f} %) | "
                     f"two masses_from_logits {t_m:.0f} ({100 * t_m / t_step:.0f} %) | selection + rows in PyTorch {t_t:.0f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
