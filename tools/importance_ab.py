"""A/B of glb_importance_step against the composition the library already had.

    kernel       HipEngine.importance_step: two launches, both matrices read once
    composition  HipEngine.step on the proposal rows (the draw, logZ, lse), HipEngine.log_softmax_rows on the target rows
                 ([N, V] written and read back), torch gathers for p_tok and q_tok

Shapes: 1024 x 50257 float32 and 512 x 128256 bfloat16, each with a separate proposal matrix and without one; masks per row
(two bit masks, ids per logits row) and per particle (a bank of 64 bit rows, ids per particle).  Runs alternate - kernel,
composition, kernel, ... - and each is timed with a pair of HIP events around it on the stream; the table gives the median
and the range of the repeats.  The floor is both matrices read once at 8 TB/s.

    python tools/importance_ab.py [--reps 20] [--out profiles/r26/importance_ab.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26", "importance_ab.txt"))
    args = ap.parse_args()
    import genlm_backend_amd  # noqa: F401
    from genlm_backend_amd._lib import MASK_BITS
    from genlm_backend_amd.engine import HipEngine

    eng = HipEngine("cuda:0")
    dev = eng.device
    lines = [f"{'shape':<22}{'proposal':<10}{'masks':<14}{'kernel us':>22}{'composition us':>24}{'floor us':>10}{'max |d|':>10}"]
    for n, V, dtype in ((1024, 50257, torch.float32), (512, 128256, torch.bfloat16)):
        g = torch.Generator(device=dev).manual_seed(V)
        p = (2 * torch.randn((n, V), generator=g, device=dev)).to(dtype)
        q_sep = (2 * torch.randn((n, V), generator=g, device=dev)).to(dtype)
        words = (V + 31) // 32
        bank = torch.randint(-2 ** 31, 2 ** 31 - 1, (64, words), generator=g, device=dev, dtype=torch.int64).to(torch.int32)
        ids_row = (torch.arange(n, device=dev) % 2).to(torch.int32)
        ids_particle = torch.randint(0, 64, (n,), generator=g, device=dev).to(torch.int32)
        row_of = torch.arange(n, dtype=torch.int32, device=dev)
        prepared = eng.prepare_masks(bank[:2].contiguous(), V, dtype)
        es = p.element_size()
        for q in (q_sep, None):
            for masks in ("per row", "per particle"):
                if masks == "per row":
                    kw_k = dict(mask_kind=MASK_BITS, mask=bank[:2], row_mask_id=ids_row)
                    kw_c = dict(mask=prepared, row_mask_id=ids_row)
                else:
                    kw_k = dict(mask_kind=MASK_BITS, mask=bank, mask_id=ids_particle)
                    kw_c = dict(mask_kind=MASK_BITS, mask=bank, mask_id=ids_particle)
                src = p if q is None else q

                def kernel():
                    return eng.importance_step(p, q, vocab=V, row_of=row_of, seed=1, offset=2, **kw_k)[0]

                def composition():
                    logZ, lse, tok = eng.step(src, vocab=V, row_of=row_of, rng_mode=1, seed=1, offset=2, **kw_c)
                    lp = eng.log_softmax_rows(p)
                    at = tok.clamp_min(0).long().unsqueeze(1)
                    log_qt = src.gather(1, at).squeeze(1).float() - lse - logZ
                    return torch.where(tok >= 0, lp.gather(1, at).squeeze(1).float() - log_qt, torch.full_like(logZ, float("-inf")))

                times = {"k": [], "c": []}
                for rep in range(args.warmup + args.reps):
                    for name, fn in (("k", kernel), ("c", composition)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        out = fn()
                        e1.record()
                        e1.synchronize()
                        if rep >= args.warmup:
                            times[name].append(e0.elapsed_time(e1) * 1e3)
                eng.check()
                # the two draw from the same distribution by different walks: compare what does not depend on the token,
                # and only with no proposal (dlogw = logZ then)
                d = float("nan")
                if q is None:
                    a, b = kernel(), composition()
                    fin = torch.isfinite(a) & torch.isfinite(b)
                    d = float((a[fin] - b[fin]).abs().max())
                floor = n * V * es * (1 if q is None else 2) / 8e12 * 1e6
                fmt = lambda t: f"{np.median(t):8.1f} ({min(t):.1f} - {max(t):.1f})"
                lines.append(f"{f'{n} x {V} {str(dtype)[6:]}':<22}{'separate' if q is not None else 'none':<10}{masks:<14}"
                             f"{fmt(times['k']):>22}{fmt(times['c']):>24}{floor:>10.1f}{d:>10.1e}")
                print(lines[-1], flush=True)
        del p, q_sep
    text = "\n".join(lines) + f"\n(median (min - max) of {args.reps} alternating repeats, HIP events around each call; floor: the logits read once at 8 TB/s)\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
