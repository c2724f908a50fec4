"""`DeviceBeam` and `batch_next_token_topk*` on the GPU over a tiny random GPT-2 (vocab 257: EOS and the 256
bytes; 2 layers, n_embd 64; tests/test_wfsa_gpu.py's `_model`, weights seeded with 3).

A device search and a host search can only be asked for the same hypotheses where the host's own numbers are not near a tie,
so every comparison of ids first asserts, on the reference's float64 numbers, that the values whose order decides the outcome
differ by more than GAP = 1e-3 (a float32 log-probability of this model is within 1e-4 of the reference's: TOL of
tests/test_score_gpu.py) - and fails, not skips, if they do not.  PROMPTS / API_CONTEXTS were chosen by running `host_beam`
on the CPU copy of the seed-3 model (torch.manual_seed(3); AutoModelForCausalLM.from_config) over 50 candidate prompts:
smallest gap seen there 3.1e-3 (beam, width 4, k 4, 5 tokens), 4.9e-3 (greedy over PROMPTS[0]), 8.4e-3 (API rows, k 5)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAP = 1e-3
EOS = 0
PROMPTS = [[72, 209, 172, 1], [197], [52, 195, 242, 13]]
API_CONTEXTS = [[5, 17, 99], [9, 10], [101, 102], [9, 10], [164, 131, 70, 79], [5, 17, 99]]


@pytest.fixture(scope="module")
def model(engine):
    from tests.test_wfsa_gpu import _model

    return _model(engine, 257)


def _rows(model, contexts):
    """float64 [n, V] next-token log-probabilities through the existing API."""
    return np.stack([torch.as_tensor(r).double().cpu().numpy() for r in model.batch_next_token_logprobs_sync(contexts)])


def host_beam(rows_of, prompts, width, k, max_tokens, eos=EOS):
    """Beam search on the host in float64 under DeviceBeam's rules: per live beam its k best tokens (equal values by lower
    id), per group the `width` best of score + logp over them and of the finished hypotheses' scores, ties by lower (b, j);
    no constraint: a hypothesis of max_tokens tokens stays alive.  Returns (per group [(tokens, score, alive)], the smallest gap
    between values whose order matters: the k-th / (k + 1)-th key of a live row, neighbours among a group's first width + 1
    candidates)."""
    groups = [[(tuple(), 0.0, True)] for _ in prompts]
    gap = np.inf
    for _ in range(max_tokens):
        live = [(g, b) for g, beams in enumerate(groups) for b, h in enumerate(beams) if h[2]]
        if not live:
            break
        rows = rows_of([list(prompts[g]) + list(groups[g][b][0]) for g, b in live])
        row_of = {gb: rows[i] for i, gb in enumerate(live)}
        for g, beams in enumerate(groups):
            cands = []
            for b, (toks, score, alive) in enumerate(beams):
                if not alive:
                    cands.append((score, b, 0, -1))
                    continue
                lp = row_of[(g, b)]
                order = np.argsort(-lp, kind="stable")
                if len(lp) > k:
                    gap = min(gap, lp[order[k - 1]] - lp[order[k]])
                cands += [(score + lp[t], b, j, int(t)) for j, t in enumerate(order[:k])]
            cands.sort(key=lambda c: -c[0])  # (stable: ties keep (b, j) order)
            for a, b_ in zip(cands[:width], cands[1:width + 1]):
                gap = min(gap, a[0] - b_[0])
            new = []
            for value, b, j, t in cands[:width]:
                toks = beams[b][0]
                new.append((toks, value, False) if t < 0 or t == eos else (toks + (t,), value, True))
            groups[g] = new
    return groups, gap


def _device(beam):
    out = beam.results()
    act = beam.active[beam.result_slots].cpu().numpy().reshape(beam.G, beam.width)
    return [[(tuple(t), float(s), bool(a)) for t, s, a in zip(toks, scores.cpu().numpy(), act[g])] for g, (toks, scores) in enumerate(out)]


def test_against_a_host_beam(model):
    from genlm_backend_amd import DeviceBeam

    want, gap = host_beam(lambda c: _rows(model, c), PROMPTS, 4, 4, 5)
    print("host beam: smallest gap", gap)
    assert gap > GAP, gap
    beam = DeviceBeam(model, 4, PROMPTS, 5, EOS, k=4)
    assert 1 <= beam.run() <= 5
    got = _device(beam)
    for g in range(len(PROMPTS)):
        fin = [h for h in got[g] if np.isfinite(h[1])]
        assert [h[0] for h in fin] == [h[0] for h in want[g]], (g, fin, want[g])
        assert [h[2] for h in fin] == [h[2] for h in want[g]], g
        err = max(abs(a[1] - b[1]) for a, b in zip(fin, want[g]))
        print(f"group {g}: max |score - host| = {err:.3g}")
        assert err <= 1e-3
    beam.reset()  # a second run gives the same hypotheses and the same score bits
    beam.run()
    assert _device(beam) == got


def test_width_one_is_greedy(model):
    from genlm_backend_amd import DeviceBeam

    toks, total, gap = [], 0.0, np.inf
    for _ in range(6):
        lp = _rows(model, [PROMPTS[0] + toks])[0]
        order = np.argsort(-lp, kind="stable")
        gap = min(gap, lp[order[0]] - lp[order[1]])
        if order[0] == EOS:
            total += lp[order[0]]
            break
        toks.append(int(order[0]))
        total += lp[order[0]]
    print("greedy: smallest gap", gap)
    assert gap > GAP, gap
    beam = DeviceBeam(model, 1, PROMPTS[0], 6, EOS)
    assert beam.k == 1
    beam.run()
    (ctx, scores), = beam.results()
    assert ctx[0] == toks and abs(float(scores[0]) - total) <= 1e-3


def _text(tokens):
    return bytes(t - 1 for t in tokens)


def _rescore(model, prompt, tokens):
    return float(model.batch_sequence_logprobs_sync([prompt], [list(tokens) + [EOS]]).logprobs[0])


def test_device_constraint_on_a_finite_language(model):
    from genlm_backend_amd import DeviceBeam
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint
    from genlm_backend_amd.sis import DeviceSIS
    from tests.test_wfsa_gpu import _byte_vocab

    strings = [b"abcd", b"cdabx", b"ab", b"z", b"cdab"]
    make = lambda: DeviceConstraint(model, ByteDFA.from_strings(strings), _byte_vocab(), EOS, skip_ids=(EOS,))
    prompt = [5, 17, 99]
    beam = DeviceBeam(model, 8, prompt, 6, EOS, constraint=make())
    beam.run()
    (ctx, scores), = beam.results()
    scores = scores.cpu().numpy()
    act = beam.active[beam.result_slots].cpu().numpy()
    found = {}
    for toks, s, a in zip(ctx, scores, act):
        if np.isfinite(s):
            assert a == 0 and _text(toks) in strings, (toks, s, a)
            assert abs(s - _rescore(model, prompt, toks)) <= 1e-3, (toks, s)
            found[_text(toks)] = s
    assert set(found) == set(strings)  # (never more than 8 live prefixes: the beam is exhaustive here)
    assert list(scores[:5]) == sorted(scores[:5], reverse=True) and np.isneginf(scores[5:]).all()
    sis = DeviceSIS(model, 256, prompt, 6, EOS, seed=11, constraint=make())
    sis.run()
    texts, lw = sis.results()
    seen = {tuple(int(t) for t in tx) for tx, w in zip(texts, lw) if np.isfinite(w)}
    assert seen and all(_text(t) in strings for t in seen)
    best = max(_rescore(model, prompt, t) for t in seen)
    print("beam best", scores[0], "best particle text", best)
    assert scores[0] >= best - 1e-3


def test_pda_constraint_gives_json(model):
    from genlm_backend_amd import DeviceBeam
    from genlm_backend_amd.constraints import BytePDA, PDAConstraint
    from tests.test_wfsa_gpu import _byte_vocab

    con = PDAConstraint(model, BytePDA.json(), _byte_vocab(), EOS, skip_ids=(EOS,), max_depth=4)
    beam = DeviceBeam(model, 8, [[5, 17, 99], [6, 7]], 12, EOS, constraint=con)
    beam.run()
    n = 0
    for g, (ctx, scores) in enumerate(beam.results()):
        for toks, s in zip(ctx, scores.cpu().numpy()):
            if np.isfinite(s):
                json.loads(_text(toks).decode("utf-8"))
                n += 1
    assert n >= 2 and int(beam.active.sum()) == 0


def test_weighted_lexicon(model):
    from genlm_backend_amd import DeviceBeam
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint
    from tests.test_wfsa_gpu import _byte_vocab

    lex = {b"abc": -0.5, b"ab": -2.0, b"abcab": -0.1, b"cab": -1.0, b"cabba": -3.0, b"bb": -0.7, b"bca": -1.3, b"ba": -0.2}
    con = DeviceConstraint(model, ByteWFSA.from_weighted_strings(lex), _byte_vocab(), EOS, skip_ids=(EOS,))
    assert con.weighted
    prompt = [9, 10]
    beam = DeviceBeam(model, 8, prompt, 6, EOS, constraint=con)
    beam.run()
    (ctx, scores), = beam.results()
    n = 0
    for toks, s in zip(ctx, scores.cpu().numpy()):
        if np.isfinite(s):
            want = _rescore(model, prompt, toks) + lex[_text(toks)]
            assert abs(s - want) <= 1e-3, (_text(toks), s, want)
            n += 1
    assert n == len(lex) and int(beam.active.sum()) == 0


def test_topk_api_against_the_logprob_rows(model):
    import asyncio

    k = 5
    lp = _rows(model, API_CONTEXTS)
    order = np.argsort(-lp, axis=1, kind="stable")[:, :k + 1]
    vals = np.take_along_axis(lp, order, 1)
    gap = (vals[:, :-1] - vals[:, 1:]).min()
    print("api rows: smallest gap among the first k + 1", gap)
    assert gap > GAP, gap
    tok, val = model.batch_next_token_topk_sync(API_CONTEXTS, k)
    assert tok.dtype == torch.int32 and val.dtype == torch.float32 and tok.shape == val.shape == (len(API_CONTEXTS), k)
    assert np.array_equal(tok.cpu().numpy(), order[:, :k])
    assert np.abs(val.cpu().numpy() - vals[:, :k]).max() <= 2e-4
    assert torch.equal(tok[1], tok[3]) and torch.equal(val[1].view(torch.int32), val[3].view(torch.int32))  # duplicated contexts
    assert torch.equal(tok[0], tok[5]) and torch.equal(val[0].view(torch.int32), val[5].view(torch.int32))
    t2, v2 = asyncio.run(model.batch_next_token_topk(API_CONTEXTS, k))
    assert torch.equal(t2, tok) and torch.equal(v2, val)
    # the device form: the same contexts as a padded matrix; at temperature 2 the ids stay, the values are softmax(x / 2)'s
    mat = torch.zeros((len(API_CONTEXTS), 8), dtype=torch.int32, device=model.device)
    for i, c in enumerate(API_CONTEXTS):
        mat[i, :len(c)] = torch.tensor(c, dtype=torch.int32)
    lens = torch.tensor([len(c) for c in API_CONTEXTS], dtype=torch.int32, device=model.device)
    t3, v3 = model.batch_next_token_topk_device(mat, lens, k)
    assert torch.equal(t3, tok) and float((v3 - val).abs().max()) <= 2e-4
    with pytest.raises(ValueError, match="k must"):
        model.batch_next_token_topk_sync(API_CONTEXTS, 0)
    with pytest.raises(ValueError, match="temperature"):
        model.batch_next_token_topk_sync(API_CONTEXTS, 2, temperature=0.0)
