"""`CpuOracleEngine` with the scoring calls of `HipEngine` (score_rows, score_seq_sums) computed by tests/score_ref.py, for the
host logic of `batch_sequence_logprobs*` without a GPU.  It records the hidden rows the head was asked for."""
import numpy as np
import torch

from tests import score_ref as SR
from tests.cpu_engine import CpuOracleEngine

_NAMES = ("logp", "lse", "logZ", "logp_masked")


class ScoreEngine(CpuOracleEngine):
    def __init__(self):
        self.score_calls = []  # rows per score_rows call

    def score_rows(self, logits, tokens, *, vocab=None, logit_scale=1.0, mask_kind=0, mask=None, row_mask_id=None, seq_start=None,
                   want=("logp",)):
        V = logits.shape[1] if vocab is None else vocab
        x = logits[:, :V].detach().to(torch.float32).numpy()
        table = None if mask is None else mask.numpy()
        ids = None if row_mask_id is None else row_mask_id.numpy()
        ref = SR.score_rows(x, tokens.numpy(), logit_scale, mask_kind, table, ids)
        self.score_calls.append(len(x))
        out = {w: torch.from_numpy(ref[:, _NAMES.index(w)].astype(np.float32)) for w in want}
        if seq_start is not None:
            for w in want:
                if w != "lse":
                    out["seq_" + w] = self.score_seq_sums(out[w], seq_start)
        return out

    def score_seq_sums(self, values, seq_start):
        return torch.from_numpy(SR.seq_sums(values.numpy(), seq_start.numpy()))


class ByteDFAConstraint:
    """The constraint interface `batch_sequence_logprobs*` walks (states0 / mask_rows / step_masks / advance / check), served
    by the CPU reference walk of tests/dfa_ref.py: bank row 0 allows nothing, row 1 EOS only, row 2 + s is state s's mask."""
    weighted = False

    def __init__(self, ref):
        self.ref = ref
        S = ref.delta.shape[0]
        rows = [ref.row_dead(), ref.row_eos()] + [ref.mask(s) for s in range(S)]
        self.bank = torch.from_numpy(np.stack(rows).view(np.int32))
        self.checked = 0
        self.mask_rows_calls = 0

    def states0(self, n):
        return torch.full((n,), self.ref.start, dtype=torch.int32)

    def mask_rows(self, states, done=None):
        self.mask_rows_calls += 1
        out = np.zeros(len(states), np.int32)
        for i, s in enumerate(states.tolist()):
            if done is not None and int(done[i]):
                out[i] = 1 if s >= 0 and self.ref.accepting[s] else 0
            else:
                out[i] = 2 + s if s >= 0 else 0
        return torch.from_numpy(out)

    def step_masks(self, logits, ids, by_row, n_particles, parity=False):
        assert by_row
        return {"mask_kind": 1, "mask": self.bank, "row_mask_id": ids}, True

    def advance(self, states, tokens, frm, to, out=None):
        st = states.tolist()
        tok = tokens.numpy()
        return torch.tensor([self.ref.advance(st[i], tok[i, int(frm[i]):int(to[i])]) for i in range(len(st))], dtype=torch.int32)

    def check(self):
        self.checked += 1
