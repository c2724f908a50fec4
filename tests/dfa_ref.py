"""The contract of the byte-level DFA constraints (include/glb.h glb_dfa_*), restated in NumPy by brute force: every state
against every token, byte by byte.  Test infrastructure: the product never imports it."""
import numpy as np


def live(delta, accepting):
    """live[s]: an accepting state is reachable from s, s included (forward search from every state)."""
    S = delta.shape[0]
    out = np.zeros(S, np.bool_)
    for s in range(S):
        seen, todo = {s}, [s]
        while todo:
            u = todo.pop()
            if accepting[u]:
                out[s] = True
                break
            for v in set(int(x) for x in delta[u] if x >= 0):
                if v not in seen:
                    seen.add(v)
                    todo.append(v)
    return out


class Ref:
    def __init__(self, delta, accepting, start, vocab, eos_id, skip_ids=()):
        self.delta = np.asarray(delta, np.int64)
        self.accepting = np.asarray(accepting, np.bool_)
        self.start, self.eos_id = int(start), int(eos_id)
        self.live = live(self.delta, self.accepting)
        self.vocab = [bytes(t) for t in vocab]
        self.V = len(self.vocab)
        self.W = (self.V + 31) // 32
        self.skip = np.zeros(self.V, np.bool_)
        for t in skip_ids:
            self.skip[t] = True
        self.lens = np.array([len(t) for t in self.vocab], np.int64)
        self.padded = np.zeros((self.V, max(1, int(self.lens.max()))), np.int64)
        for i, t in enumerate(self.vocab):
            self.padded[i, :len(t)] = list(t)

    def next(self, s, t):
        """next(s, t) for one state and one token id, byte by byte."""
        if s < 0 or t < 0 or t >= self.V or self.skip[t] or len(self.vocab[t]) == 0:
            return -1
        for b in self.vocab[t]:
            s = int(self.delta[s, b])
            if s < 0:
                return -1
        return s if self.live[s] else -1

    def next_all(self, s):
        """next(s, t) for every token t (all tokens walked side by side, one byte position at a time)."""
        cur = np.full(self.V, s, np.int64)
        for j in range(self.padded.shape[1]):
            on = (j < self.lens) & (cur >= 0)
            cur = np.where(on, self.delta[np.maximum(cur, 0), self.padded[:, j]], cur)
        ok = (cur >= 0) & (self.lens > 0) & ~self.skip
        ok &= self.live[np.maximum(cur, 0)]
        return np.where(ok, cur, -1) if s >= 0 else np.full(self.V, -1, np.int64)

    def _pack(self, allowed):
        bits = np.zeros(self.W * 32, np.uint8)
        bits[:self.V] = allowed
        return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)

    def mask(self, s):
        """uint32 [ceil(V / 32)]: the mask row of state s."""
        allowed = self.next_all(s) >= 0
        if 0 <= self.eos_id < self.V:
            allowed[self.eos_id] = bool(self.accepting[s]) if s >= 0 else False
        return self._pack(allowed)

    def row_dead(self):
        return np.zeros(self.W, np.uint32)

    def row_eos(self):
        allowed = np.zeros(self.V, np.bool_)
        allowed[self.eos_id] = True
        return self._pack(allowed)

    def particle_mask(self, s, n_generated, max_tokens):
        """The mask of a particle in state s that has generated n_generated tokens."""
        if n_generated >= max_tokens:
            return self.row_eos() if s >= 0 and self.accepting[s] else self.row_dead()
        return self.mask(s) if s >= 0 else self.row_dead()

    def advance(self, s, tokens):
        for t in tokens:
            s = self.next(s, int(t))
        return s


def synth_vocab(V, seed):
    """(vocab, eos_id, skip_ids): all 256 single bytes, an empty token, a skipped special, an EOS (skipped too, as tokenizers
    list it among their special ids), and tokens of 2 .. 70 bytes over a small alphabet, many grown out of earlier ones."""
    assert V >= 300
    rng = np.random.default_rng(seed)
    vocab = [bytes([b]) for b in range(256)] + [b"", b"<special>", b"<eos>"]
    eos_id, skip = 258, (257, 258)
    alphabet = b"0123456789abyesno"
    pick = lambda chars, n: bytes(rng.choice(np.frombuffer(chars, np.uint8), n))
    fixed = [b"ye", b"yes", b"no", b"yesno", b"12", b"123", b"0" * 70, b"9" * 69 + b"a"]
    vocab += fixed
    while len(vocab) < V:
        n = int(rng.integers(2, 71)) if rng.random() < 0.2 else int(rng.integers(2, 6))
        if rng.random() < 0.5:
            base = vocab[int(rng.integers(259, len(vocab)))]
            tok = (base + pick(alphabet, max(1, n - len(base))))[:70]
        else:
            tok = pick(alphabet[:10] if rng.random() < 0.5 else alphabet, n)
        vocab.append(tok)
    return vocab, eos_id, skip


def automata(seed=0):
    """name -> (delta, accepting, start): the automata of tests/test_dfa_gpu.py."""
    out = {}
    d = np.full((2, 256), -1, np.int32)
    d[0, 48:58] = 1
    d[1, 48:58] = 1
    out["digits"] = (d, np.array([False, True]), 0)  # [0-9]+
    out["everything"] = (np.zeros((1, 256), np.int32), np.array([True]), 0)
    d = np.full((4, 256), -1, np.int32)  # state 2 is a trap, state 3 reaches only the trap: neither is live
    d[0, ord("y")], d[0, ord("n")], d[0, ord("0")] = 1, 2, 3
    d[1, :] = 1
    d[2, :] = 2
    d[3, :] = 2
    out["trap"] = (d, np.array([False, True, False, False]), 0)
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 37, (37, 256)).astype(np.int32)
    d[rng.random((37, 256)) < 0.3] = -1
    acc = rng.random(37) < 0.2
    acc[5] = True
    out["random37"] = (d, acc, 3)
    return out
