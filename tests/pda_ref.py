"""The contract of `constraints.PDAConstraint` (include/glb.h glb_pda_*), restated in plain Python and NumPy.
Test infrastructure: the package never imports it, and it holds no device code.

  - The automaton: delta int32 [S, G + 1, 256], the middle index the top of the stack (plane 0: the empty stack); an entry is
    -1 or next | op << 24, op 0 (keep), g in 1 .. G (push g) or 127 (pop).
  - A configuration is (state, stack), the stack a `bytes`, bottom first, at most `max_depth` long.  Id 0 is (start, b"").
    The dead configuration is no state: it is -1.  A configuration accepts where its state does and its stack is empty.
  - step(c, b): the entry delta[state, top(c), b]; dead on -1, on a push at depth == max_depth, on a pop from the empty stack
    and on an entry whose fields are out of range.
  - next(c, t): step over the bytes of token t; dead for a skipped token, an empty token and an id outside [0, V).
  - `advance` walks tokens[i, frm[i] .. to[i]) from states[i]'s configuration (None: id 0).  A range outside [0, ld], frm > to
    or a state that was not numbered before the call give -1; frm == to gives the state back.  Only the configuration a
    particle ends in is numbered.
  - The new configurations of a call get consecutive ids in the order of the smallest particle index that reached them; one
    that finds every id below max_states taken gets none: its particles are -1 and `overflow` is set.
  - Row of a state: bit t where next(config, t) is not dead; the EOS bit where the configuration accepts."""
import numpy as np

POP = 127


class Ref:
    def __init__(self, pda, vocab, eos_id, skip_ids=(), max_depth=32, max_states=65536):
        self.delta = np.asarray(pda.delta, np.int64)
        self.acc = np.asarray(pda.accepting, np.bool_)
        self.S, self.G = self.delta.shape[0], self.delta.shape[1] - 1
        self.max_depth, self.max_states, self.overflow = int(max_depth), int(max_states), False
        self.order = [(int(pda.start), b"")]
        self.ids = {self.order[0]: 0}
        self.vocab = [bytes(t) for t in vocab]
        self.V, self.eos_id = len(self.vocab), int(eos_id)
        self.skip = np.zeros(self.V, np.bool_)
        self.skip[list(skip_ids)] = True

    # ---- configurations --------------------------------------------------------------------------------------------------
    def step(self, config, byte):
        state, stack = config
        top = stack[-1] if stack else 0
        if top > self.G:
            return None
        e = int(self.delta[state, top, byte])
        if e < 0:
            return None
        nxt, op = e & 0xffffff, e >> 24
        if nxt >= self.S:
            return None
        if op == 0:
            return (nxt, stack)
        if op == POP:
            return (nxt, stack[:-1]) if stack else None
        if op > self.G or len(stack) >= self.max_depth:
            return None
        return (nxt, stack + bytes([op]))

    def token(self, config, t):
        """The configuration after token t, or None: dead, or a token that is skipped, empty or outside the vocabulary."""
        if t < 0 or t >= self.V or self.skip[t] or not self.vocab[t]:
            return None
        for b in self.vocab[t]:
            config = self.step(config, b)
            if config is None:
                return None
        return config

    n_states = property(lambda self: len(self.order))

    def configs(self):
        return list(self.order)

    def accepts(self, config):
        return bool(self.acc[config[0]]) and not config[1]

    def accepting(self):
        return np.array([self.accepts(c) for c in self.order], np.bool_)

    def words(self):
        """uint64 [n_states, W]: the configurations as the device keeps them."""
        W = 1 + -(-self.max_depth // 8)
        out = np.zeros((len(self.order), W), np.uint64)
        for i, (state, stack) in enumerate(self.order):
            out[i, 0] = state | len(stack) << 32
            out[i, 1:] = np.frombuffer(stack + bytes(8 * (W - 1) - len(stack)), "<u8")
        return out

    # ---- advance: the numbering rule of one call ---------------------------------------------------------------------------
    def advance(self, states, tokens, frm, to):
        tokens = np.asarray(tokens).reshape(len(frm), -1)
        n, ld = tokens.shape
        known = len(self.order)
        out = np.full(n, -1, np.int32)
        for i in range(n):
            s = 0 if states is None else int(states[i])
            f, t = int(frm[i]), int(to[i])
            if not (0 <= s < known and 0 <= f <= t <= ld):
                continue
            if f == t:
                out[i] = s
                continue
            config = self.order[s]
            for j in range(f, t):
                config = self.token(config, int(tokens[i, j]))
                if config is None:
                    break
            if config is None:
                continue
            if config not in self.ids:
                if len(self.order) >= self.max_states:
                    self.overflow = True
                    continue
                self.ids[config] = len(self.order)
                self.order.append(config)
            out[i] = self.ids[config]
        return out

    # ---- rows ------------------------------------------------------------------------------------------------------------
    def allowed(self, s):
        """bool [V]: the row of state s."""
        config = self.order[s]
        out = np.array([self.token(config, t) is not None for t in range(self.V)], np.bool_)
        if 0 <= self.eos_id < self.V:
            out[self.eos_id] = self.accepts(config)
        return out

    def pack(self, allowed):
        bits = np.zeros((self.V + 31) // 32 * 32, np.uint8)
        bits[:self.V] = allowed
        return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)

    def mask(self, s):
        """uint32 [ceil(V / 32)]: the bank row of state s."""
        return self.pack(self.allowed(s))

    def row_dead(self):
        return self.pack(np.zeros(self.V, np.bool_))

    def row_eos(self):
        allowed = np.zeros(self.V, np.bool_)
        allowed[self.eos_id] = True
        return self.pack(allowed)
