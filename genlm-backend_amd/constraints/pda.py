"""`BytePDA` and `PDAConstraint`: a real-time deterministic pushdown automaton over bytes - nested brackets,
JSON - and the constraint that serves it from the device (include/glb.h glb_pda_*).  A state of the constraint is a
configuration, the automaton's state and a bounded stack, numbered on the device when a particle ends a call in it; the same
duck type as `DeviceConstraint` and `LazyConstraint`."""
import ctypes as C

import numpy as np

from .. import _lib
from .automata import ByteDFA, ByteWFSA
from .numbered import _Numbered
from .tables import _put

POP = _lib.PDA_POP
_MAX_AUTOMATON = 1 << 24


def _entry(nxt, op=0):
    return nxt | op << 24


def _json_tables():
    """(delta, accepting, start) of `BytePDA.json()` as written down by hand, before `trim()`."""
    names = ["value", "arr_first", "obj_first", "obj_key", "colon", "after",
             "minus", "zero", "int", "dot", "frac", "e", "esign", "exp",
             "t1", "t2", "t3", "f1", "f2", "f3", "f4", "n1", "n2", "n3"]
    string = ["s", "esc", "u1", "u2", "u3", "u4", "c1", "c2", "c3", "e0", "ed", "f0", "f4x"]
    names += ["k_" + s for s in string] + ["v_" + s for s in string]  # a key's string and a value's: what follows differs
    q = {name: i for i, name in enumerate(names)}
    OBJ, ARR = 1, 2
    delta = np.full((len(names), 3, 256), -1, np.int32)
    ws, digits, hexes = b" \t\n\r", b"0123456789", b"0123456789abcdefABCDEF"

    def arc(src, bs, dst, op=0, planes=(0, OBJ, ARR)):
        for p in planes:
            delta[q[src], p, list(bs)] = _entry(q[dst], op)

    def value(src, planes=(0, OBJ, ARR)):  # the first byte of a value
        for bs, dst, op in ((b'"', "v_s", 0), (b"-", "minus", 0), (b"0", "zero", 0), (b"123456789", "int", 0), (b"t", "t1", 0),
                            (b"f", "f1", 0), (b"n", "n1", 0), (b"{", "obj_first", OBJ), (b"[", "arr_first", ARR)):
            arc(src, bs, dst, op, planes)

    def end(src):  # what may follow a finished value
        arc(src, ws, "after")
        arc(src, b",", "obj_key", planes=(OBJ,)), arc(src, b"}", "after", POP, planes=(OBJ,))
        arc(src, b",", "value", planes=(ARR,)), arc(src, b"]", "after", POP, planes=(ARR,))

    arc("value", ws, "value"), value("value")
    arc("arr_first", ws, "arr_first", planes=(ARR,)), arc("arr_first", b"]", "after", POP, planes=(ARR,))
    value("arr_first", planes=(ARR,))  # (reached with an array on top only)
    arc("obj_first", ws, "obj_first", planes=(OBJ,)), arc("obj_first", b'"', "k_s", planes=(OBJ,))
    arc("obj_first", b"}", "after", POP, planes=(OBJ,))
    arc("obj_key", ws, "obj_key", planes=(OBJ,)), arc("obj_key", b'"', "k_s", planes=(OBJ,))
    arc("colon", ws, "colon", planes=(OBJ,)), arc("colon", b":", "value", planes=(OBJ,))
    end("after")
    # numbers: -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?
    arc("minus", b"0", "zero"), arc("minus", b"123456789", "int")
    arc("int", digits, "int")
    for src in ("zero", "int"):
        arc(src, b".", "dot"), arc(src, b"eE", "e"), end(src)
    arc("dot", digits, "frac"), arc("frac", digits, "frac"), arc("frac", b"eE", "e"), end("frac")
    arc("e", b"+-", "esign"), arc("e", digits, "exp"), arc("esign", digits, "exp"), arc("exp", digits, "exp"), end("exp")
    for word, first in ((b"true", "t1"), (b"false", "f1"), (b"null", "n1")):
        at = first
        for i, b in enumerate(word[1:], 2):
            nxt = "after" if i == len(word) else first[0] + str(i)
            arc(at, bytes([b]), nxt)
            at = nxt
    for k, closed in (("k_", "colon"), ("v_", "after")):
        s = k + "s"
        arc(s, bytes(b for b in range(0x20, 0x80) if b not in b'"\\'), s)
        arc(s, b'"', closed), arc(s, b"\\", k + "esc")
        arc(k + "esc", b'"\\/bfnrt', s), arc(k + "esc", b"u", k + "u1")
        for i in (1, 2, 3, 4):
            arc(k + f"u{i}", hexes, s if i == 4 else k + f"u{i + 1}")
        # UTF-8: C2 .. DF one more byte; E0 A0 .. BF, E1 .. EC, ED 80 .. 9F, EE .. EF two; F0 90 .. BF, F1 .. F3, F4 80 .. 8F three
        cont = bytes(range(0x80, 0xc0))
        arc(s, bytes(range(0xc2, 0xe0)), k + "c1"), arc(s, b"\xe0", k + "e0"), arc(s, b"\xed", k + "ed")
        arc(s, bytes(b for b in range(0xe1, 0xf0) if b != 0xed), k + "c2")
        arc(s, b"\xf0", k + "f0"), arc(s, b"\xf1\xf2\xf3", k + "c3"), arc(s, b"\xf4", k + "f4x")
        arc(k + "c1", cont, s), arc(k + "c2", cont, k + "c1"), arc(k + "c3", cont, k + "c2")
        arc(k + "e0", bytes(range(0xa0, 0xc0)), k + "c1"), arc(k + "ed", bytes(range(0x80, 0xa0)), k + "c1")
        arc(k + "f0", bytes(range(0x90, 0xc0)), k + "c2"), arc(k + "f4x", bytes(range(0x80, 0x90)), k + "c2")
    accepting = np.zeros(len(names), np.bool_)
    accepting[[q[n] for n in ("after", "zero", "int", "frac", "exp")]] = True
    return delta, accepting, q["value"]


class BytePDA:
    """A deterministic pushdown automaton that reads one byte a step (no empty moves).

    delta      int32 [S, G + 1, 256], the middle index the top of the stack: plane 0 the empty stack, planes 1 .. G the stack
               symbols, 1 <= G <= 126.  An entry is -1 (dead) or next | op << 24: next in [0, S), S <= 2^24; op 0 (keep), g
               in 1 .. G (push symbol g) or 127 (pop).  A pop in plane 0 is refused.
    accepting  bool [S]
    start      in [0, S)

    A byte string is accepted when its walk from (start, the empty stack) never dies and ends in an accepting state with an
    EMPTY stack.  A configuration is (state, stack) with the stack a `bytes`, bottom first."""

    def __init__(self, delta, accepting, start):
        delta, accepting = np.asarray(delta), np.asarray(accepting)
        if delta.dtype != np.int32:
            raise ValueError(f"delta must be int32, got {delta.dtype}")
        if delta.ndim != 3 or delta.shape[2] != 256 or delta.shape[0] == 0 or not 2 <= delta.shape[1] <= _lib.PDA_MAX_SYMBOLS + 1:
            raise ValueError(f"delta must be [S, G + 1, 256] with S >= 1 and 1 <= G <= {_lib.PDA_MAX_SYMBOLS}, got {delta.shape}")
        S, G = delta.shape[0], delta.shape[1] - 1
        if S > _MAX_AUTOMATON:
            raise ValueError(f"delta has {S} states: next takes 24 bits of an entry, at most {_MAX_AUTOMATON} states")
        if delta.min() < -1:
            raise ValueError("delta entries must be -1 or next | op << 24")
        on = delta >= 0
        nxt, op = delta & 0xffffff, delta >> 24
        if (nxt[on] >= S).any():
            raise ValueError(f"delta holds a next outside [0, {S})")
        if ((op > G) & (op < POP) & on).any():
            raise ValueError(f"delta holds an op in ({G}, {POP}): neither keep (0), a push of a symbol in 1 .. {G}, nor pop ({POP})")
        if ((op[:, 0, :] == POP) & on[:, 0, :]).any():
            raise ValueError("delta holds a pop in plane 0, the empty stack")
        if accepting.shape != (S,):
            raise ValueError(f"accepting must be [{S}], got {accepting.shape}")
        if accepting.dtype != np.bool_:
            raise ValueError(f"accepting must be bool, got {accepting.dtype}")
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= int(start) < S:
            raise ValueError(f"start must be an int in [0, {S})")
        self.delta, self.accepting, self.start = np.ascontiguousarray(delta), np.ascontiguousarray(accepting), int(start)
        self.n_states, self.n_symbols = S, G

    # ---- the walk ------------------------------------------------------------------------------------------------------
    def step(self, config, byte, max_depth):
        """The configuration after `byte` from `config` = (state, stack bytes), or None: no entry, or a push at depth
        `max_depth`."""
        if config is None:
            return None
        state, stack = config
        e = int(self.delta[state, stack[-1] if stack else 0, byte])
        if e < 0:
            return None
        nxt, op = e & 0xffffff, e >> 24
        if op == POP:
            return (nxt, stack[:-1])  # (never in plane 0)
        if op:
            return (nxt, stack + bytes([op])) if len(stack) < max_depth else None
        return (nxt, stack)

    def accepts(self, data, max_depth):
        """Whether the walk over `data` stays alive with at most `max_depth` symbols on the stack and ends in an accepting
        state with the empty stack."""
        config = (self.start, b"")
        for b in bytes(data):
            config = self.step(config, b, max_depth)
            if config is None:
                return False
        return bool(self.accepting[config[0]]) and not config[1]

    # ---- trimming ------------------------------------------------------------------------------------------------------
    def _live_pairs(self):
        """bool [S, G + 1]: the pairs (state, top) from which acceptance may be reached (see `trim`)."""
        S, G = self.n_states, self.n_symbols
        on = self.delta >= 0
        nxt, op = self.delta & 0xffffff, np.where(on, self.delta >> 24, -1)
        # distinct moves (q, g) -> (q', op), bytes forgotten
        moves = {k: set() for k in ("keep", "push", "pop")}
        for q, g, b in zip(*np.nonzero(on)):
            o = int(op[q, g, b])
            moves["keep" if o == 0 else "pop" if o == POP else "push"].add((int(q), int(g), int(nxt[q, g, b]), o))
        # pops_to[(q, h)]: the states a run from (q, h) that never goes below its h may pop that h into
        pops_to = {(q, h): set() for q in range(S) for h in range(1, G + 1)}
        for q, g, q2, _ in moves["pop"]:
            pops_to[(q, g)].add(q2)
        changed = True
        while changed:
            changed = False
            for q, g, q2, _ in moves["keep"]:
                if g and not pops_to[(q2, g)] <= pops_to[(q, g)]:
                    pops_to[(q, g)] |= pops_to[(q2, g)]
                    changed = True
            for q, g, q1, k in moves["push"]:
                if g:
                    for q2 in list(pops_to[(q1, k)]):
                        if not pops_to[(q2, g)] <= pops_to[(q, g)]:
                            pops_to[(q, g)] |= pops_to[(q2, g)]
                            changed = True
        live = np.zeros((S, G + 1), np.bool_)
        live[:, 0] = self.accepting
        changed = True
        while changed:
            changed = False
            for q, g, q2, _ in moves["keep"]:
                if live[q2, g] and not live[q, g]:
                    live[q, g] = changed = True
            for q, g, q1, k in moves["push"]:  # the summary edge: push k, a run that pops it again, back on g
                if not live[q, g] and any(live[q2, g] for q2 in pops_to[(q1, k)]):
                    live[q, g] = changed = True
            for q, g, q2, _ in moves["pop"]:  # the top that a pop uncovers is not known: any will do
                if not live[q, g] and live[q2].any():
                    live[q, g] = changed = True
        return live

    def trim(self):
        """A copy in which every keep or push entry whose target pair (state, resulting top) cannot reach acceptance under
        any stack is -1.

        The limits of this.  It is a fixed point over (state, top) pairs, not over configurations: a pair is kept when an
        accepting state on the empty stack is reachable from it over keep entries, over pop-summary edges - a push, a run
        that stays above it, the pop of what was pushed - and over pop entries into ANY top.  That is necessary, not
        sufficient, for a configuration with that state and top to be live: what lies deeper in the stack may still
        strand it.  Pop entries are left alone, because the top that a pop uncovers is not known statically.  The depth
        bound of `accepts` and `PDAConstraint` is ignored: a pair that is live only through a deeper stack than a caller's
        `max_depth` stays."""
        live = self._live_pairs()
        delta = self.delta.copy()
        on = delta >= 0
        nxt, op = delta & 0xffffff, delta >> 24
        top = np.where(op == 0, np.arange(self.n_symbols + 1)[None, :, None], op)  # the top after a keep or a push
        dead = on & (op != POP)
        dead[dead] = ~live[nxt[dead], top[dead]]
        delta[dead] = -1
        return BytePDA(delta, self.accepting.copy(), self.start)

    # ---- constructors ----------------------------------------------------------------------------------------------------
    @classmethod
    def from_dfa(cls, dfa):
        """`dfa` as a pushdown automaton that never touches its stack: G = 1, both planes the automaton's table."""
        if isinstance(dfa, ByteWFSA):
            raise ValueError("BytePDA takes unweighted automata: a ByteWFSA's weights would be lost")
        if not isinstance(dfa, ByteDFA):
            raise ValueError(f"from_dfa needs a ByteDFA, got {type(dfa).__name__}")
        return cls(np.repeat(dfa.delta[:, None, :], 2, axis=1).astype(np.int32), dfa.accepting.copy(), dfa.start)

    @classmethod
    def dyck(cls, pairs, other=b""):
        """Balanced brackets: one state; each (open, close) byte pair pushes and pops its own symbol, the bytes of `other`
        keep, everything else is dead."""
        pairs = [(bytes(o), bytes(c)) for o, c in pairs]
        used = b"".join(o + c for o, c in pairs) + bytes(other)
        if not 1 <= len(pairs) <= _lib.PDA_MAX_SYMBOLS or any(len(o) != 1 or len(c) != 1 for o, c in pairs) or len(set(used)) != len(used):
            raise ValueError(f"dyck needs 1 .. {_lib.PDA_MAX_SYMBOLS} pairs of single bytes, all bytes (those of `other` too) distinct")
        delta = np.full((1, len(pairs) + 1, 256), -1, np.int32)
        delta[0, :, list(bytes(other))] = _entry(0)
        for g, (o, c) in enumerate(pairs, 1):
            delta[0, :, o[0]] = _entry(0, g)
            delta[0, g, c[0]] = _entry(0, POP)
        return cls(delta, np.ones(1, np.bool_), 0)

    @classmethod
    def json(cls):
        """One RFC 8259 value with whitespace round it, what `json.loads` takes of UTF-8 bytes without `NaN` and `Infinity`:
        objects push symbol 1, arrays symbol 2, `,` and the closers branch on the top plane; a number is ended by the byte
        that follows it, and at top level a number state accepts on the empty stack; strings carry the escapes, \\uXXXX and
        well-formed UTF-8 (no byte below 0x20, no overlong form, no surrogate, nothing above F4 8F).  The nesting depth of a
        value is what the stack holds: `accepts(text, d)` takes values nested at most d deep, `[]` being one deep."""
        # a key's string lives inside an object: with anything else on top its states lead nowhere, which trim() finds
        return cls(*_json_tables()).trim()


class PDAConstraint(_Numbered):
    """A `BytePDA` over a vocabulary's byte strings, served from the device.

    A state is a configuration of the automaton: its state and a stack of at most `max_depth` symbols, W = 1 +
    ceil(max_depth / 8) 64-bit words (word 0: state | depth << 32; then the stack, a byte a symbol, bottom first, zero above
    the depth).  State 0 is (start, the empty stack); the dead configuration is no state but -1.  `advance` walks every
    particle's tokens byte by byte from its state's configuration - a missing entry, a push at depth `max_depth`, a skipped
    or empty token kill the walk - and numbers only the configuration it ends in: within a call the new ones get consecutive
    ids in the order of the smallest particle index that reached them, across calls the ids go on upward.  A state's bank
    row has bit t set where token t can be walked from the configuration, and the EOS bit where its state accepts and its
    stack is empty.  A set bit says that the walk survives the token, not that the text can still be completed: see
    `BytePDA.trim` for what is cut beforehand.

    llm_or_engine, byte_vocab, eos_id, skip_ids, mask_bank_bytes, on_full
                     as `DeviceConstraint` has them; the states of the bank are the ids [0, max_states).
    pda              a `BytePDA`.
    max_depth        an int in [1, 504]: the symbols a stack may hold; a deeper nesting is dead.
    max_states       an int in [1, 2^22]: the configurations that get an id.  One beyond gets none - its particles are -1 and
                     are served the empty mask - and `check()` raises.  Allocated at once: W words and a byte a state, and
                     a hash table of 12 bytes a slot, 2 * max_states slots rounded up to a power of two.

    `n_states`, `configs()` synchronise, as `stats()` and `check()` do; nothing else does."""

    _distinct, _beyond = "configurations of the automaton", "ones"

    def __init__(self, llm_or_engine, pda, byte_vocab, eos_id, skip_ids=None, max_depth=32, max_states=65536, mask_bank_bytes=256 << 20,
                 on_full="error", *, _hash_mask=0):
        self._check_on_full(on_full)
        if not isinstance(pda, BytePDA):
            raise ValueError(f"PDAConstraint needs a BytePDA (BytePDA.from_dfa takes a ByteDFA), got {type(pda).__name__}")
        if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or not 1 <= max_depth <= _lib.PDA_MAX_DEPTH:
            raise ValueError(f"max_depth must be an int in [1, {_lib.PDA_MAX_DEPTH}], got {max_depth!r}")
        self._check_max_states(max_states)
        V = len(byte_vocab)
        if V == 0:
            raise ValueError("empty vocabulary")
        self.max_depth = int(max_depth)
        self.W = 1 + -(-self.max_depth // 8)
        rows = self._size_bank(V, max_states, mask_bank_bytes, on_full)
        import torch

        eng = getattr(llm_or_engine, "engine", llm_or_engine)
        self.eng, self.dev, self.pda = eng, eng.device, pda
        self._upload_vocab(llm_or_engine, byte_vocab, eos_id, skip_ids)
        self.max_token_bytes = max(1, max(len(bytes(getattr(t, "byte_string", t))) for t in byte_vocab))
        self._hash_mask = int(_hash_mask)
        self._delta, self._acc = _put(eng, pda.delta), _put(eng, pda.accepting.astype(np.uint8))
        new = self._allocate(rows)
        self._configs, self._accepting = new(torch.int64, self.max_states, self.W), new(torch.uint8, self.max_states)
        self._call("glb_pda_init", self._block())

    # ---- the blocks ----------------------------------------------------------------------------------------------------
    def _block(self, a=None):
        p = _lib.PdaArgs()
        p.struct_size, p.dfa = C.sizeof(_lib.PdaArgs), self._args() if a is None else a
        p.n_pda_states, p.n_symbols, p.start = self.pda.n_states, self.pda.n_symbols, self.pda.start
        p.max_depth, p.n_words, p.max_states = self.max_depth, self.W, self.max_states
        p.delta, p.accepting, p.hash_mask = self._delta.data_ptr(), self._acc.data_ptr(), self._hash_mask
        p.table, p.table_slots = self._table.data_ptr(), self._slots
        p.configs, p.accepting_out, p.status = self._configs.data_ptr(), self._accepting.data_ptr(), self._status.data_ptr()
        p.max_token_bytes = self.max_token_bytes
        if self._cand is not None:
            p.cand, p.counts, p.cand_rows = self._cand.data_ptr(), self._counts.data_ptr(), self._cand.shape[0]
        if self._evicting:
            self._evict_fields(p)
        return p

    def _call(self, name, p):
        self.eng.pda_call(name, p)

    # ---- states --------------------------------------------------------------------------------------------------------
    def advance(self, states, tokens, frm, to, out=None):
        """The states after tokens[i, frm[i] .. to[i]) (int32 [n, ld], unit inner stride), from states[i] (None: state 0);
        -1 once dead, for a state that is none of the states numbered before the call, and for a configuration that found
        no id below `max_states`.  Six launches for every chunk of particles whose end configurations fit 64 MB
        (glb_pda_advance)."""
        return self._advance_walk("glb_pda_advance", states, tokens, frm, to, out)

    def mask_rows(self, states, done=None):
        """int32 [n]: the bank row of every state, as `DeviceConstraint.mask_rows` gives it - the rows that are missing
        claimed (under on_full="evict" in a bank smaller than `max_states`: taken from the states requested longest ago)
        and filled from the states' configurations first, one call (glb_pda_serve); no host synchronisation.  `states` are
        ids that `advance` or `states0` returned: an id below `max_states` that no configuration has yet is served row 0
        like a dead state, and costs a bank that does not evict one row for good."""
        return self._serve("glb_pda_serve", states, done)

    # ---- inspection (every call synchronises) ------------------------------------------------------------------------------
    def configs(self):
        """Host list of (state, stack bytes), one for every numbered state."""
        words = np.ascontiguousarray(self._configs[:self.n_states].cpu().numpy().view(np.uint64))
        out = []
        for row in words:
            state, depth = int(row[0]) & 0xffffffff, int(row[0]) >> 32
            out.append((state, row[1:].tobytes()[:depth]))
        return out
