"""`ConstraintProduct`: the conjunction of 2 to 8 constraints - `DeviceConstraint`, `LazyConstraint`,
`PDAConstraint` or another product - served as one from the device (include/glb.h glb_conj_*).  No product automaton is made:
a state is the tuple of the parts' states, numbered on the device when a particle ends a call in it, and its bank row is
combined from the parts' rows; the same duck type as its parts."""
import ctypes as C

import numpy as np

from .. import _lib
from .device import DeviceConstraint
from .lazy import LazyConstraint
from .numbered import _Numbered
from .pda import PDAConstraint

_CHUNK = 1 << 20  # the particles one chunk of glb_conj_number takes at the most


class ConstraintProduct(_Numbered):
    """The conjunction of `parts`: a token is allowed exactly where every part allows it, and weighs what the weighted parts
    make it weigh together.

    llm_or_engine    as the parts have it: an `AsyncAmdLM` or a `HipEngine`, the one every part was made on.
    parts            a sequence of 2 to 8 `DeviceConstraint`, `LazyConstraint`, `PDAConstraint` or `ConstraintProduct` objects
                     (products nest), all over the same engine, vocabulary bytes and `eos_id`, no object twice.  A part may
                     also be used alone or in another product at the same time: the product calls its `advance` and
                     `mask_rows` on state arrays of its own and keeps nothing in it, so only the lifetime of its row ids, as
                     documented on `DeviceConstraint`, applies - the rows a part's `mask_rows` call returned are good until the
                     next such call on that part, and the product reads them before it returns.
    max_states       an int in [1, 2^22]: the tuples that get an id.  One beyond gets none - its particles are -1 and are
                     served the empty mask - and `check()` raises.  Allocated at once: W = ceil(K / 2) 64-bit words and an
                     int32 a state, and a hash table of 12 bytes a slot, 2 * max_states slots rounded up to a power of two.
    mask_bank_bytes, on_full
                     as `DeviceConstraint` has them, for the product's own bank: bit rows, or float32 rows when a part is
                     weighted.  The states of the bank are the ids [0, max_states).

    A state is the tuple of the K part states, int32 each, two to a 64-bit word (part 2 j in the low half of word j; for odd K
    the upper half of the last word is zero).  State 0 is the tuple of every part's `states0(1)`; a tuple with a dead part is
    no state but -1.  `advance` unpacks the states (one launch), calls every part's own `advance`, and numbers the tuples that
    come out (five launches): within a call the new ones get consecutive ids in the order of the smallest particle index
    that reached them, across calls the ids go on upward.  `mask_rows` unpacks, takes every part's `mask_rows` - the parts
    claim, fill and evict as they do alone - and serves: a state without a row claims one, filled from the part rows of one
    particle that holds it - bit rows ANDed; with weights the float32 sum of the weighted parts' rows in part order from 0.0f,
    -inf where an unweighted part's bit is clear.  Where `done` is set the row is 1 when every part served its row 1, else 0.

    `weighted` is true when a part is; `start_logw` is the sum of the parts'; `forced_final_logw` the sum of the weighted parts'
    in part order.  `n_states`, `tuples()`, `stats()` and `check()` synchronise; nothing else does, and nothing allocates
    after the first call of a given size."""

    _distinct, _beyond = "tuples of the parts' states", "ones"
    _walks = False  # (the parts walk the vocabulary)

    def __init__(self, llm_or_engine, parts, max_states=65536, mask_bank_bytes=256 << 20, on_full="error", *, _hash_mask=0):
        self._check_on_full(on_full)
        self._check_max_states(max_states)
        parts = list(parts)
        if not 2 <= len(parts) <= _lib.CONJ_MAX_PARTS:
            raise ValueError(f"a product takes 2 to {_lib.CONJ_MAX_PARTS} parts, got {len(parts)}")
        eng = getattr(llm_or_engine, "engine", llm_or_engine)
        first = parts[0]
        for k, p in enumerate(parts):
            if not isinstance(p, (DeviceConstraint, LazyConstraint, PDAConstraint, ConstraintProduct)):
                raise ValueError(f"part {k} is a {type(p).__name__}: a product takes DeviceConstraint, LazyConstraint, PDAConstraint and "
                                 "ConstraintProduct objects")
            if any(p is q for q in parts[:k]):
                raise ValueError(f"part {k} is the same object as an earlier part: a constraint is given once")
            if p.eng is not eng or p.dev != getattr(eng, "device", None):
                raise ValueError(f"part {k} was made on a different engine or device than the product's")
            if p.vocab != first.vocab or p.eos_id != first.eos_id:
                raise ValueError(f"part {k} has vocab={p.vocab}, eos_id={p.eos_id}; part 0 has vocab={first.vocab}, eos_id={first.eos_id}")
        import torch

        for k, p in enumerate(parts[1:], 1):  # (once, here: a synchronisation)
            if p._ptr.shape != first._ptr.shape or p._bytes.shape != first._bytes.shape or not torch.equal(p._ptr, first._ptr) \
                    or not torch.equal(p._bytes, first._bytes):
                raise ValueError(f"part {k}'s vocabulary bytes differ from part 0's")
        self.parts, self.K, self.W = parts, len(parts), (len(parts) + 1) // 2
        self.weighted = any(p.weighted for p in parts)
        self.start_logw = float(sum(p.start_logw for p in parts))
        self.vocab, self.eos_id, self.words, self.n_bytes = first.vocab, first.eos_id, first.words, first.n_bytes
        self._bytes, self._ptr, self._gathered, self._cus = first._bytes, first._ptr, None, None
        rows = self._size_bank(self.vocab, max_states, mask_bank_bytes, on_full)
        self.eng, self.dev = eng, eng.device
        self._hash_mask = int(_hash_mask)
        self._start = [int(p.states0(1).item()) for p in parts]  # (DeviceConstraint starts at dfa.start, not at 0)
        new = self._allocate(rows)
        self._tuples, self._rep = new(torch.int64, self.max_states, self.W), new(torch.int32, self.max_states)
        self._part_states = self._claim = None
        self._call("glb_conj_init", self._block())

    # ---- the blocks ----------------------------------------------------------------------------------------------------
    def _block(self, a=None):
        p = _lib.ConjArgs()
        p.struct_size, p.dfa = C.sizeof(_lib.ConjArgs), self._args() if a is None else a
        p.n_parts, p.n_words, p.max_states, p.hash_mask = self.K, self.W, self.max_states, self._hash_mask
        for k, s in enumerate(self._start):
            p.part_start[k] = s
        p.table, p.table_slots = self._table.data_ptr(), self._slots
        p.tuples, p.status, p.rep = self._tuples.data_ptr(), self._status.data_ptr(), self._rep.data_ptr()
        if self._part_states is not None:
            p.part_states, p.part_ld = self._part_states.data_ptr(), self._part_states.stride(0)
            p.counts, p.cand_rows = self._counts.data_ptr(), self._chunk
        if self.weighted:
            p.wbank, p.wbank_ld = self.bank.data_ptr(), self.bank.stride(0)
        if self._evicting:
            self._evict_fields(p)
        return p

    def _call(self, name, p):
        self.eng.conj_call(name, p)

    def _scratch(self, n):
        """The [K, n] part states, the [n] claim states and the chunk counts, kept and grown only."""
        import torch

        if self._part_states is None or self._part_states.shape[1] < n:
            self._part_states = torch.empty((self.K, n), dtype=torch.int32, device=self.dev)
            self._claim = torch.empty(n, dtype=torch.int32, device=self.dev)
            self._chunk = int(max(1, min(n, _CHUNK, self._slots - self.max_states)))
            self._counts = torch.empty(-(-self._chunk // 256), dtype=torch.int32, device=self.dev)

    def _unpack(self, states, n, done=None, claim=False):
        """K contiguous int32 [n] views of the scratch: every particle's part states (one launch)."""
        self._scratch(n)
        a = self._args()
        a.n, a.state_in = n, None if states is None else self._states(states).data_ptr()
        if claim and done is not None:
            a.done = done.data_ptr()
        p = self._block(a)
        if claim:
            p.claim_states = self._claim.data_ptr()
        self._call("glb_conj_unpack", p)
        return [self._part_states[k, :n] for k in range(self.K)]

    # ---- states --------------------------------------------------------------------------------------------------------
    def advance(self, states, tokens, frm, to, out=None):
        """The states after tokens[i, frm[i] .. to[i]) (int32 [n, ld], unit inner stride), from states[i] (None: state 0);
        -1 once a part is dead, for a state that is none of the states numbered before the call, and for a tuple that found
        no id below `max_states`.  One launch, the parts' own `advance` calls, five launches (glb_conj_unpack,
        glb_conj_number)."""
        tokens, out = self._check_advance_args(tokens, frm, to, out)
        n = tokens.shape[0]
        if n == 0:
            return out
        for part, s in zip(self.parts, self._unpack(states, n)):
            part.advance(s, tokens, frm, to, out=s)
        a = self._args()
        a.n, a.state_out = n, out.data_ptr()
        self._call("glb_conj_number", self._block(a))
        return out

    def mask_rows(self, states, done=None):
        """int32 [n]: the bank row of every state, as `DeviceConstraint.mask_rows` gives it: the parts' own `mask_rows` calls
        over the unpacked states, then one call (glb_conj_serve) in which the states without a row claim one - under
        on_full="evict" in a bank smaller than `max_states`, from the states requested longest ago - and the new rows are
        combined from the parts' rows.  Where `done` is set: row 1 when every part served its row 1, else row 0.  `states`
        are ids that `advance` or `states0` returned: an id that no tuple has yet is served row 0 like a dead state and claims
        nothing.  No host synchronisation."""
        import torch

        n = states.numel()
        out = torch.empty(n, dtype=torch.int32, device=self.dev)
        if n == 0:
            return out
        self._check_done(done, n)
        rows = [part.mask_rows(s, done=done) for part, s in zip(self.parts, self._unpack(states, n, done, claim=True))]
        a = self._args()
        a.n, a.state_in, a.out_rows = n, self._states(states).data_ptr(), out.data_ptr()
        if done is not None:
            a.done = done.data_ptr()
        a.max_work = min(n, self.max_states, self.capacity - 2)
        p = self._block(a)
        p.claim_states = self._claim.data_ptr()
        for k, (part, r) in enumerate(zip(self.parts, rows)):
            p.part_rows[k], p.part_bank[k] = r.data_ptr(), part.bank.data_ptr()
            p.part_bank_ld[k], p.part_capacity[k], p.part_weighted[k] = part.bank.stride(0), part.bank.shape[0], int(part.weighted)
        self._call("glb_conj_serve", p)
        return out

    def forced_final_logw(self, states, forced):
        """float32 [n]: what a particle made to end in `states[i]` (`forced`: it was served row 1) still has to weigh - the sum,
        in part order, of the weighted parts' `forced_final_logw` on the unpacked part states; 0.0 elsewhere.  One launch and
        the parts' own; no synchronisation."""
        import torch

        n = states.numel()
        total = torch.zeros(n, dtype=torch.float32, device=self.dev)
        if n == 0 or not self.weighted:
            return total
        for part, s in zip(self.parts, self._unpack(states, n)):
            if part.weighted:
                total = total + part.forced_final_logw(s, forced)
        return total

    # ---- inspection (every call synchronises) ------------------------------------------------------------------------------
    def tuples(self):
        """Host list of K-tuples of part state ids, one for every numbered state."""
        halves = np.ascontiguousarray(self._tuples[:self.n_states].cpu().numpy()).view(np.int32).reshape(-1, 2 * self.W)
        return [tuple(int(v) for v in row[:self.K]) for row in halves]

    def check(self, word=None):
        """Raises when a tuple found no id below `max_states`, what `DeviceConstraint.check` raises for the product's own bank,
        and then whatever every part's `check()` raises.  Always synchronises, `word` given or not."""
        super().check(word)
        for part in self.parts:
            part.check()
