"""`ConstraintProduct`: the conjunction of 2 to 8 constraints - `DeviceConstraint`, `LazyConstraint`,
`PDAConstraint` or another product - served as one from the device (include/glb.h glb_conj_*).  No product automaton is made:
a state is the tuple of the parts' states, numbered on the device when a particle ends a call in it, and its bank row is
combined from the parts' rows; the same duck type as its parts."""
import ctypes as C

import numpy as np

from .. import _lib
from .device import _BIT_BANK, _FLOAT_BANK, _Bank, DeviceConstraint
from .lazy import LazyConstraint
from .pda import PDAConstraint

_MAX_TUPLES = 1 << 22
_CHUNK = 1 << 20  # the particles one chunk of glb_conj_number takes at the most


class ConstraintProduct(_Bank):
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

    def __init__(self, llm_or_engine, parts, max_states=65536, mask_bank_bytes=256 << 20, on_full="error", *, _hash_mask=0):
        if on_full not in ("error", "evict"):
            raise ValueError(f'on_full must be "error" or "evict", got {on_full!r}')
        if isinstance(max_states, bool) or not isinstance(max_states, (int, np.integer)) or not 1 <= max_states <= _MAX_TUPLES:
            raise ValueError(f"max_states must be an int in [1, {_MAX_TUPLES}], got {max_states!r}")
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
        self.max_states, self.mask_bank_bytes, self.on_full = int(max_states), int(mask_bank_bytes), on_full
        self.weighted = any(p.weighted for p in parts)
        self.start_logw = float(sum(p.start_logw for p in parts))
        self.vocab, self.eos_id, self.words, self.n_bytes = first.vocab, first.eos_id, first.words, first.n_bytes
        self._bytes, self._ptr, self._gathered, self._cus = first._bytes, first._ptr, None, None
        self._kind = kind = _FLOAT_BANK if self.weighted else _BIT_BANK
        self.row_elems = kind.row_elems(self.vocab)
        rows = int(getattr(_lib.load(), kind.rows)(self.mask_bank_bytes, self.vocab, self.max_states))
        if rows < 3:
            raise ValueError(f"mask_bank_bytes={mask_bank_bytes} holds no state's mask: a row of this vocabulary takes "
                             f"{self.row_elems * 4} bytes{' (float32 weights: 32 times a bit row)' if self.weighted else ''} "
                             "and the bank needs at least three")
        self.eng, self.dev = eng, eng.device
        self._hash_mask = int(_hash_mask)
        self._start = [int(p.states0(1).item()) for p in parts]  # (DeviceConstraint starts at dfa.start, not at 0)
        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=self.dev)
        self._slots = 1 << max(1, (2 * self.max_states - 1).bit_length())
        self._table = new(torch.int64, self._slots * 12 // 8)
        self._tuples, self._rep = new(torch.int64, self.max_states, self.W), new(torch.int32, self.max_states)
        self._status = torch.zeros(_lib.CONJ_STATUS, dtype=torch.int32, device=self.dev)
        self._counts = self._part_states = self._claim = self._zeros = None
        self._row_of_state = new(torch.int32, self.max_states)
        self._counters = torch.zeros(_lib.DFA_COUNTERS, dtype=torch.int32, device=self.dev)
        self.bank = torch.zeros((rows, self.row_elems), dtype=getattr(torch, kind.dtype), device=self.dev)
        self._work = torch.zeros((rows, 2), dtype=torch.int32, device=self.dev)
        self._evicting = on_full == "evict" and self.max_states + 2 > rows
        self._evict_tables = self._new_evict_tables() if self._evicting else None
        self._call("glb_conj_init", self._block())

    # ---- the blocks ----------------------------------------------------------------------------------------------------
    def _args(self):
        """The embedded glb_dfa_args: the vocabulary's size, the bank's bookkeeping; nothing of an automaton."""
        a = _lib.DfaArgs()
        a.struct_size = C.sizeof(_lib.DfaArgs)
        a.n_states, a.start, a.eos_id, a.vocab = self.max_states, 0, self.eos_id, self.vocab
        if not self.weighted:
            a.bank, a.bank_ld = self.bank.data_ptr(), self.bank.stride(0)
        a.capacity = self.bank.shape[0]
        a.row_of_state, a.work, a.counters = self._row_of_state.data_ptr(), self._work.data_ptr(), self._counters.data_ptr()
        return a

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
    def states0(self, n):
        import torch

        return torch.zeros(n, dtype=torch.int32, device=self.dev)

    def advance(self, states, tokens, frm, to, out=None):
        """The states after tokens[i, frm[i] .. to[i]) (int32 [n, ld], unit inner stride), from states[i] (None: state 0);
        -1 once a part is dead, for a state that is none of the states numbered before the call, and for a tuple that found
        no id below `max_states`.  One launch, the parts' own `advance` calls, five launches (glb_conj_unpack,
        glb_conj_number)."""
        import torch

        if tokens.dtype != torch.int32 or tokens.dim() != 2 or tokens.device != self.dev:
            raise ValueError("tokens must be an int32 [n, ld] tensor on the engine's device")
        tokens = tokens.contiguous()
        n = tokens.shape[0]
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.dev)
        if n == 0:
            return out
        for t in (frm, to):
            if t.dtype != torch.int32 or t.shape != (n,) or t.device != self.dev or not t.is_contiguous():
                raise ValueError("frm / to must be contiguous int32 [n] tensors on the engine's device")
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
        if done is not None and (done.dtype != torch.int32 or done.shape != (n,) or not done.is_contiguous() or done.device != self.dev):
            raise ValueError("done must be a contiguous int32 [n] tensor on the engine's device")
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
    @property
    def n_states(self):
        """The tuples numbered so far."""
        return int(self._status[0].item())

    def tuples(self):
        """Host list of K-tuples of part state ids, one for every numbered state."""
        halves = np.ascontiguousarray(self._tuples[:self.n_states].cpu().numpy()).view(np.int32).reshape(-1, 2 * self.W)
        return [tuple(int(v) for v in row[:self.K]) for row in halves]

    def stats(self):
        """`DeviceConstraint.stats()` and "states": the tuples numbered so far (synchronises)."""
        return dict(super().stats(), states=self.n_states)

    def check(self, word=None):
        """Raises when a tuple found no id below `max_states`, what `DeviceConstraint.check` raises for the product's own bank,
        and then whatever every part's `check()` raises.  Always synchronises, `word` given or not."""
        flags = int(self._status[1].item())
        if flags & _lib.CONJ_BUG:
            raise RuntimeError(f"ConstraintProduct: the table held a reference out of range (flags {flags})")
        if flags & _lib.CONJ_OVERFLOW:
            raise RuntimeError(f"the particles reached more than max_states={self.max_states} distinct tuples of the parts' states: "
                               "the ones beyond got no id, and their particles were served the empty mask.  Raise max_states.")
        super().check(word)
        for part in self.parts:
            part.check()
