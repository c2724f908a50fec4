"""`_Numbered`: what the constraints share whose states are numbered on the device when a particle reaches them -
`LazyConstraint` (a set of NFA states), `PDAConstraint` (a configuration), `ConstraintProduct` (a tuple of part states).  Each is
W 64-bit words a state, looked up in one hash table (12 bytes a slot, 2 * max_states slots rounded up to a power of two) and
given a dense int32 id; the bank of rows over the ids [0, max_states) is `_Bank`'s."""
import ctypes as C

import numpy as np

from .. import _lib
from .device import _BIT_BANK, _FLOAT_BANK, _Bank

_CAND_BYTES = 64 << 20  # what the end states of one chunk of particles may take: W words a particle
_OVERFLOW, _BUG = 1, 2  # the flags of status word 1, the same in the three blocks
assert (_lib.LAZY_OVERFLOW, _lib.LAZY_BUG) == (_lib.PDA_OVERFLOW, _lib.PDA_BUG) == (_lib.CONJ_OVERFLOW, _lib.CONJ_BUG) == (_OVERFLOW, _BUG)
assert _lib.LAZY_STATUS == _lib.PDA_STATUS == _lib.CONJ_STATUS


class _Numbered(_Bank):
    """A subclass sets `_distinct` and `_beyond` (what `check()` calls its states), `_walks` (whether it uploads a vocabulary and
    walks it: `_args()` then carries the vocabulary's bytes), `W`, its automaton and the states' rows ([max_states, W] int64),
    and has `_block(a)`, the library's block round the embedded `glb_dfa_args`, and `_call(name, block)`.  Its `__init__`
    runs, in this order: `_check_on_full`, `_check_max_states`, `_size_bank`, its own uploads, `_allocate`, and last its
    `*_init` entry."""

    weighted = False
    start_logw = 0.0
    _max_states_most = 1 << 22
    _distinct, _beyond = "states", "ones"
    _walks = True

    # ---- __init__'s steps ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_on_full(on_full):
        if on_full not in ("error", "evict"):
            raise ValueError(f'on_full must be "error" or "evict", got {on_full!r}')

    @classmethod
    def _check_max_states(cls, max_states):
        if isinstance(max_states, bool) or not isinstance(max_states, (int, np.integer)) or not 1 <= max_states <= cls._max_states_most:
            raise ValueError(f"max_states must be an int in [1, {cls._max_states_most}], got {max_states!r}")

    def _size_bank(self, V, max_states, mask_bank_bytes, on_full):
        """`max_states`, `mask_bank_bytes`, `on_full`, `_kind` (by `weighted`) and `row_elems`; returns the rows the bank gets."""
        self.max_states, self.mask_bank_bytes, self.on_full = int(max_states), int(mask_bank_bytes), on_full
        self._kind = kind = _FLOAT_BANK if self.weighted else _BIT_BANK
        self.row_elems = kind.row_elems(V)
        rows = int(getattr(_lib.load(), kind.rows)(self.mask_bank_bytes, V, self.max_states))
        if rows < 3:
            raise ValueError(f"mask_bank_bytes={mask_bank_bytes} holds no state's mask: a row of this vocabulary takes "
                             f"{self.row_elems * 4} bytes{' (float32 weights: 32 times a bit row)' if self.weighted else ''} "
                             "and the bank needs at least three")
        return rows

    def _allocate(self, rows):
        """The table, the status words, the row map, the counters, the bank of `rows` rows, its work list and, where the bank
        evicts, its tables; returns `new(dtype, *shape)` for the subclass's own arrays."""
        import torch

        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=self.dev)
        self._slots = 1 << max(1, (2 * self.max_states - 1).bit_length())
        self._table = new(torch.int64, self._slots * 12 // 8)
        self._status = torch.zeros(_lib.LAZY_STATUS, dtype=torch.int32, device=self.dev)
        self._cand = self._counts = None
        self._row_of_state = new(torch.int32, self.max_states)
        self._counters = torch.zeros(_lib.DFA_COUNTERS, dtype=torch.int32, device=self.dev)
        self.bank = torch.zeros((rows, self.row_elems), dtype=getattr(torch, self._kind.dtype), device=self.dev)
        self._work = torch.zeros((rows, 2), dtype=torch.int32, device=self.dev)
        self._evicting = self.on_full == "evict" and self.max_states + 2 > rows
        self._evict_tables = self._new_evict_tables() if self._evicting else None
        return new

    # ---- the blocks ----------------------------------------------------------------------------------------------------
    def _args(self):
        """The embedded glb_dfa_args: the vocabulary (its bytes where the class walks them), the bank and its counters; the
        automaton's fields are not read."""
        a = _lib.DfaArgs()
        a.struct_size = C.sizeof(_lib.DfaArgs)
        a.n_states, a.start, a.eos_id, a.vocab = self.max_states, 0, self.eos_id, self.vocab
        if self._walks:
            a.tok_bytes, a.n_bytes = self._bytes.data_ptr(), self.n_bytes
            a.tok_ptr, a.skip = self._ptr.data_ptr(), self._skip.data_ptr()
        if not self.weighted:  # (a float bank goes into the block round this one)
            a.bank, a.bank_ld = self.bank.data_ptr(), self.bank.stride(0)
        a.capacity = self.bank.shape[0]
        a.row_of_state, a.work, a.counters = self._row_of_state.data_ptr(), self._work.data_ptr(), self._counters.data_ptr()
        return a

    # ---- states --------------------------------------------------------------------------------------------------------
    def states0(self, n):
        import torch

        return torch.zeros(n, dtype=torch.int32, device=self.dev)

    def _check_advance_args(self, tokens, frm, to, out):
        """(`tokens` contiguous, `out` - made here when None): the arguments of `advance` checked; with no particle `frm` and
        `to` are not looked at."""
        import torch

        if tokens.dtype != torch.int32 or tokens.dim() != 2 or tokens.device != self.dev:
            raise ValueError("tokens must be an int32 [n, ld] tensor on the engine's device")
        tokens = tokens.contiguous()
        n = tokens.shape[0]
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.dev)
        for t in (frm, to) if n else ():
            if t.dtype != torch.int32 or t.shape != (n,) or t.device != self.dev or not t.is_contiguous():
                raise ValueError("frm / to must be contiguous int32 [n] tensors on the engine's device")
        return tokens, out

    def _check_done(self, done, n):
        import torch

        if done is not None and (done.dtype != torch.int32 or done.shape != (n,) or not done.is_contiguous() or done.device != self.dev):
            raise ValueError("done must be a contiguous int32 [n] tensor on the engine's device")

    def _advance_walk(self, entry, states, tokens, frm, to, out):
        """`advance` of a class that walks the tokens itself: one call of `entry`, which takes the particles in chunks whose end
        states fit `cand`."""
        import torch

        tokens, out = self._check_advance_args(tokens, frm, to, out)
        n = tokens.shape[0]
        if n == 0:
            return out
        rows = int(max(1, min(n, _CAND_BYTES // (8 * self.W), self._slots - self.max_states)))
        if self._cand is None or self._cand.shape[0] < rows:
            self._cand = torch.empty((rows, self.W), dtype=torch.int64, device=self.dev)
            self._counts = torch.empty(-(-rows // 256), dtype=torch.int32, device=self.dev)
        a = self._args()
        a.n, a.tokens, a.ld = n, tokens.data_ptr(), tokens.shape[1]
        if tokens.shape[1] == 0:  # nothing to walk: from == to == 0 is the only range inside, every other becomes from > to
            a.tokens, a.ld = self._ptr.data_ptr(), 1
            frm = ((frm != 0) | (to != 0)).to(torch.int32)
            to = torch.zeros_like(frm)
        a.from_, a.to = frm.data_ptr(), to.data_ptr()
        a.state_in = None if states is None else self._states(states).data_ptr()
        a.state_out = out.data_ptr()
        self._call(entry, self._block(a))
        return out

    def _serve(self, entry, states, done):
        """`mask_rows` of a class that fills its rows itself: one call of `entry`."""
        import torch

        n = states.numel()
        out = torch.empty(n, dtype=torch.int32, device=self.dev)
        if n == 0:
            return out
        a = self._args()
        a.n, a.state_in, a.out_rows = n, self._states(states).data_ptr(), out.data_ptr()
        self._check_done(done, n)
        if done is not None:
            a.done = done.data_ptr()
        a.max_work = min(n, self.max_states, self.capacity - 2)
        self._call(entry, self._block(a))
        return out

    # ---- inspection (every call synchronises) ------------------------------------------------------------------------------
    @property
    def n_states(self):
        """The states numbered so far."""
        return int(self._status[0].item())

    def stats(self):
        """`DeviceConstraint.stats()` and "states": the states numbered so far (synchronises)."""
        return dict(super().stats(), states=self.n_states)

    def check(self, word=None):
        """Raises when a state found no id below `max_states`, and what `DeviceConstraint.check` raises for the bank.  Always
        synchronises, `word` given or not: `word` is the bank's overflow word, and the states' overflow bit lies in the status
        words of the block, which are read here."""
        flags = int(self._status[1].item())
        if flags & _BUG:
            raise RuntimeError(f"{type(self).__name__}: the table held a reference out of range (flags {flags})")
        if flags & _OVERFLOW:
            raise RuntimeError(f"the particles reached more than max_states={self.max_states} distinct {self._distinct}: "
                               f"the {self._beyond} beyond got no id, and their particles were served the empty mask.  Raise max_states.")
        super().check(word)
