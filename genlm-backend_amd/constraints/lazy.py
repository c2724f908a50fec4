"""`LazyConstraint`: a `ByteNFA` served as a constraint, its subset states made on the device when a particle
reaches them (include/glb.h glb_lazy_*).  The same duck type as `DeviceConstraint`: `DeviceSIS(constraint=...)` and
`batch_next_token_step_device(constraint=...)` take either."""
import ctypes as C

import numpy as np

from .. import _lib
from .automata import ByteDFA
from .device import _BIT_BANK, _Bank
from .nfa import ByteNFA
from .tables import _iterate, _nfa_arrays, _put

_CAND_BYTES = 64 << 20  # what the end sets of one chunk of particles may take: W words a particle


def useful_states(nfa):
    """bool [n_states]: the states of `nfa` from which an accepting state can be reached, over the empty arcs and the byte
    arcs that read at least one byte (a fixed point over the arc arrays; no loop over states)."""
    reads = nfa.arc_set.any(axis=1)
    src = np.concatenate([nfa.arc_src[reads], nfa.eps_src])
    dst = np.concatenate([nfa.arc_dst[reads], nfa.eps_dst])
    reach = nfa.accepting.copy()
    while True:
        more = np.zeros_like(reach)
        more[src[reach[dst]]] = True
        more &= ~reach
        if not more.any():
            return reach
        reach |= more


class LazyConstraint(_Bank):
    """A `ByteNFA` over a vocabulary's byte strings, served without determinising it first.

    A state is a set of the automaton's important states (those with a byte arc, and the accepting ones) closed under empty
    arcs and cut down to the states from which something is still accepted, a bitset of W = max(1, ceil(n_important / 64))
    words.  State 0 is the closure of the start; the empty set is no state but -1, the dead state.  `advance` walks every
    particle's tokens byte by byte from its state's set and numbers only the set it ends in: within a call the new sets get
    consecutive ids in the order of the smallest particle index that reached them, across calls the ids go on upward.  A
    state's bank row has bit t set where token t leads from the set to a set that is not empty, and the EOS bit where the
    set holds an accepting state.

    llm_or_engine, byte_vocab, eos_id, skip_ids, mask_bank_bytes, on_full
                     as `DeviceConstraint` has them; the states of the bank are the ids [0, max_states).
    nfa              a `ByteNFA`; a `ByteDFA` is taken through `ByteNFA.from_dfa`.  At most 4096 important states.
    max_states       an int in [1, 2^22]: the sets that get an id.  A set beyond gets none - its particles are -1 and are
                     served the empty mask - and `check()` raises.  Allocated at once: W words and a byte a state, and a
                     hash table of 12 bytes a slot, 2 * max_states slots rounded up to a power of two.

    `n_states`, `sets()`, `to_dfa()` synchronise, as `stats()` and `check()` do; nothing else does."""

    weighted = False
    start_logw = 0.0

    def __init__(self, llm_or_engine, nfa, byte_vocab, eos_id, skip_ids=None, max_states=65536, mask_bank_bytes=256 << 20,
                 on_full="error", *, _hash_mask=0, _force_wave=False):
        if on_full not in ("error", "evict"):
            raise ValueError(f'on_full must be "error" or "evict", got {on_full!r}')
        if isinstance(nfa, ByteDFA):
            nfa = ByteNFA.from_dfa(nfa)  # (a ByteWFSA is refused there)
        if not isinstance(nfa, ByteNFA):
            raise ValueError(f"LazyConstraint needs a ByteNFA or a ByteDFA, got {type(nfa).__name__}")
        if isinstance(max_states, bool) or not isinstance(max_states, (int, np.integer)) or not 1 <= max_states <= _lib.NFA_MAX_STATES:
            raise ValueError(f"max_states must be an int in [1, {_lib.NFA_MAX_STATES}], got {max_states!r}")
        n_imp = int(nfa.important.sum())
        if n_imp > _lib.NFA_MAX_IMPORTANT:
            raise ValueError(f"LazyConstraint: {n_imp} important states (those with a byte arc, and the accepting ones) pass the cap "
                             f"of {_lib.NFA_MAX_IMPORTANT}: a set of them is one wave of 64-bit words")
        V = len(byte_vocab)
        if V == 0:
            raise ValueError("empty vocabulary")
        self.max_states, self.mask_bank_bytes, self.on_full = int(max_states), int(mask_bank_bytes), on_full
        self._kind, self.row_elems = _BIT_BANK, (V + 31) // 32
        rows = int(_lib.load().glb_dfa_bank_rows(self.mask_bank_bytes, V, self.max_states))
        if rows < 3:
            raise ValueError(f"mask_bank_bytes={mask_bank_bytes} holds no state's mask: a row of this vocabulary takes "
                             f"{self.row_elems * 4} bytes and the bank needs at least three")
        import torch

        eng = getattr(llm_or_engine, "engine", llm_or_engine)
        self.eng, self.dev, self.nfa = eng, eng.device, nfa
        self._upload_vocab(llm_or_engine, byte_vocab, eos_id, skip_ids)
        self.force_wave, self._hash_mask = bool(_force_wave), int(_hash_mask)
        a = self._arrays = _nfa_arrays(nfa)
        self.bit_state, self.W = a["states"], a["n_words"]
        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=self.dev)
        self._nfa_buf = {k: _put(eng, a[k].view(np.int64) if a[k].dtype == np.uint64 else a[k])
                         for k in ("eps_off", "eps_to", "bit_of", "arc_off", "arc_dst", "arc_bytes", "accepting_mask")}
        self._eclose = new(torch.int64, a["n_states"], self.W)
        self._closure()
        self._slots = 1 << max(1, (2 * self.max_states - 1).bit_length())
        self._table = new(torch.int64, self._slots * 12 // 8)
        self._sets, self._accepting = new(torch.int64, self.max_states, self.W), new(torch.uint8, self.max_states)
        self._status = torch.zeros(_lib.LAZY_STATUS, dtype=torch.int32, device=self.dev)
        self._cand = self._counts = None
        self._row_of_state = new(torch.int32, self.max_states)
        self._counters = torch.zeros(_lib.DFA_COUNTERS, dtype=torch.int32, device=self.dev)
        self.bank = torch.zeros((rows, self.row_elems), dtype=torch.int32, device=self.dev)
        self._work = torch.zeros((rows, 2), dtype=torch.int32, device=self.dev)
        self._evicting = on_full == "evict" and self.max_states + 2 > rows
        self._evict_tables = self._new_evict_tables() if self._evicting else None
        self._call("glb_lazy_init", self._block())

    def _closure(self):
        """`_eclose`: the empty-arc closure of every state (glb_nfa_closure, which reads nothing of its block but the empty
        arcs and the bit indices), every row then cut down to the useful states."""
        import torch

        a = self._arrays
        status = torch.zeros(_lib.NFA_STATUS, dtype=torch.int32, device=self.dev)
        p = _lib.NfaArgs()
        p.struct_size = C.sizeof(_lib.NfaArgs)
        for k in ("n_states", "start", "n_important", "n_words", "n_eps"):
            setattr(p, k, a[k])
        for k in ("eps_off", "eps_to", "bit_of"):
            setattr(p, k, self._nfa_buf[k].data_ptr())
        p.eclose, p.status = self._eclose.data_ptr(), status.data_ptr()
        sweeps, converged, flags = _iterate(self.eng, "glb_nfa_closure", p, status[_lib.NFA_CLOSURE_STATUS:], a["n_states"] + 1, count="rounds")
        if flags or not converged:
            raise RuntimeError(f"LazyConstraint: the empty-arc closure had not settled after {sweeps} sweeps over {a['n_states']} states")
        useful = np.zeros(self.W * 64, np.bool_)
        useful[:a["n_important"]] = useful_states(self.nfa)[a["states"]]
        words = np.ascontiguousarray(np.packbits(useful, bitorder="little")).view("<u8")
        self._eclose &= _put(self.eng, words.view(np.int64))[None, :]

    # ---- the blocks ----------------------------------------------------------------------------------------------------
    def _args(self):
        """The embedded glb_dfa_args: the vocabulary, the bank and its counters; the automaton's fields are not read."""
        a = _lib.DfaArgs()
        a.struct_size = C.sizeof(_lib.DfaArgs)
        a.n_states, a.start, a.eos_id = self.max_states, 0, self.eos_id
        a.vocab, a.tok_bytes, a.n_bytes = self.vocab, self._bytes.data_ptr(), self.n_bytes
        a.tok_ptr, a.skip = self._ptr.data_ptr(), self._skip.data_ptr()
        a.bank, a.bank_ld, a.capacity = self.bank.data_ptr(), self.bank.stride(0), self.bank.shape[0]
        a.row_of_state, a.work, a.counters = self._row_of_state.data_ptr(), self._work.data_ptr(), self._counters.data_ptr()
        return a

    def _block(self, a=None):
        p = _lib.LazyArgs()
        p.struct_size, p.dfa = C.sizeof(_lib.LazyArgs), self._args() if a is None else a
        arr = self._arrays
        p.n_nfa_states, p.nfa_start, p.n_important, p.n_words, p.n_arcs = (arr[k] for k in ("n_states", "start", "n_important", "n_words", "n_arcs"))
        p.max_states, p.hash_mask, p.force_wave = self.max_states, self._hash_mask, int(self.force_wave)
        for k in ("arc_off", "arc_dst", "arc_bytes", "accepting_mask"):
            setattr(p, k, self._nfa_buf[k].data_ptr())
        p.eclose, p.table, p.table_slots = self._eclose.data_ptr(), self._table.data_ptr(), self._slots
        p.sets, p.accepting_out, p.status = self._sets.data_ptr(), self._accepting.data_ptr(), self._status.data_ptr()
        if self._cand is not None:
            p.cand, p.counts, p.cand_rows = self._cand.data_ptr(), self._counts.data_ptr(), self._cand.shape[0]
        if self._evicting:
            self._evict_fields(p)
        return p

    def _call(self, name, p):
        self.eng.lazy_call(name, p)

    # ---- states --------------------------------------------------------------------------------------------------------
    def states0(self, n):
        import torch

        return torch.zeros(n, dtype=torch.int32, device=self.dev)

    def advance(self, states, tokens, frm, to, out=None):
        """The states after tokens[i, frm[i] .. to[i]) (int32 [n, ld], unit inner stride), from states[i] (None: state 0);
        -1 once dead, for a state that is none of the states numbered before the call, and for a set that found no id
        below `max_states`.  Six launches for every chunk of particles whose end sets fit 64 MB (glb_lazy_advance)."""
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
        self._call("glb_lazy_advance", self._block(a))
        return out

    def mask_rows(self, states, done=None):
        """int32 [n]: the bank row of every state, as `DeviceConstraint.mask_rows` gives it - the rows that are missing
        claimed (under on_full="evict" in a bank smaller than `max_states`: taken from the states requested longest ago)
        and filled from the states' sets first, one call (glb_lazy_serve); no host synchronisation.  `states` are ids that
        `advance` or `states0` returned: an id below `max_states` that no set has yet is served row 0 like a dead state, and
        costs a bank that does not evict one row for good."""
        import torch

        n = states.numel()
        out = torch.empty(n, dtype=torch.int32, device=self.dev)
        if n == 0:
            return out
        a = self._args()
        a.n, a.state_in, a.out_rows = n, self._states(states).data_ptr(), out.data_ptr()
        if done is not None:
            if done.dtype != torch.int32 or done.shape != (n,) or not done.is_contiguous() or done.device != self.dev:
                raise ValueError("done must be a contiguous int32 [n] tensor on the engine's device")
            a.done = done.data_ptr()
        a.max_work = min(n, self.max_states, self.capacity - 2)
        self._call("glb_lazy_serve", self._block(a))
        return out

    # ---- inspection (every call synchronises) ------------------------------------------------------------------------------
    @property
    def n_states(self):
        """The sets numbered so far."""
        return int(self._status[0].item())

    def sets(self):
        """Host uint64 [n_states, W]: every numbered state's set (bit i: word i // 64, bit i % 64, the state `bit_state[i]`)."""
        return np.ascontiguousarray(self._sets[:self.n_states].cpu().numpy().view(np.uint64))

    def to_dfa(self):
        """The partial `ByteDFA` over the sets numbered so far, state 0 the start: an arc into a set that has no id yet, or
        into the empty set, is -1.  Built on the host from `sets()`; for tests and debugging."""
        a, sets = self._arrays, self.sets()
        as_int = lambda row: int.from_bytes(row.tobytes(), "little")
        ids = {as_int(r): i for i, r in enumerate(sets)}
        eclose = [as_int(r) for r in self._eclose.cpu().numpy().view(np.uint64)]
        reads = np.unpackbits(a["arc_bytes"].view(np.uint8).reshape(-1, 32), axis=1, bitorder="little").astype(np.bool_)
        delta = np.full((len(sets), 256), -1, np.int32)
        for s, row in enumerate(sets):
            for g, byte in enumerate(a["group_lo"].tolist()):
                cur, target = as_int(row), 0
                while cur:
                    m = (cur & -cur).bit_length() - 1
                    cur &= cur - 1
                    for k in range(a["arc_off"][m], a["arc_off"][m + 1]):
                        if reads[k, byte]:
                            target |= eclose[a["arc_dst"][k]]
                if target:
                    delta[s, a["group_of"] == g] = ids.get(target, -1)
        return ByteDFA(delta, self._accepting[:len(sets)].cpu().numpy().astype(np.bool_), 0)

    def stats(self):
        """`DeviceConstraint.stats()` and "states": the sets numbered so far (synchronises)."""
        return dict(super().stats(), states=self.n_states)

    def check(self, word=None):
        """Raises when a set found no id below `max_states`, and what `DeviceConstraint.check` raises for the bank.  Always
        synchronises, `word` given or not: `word` is the bank's overflow word, and the sets' overflow bit lies in the status
        words of the block, which are read here."""
        flags = int(self._status[1].item())
        if flags & _lib.LAZY_BUG:
            raise RuntimeError(f"LazyConstraint: the table held a reference out of range (flags {flags})")
        if flags & _lib.LAZY_OVERFLOW:
            raise RuntimeError(f"the particles reached more than max_states={self.max_states} distinct sets of the automaton's states: "
                               "the sets beyond got no id, and their particles were served the empty mask.  Raise max_states.")
        super().check(word)
