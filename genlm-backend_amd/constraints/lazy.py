"""`LazyConstraint`: a `ByteNFA` served as a constraint, its subset states made on the device when a particle
reaches them (include/glb.h glb_lazy_*).  The same duck type as `DeviceConstraint`: `DeviceSIS(constraint=...)` and
`batch_next_token_step_device(constraint=...)` take either."""
import ctypes as C

import numpy as np

from .. import _lib
from .automata import ByteDFA
from .nfa import ByteNFA
from .numbered import _Numbered
from .tables import _iterate, _nfa_arrays, _put


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


class LazyConstraint(_Numbered):
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

    _distinct, _beyond = "sets of the automaton's states", "sets"

    def __init__(self, llm_or_engine, nfa, byte_vocab, eos_id, skip_ids=None, max_states=65536, mask_bank_bytes=256 << 20,
                 on_full="error", *, _hash_mask=0, _force_wave=False):
        self._check_on_full(on_full)
        if isinstance(nfa, ByteDFA):
            nfa = ByteNFA.from_dfa(nfa)  # (a ByteWFSA is refused there)
        if not isinstance(nfa, ByteNFA):
            raise ValueError(f"LazyConstraint needs a ByteNFA or a ByteDFA, got {type(nfa).__name__}")
        self._check_max_states(max_states)
        n_imp = int(nfa.important.sum())
        if n_imp > _lib.NFA_MAX_IMPORTANT:
            raise ValueError(f"LazyConstraint: {n_imp} important states (those with a byte arc, and the accepting ones) pass the cap "
                             f"of {_lib.NFA_MAX_IMPORTANT}: a set of them is one wave of 64-bit words")
        V = len(byte_vocab)
        if V == 0:
            raise ValueError("empty vocabulary")
        rows = self._size_bank(V, max_states, mask_bank_bytes, on_full)
        import torch

        eng = getattr(llm_or_engine, "engine", llm_or_engine)
        self.eng, self.dev, self.nfa = eng, eng.device, nfa
        self._upload_vocab(llm_or_engine, byte_vocab, eos_id, skip_ids)
        self.force_wave, self._hash_mask = bool(_force_wave), int(_hash_mask)
        a = self._arrays = _nfa_arrays(nfa)
        self.bit_state, self.W = a["states"], a["n_words"]
        self._nfa_buf = {k: _put(eng, a[k].view(np.int64) if a[k].dtype == np.uint64 else a[k])
                         for k in ("eps_off", "eps_to", "bit_of", "arc_off", "arc_dst", "arc_bytes", "accepting_mask")}
        self._eclose = torch.empty((a["n_states"], self.W), dtype=torch.int64, device=self.dev)
        self._closure()
        new = self._allocate(rows)
        self._sets, self._accepting = new(torch.int64, self.max_states, self.W), new(torch.uint8, self.max_states)
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
    def advance(self, states, tokens, frm, to, out=None):
        """The states after tokens[i, frm[i] .. to[i]) (int32 [n, ld], unit inner stride), from states[i] (None: state 0);
        -1 once dead, for a state that is none of the states numbered before the call, and for a set that found no id
        below `max_states`.  Six launches for every chunk of particles whose end sets fit 64 MB (glb_lazy_advance)."""
        return self._advance_walk("glb_lazy_advance", states, tokens, frm, to, out)

    def mask_rows(self, states, done=None):
        """int32 [n]: the bank row of every state, as `DeviceConstraint.mask_rows` gives it - the rows that are missing
        claimed (under on_full="evict" in a bank smaller than `max_states`: taken from the states requested longest ago)
        and filled from the states' sets first, one call (glb_lazy_serve); no host synchronisation.  `states` are ids that
        `advance` or `states0` returned: an id below `max_states` that no set has yet is served row 0 like a dead state, and
        costs a bank that does not evict one row for good."""
        return self._serve("glb_lazy_serve", states, done)

    # ---- inspection (every call synchronises) ------------------------------------------------------------------------------
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
