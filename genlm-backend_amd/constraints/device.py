"""`DeviceConstraint`: an automaton's tables (tables.py), the bank of rows made from them and every particle's row."""
import ctypes as C
from collections import namedtuple

import numpy as np

from .. import _lib
from .automata import ByteWFSA
from .tables import DeviceTables, _kept, _put

# The two kinds of bank: a row's elements (bit words; with weights the floats of a 256-byte aligned row), V -> how many a row has
# and a caller's bank needs, the step's mask kind, the library's calls and (constraint, DfaArgs) -> the block init and fill take
_BankKind = namedtuple("_BankKind", "dtype row_elems row_need mask_kind rows init fill args")
_BIT_BANK = _BankKind("int32", lambda V: (V + 31) // 32, lambda V: (V + 31) // 32, _lib.MASK_BITS, "glb_dfa_bank_rows",
                      "glb_dfa_bank_init", "glb_dfa_fill_masks", lambda c, a: a)
_FLOAT_BANK = _BankKind("float32", lambda V: (V + 63) // 64 * 64, lambda V: V, _lib.MASK_F32, "glb_dfa_weight_bank_rows",
                        "glb_dfa_weight_bank_init", "glb_dfa_fill_weights", lambda c, a: c._weight_args(a))


class _Bank:
    """What every constraint that serves rows of a bank shares - `DeviceConstraint`, and through `numbered._Numbered` the three
    whose states are numbered on the device, `LazyConstraint`, `PDAConstraint` and `ConstraintProduct`: the vocabulary on
    the device, the bank's row ids as the fused step takes them, its counters and what `check()` says of a full bank.  A
    subclass sets `eng`, `dev`, `bank`, `_kind`, `weighted`, `_counters`, `_evicting`, `_evict_tables`, `mask_bank_bytes` and
    `row_elems`."""

    def _upload_vocab(self, llm_or_engine, byte_vocab, eos_id, skip_ids):
        """The byte strings of the vocabulary back to back, their offsets and the skipped ids on `self.eng`'s device;
        `vocab`, `eos_id`, `words`, `n_bytes`."""
        toks = [bytes(getattr(t, "byte_string", t)) for t in byte_vocab]
        V = len(toks)
        if V == 0:
            raise ValueError("empty vocabulary")
        if skip_ids is None:
            skip_ids = getattr(getattr(llm_or_engine, "tokenizer", None), "all_special_ids", None) or ()
        skip = np.zeros(V, np.uint8)
        for t in skip_ids:
            if 0 <= int(t) < V:
                skip[int(t)] = 1
        ptr = np.zeros(V + 1, np.int64)
        np.cumsum([len(t) for t in toks], out=ptr[1:])
        if ptr[-1] > 0x7fffffff:
            raise ValueError("the vocabulary's byte strings exceed 2^31 bytes")
        flat = np.frombuffer(b"".join(toks) or b"\0", np.uint8).copy()
        self.vocab, self.eos_id, self.words = V, int(eos_id), (V + 31) // 32
        self.n_bytes = int(ptr[-1])
        eng = self.eng
        self._bytes, self._ptr, self._skip = _put(eng, flat), _put(eng, ptr.astype(np.int32)), _put(eng, skip)
        self._gathered, self._cus = None, None

    capacity = property(lambda self: self.bank.shape[0])

    def _states(self, states):
        import torch

        if states.dtype != torch.int32 or states.dim() != 1 or states.device != self.dev or not states.is_contiguous():
            raise ValueError("states must be a contiguous int32 [n] tensor on the engine's device")
        return states

    def step_masks(self, logits, ids, by_row, n_particles, parity=False):
        """The fused step's mask arguments (masks.py; `logits` is not read) for bank rows `ids` (int32 [n_units]: per logits
        row when `by_row`, else per particle), and whether the bank itself is handed over.  `GLB_MASK_BITS` rows are read as they are only by the
        step's one-launch form; its two-launch form first brings ALL rows of the table it is given into the kernels'
        layout.  So the bank is handed over where glb_logprob_mask_sample takes the one-launch form (csrc/glb_api.hip,
        `fused`: no parity draw, more than 512 (unit, 4096-token chunk) items, at most 16 x 8 x CUs particles), and
        otherwise only the units' rows, gathered into a buffer of this object.  This is the one place the rule is
        restated; where it guesses wrong (a stream being captured, a workspace nobody registered) the step still computes
        the same results from the whole bank, only slower.
        A weight bank (`GLB_MASK_F32`) is read where it lies by both forms: always handed over, nothing gathered."""
        import torch

        key = "row_mask_id" if by_row else "mask_id"
        n_units = ids.numel()
        if self._cus is None:
            self._cus = torch.cuda.get_device_properties(self.dev).multi_processor_count
        if self.weighted or (not parity and n_units * ((self.vocab + 4095) // 4096) > 512 and n_particles <= 16 * 8 * self._cus):
            return {"mask_kind": self._kind.mask_kind, "mask": self.bank, key: ids}, True
        if self._gathered is None or self._gathered[0].shape[0] != n_units:
            self._gathered = (torch.empty((n_units, self.words), dtype=torch.int32, device=self.dev),
                              torch.arange(n_units, dtype=torch.int32, device=self.dev))
        buf, own = self._gathered
        self.eng.gather_rows_i32(self.bank[:, :self.words], ids, out=buf)
        return {"mask_kind": _lib.MASK_BITS, "mask": buf, key: own}, False

    def _new_evict_tables(self):
        """The tables of an evicting bank, one allocation: four int32 [capacity], the eviction counters, the epoch."""
        import torch

        return torch.zeros(4 * self.capacity + _lib.DFA_EVICT_COUNTERS + 1, dtype=torch.int32, device=self.dev)

    def _evict_fields(self, e):
        """(the six fields of the eviction tables, of either block that carries them)"""
        cap, base = self.capacity, self._evict_tables.data_ptr()
        e.row_state, e.row_stamp, e.claimants, e.victims = (base + 4 * cap * i for i in range(4))
        e.ecounters = base + 16 * cap
        e.epoch = e.ecounters + 4 * _lib.DFA_EVICT_COUNTERS
        return e

    def _overflow_word(self):
        """int32 [1] device view of the sticky overflow word, for hosts that let it ride on a copy they make anyway."""
        return self._counters[2:3]

    def _rows_in_use(self):
        """(synchronises)"""
        return int(self._counters[0].item())

    def stats(self):
        """{"rows_in_use", "fills", "evictions"}: the bank's rows that hold something (its own two included), the rows
        filled so far and how many of those were taken from another state (synchronises)."""
        rows, filled = self._counters[:2].tolist()
        if not self._evicting:
            return {"rows_in_use": rows, "fills": filled, "evictions": 0}
        fills, evictions = self._evict_tables[4 * self.capacity + 2:4 * self.capacity + 4].tolist()
        return {"rows_in_use": rows, "fills": fills, "evictions": evictions}

    def check(self, word=None):
        """Raises when a state found no row in the bank (synchronises unless `word`, the overflow word's value already on
        the host, is given).  Under eviction that is: one call asked for more distinct states than the bank has rows."""
        if not (int(self._counters[2].item()) if word is None else int(word)):
            return
        if self._evicting:
            raise RuntimeError(f"the constraint's mask bank is smaller than one step's working set: a single mask_rows call "
                               f"asked for more distinct automaton states than its {self.capacity - 2} rows for states "
                               f"({self.capacity} rows of {self.row_elems * 4} bytes, mask_bank_bytes={self.mask_bank_bytes}); "
                               "the states left over were served the empty mask.  The bank must hold at least as many rows "
                               "as the particles occupy distinct states, plus two.  Raise mask_bank_bytes.")
        raise RuntimeError(f"the constraint's mask bank is full: {self.capacity} rows of {self.row_elems * 4} bytes "
                           f"(mask_bank_bytes={self.mask_bank_bytes}) do not hold the automaton states the particles "
                           "reached; their masks were empty.  Raise mask_bank_bytes.")


class DeviceConstraint(_Bank):
    """A `ByteDFA` over a vocabulary's byte strings, resident on the device.

    llm_or_engine    an `AsyncAmdLM` (its engine and, for the default `skip_ids`, its tokenizer's `all_special_ids`) or a
                     `HipEngine`
    byte_vocab       the byte string of every token id (`llm.byte_vocab`); objects with a `byte_string` are accepted
    eos_id           allowed exactly in accepting states
    skip_ids         tokens never allowed (special tokens)
    mask_bank_bytes  budget of the mask bank: one row of ceil(V / 32) words per distinct state reached, plus two.  What
                     happens when a state a particle reaches finds the bank full is `on_full`'s to say.
    on_full          "error" (default): the state gets no row, its particles the empty mask, and `check()` raises.
                     "evict": the bank is a cache over the states (include/glb.h glb_dfa_evict_*) - a
                     `mask_rows` call recycles the least recently requested rows for the states that have none and fills
                     them again, all on the device; rows requested in the same call are never taken.  The bank then only has
                     to hold one step's working set: as many rows as the particles occupy distinct states, plus two
                     (`check()` raises when a single call asked for more).  A bank that holds every state (S + 2 rows)
                     never evicts and takes the path of "error".

    push             None (default): the automaton's weights are served as they are.  "log" / "max" (a `ByteWFSA` only): the
                     weights are pushed toward the start state on the device before anything is served (include/glb.h
                     glb_dfa_backward / glb_dfa_push_weights).  `backward` (float32 [S] device tensor) holds
                     beta[s], the semiring sum ("log": logsumexp, "max": the best) over all accepted byte strings from s;
                     every arc becomes arc + beta[next] - beta[s], every final weight final - beta[s].  An accepted
                     string then weighs what it weighed minus `start_logw` = beta[start], but every state's row carries
                     the look-ahead: a particle sees the weight of a branch when it enters it, not at EOS.  `DeviceSIS`
                     starts its particles at `start_logw`; `push_stats()`, `pushed_wfsa()` are for inspection.
    push_tol         "log": the sweeps stop when no state moved by more than push_tol * max(1, |beta|); the default 2^-20 is
                     four float32 ulps, above the one-ulp oscillation of a converged float32 iteration.
    push_max_sweeps  ValueError when the backward weights have not converged after this many sweeps (or, under "max",
                     after S + 1): the weights do not sum - a cycle of total mass >= 1 under "log".

    minimize         False (default): the automaton is served as it is.  True: equivalent states are merged on the device
                     before anything is served (include/glb.h glb_dfa_refine / glb_dfa_quotient) - after the
                     push, if any, on the tables the push left.  The constraint then serves the quotient: `dfa` is the
                     quotient's host automaton (with a push: carrying the pushed weights), and `n_states`, `start`, `live`,
                     the bank's rows, `warm()`, eviction and `pushed_wfsa()` are the quotient's.  `source_dfa` is what
                     the caller passed, `state_map` (int32 [S] device tensor) every source state's quotient state, -1 for
                     the states dropped (not live, or not reachable from the start); `minimize_stats()`.  States and
                     the ids `advance` returns are the quotient's.  `start_logw` and `backward` keep their meaning;
                     `backward` stays indexed by the SOURCE automaton's states.  A `ByteWFSA` merges states whose weights
                     are equal bit for bit (after a push: what weighted minimisation merges, where rounding left equal
                     bits); every string weighs what it weighed, bit for bit.

    Lifetime of row ids: the ids a `mask_rows` call returns are valid until the next `mask_rows` / `warm` call on this
    constraint - under "evict" that call may hand their rows to other states.  Stream order makes this safe for `DeviceSIS`
    and `batch_next_token_step_device`: each makes one `mask_rows` call a step and enqueues the step that reads the ids
    before the next one.

    With a `ByteWFSA` the bank holds float32 rows [rows, ld] instead (ld: V rounded up to 64 floats), the token log-weights
    from each state (include/glb.h glb_dfa_weight_*): rows = min(S + 2, 65535, mask_bank_bytes / (4 ld)).  A row is 32 times
    a bit row - about 201 KB at V = 50257, so the default 256 MiB hold 1332 states.  `step_masks` then hands the bank over
    as `MASK_F32` in either form of the step; everything else keeps its meaning.
    """

    def __init__(self, llm_or_engine, dfa, byte_vocab, eos_id, skip_ids=None, mask_bank_bytes=256 << 20, on_full="error",
                 push=None, push_tol=2.0 ** -20, push_max_sweeps=4096, minimize=False):
        if on_full not in ("error", "evict"):
            raise ValueError(f'on_full must be "error" or "evict", got {on_full!r}')
        if push not in (None, "log", "max"):
            raise ValueError(f'push must be None, "log" or "max", got {push!r}')
        if push is not None:
            if not isinstance(dfa, ByteWFSA):
                raise ValueError(f"push={push!r} needs a ByteWFSA: a ByteDFA has no weights to push")
            if not float(push_tol) >= 0.0:
                raise ValueError(f"push_tol must be >= 0, got {push_tol!r}")
            if isinstance(push_max_sweeps, bool) or not isinstance(push_max_sweeps, (int, np.integer)) or push_max_sweeps < 1:
                raise ValueError(f"push_max_sweeps must be an int >= 1, got {push_max_sweeps!r}")
        if not isinstance(minimize, bool):
            raise ValueError(f"minimize must be True or False, got {minimize!r}")
        import torch

        self.on_full = on_full
        eng = getattr(llm_or_engine, "engine", llm_or_engine)
        self.eng, self.dev, self.dfa = eng, eng.device, dfa
        self._upload_vocab(llm_or_engine, byte_vocab, eos_id, skip_ids)
        V = self.vocab
        self.mask_bank_bytes = int(mask_bank_bytes)
        self.tables = DeviceTables.upload(eng, dfa)
        self.weighted = self.tables.weighted
        self.push, self.backward, self.start_logw, self._push_sweeps = push, None, 0.0, 0
        if push is not None:
            self._push_weights(float(push_tol), int(push_max_sweeps))
        self.source_dfa, self.state_map, self._min_rounds = dfa, None, 0
        if minimize:  # the quotient's tables, and its host automaton, which becomes `dfa`
            self.tables, new_id, self._min_rounds = self.tables.minimized(_kept(dfa), None)
            self.dfa = dfa = self.tables.to_host(type(dfa))
            self.tables.live = _put(eng, dfa.live.astype(np.uint8))
            self.state_map = _put(eng, new_id)
        self._kind = kind = _FLOAT_BANK if self.weighted else _BIT_BANK
        self.row_elems = kind.row_elems(V)
        rows = int(getattr(eng.lib, kind.rows)(self.mask_bank_bytes, V, dfa.n_states))
        if rows < 3:
            raise ValueError(f"mask_bank_bytes={mask_bank_bytes} holds no state's mask: a row of this vocabulary takes "
                             f"{self.row_elems * 4} bytes{' (float32 weights: 32 times a bit row)' if self.weighted else ''} "
                             "and the bank needs at least three")
        self._row_of_state = torch.empty(dfa.n_states, dtype=torch.int32, device=self.dev)
        self._counters = torch.zeros(_lib.DFA_COUNTERS, dtype=torch.int32, device=self.dev)
        self._set_bank(torch.zeros((rows, self.row_elems), dtype=getattr(torch, kind.dtype), device=self.dev))

    _delta = property(lambda self: self.tables.delta)
    _acc = property(lambda self: self.tables.accepting)
    _live = property(lambda self: self.tables.live)
    _arc_logw = property(lambda self: self.tables.arc_logw, lambda self, t: setattr(self.tables, "arc_logw", t))
    _final_logw = property(lambda self: self.tables.final_logw, lambda self, t: setattr(self.tables, "final_logw", t))

    def _push_weights(self, tol, max_sweeps):
        """The tables replaced by the ones pushed under `self.push`; `backward`, `start_logw` and the sweep count kept."""
        self.tables, self.backward, self._push_sweeps = self.tables.pushed(self.push, tol, max_sweeps)
        self.start_logw = float(self.backward[self.dfa.start].item())

    def minimize_stats(self):
        """{"states_in", "states_out", "rounds"}: the source automaton's states, the states served, and the refinement
        rounds taken, the one that found nothing to split included (0: nothing was minimised)."""
        return {"states_in": self.source_dfa.n_states, "states_out": self.dfa.n_states, "rounds": self._min_rounds}

    def push_stats(self):
        """{"semiring", "sweeps"}: what `push` was (None: nothing pushed) and the Jacobi sweeps the backward weights took,
        the one that found nothing moving included."""
        return {"semiring": self.push, "sweeps": self._push_sweeps}

    def pushed_wfsa(self):
        """A host `ByteWFSA` of the weights this constraint serves (the pushed ones; under push=None the automaton's own),
        for inspection: the arcs into states that are not live weigh -inf and are gone from its `delta` (copies the tables
        from the device)."""
        if not self.weighted:
            raise ValueError("a ByteDFA has no weights")
        return ByteWFSA(self.dfa.delta, self._arc_logw.cpu().numpy(), self._final_logw.cpu().numpy(), self.dfa.start)

    # ---- the bank ------------------------------------------------------------------------------------------------------
    def _set_bank(self, bank):
        """Use `bank` (int32 [rows, >= ceil(V / 32)], with weights float32 [rows, >= V]; unit inner stride; rows may be
        padded) and start it over."""
        import torch

        if bank.dtype != getattr(torch, self._kind.dtype) or bank.dim() != 2 or bank.stride(1) != 1 or bank.shape[0] < 3 \
                or bank.shape[1] < self._kind.row_need(self.vocab) or bank.device != self.dev:
            raise ValueError("bank must be an int32 [rows >= 3, >= ceil(V / 32)] (with weights: float32 [rows >= 3, >= V]) "
                             "device tensor with unit inner stride")
        self.bank = bank
        self._work = torch.zeros((bank.shape[0], 2), dtype=torch.int32, device=self.dev)
        # a bank that cannot hold every state, allowed to evict: the tables of glb_dfa_evict_args, one allocation
        self._evicting = self.on_full == "evict" and self.dfa.n_states + 2 > bank.shape[0]
        self._evict_tables = self._new_evict_tables() if self._evicting else None
        self._reset_bank()

    def _reset_bank(self):
        """Forget every state's row (rows 0 and 1 are written again, the overflow word cleared)."""
        self._warm = False
        if self._evicting:
            self._call("glb_dfa_evict_bank_init", self._evict_args(self._args()))
        else:
            self._call(self._kind.init, self._kind.args(self, self._args()))

    def _args(self):
        a = _lib.DfaArgs()
        a.struct_size = C.sizeof(_lib.DfaArgs)
        a.n_states, a.start, a.eos_id = self.dfa.n_states, self.dfa.start, self.eos_id
        a.delta, a.accepting, a.live = self._delta.data_ptr(), self._acc.data_ptr(), self._live.data_ptr()
        a.vocab, a.tok_bytes, a.n_bytes = self.vocab, self._bytes.data_ptr(), self.n_bytes
        a.tok_ptr, a.skip = self._ptr.data_ptr(), self._skip.data_ptr()
        a.bank, a.bank_ld, a.capacity = self.bank.data_ptr(), self.bank.stride(0), self.bank.shape[0]
        a.row_of_state, a.work, a.counters = self._row_of_state.data_ptr(), self._work.data_ptr(), self._counters.data_ptr()
        return a

    def _weight_args(self, a):
        """The block of glb_dfa_weight_bank_init / glb_dfa_fill_weights round `a`."""
        w = _lib.DfaWeightArgs()
        w.struct_size, w.dfa = C.sizeof(_lib.DfaWeightArgs), a
        return self._float_bank(w)

    def _float_bank(self, block):
        """(the four fields of a float bank)"""
        block.arc_logw, block.final_logw = self._arc_logw.data_ptr(), self._final_logw.data_ptr()
        block.wbank, block.wbank_ld = self.bank.data_ptr(), self.bank.stride(0)
        return block

    def _evict_args(self, a):
        """The block of glb_dfa_evict_bank_init / glb_dfa_evict_serve round `a`, for either kind of bank."""
        e = _lib.DfaEvictArgs()
        e.struct_size, e.dfa = C.sizeof(_lib.DfaEvictArgs), a
        if self.weighted:
            self._float_bank(e)
        return self._evict_fields(e)

    def _call(self, name, a):
        self.eng.dfa_call(name, a)

    # ---- states --------------------------------------------------------------------------------------------------------
    def states0(self, n):
        import torch

        return torch.full((n,), self.dfa.start, dtype=torch.int32, device=self.dev)

    def advance(self, states, tokens, frm, to, out=None):
        """The states after tokens[i, frm[i] .. to[i]) (int32 [n, ld], unit inner stride), from states[i] (None: the start
        state); -1 once dead.  One launch (glb_dfa_advance)."""
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
        a = self._args()
        a.n, a.tokens, a.ld = n, tokens.data_ptr(), tokens.shape[1]
        if tokens.shape[1] == 0:  # nothing to walk: from == to == 0 is the only range inside
            a.tokens, a.ld = self._ptr.data_ptr(), 1
            to = torch.minimum(to, frm)
        a.from_, a.to = frm.data_ptr(), to.data_ptr()
        a.state_in = None if states is None else self._states(states).data_ptr()
        a.state_out = out.data_ptr()
        self._call("glb_dfa_advance", a)
        return out

    def _claim_and_fill(self, states):
        """Every state of `states` that has no bank row yet gets one, and the new rows are filled (two launches)."""
        n = states.numel()
        if n == 0:
            return
        a = self._args()
        a.n, a.state_in = n, self._states(states).data_ptr()
        self._call("glb_dfa_claim_rows", a)
        a.max_work = min(n, self.dfa.n_states, self.capacity)
        self._call(self._kind.fill, self._kind.args(self, a))

    def mask_rows(self, states, done=None):
        """int32 [n]: the bank row of every state - 0 (nothing allowed) for a dead one; where `done` (int32 [n]) is set, row
        1 (EOS only) if the state is accepting, else 0.  Claims and fills what is missing first - under on_full="evict" in
        a bank smaller than the automaton, in rows taken from the states requested longest ago; no host synchronisation.
        The ids are valid until the next `mask_rows` / `warm` call on this constraint."""
        import torch

        n = states.numel()
        out = torch.empty(n, dtype=torch.int32, device=self.dev)
        if n == 0:
            return out
        if not self._warm and not self._evicting:
            self._claim_and_fill(states)
        a = self._args()
        a.n, a.state_in, a.out_rows = n, self._states(states).data_ptr(), out.data_ptr()
        if done is not None:
            if done.dtype != torch.int32 or done.shape != (n,) or not done.is_contiguous() or done.device != self.dev:
                raise ValueError("done must be a contiguous int32 [n] tensor on the engine's device")
            a.done = done.data_ptr()
        if self._evicting:  # touch, select, fill and ids in one call: rows are recycled for the states that have none
            a.max_work = min(n, self.dfa.n_states, self.capacity - 2)
            self._call("glb_dfa_evict_serve", self._evict_args(a))
        else:
            self._call("glb_dfa_mask_ids", a)
        return out

    def forced_final_logw(self, states, forced):
        """float32 [n]: final_logw[states[i]] where `forced` (bool [n]: the particle was served row 1 and ended) and 0.0
        elsewhere - what a caller adds to the log-weight of a particle made to end, so that it weighs what one that chose
        EOS from its state's own row does.  One gather, one select; no synchronisation."""
        import torch

        fw = self._final_logw[states.clamp(min=0).long()]
        return torch.where(forced & (states >= 0), fw, torch.zeros_like(fw))

    def warm(self):
        """Fill the rows of ALL states when the bank holds them (later `mask_rows` calls are then one small launch).
        Returns whether it did."""
        import torch

        if self.dfa.n_states + 2 > self.capacity:
            return False
        if not self._warm:
            self._claim_and_fill(torch.arange(self.dfa.n_states, dtype=torch.int32, device=self.dev))
            self._warm = True
        return True
