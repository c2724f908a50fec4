"""An automaton's tables on the device, pushed and minimised (§21) there before they are served:
`DeviceConstraint` and the standalone `minimize` prepare theirs through the same three calls, `upload`, `pushed`, `minimized`;
`product` (§22) makes the tables of two automata's conjunction, union or difference there, in front of that pipeline, and
`determinize` (§23) those of a `ByteNFA`."""
import ctypes as C
import dataclasses

import numpy as np

from .. import _lib
from .automata import ByteDFA, ByteWFSA

_BATCH = 64  # launches enqueued between two reads of the status words


@dataclasses.dataclass(eq=False)
class DeviceTables:
    """delta int32 [S, 256], accepting and live uint8 [S], with weights arc_logw float32 [S, 256] and final_logw float32 [S]
    (else both None), on `eng`'s device.  `live` is None on what `minimized` returns, until a host automaton gives it."""
    eng: object
    delta: object
    accepting: object
    live: object
    arc_logw: object
    final_logw: object
    start: int

    n_states = property(lambda self: self.delta.shape[0])
    weighted = property(lambda self: self.arc_logw is not None)

    @classmethod
    def upload(cls, eng, automaton):
        """The tables of a `ByteDFA` or a `ByteWFSA`: the one place that asks which of the two it is."""
        arc, fin = (_put(eng, automaton.arc_logw), _put(eng, automaton.final_logw)) if isinstance(automaton, ByteWFSA) else (None, None)
        return cls(eng=eng, delta=_put(eng, automaton.delta), accepting=_put(eng, automaton.accepting.astype(np.uint8)),
                   live=_put(eng, automaton.live.astype(np.uint8)), arc_logw=arc, final_logw=fin, start=automaton.start)

    def to_host(self, kind):
        """The host automaton of these tables: a `ByteWFSA` where `kind` is one, else a `ByteDFA`."""
        host = lambda t: t.cpu().numpy()
        if issubclass(kind, ByteWFSA):
            return ByteWFSA(host(self.delta), host(self.arc_logw), host(self.final_logw), self.start)
        return ByteDFA(host(self.delta), host(self.accepting).astype(np.bool_), self.start)

    def _iterate(self, name, p, status, budget, *, count, stop=lambda n: False):
        """The host side of an iteration whose stop rule is the device's: `name` called with up to `_BATCH` launches a time
        (`count`: the block's field for their number; the first call restarts) and the status words (iterations performed,
        converged, flags) read after each, until converged, flagged, `budget` iterations or `stop(iterations)`; the words."""
        return _iterate(self.eng, name, p, status, budget, count=count, stop=stop)

    def pushed(self, semiring, tol, max_sweeps):
        """(tables, beta, sweeps): backward weights by Jacobi sweeps on the device (glb_dfa_backward, in batches), then the
        automaton reweighted by them (glb_dfa_push_weights): the tables with the pushed `arc_logw` / `final_logw`, served
        downstream as any `ByteWFSA`'s.  `semiring`: "log" or "max"; ValueError when the weights do not sum."""
        import torch

        S, dev = self.n_states, self.eng.device
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        beta, scratch, arc_out, final_out = f32(S), f32(S), f32(S, 256), f32(S)
        status = torch.zeros(_lib.DFA_PUSH_STATUS, dtype=torch.int32, device=dev)
        p = _lib.DfaPushArgs()
        p.struct_size = C.sizeof(_lib.DfaPushArgs)
        p.n_states, p.start = S, self.start
        p.semiring = _lib.DFA_PUSH_LOG if semiring == "log" else _lib.DFA_PUSH_MAX
        p.delta, p.arc_logw, p.final_logw = self.delta.data_ptr(), self.arc_logw.data_ptr(), self.final_logw.data_ptr()
        p.beta, p.scratch, p.arc_out, p.final_out = beta.data_ptr(), scratch.data_ptr(), arc_out.data_ptr(), final_out.data_ptr()
        p.status, p.tol = status.data_ptr(), tol
        too_long = lambda sweeps: semiring == "max" and sweeps > S + 1
        sweeps, converged, flags = self._iterate("glb_dfa_backward", p, status, max_sweeps, count="sweeps", stop=too_long)
        if flags or not converged or too_long(sweeps):
            raise ValueError(f"the automaton's weights do not sum: the backward weights "
                             f"{'overflowed' if flags else 'had not converged'} after {sweeps} sweeps under push={semiring!r} "
                             '(under "log": a cycle of total mass >= 1; under "max": a cycle of positive weight).  '
                             'push="max" needs only that no cycle gains weight; push=None serves the weights as they are.')
        p.sweeps = 1
        self.eng.dfa_call("glb_dfa_push_weights", p)
        return dataclasses.replace(self, arc_logw=arc_out, final_logw=final_out), beta, sweeps

    def minimized(self, keep, max_rounds):
        """(tables, new_id, rounds): refinement and quotient on the device (`keep` a host bool [S]; `max_rounds` None: S + 1)
        - the quotient's tables (`live` left None), new_id host int32 [S] (every state's quotient state, -1 where not kept)
        and the rounds taken.  States merge on their labels: with weights the bits of `final_logw` and `arc_logw`, else
        `accepting`.  Quotient states are numbered by their smallest member, in increasing order: state 0's class is state 0."""
        import torch

        dev, S = self.eng.device, self.n_states
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        final_bits, arc_bits = (self.final_logw, self.arc_logw) if self.weighted else (self.accepting.to(torch.int32), None)
        slots = 1 << max(1, (2 * S - 1).bit_length())
        cls, scratch, table = i32(S), i32(S), torch.empty(slots * 12 // 8, dtype=torch.int64, device=dev)
        status = torch.zeros(_lib.DFA_MIN_STATUS, dtype=torch.int32, device=dev)
        keep_d = _put(self.eng, np.ascontiguousarray(keep, dtype=np.uint8))
        p = _lib.DfaMinArgs()
        p.struct_size, p.n_states = C.sizeof(_lib.DfaMinArgs), S
        p.delta, p.keep, p.final_bits = self.delta.data_ptr(), keep_d.data_ptr(), final_bits.data_ptr()
        p.arc_bits = None if arc_bits is None else arc_bits.data_ptr()
        p.cls, p.scratch, p.table, p.table_slots, p.status = cls.data_ptr(), scratch.data_ptr(), table.data_ptr(), slots, status.data_ptr()
        limit = S + 1 if max_rounds is None else int(max_rounds)
        rounds, converged, flags = self._iterate("glb_dfa_refine", p, status, limit, count="rounds")
        if flags:
            raise RuntimeError(f"minimize: the refinement raised its flag word ({flags}: bit 0 - two different signatures shared a "
                               f"64-bit hash; bit 1 - a key found no slot) after {rounds} rounds; nothing was merged on that ground")
        if not converged:
            raise RuntimeError(f"minimize: the partition was still splitting after max_rounds={limit} rounds")
        c = cls.cpu().numpy()
        rep = np.unique(c[c >= 0]).astype(np.int32)
        new_id = np.where(c >= 0, np.searchsorted(rep, c), -1).astype(np.int32)
        n_new = len(rep)
        both = _put(self.eng, np.concatenate([new_id, rep]))  # (one upload)
        out = DeviceTables(eng=self.eng, delta=i32(n_new, 256), accepting=torch.empty(n_new, dtype=torch.uint8, device=dev), live=None,
                           arc_logw=None, final_logw=None, start=int(new_id[self.start]))
        p.new_id, p.rep, p.n_new, p.delta_out = both.data_ptr(), both.data_ptr() + 4 * S, n_new, out.delta.data_ptr()
        if self.weighted:
            out.arc_logw = torch.empty((n_new, 256), dtype=torch.float32, device=dev)
            out.final_logw = torch.empty(n_new, dtype=torch.float32, device=dev)
            p.arc_logw, p.final_logw = self.arc_logw.data_ptr(), self.final_logw.data_ptr()
            p.arc_out, p.final_out = out.arc_logw.data_ptr(), out.final_logw.data_ptr()
        p.accepting, p.accepting_out = self.accepting.data_ptr(), out.accepting.data_ptr()
        self.eng.dfa_call("glb_dfa_quotient", p)
        return out, new_id, rounds


    def _product_block(self, other, op, cap):
        """(block, buffers): the glb_fsa_product_args of these tables (A) with `other` (B) and its device buffers, the outputs
        allocated for `cap` rows."""
        import torch

        dev = self.eng.device
        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
        slots = 1 << max(1, (2 * cap - 1).bit_length())
        buf = dict(table=new(torch.int64, 2 * slots), pairs=new(torch.int32, cap, 2), delta=new(torch.int32, cap, 256),
                   accepting=new(torch.uint8, cap), live=new(torch.uint8, cap), counts=new(torch.int32, cap),
                   status=torch.zeros(_lib.FSA_STATUS, dtype=torch.int32, device=dev), arc=None, final=None)
        p = _lib.FsaProductArgs()
        p.struct_size, p.op = C.sizeof(_lib.FsaProductArgs), {"and": _lib.FSA_AND, "or": _lib.FSA_OR, "sub": _lib.FSA_SUB}[op]
        p.n_a, p.n_b, p.start_a, p.start_b = self.n_states, other.n_states, self.start, other.start
        p.delta_a, p.accepting_a, p.live_a = self.delta.data_ptr(), self.accepting.data_ptr(), self.live.data_ptr()
        p.delta_b, p.accepting_b, p.live_b = other.delta.data_ptr(), other.accepting.data_ptr(), other.live.data_ptr()
        if self.weighted:
            p.arc_a, p.final_a = self.arc_logw.data_ptr(), self.final_logw.data_ptr()
        if other.weighted:
            p.arc_b, p.final_b = other.arc_logw.data_ptr(), other.final_logw.data_ptr()
        if self.weighted or other.weighted:
            buf["arc"], buf["final"] = new(torch.float32, cap, 256), new(torch.float32, cap)
            p.arc_out, p.final_out = buf["arc"].data_ptr(), buf["final"].data_ptr()
        p.max_states, p.table, p.table_slots = cap, buf["table"].data_ptr(), slots
        p.pairs, p.delta_out, p.accepting_out = buf["pairs"].data_ptr(), buf["delta"].data_ptr(), buf["accepting"].data_ptr()
        p.live, p.counts, p.status = buf["live"].data_ptr(), buf["counts"].data_ptr(), buf["status"].data_ptr()
        return p, buf

    def _product_search(self, p, status):
        """The batch loops of `product` over a block of `_product_block`: the rounds of the search, then the liveness sweeps,
        the status words read between batches and nothing else; {"rounds", "sweeps", "states"}.  The block's outputs then
        hold "states" rows, nothing trimmed.  ValueError when the search passes the block's max_states."""
        cap = p.max_states
        rounds, converged, flags = self._iterate("glb_fsa_product_round", p, status, cap + 1, count="rounds")
        if flags & 1:
            raise ValueError(f"product: the search passed max_states={cap}: it had reached at least {int(status[7])} states in round "
                             f"{rounds + 1} and was not at its end; nothing is returned")
        if flags:
            raise RuntimeError(f"product: the search raised flag bit 1 (flags {flags}: an id out of range) after {rounds} rounds")
        if not converged:
            raise RuntimeError(f"product: the search had not ended after {rounds} rounds over at most {cap} states")
        p.n_states = n = int(status[3])
        sweeps, converged, flags = self._iterate("glb_fsa_live", p, status[_lib.FSA_LIVE_STATUS:], n + 1, count="rounds")
        if flags or not converged:
            raise RuntimeError(f"product: liveness had not settled after {sweeps} sweeps over {n} states")
        return dict(rounds=rounds, sweeps=sweeps, states=n)

    def product(self, other, op, max_states):
        """(tables, pairs, stats): the product of these tables (A) with `other` (B) under `op` ("and", "or", "sub"), searched,
        swept for joint liveness and trimmed on the device (glb_fsa_product_round, glb_fsa_live, glb_dfa_quotient over the
        live states with every state its own class; include/glb.h).  pairs: host int32 [S, 2], every state's
        (A state, B state), -1 for a side that is out.  State 0 is the start pair, kept whatever it is; the others keep the
        order of the queue search.  `live` of the result is the device's.  ValueError when the search passes `max_states`."""
        import torch

        dev = self.eng.device
        p, buf = self._product_block(other, op, max_states)
        stats = self._product_search(p, buf["status"])
        n = stats["states"]
        live = buf["live"][:n].cpu().numpy().astype(np.bool_)
        keep = live.copy()
        keep[0] = True
        rep = np.nonzero(keep)[0].astype(np.int32)
        new_id = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        n_new = len(rep)
        up, keep_d = _put(self.eng, np.concatenate([new_id, rep])), _put(self.eng, keep.astype(np.uint8))
        out = DeviceTables(eng=self.eng, delta=torch.empty((n_new, 256), dtype=torch.int32, device=dev),
                           accepting=torch.empty(n_new, dtype=torch.uint8, device=dev), live=_put(self.eng, live[rep].astype(np.uint8)),
                           arc_logw=None, final_logw=None, start=0)
        q = _lib.DfaMinArgs()
        q.struct_size, q.n_states = C.sizeof(_lib.DfaMinArgs), n
        q.delta, q.keep, q.new_id, q.rep, q.n_new = buf["delta"].data_ptr(), keep_d.data_ptr(), up.data_ptr(), up.data_ptr() + 4 * n, n_new
        q.accepting, q.delta_out, q.accepting_out = buf["accepting"].data_ptr(), out.delta.data_ptr(), out.accepting.data_ptr()
        if buf["arc"] is not None:
            out.arc_logw = torch.empty((n_new, 256), dtype=torch.float32, device=dev)
            out.final_logw = torch.empty(n_new, dtype=torch.float32, device=dev)
            q.arc_logw, q.final_logw = buf["arc"].data_ptr(), buf["final"].data_ptr()
            q.arc_out, q.final_out = out.arc_logw.data_ptr(), out.final_logw.data_ptr()
        self.eng.dfa_call("glb_dfa_quotient", q)
        pairs = buf["pairs"][:n].cpu().numpy()[rep]
        return out, np.ascontiguousarray(pairs), dict(stats, states_out=n_new)


def _put(eng, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _iterate(eng, name, p, status, budget, *, count, stop=lambda n: False, batch=_BATCH):
    """`DeviceTables._iterate`, for any engine: the entry's prefix says which of the engine's calls takes it."""
    call = eng.fsa_call if name.startswith("glb_fsa_") else eng.nfa_call if name.startswith("glb_nfa_") else eng.dfa_call
    p.restart = 1
    n = converged = flags = 0
    while not converged and not flags and n < budget and not stop(n):
        setattr(p, count, min(batch, budget - n))
        call(name, p)
        p.restart = 0
        n, converged, flags = status[:3].tolist()
    return n, converged, flags


def _nfa_arrays(nfa):
    """What the device reads of a `ByteNFA` (include/glb.h glb_nfa_args), as host arrays: the important states and their bit
    indices, the empty arcs and the byte arcs as CSRs by source, the arcs' byte sets as four 64-bit words, the accepting
    bits, and the byte groups - bytes that no arc's set tells apart - in the order of their lowest bytes.  No loop over
    states.  Arrays the automaton leaves empty hold one unused element: the device is never handed a null pointer."""
    n = nfa.n_states
    imp = nfa.important
    states = np.nonzero(imp)[0].astype(np.int32)
    n_imp = len(states)
    W = max(1, -(-n_imp // 64))
    bit_of = np.where(imp, np.cumsum(imp) - 1, -1).astype(np.int32)
    some = lambda a: a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype)
    order = np.argsort(nfa.eps_src, kind="stable")
    eps_off = np.searchsorted(nfa.eps_src[order], np.arange(n + 1)).astype(np.int32)
    order_a = np.argsort(bit_of[nfa.arc_src], kind="stable")
    arc_off = np.searchsorted(bit_of[nfa.arc_src][order_a], np.arange(n_imp + 1)).astype(np.int32)
    arc_set = nfa.arc_set[order_a]
    bits = lambda b: np.ascontiguousarray(np.packbits(b, axis=-1, bitorder="little")).view("<u8")
    if len(arc_set):
        _, lo, group = np.unique(arc_set, axis=1, return_index=True, return_inverse=True)
        rank = np.argsort(lo)  # (the groups in the order of their lowest bytes)
        group_of = np.argsort(rank)[np.asarray(group).reshape(-1)].astype(np.int32)
        group_lo = lo[rank].astype(np.int32)
    else:
        group_of, group_lo = np.zeros(256, np.int32), np.zeros(1, np.int32)
    acc = np.zeros(W * 64, np.bool_)
    acc[:n_imp] = nfa.accepting[states]
    return dict(n_states=n, start=nfa.start, n_important=n_imp, n_words=W, n_arcs=len(arc_set), n_eps=len(order), n_groups=len(group_lo),
                states=states, bit_of=bit_of, eps_off=eps_off, eps_to=some(nfa.eps_dst[order]), arc_off=arc_off,
                arc_dst=some(nfa.arc_dst[order_a]), arc_bytes=some(bits(arc_set).reshape(-1, 4)), accepting_mask=bits(acc),
                group_of=group_of, group_lo=group_lo)


_NFA_CAND_BYTES = 64 << 20  # what the candidate sets of one round may take: `chunk` states of n_groups * n_words words each


def _nfa_block(eng, arrays, cap, hash_mask=0):
    """(block, buffers): a glb_nfa_args over `arrays` (`_nfa_arrays`) on `eng`'s device, the outputs allocated for `cap`
    states and the candidate sets for as many states a round as `_NFA_CAND_BYTES` holds."""
    import torch

    dev = eng.device
    new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
    G, W = arrays["n_groups"], arrays["n_words"]
    chunk = int(max(1, min(cap, _NFA_CAND_BYTES // (8 * G * W))))
    slots = 1 << max(1, (2 * cap - 1).bit_length())
    # (uint64 arrays travel as int64: the bits are what the device reads)
    buf = {k: _put(eng, v.view(np.int64) if v.dtype == np.uint64 else v) for k, v in arrays.items() if isinstance(v, np.ndarray)}
    buf.update(eclose=new(torch.int64, arrays["n_states"], W), table=new(torch.int64, slots * 12 // 8), cand=new(torch.int64, chunk * G * W),
               sets=new(torch.int64, cap, W), delta=new(torch.int32, cap, 256), accepting=new(torch.uint8, cap), counts=new(torch.int32, chunk),
               status=torch.zeros(_lib.NFA_STATUS, dtype=torch.int32, device=dev))
    p = _lib.NfaArgs()
    p.struct_size = C.sizeof(_lib.NfaArgs)
    for k in ("n_states", "start", "n_important", "n_words", "n_arcs", "n_eps", "n_groups"):
        setattr(p, k, arrays[k])
    for k in ("eps_off", "eps_to", "bit_of", "arc_off", "arc_dst", "arc_bytes", "accepting_mask", "group_of", "group_lo", "eclose", "table",
              "cand", "sets", "counts", "status"):
        setattr(p, k, buf[k].data_ptr())
    p.delta_out, p.accepting_out = buf["delta"].data_ptr(), buf["accepting"].data_ptr()
    p.hash_mask, p.max_states, p.chunk, p.table_slots = hash_mask, cap, chunk, slots
    return p, buf


def _nfa_search(eng, p, status, batch=_BATCH):
    """The batch loops of `determinize` over a block of `_nfa_block`: the sweeps of the closure, then the rounds of the
    search, the status words read between batches and nothing else; {"sweeps", "rounds", "states"}.  ValueError when the
    search passes the block's max_states."""
    cap = p.max_states
    sweeps, converged, flags = _iterate(eng, "glb_nfa_closure", p, status[_lib.NFA_CLOSURE_STATUS:], p.n_states + 1, count="rounds", batch=batch)
    if flags or not converged:
        raise RuntimeError(f"determinize: the empty-arc closure had not settled after {sweeps} sweeps over {p.n_states} states")
    rounds, converged, flags = _iterate(eng, "glb_nfa_subset_round", p, status, cap + 1, count="rounds", batch=batch)
    if flags & 1:
        raise ValueError(f"determinize: the search passed max_states={cap}: it had reached at least {int(status[7])} states in round "
                         f"{rounds + 1} and was not at its end; nothing is returned")
    if flags:
        raise RuntimeError(f"determinize: the search raised flag bit 1 (flags {flags}: a reference out of range) after {rounds} rounds")
    if not converged:
        raise RuntimeError(f"determinize: the search had not ended after {rounds} rounds over at most {cap} states")
    return dict(sweeps=sweeps, rounds=rounds, states=int(status[3]))


def _nfa_live(eng, delta, accepting, n):
    """uint8 [n] on the device: glb_fsa_live over the first n rows of `delta` / `accepting` (it reads nothing else of its block)."""
    import torch

    live = torch.empty(n, dtype=torch.uint8, device=eng.device)
    status = torch.zeros(_lib.FSA_STATUS, dtype=torch.int32, device=eng.device)
    q = _lib.FsaProductArgs()
    q.struct_size, q.n_states, q.max_states = C.sizeof(_lib.FsaProductArgs), n, n
    q.delta_out, q.accepting_out, q.live, q.status = delta.data_ptr(), accepting.data_ptr(), live.data_ptr(), status.data_ptr()
    sweeps, converged, flags = _iterate(eng, "glb_fsa_live", q, status[_lib.FSA_LIVE_STATUS:], n + 1, count="rounds")
    if flags or not converged:
        raise RuntimeError(f"determinize: liveness had not settled after {sweeps} sweeps over {n} states")
    return live


def _kept(automaton):
    """live & reachable, and the start state whatever it is: the quotient always has one."""
    keep = automaton.live & automaton.reachable
    keep[automaton.start] = True
    return keep


def minimize(llm_or_engine, automaton, max_rounds=None):
    """(minimal, state_map): the smallest automaton that `automaton`'s labels allow, made on the device (include/glb.h
    glb_dfa_refine / glb_dfa_quotient), and int32 [S] - every state's state in it, -1 for the states dropped
    (those not live or not reachable from the start).  A `ByteDFA` gives the minimal `ByteDFA` of its language.  A
    `ByteWFSA` gives the quotient by the coarsest bisimulation on (byte, weight bits): states merge where their final
    weights and the weights of their arcs are equal bit for bit, so `path_logw` of every string is unchanged bit for bit;
    nothing is merged within a tolerance.  Quotient states are numbered in the order of their smallest members, so a start
    state 0 stays 0.  `max_rounds` (None: S + 1, which always suffices): RuntimeError when the partition still splits
    after that many rounds, or when the device reports a hash collision."""
    if not isinstance(automaton, ByteDFA):
        raise ValueError("minimize needs a ByteDFA or a ByteWFSA")
    if max_rounds is not None and (isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or max_rounds < 1):
        raise ValueError(f"max_rounds must be None or an int >= 1, got {max_rounds!r}")
    tables = DeviceTables.upload(getattr(llm_or_engine, "engine", llm_or_engine), automaton)
    small, new_id, _ = tables.minimized(_kept(automaton), max_rounds)
    return small.to_host(type(automaton)), new_id


def product(llm_or_engine, a, b, op="and", max_states=1 << 18):
    """(automaton, pairs): the automaton of the byte strings that `a` and `b` both accept (op="and"), that either accepts
    ("or"), or that `a` accepts and `b` does not ("sub"), made on the device (include/glb.h glb_fsa_product_round /
    glb_fsa_live), and host int32 [S, 2]: every state's (state of a, state of b), -1 for a side that has left
    its automaton (a side that is not live there counts as having left).  `a` and `b`: each a `ByteDFA` or a `ByteWFSA`;
    "or" takes no weights, "sub" takes `a`'s alone.  The result is a `ByteWFSA` when an operand has weights: under "and" of
    two weighted automata the arc and final weights are added, one float32 addition each (a + b); where one side has
    weights its bits pass through.  State 0 is the start; the states are numbered in the order of a queue search over the
    pairs (states in id order, bytes ascending) and then trimmed to those from which some string is still accepted, the
    start always kept: an empty language gives one state without arcs.  `live` of the result comes from the device.
    ValueError for an argument the above does not admit, before the device is touched, and when the search passes
    `max_states` states before it ends (nothing partial is returned; the message names `max_states` and the count reached
    when the search stopped - it stops in the middle of a round, so a wide search reports a count of its own, at least
    max_states + 1).  The outputs are allocated for `max_states` rows before the search, 1 KB a row (2 KB with weights);
    no product has more than (a.n_states + 1) * (b.n_states + 1) states, so a larger `max_states` allocates that many.  The
    device numbers at most 2^22 states: ValueError, before the device is touched too, when the smaller of the two numbers
    exceeds that - a `max_states` above 2^22 is accepted only where the operands are small enough to make it moot."""
    if op not in ("and", "or", "sub"):
        raise ValueError(f'op must be "and", "or" or "sub", got {op!r}')
    for name, x in (("a", a), ("b", b)):
        if not isinstance(x, ByteDFA):
            raise ValueError(f"product needs a ByteDFA or a ByteWFSA for {name}, got {type(x).__name__}")
    if op == "or" and (isinstance(a, ByteWFSA) or isinstance(b, ByteWFSA)):
        raise ValueError('op="or" takes unweighted operands: the union of weighted automata needs a sum per string')
    if op == "sub" and isinstance(b, ByteWFSA):
        raise ValueError('op="sub" takes an unweighted `b`: the strings removed carry no weight')
    if isinstance(max_states, bool) or not isinstance(max_states, (int, np.integer)) or max_states < 1:
        raise ValueError(f"max_states must be an int >= 1, got {max_states!r}")
    cap = int(min(int(max_states), (a.n_states + 1) * (b.n_states + 1)))  # (no product has more pairs)
    if cap > _lib.FSA_MAX_STATES:
        raise ValueError(f"max_states={max_states}: the device search numbers at most {_lib.FSA_MAX_STATES} states")
    eng = getattr(llm_or_engine, "engine", llm_or_engine)
    tables, pairs, _ = DeviceTables.upload(eng, a).product(DeviceTables.upload(eng, b), op, cap)  # (it can pass cap only where cap is max_states)
    kind = ByteWFSA if tables.weighted else ByteDFA
    host = lambda t: t.cpu().numpy()
    if tables.weighted:
        fin = host(tables.final_logw)
        return kind._from_device(host(tables.delta), fin > -np.inf, 0, host(tables.live), host(tables.arc_logw), fin), pairs
    return kind._from_device(host(tables.delta), host(tables.accepting), 0, host(tables.live)), pairs


def determinize(llm_or_engine, nfa, max_states=65536, *, _hash_mask=0, _batch=_BATCH):
    """(automaton, sets, states): the `ByteDFA` of the byte strings that the `ByteNFA` `nfa` accepts, by the subset
    construction on the device (include/glb.h glb_nfa_closure / glb_nfa_subset_round); host uint64 [S, W], every
    state's set of NFA states as a bitset; and int32 [n_important], the NFA state behind every bit (bit i of a set is word
    i // 64, bit i % 64).  A state of `nfa` is important when it has a byte arc or accepts; a state of the result is the set
    of important states inside the empty-arc closure of what was reached, W = max(1, ceil(n_important / 64)).  State 0 is the
    closure of the start; the empty set is no state - an arc into it is -1 - and a state accepts where its set holds an
    accepting state.  The states are numbered in the order in which a queue search first meets the sets (states in id
    order, bytes ascending), the rule of `product`; nothing is trimmed or merged (`minimize`, `DeviceConstraint(minimize=
    True)`), and `live` of the result comes from the device.  ValueError, before the device is touched, for something that
    is no `ByteNFA`, a `max_states` that is no int >= 1, and more than 4096 important states (a set is one wave of 64-bit
    words); and when the search passes `max_states` states before it ends: nothing partial is returned, the message names
    `max_states` and the count reached when the search stopped.  The outputs are allocated for `max_states` rows before the
    search (1 KB and W words a row); no automaton has more than 2^n_important states, so a larger `max_states` allocates
    that many, and the device numbers at most 2^22."""
    from .nfa import ByteNFA

    if isinstance(nfa, ByteWFSA):
        raise ValueError("determinize takes an unweighted ByteNFA: weighted determinisation need not terminate")
    if not isinstance(nfa, ByteNFA):
        raise ValueError(f"determinize needs a ByteNFA (ByteNFA.from_dfa wraps a ByteDFA), got {type(nfa).__name__}")
    if isinstance(max_states, bool) or not isinstance(max_states, (int, np.integer)) or max_states < 1:
        raise ValueError(f"max_states must be an int >= 1, got {max_states!r}")
    n_imp = int(nfa.important.sum())
    if n_imp > _lib.NFA_MAX_IMPORTANT:
        raise ValueError(f"determinize: {n_imp} important states (those with a byte arc, and the accepting ones) pass the cap of "
                         f"{_lib.NFA_MAX_IMPORTANT}: a set of them is one wave of 64-bit words")
    cap = int(min(int(max_states), 1 << min(n_imp, 30)))  # (no automaton has more sets)
    if cap > _lib.NFA_MAX_STATES:
        raise ValueError(f"max_states={max_states}: the device search numbers at most {_lib.NFA_MAX_STATES} states")
    eng = getattr(llm_or_engine, "engine", llm_or_engine)
    arrays = _nfa_arrays(nfa)
    p, buf = _nfa_block(eng, arrays, cap, _hash_mask)
    n = _nfa_search(eng, p, buf["status"], _batch)["states"]  # (it can pass cap only where cap is max_states)
    live = _nfa_live(eng, buf["delta"], buf["accepting"], n)
    host = lambda t: t[:n].cpu().numpy()
    dfa = ByteDFA._from_device(host(buf["delta"]), host(buf["accepting"]), 0, host(live))
    return dfa, np.ascontiguousarray(host(buf["sets"]).view(np.uint64)), arrays["states"]
