"""An automaton's tables on the device, pushed and minimised (§21) there before they are served:
`DeviceConstraint` and the standalone `minimize` prepare theirs through the same three calls, `upload`, `pushed`, `minimized`."""
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
        p.restart = 1
        n = converged = flags = 0
        while not converged and not flags and n < budget and not stop(n):
            setattr(p, count, min(_BATCH, budget - n))
            self.eng.dfa_call(name, p)
            p.restart = 0
            n, converged, flags = status[:3].tolist()
        return n, converged, flags

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


def _put(eng, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


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
