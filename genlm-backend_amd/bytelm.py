"""A byte-level language model out of a token model: next-byte distributions from a beam over tokenisations.

`p(next byte | byte prefix)` of a token model sums over every token sequence that spells the prefix (Vieira et al. 2024, "From
Language Models over Tokens to Language Models over Characters").  `ByteBeam` keeps, per prefix, the `width` heaviest
candidates (token context x, trie node n, u = log p(x)): the tokens committed so far and the bytes read since, as a node of
the token -> byte trie.  A candidate's weight is w = u + log M_x[n], M_x the trie masses (`TokenByteTrie.masses_from_logits`)
of x's next-token distribution.  One byte costs two selections' masses, three small kernels (glb_bytelm_children /
_extend / _next) and a forward over the candidates that just committed a token - the others keep their logits row.

Under a byte automaton (`ByteBeam(constraint=...)`) a state constrains the next byte with one 256-entry row of
its `delta`: no row bank, no fill, nothing that depends on the tokeniser.  glb_bytelm_step does the row, the automaton's row,
the renormalisation, the draw and the advance in one launch; `ByteSIS` is sequential importance sampling over bytes on top.

Not here: more than one device, LoRA names, byte-level `BytePDA`s and lazy `ByteNFA`s (determinise an NFA first), token-level
`*Constraint` objects, one automaton per group, proposals other than the constrained row, and pruning by a threshold
relative to the best weight."""
import math

import numpy as np
import torch

from .tokenization import Token
from .trie import TokenByteTrie

MAX_LEAVES = 4  # leaf children of one node (equal byte strings under different ids; the EOS ids at the root): GLB_BYTELM_LEAVES
MAX_WIDTH = 64
EOS = 256  # the EOS column of a next-byte row, and the "byte" that ends a group


def check_width(width):
    if not isinstance(width, int) or isinstance(width, bool) or not 1 <= width <= MAX_WIDTH:
        raise ValueError(f"width must be an integer in 1..{MAX_WIDTH}, got {width!r}")
    return width


def check_constraint(constraint):
    """`constraint` if a byte beam can serve it - None, a `ByteDFA`, a `ByteWFSA` or a `DeviceTables` with `live` - else
    ValueError naming its kind.  Touches no device."""
    from .constraints.automata import ByteDFA
    from .constraints.nfa import ByteNFA
    from .constraints.tables import DeviceTables

    if constraint is None or isinstance(constraint, ByteDFA):
        return constraint
    if isinstance(constraint, DeviceTables):
        if constraint.live is None:
            raise ValueError("constraint is a DeviceTables without `live` (as `minimized` returns them): upload a host automaton")
        return constraint
    kind = type(constraint).__name__
    if isinstance(constraint, ByteNFA):
        raise ValueError(f"constraint is a {kind}: a byte beam follows one state per group - `determinize` the NFA first and "
                         f"pass the ByteDFA")
    raise ValueError(f"constraint must be a ByteDFA, a ByteWFSA or a DeviceTables, got a {kind} (a BytePDA and the token-level "
                     f"*Constraint objects are not served at byte level; `determinize` a ByteNFA first)")


def byte_trie(byte_vocab, eos_ids, ignore_ids=(), engine=None):
    """The `TokenByteTrie` a byte beam walks: token k spells byte_vocab[k]; the tokens of `eos_ids` (1 to 4) and of
    `ignore_ids` spell nothing, so their leaves hang off the root - the EOS leaves are the root's leaf children, the ignored
    ones are never selected (`child_sym` -2).  Refused by name: an empty token that is in neither list, and a node with more
    than four leaf children."""
    vocab = [bytes(t) for t in byte_vocab]
    eos = [int(t) for t in eos_ids]
    ignore = sorted({int(t) for t in ignore_ids})
    if not 1 <= len(eos) <= MAX_LEAVES or len(set(eos)) != len(eos):
        raise ValueError(f"eos_ids must name 1..{MAX_LEAVES} distinct tokens, got {list(eos_ids)!r}")
    for t in eos + ignore:
        if not 0 <= t < len(vocab):
            raise ValueError(f"token id {t} outside the vocabulary of {len(vocab)} tokens")
    if set(eos) & set(ignore):
        raise ValueError(f"tokens {sorted(set(eos) & set(ignore))} are both EOS and ignored")
    silent = set(eos) | set(ignore)
    for k, word in enumerate(vocab):
        if not word and k not in silent:
            raise ValueError(f"token {k} has an empty byte string and is neither in eos_ids nor in ignore_ids")
    trie = TokenByteTrie([Token(k, b"" if k in silent else word) for k, word in enumerate(vocab)], engine=engine, ignore_ids=ignore)
    f = trie.flat()
    over = np.nonzero(f["child_sym"] >= 256 + MAX_LEAVES)[0]
    if len(over):
        at = int(np.searchsorted(f["child_ptr"], over[0], side="right") - 1)
        ids = [int(sym[1]) for sym in trie.children[at] if isinstance(sym, tuple) and sym[0] is None and sym[1] not in trie.ignore_ids]
        raise ValueError(f"tokens {ids} all spell {bytes(trie.node2prefix[at])!r}: more than {MAX_LEAVES} tokens with equal bytes")
    return trie


def byte_trie_arrays(trie):
    """Host arrays of the glb_bytelm_* calls over `byte_trie(...)`: the CSR with its edge symbols, the leaf -> token table,
    the root.  `HipEngine.bytelm_*` take the same dict with the arrays on the device."""
    f = trie.flat()
    leaf_token = np.full(f["n_nodes"], -1, np.int32)
    leaf_token[trie.idx_to_leaf[:, 1]] = trie.idx_to_leaf[:, 0]
    return dict(n_nodes=int(f["n_nodes"]), root=int(trie.root), child_ptr=f["child_ptr"], child_idx=f["child_idx"],
                child_sym=f["child_sym"], leaf_token=leaf_token)


def children_table(trie, nodes):
    """What glb_bytelm_children writes for alive slots at `nodes`, on the host: int32 [len(nodes), 260]."""
    f = trie.flat()
    out = np.full((len(nodes), 260), -1, np.int32)
    for r, n in enumerate(nodes):
        lo, hi = f["child_ptr"][n], f["child_ptr"][n + 1]
        sym = f["child_sym"][lo:hi].astype(np.int64)
        ok = (sym >= 0) & (sym < 260)
        out[r, sym[ok]] = f["child_idx"][lo:hi][ok]
    return out


class ByteBeam:
    """Next-byte distributions of `llm` over `n` byte prefixes at once, each a group of at most `width` candidates.

    byte_vocab   the byte string of every token id (bytes or `Token`s, as `decode_vocab` returns them)
    eos_ids      1 to 4 token ids that end a text: column 256 of a row is their summed probability at a token boundary
    ignore_ids   tokens that can never be part of a text (padding, other specials): their mass is dropped and the rows'
                 normalisation absorbs it; an empty byte string that is in neither list is refused
    prompt_ids   the token context every group starts from (default [bos_token_id] when the tokenizer has one)
    max_bytes    bytes a group may be advanced by; the token capacity of a context is prompt + max_bytes + 1
    constraint   None, or a byte automaton every group follows from its start state: a `ByteDFA`, a `ByteWFSA` (uploaded
                 once) or a `DeviceTables`.  Then the rows are constrained and renormalised, and per group there are
                 `state` int32 [n] (-1 once ended or dead), `ended` int32 [n] (1 after EOS from an accepting state) and
                 `log_weights` float32 [n]: the sum of what the automaton gave the bytes read (`advance`: the byte's weight,
                 0 for an allowed byte of a `ByteDFA`, -inf for a forbidden one) and of log Zc for the bytes drawn (`step`).
                 Without one, none of the three exists.

    State per slot (group g owns slots g * width .. g * width + width - 1; a candidate never moves): `node`, `alive` int32,
    `u`, `w` float32, `contexts` int32 [n * width, cap] and `lengths`, the logits row store [n * width, V] in the model's
    logits dtype with `lse`; `logp` float32 [n] per group."""

    def __init__(self, llm, byte_vocab, eos_ids, width=16, n=1, prompt_ids=None, temperature=1.0, max_bytes=256, ignore_ids=(),
                 constraint=None):
        check_width(width)
        check_constraint(constraint)
        if not isinstance(n, int) or n < 1:
            raise ValueError(f"n must be a positive integer, got {n!r}")
        if not isinstance(max_bytes, int) or max_bytes < 1:
            raise ValueError(f"max_bytes must be a positive integer, got {max_bytes!r}")
        if not float(temperature) > 0.0:
            raise ValueError(f"temperature must be > 0, got {temperature!r}")
        self.trie = byte_trie(byte_vocab, eos_ids, ignore_ids, engine=getattr(llm, "engine", None))
        if prompt_ids is None:
            bos = getattr(getattr(llm, "tokenizer", None), "bos_token_id", None)
            if bos is None:
                raise ValueError("the tokenizer has no bos token: give prompt_ids")
            prompt_ids = [int(bos)]
        prompt = [int(t) for t in prompt_ids]
        if not prompt:
            raise ValueError("prompt_ids needs at least one token")
        self.llm, self.eng, self.dev = llm, llm.engine, llm.device
        self.width, self.n, self.N = width, n, n * width
        self.scale, self.max_bytes, self.prompt = 1.0 / float(temperature), max_bytes, prompt
        self.eos_ids = [int(t) for t in eos_ids]
        self.cap = len(prompt) + max_bytes + 1
        host = byte_trie_arrays(self.trie)
        self._trie = {k: (torch.from_numpy(v).to(self.dev) if isinstance(v, np.ndarray) else v) for k, v in host.items()}
        self.root = host["root"]
        ctx = np.zeros((self.N, self.cap), np.int32)
        ctx[:, :len(prompt)] = prompt
        self._ctx0 = torch.from_numpy(ctx).to(self.dev)
        slot = torch.arange(self.N, device=self.dev)
        self._first = slot % width == 0
        self._first_slots = slot[self._first].to(torch.int32).contiguous()
        self.store = self.lse = None
        self.forwarded = 0  # contexts handed to the model so far (equal ones are encoded once: `llm._count`)
        self.tables = None
        if constraint is not None:
            from .constraints.tables import DeviceTables

            self.tables = constraint if isinstance(constraint, DeviceTables) else DeviceTables.upload(self.eng, constraint)
        self.reset()

    def reset(self):
        """Every group back to one candidate: the prompt, nothing read, logp 0.  The logits rows are fetched again."""
        dev, N = self.dev, self.N
        ninf = torch.full((N,), float("-inf"), dtype=torch.float32, device=dev)
        self.contexts = self._ctx0.clone()
        self.lengths = torch.full((N,), len(self.prompt), dtype=torch.int32, device=dev)
        self.node = torch.full((N,), self.root, dtype=torch.int32, device=dev)
        self.alive = self._first.to(torch.int32)
        self.u = torch.where(self._first, torch.zeros_like(ninf), ninf)
        self.w = self.u.clone()
        self.logp = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.fresh = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.t = 0
        if self.tables is not None:
            self.state = torch.full((self.n,), self.tables.start, dtype=torch.int32, device=dev)
            self.ended = torch.zeros(self.n, dtype=torch.int32, device=dev)
            self.log_weights = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self._pending = (self._first_slots, self.n)  # slots whose logits row is still to be fetched
        self._sel = self._mass = self._row = self._logZ = None

    # ---- the model ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _forward(self, slots, count):
        """Logits rows of the contexts in `slots` (int32 [count], on the device) into the store, through the device pipeline of
        `batch_next_token_topk_device`: equal contexts are encoded once, KV rows serve one-token extensions."""
        idx = slots.long()

        def finish(logits, row_of, group_of, U, n, mid_d, row_mid, by_row, constraint=None):
            rows = logits[:U]
            if self.store is None:
                self.store = torch.zeros((self.N, rows.shape[1]), dtype=rows.dtype, device=self.dev)
                self.lse = torch.zeros(self.N, dtype=torch.float32, device=self.dev)
            pick = row_of.long()
            self.store.index_copy_(0, idx, rows[pick])
            self.lse.index_copy_(0, idx, self.eng.row_lse(rows, vocab=len(self.trie.decode), logit_scale=self.scale)[pick])
            self.llm._count(n, U, U)
            return None

        self.llm._batch_step(self.contexts.view(-1), idx * self.cap, self.lengths[idx].contiguous(), count, None, l_max=None,
                             finish=finish)
        self.forwarded += count

    def _masses(self, wide):
        self._sel = self.eng.bytelm_children(self._trie, self.node, self.alive, self.width)
        self._mass = self.trie.masses_from_logits(self.store, lse=self.lse, nodes=self._sel, logit_scale=self.scale,
                                                  wide_selections=wide)

    @torch.no_grad()
    def _prepare(self):
        """Steps 1 and 2 of a byte step: extend the groups that moved, forward the spawned candidates; afterwards `_sel` and
        `_mass` describe the state the rows are read from and an advance moves."""
        if self._sel is not None:
            return
        at_start = self._pending is not None
        if at_start:
            self._forward(*self._pending)
            self._pending = None
        self._masses(wide=at_start)
        out = self.eng.bytelm_extend(self._trie, self.node, self.u, self.w, self.alive, self._sel, self._mass, self.width, fresh=self.fresh)
        count = int(out["n_spawned"].item())  # the step's one D2H copy: how many contexts the model is asked for
        self.node, self.u, self.w, self.alive = out["node"], out["u"], out["w"], out["alive"]
        if count:
            slots = out["spawned"][:count]
            idx = slots.long()
            parent = out["parent"][idx].long()
            ctx, ln = self.contexts[parent], self.lengths[parent]  # (copies: a parent's slot may be one of the targets)
            ctx[torch.arange(count, device=self.dev), ln.long()] = out["token"][idx]
            self.contexts.index_copy_(0, idx, ctx)
            self.lengths.index_copy_(0, idx, ln + 1)
            self._forward(slots, count)
            self._masses(wide=True)

    # ---- the interface --------------------------------------------------------------------------------------------------------
    def _step(self, **kw):
        """glb_bytelm_step over the beam's state as it stands after `_prepare`."""
        return self.eng.bytelm_step(self._trie, self.node, self.u, self.w, self.alive, self._sel, self._mass, self.width, self.tables,
                                    self.state, self.ended, self.log_weights, self.logp, fresh=self.fresh, **kw)

    def next_byte_logprobs(self):
        """float32 [n, 257] on the device: log p(next byte | the bytes so far) for the 256 bytes and, in column 256, EOS.  A
        group without a live candidate (ended, or advanced by a byte no tokenisation spells) has a row of -inf.  Under a
        constraint: the row restricted to what the group's state allows and renormalised - forbidden columns are exactly
        -inf, a dead group's row is all -inf.  The same tensor until the next `advance` or `step`."""
        if self._row is None:
            self._prepare()
            if self.tables is None:
                self._row, self._logZ = self.eng.bytelm_next(self._trie, self.node, self.u, self.w, self.alive, self._sel, self._mass, self.width)
            else:
                out = self._step(peek=True, want_row=True)
                self._row, self._logZ = out["row"], out["logZc"]
        return self._row

    def next_byte_logZ(self):
        """float32 [n] beside `next_byte_logprobs()`: under a constraint log Zc, the log of the mass the unconstrained row
        (weighted by the automaton's arcs) leaves on what the state allows; without one the log of the candidates' mass."""
        self.next_byte_logprobs()
        return self._logZ

    def _bytes(self, byte):
        if not torch.is_tensor(byte):
            byte = torch.tensor([int(b) for b in byte], dtype=torch.int32, device=self.dev)
        if byte.dtype != torch.int32 or byte.shape != (self.n,) or byte.device != self.dev:
            raise ValueError(f"byte must be an int32 [{self.n}] tensor on {self.dev}, or a list of {self.n} ints")
        if self.t >= self.max_bytes:
            raise ValueError(f"max_bytes = {self.max_bytes} bytes have been read")
        return byte.contiguous()

    def advance(self, byte):
        """Read one byte per group: an int32 [n] device tensor or a list of ints - 0..255, 256 to end the group with EOS, -1 to
        leave it where it is.  `logp` grows by the unconstrained row's entry; under a constraint the state moves and
        `log_weights` grows by the weight the automaton gives the byte (a forbidden byte kills the group: weight -inf)."""
        byte = self._bytes(byte)
        self._prepare()
        if self.tables is None:
            self.eng.bytelm_next(self._trie, self.node, self.u, self.w, self.alive, self._sel, self._mass, self.width,
                                 byte=byte, logp=self.logp, fresh=self.fresh)
        else:
            self._step(byte=byte)
        self.t += 1
        self._sel = self._mass = self._row = self._logZ = None

    def step(self, seed=None, uniform=None):
        """Under a constraint: draw one byte per group from the constrained row and read it, one launch after `_prepare()`.
        `uniform` float32 [n] in [0, 1): the first column whose cumulative probability exceeds it; else one Philox uniform
        per group from (`seed` (None: 0), the number of bytes read so far, the group).  `log_weights` grows by log Zc.
        Returns the bytes, int32 [n] on the device: 256 for EOS, -1 for a group that has ended or died."""
        if self.tables is None:
            raise ValueError("step() draws under a constraint: this beam has none (generate() draws from the plain rows)")
        if self.t >= self.max_bytes:
            raise ValueError(f"max_bytes = {self.max_bytes} bytes have been read")
        if uniform is not None and (not torch.is_tensor(uniform) or uniform.dtype != torch.float32 or uniform.shape != (self.n,)):
            raise ValueError(f"uniform must be a float32 [{self.n}] tensor")
        self._prepare()
        out = self._step(uniform=uniform, seed=0 if seed is None else int(seed), offset=self.t)
        self.t += 1
        self._sel = self._mass = self._row = self._logZ = None
        return out["byte"]

    def prefill(self, prefixes):
        """Advance group g through the bytes object prefixes[g] (shorter ones wait for the longest)."""
        if len(prefixes) != self.n:
            raise ValueError(f"{len(prefixes)} prefixes for {self.n} groups")
        prefixes = [bytes(p) for p in prefixes]
        for i in range(max(len(p) for p in prefixes)):
            self.advance([p[i] if i < len(p) else -1 for p in prefixes])

    def candidates(self, g):
        """Group g's live candidates on the host, for inspection: [(committed tokens, the bytes read since the last of them,
        u, w)], in slot order."""
        lo, hi = g * self.width, (g + 1) * self.width
        P = len(self.prompt)
        ctx, ln = self.contexts[lo:hi].cpu().numpy(), self.lengths[lo:hi].cpu().numpy()
        node, alive = self.node[lo:hi].cpu().numpy(), self.alive[lo:hi].cpu().numpy()
        u, w = self.u[lo:hi].cpu().numpy(), self.w[lo:hi].cpu().numpy()
        return [([int(t) for t in ctx[i, P:ln[i]]], bytes(self.trie.node2prefix[int(node[i])]), float(u[i]), float(w[i]))
                for i in range(self.width) if alive[i]]

    @torch.no_grad()
    def generate(self, max_bytes=64, seed=0, greedy=False):
        """Draw up to `max_bytes` further bytes per group from the rows (`torch.multinomial` on the [n, 257] matrix; greedy:
        the most probable entry), stopping a group at EOS.  Returns one bytes object per group.  Under a constraint the draws
        are `step(seed)`'s, one Philox offset per byte position, and the greedy choice is the constrained row's: every text
        is a prefix of a string of the language."""
        steps = min(max_bytes, self.max_bytes - self.t)
        if self.tables is not None and not greedy:
            picked = [self.step(seed=seed) for _ in range(steps)]
            return self._texts(picked)
        gen = torch.Generator(device=self.dev)
        gen.manual_seed(int(seed))
        done = torch.zeros(self.n, dtype=torch.bool, device=self.dev)
        picked = []
        for _ in range(steps):
            row = self.next_byte_logprobs()
            done = done | ~torch.isfinite(row.max(dim=1).values)
            p = torch.where(done[:, None], torch.ones_like(row), row.exp())  # (a finished group's draw is not used)
            choice = p.argmax(dim=1) if greedy else torch.multinomial(p, 1, generator=gen)[:, 0]
            byte = torch.where(done, torch.full_like(choice, -1), choice).to(torch.int32)
            picked.append(byte)
            self.advance(byte)
            done = done | (byte == EOS)
        return self._texts(picked)

    def _texts(self, picked):
        if not picked:
            return [b""] * self.n
        host = torch.stack(picked, dim=1).cpu().numpy()
        return [bytes(int(b) for b in host[g] if 0 <= b < 256) for g in range(self.n)]


class ByteSIS:
    """Sequential importance sampling over bytes under a byte automaton: the byte-level twin of `DeviceSIS`.

    A particle is one group of a `ByteBeam(width=width, n=n, constraint=automaton)`.  A step draws every particle's next byte
    from the model's next-byte row restricted to what the automaton's state allows (weighted by its arcs) and multiplies
    the particle's weight by the mass Zc that row had before it was renormalised (glb_bytelm_step: one launch a step beside
    the beam's own).  `run()` steps until every particle has ended (EOS from an accepting state) or died (nothing allowed
    had mass), or `max_bytes` steps; it reads back one small flag every `CHECK_EVERY` steps (with `resample_ess`: two
    scalars every step), never a row.  The drawn bytes stay on the device, int32 [n, max_bytes], until `results()`.

    automaton     a `ByteDFA`, a `ByteWFSA` or a `DeviceTables`; a weight of the `ByteWFSA` multiplies the target
    prefix        bytes every particle reads first (`ByteBeam.prefill`: the automaton moves along, its weights for them count)
    resample_ess  None: never.  r: after a step, when the effective sample size of the weights is below r * n, ancestors are
                  drawn systematically (`HipEngine.resample_systematic`, as `DeviceSIS`: ended particles take part, dead ones
                  have no weight) and every per-group and per-slot tensor is gathered by ancestor - slot j of group g from
                  slot j of group anc[g] - the logits store included: n * width * V elements copied per resampling
                  (DESIGN.md §33); the weights become their mean.

    `results()`: (texts, log_weights, finished).  A FINITE returned weight means the text is in the automaton's language and
    ended with EOS; a particle that died, or that had neither ended nor died after `max_bytes`, is returned with -inf
    (`sis.log_weights` keeps the raw value) and only an ended particle is `finished`."""

    CHECK_EVERY = 4  # steps between two reads of the stop flag

    def __init__(self, llm, n, automaton, byte_vocab, eos_ids, width=8, prompt_ids=None, prefix=b"", max_bytes=64, temperature=1.0,
                 seed=0, resample_ess=None, ignore_ids=()):
        if automaton is None:
            raise ValueError("ByteSIS needs an automaton: a ByteDFA, a ByteWFSA or a DeviceTables")
        if not isinstance(max_bytes, int) or max_bytes < 1:
            raise ValueError(f"max_bytes must be a positive integer, got {max_bytes!r}")
        if resample_ess is not None and not 0.0 < float(resample_ess) <= 1.0:
            raise ValueError(f"resample_ess must be None or in (0, 1], got {resample_ess!r}")
        self.prefix = bytes(prefix)
        self.beam = ByteBeam(llm, byte_vocab, eos_ids, width=width, n=n, prompt_ids=prompt_ids, temperature=temperature,
                             max_bytes=len(self.prefix) + max_bytes, ignore_ids=ignore_ids, constraint=automaton)
        self.n, self.width, self.max_bytes, self.seed, self.resample_ess = n, width, max_bytes, int(seed), resample_ess
        self.eng, self.dev = self.beam.eng, self.beam.dev
        self.reset()

    def reset(self):
        self.beam.reset()
        if self.prefix:
            self.beam.prefill([self.prefix] * self.n)
        self.bytes = torch.full((self.n, self.max_bytes), -1, dtype=torch.int32, device=self.dev)
        self.t = self.n_resamples = 0

    log_weights = property(lambda self: self.beam.log_weights)
    logp = property(lambda self: self.beam.logp)

    def _open(self):
        """bool [n]: the particles that have neither ended nor died."""
        return (self.beam.ended == 0) & (self.beam.state >= 0)

    @torch.no_grad()
    def step(self):
        """One byte per particle; returns whether to go on when that was read back this step (else None)."""
        self.bytes[:, self.t] = self.beam.step(seed=self.seed)
        self.t += 1
        if self.resample_ess is None:
            return None
        lw = self.beam.log_weights
        wt = torch.exp(lw - lw.max().clamp_min(-3.0e38))  # (all dead: zeros)
        ess, n_open = torch.stack([wt.sum() ** 2 / (wt * wt).sum().clamp_min(1e-30), self._open().sum().float()]).tolist()
        if n_open and self.t < self.max_bytes and ess < self.resample_ess * self.n:  # (ess 0: no weight left, nothing to draw from)
            if ess > 0.0:
                anc, _ = self.eng.resample_systematic(lw, self.seed ^ 0x5eed5a11, self.t)
                self._resample(anc)
        return bool(n_open)

    @torch.no_grad()
    def _resample(self, anc):
        """Particle g becomes a copy of particle anc[g] (int32 / int64 [n] on the device, or a list): torch indexing only."""
        b, n, width = self.beam, self.n, self.width
        if not torch.is_tensor(anc):
            anc = torch.tensor([int(a) for a in anc], device=self.dev)
        a = anc.long()
        if a.shape != (n,):
            raise ValueError(f"anc must name an ancestor for each of the {n} particles")
        slots = (a[:, None] * width + torch.arange(width, device=self.dev)[None, :]).reshape(-1)
        for name in ("contexts", "lengths", "node", "alive", "u", "w", "store", "lse"):
            t = getattr(b, name)
            if t is not None:
                setattr(b, name, t[slots].contiguous())
        for name in ("fresh", "logp", "state", "ended"):
            setattr(b, name, getattr(b, name)[a].contiguous())
        self.bytes = self.bytes[a].contiguous()
        mean = torch.logsumexp(b.log_weights, 0) - math.log(n)
        b.log_weights = mean.expand(n).contiguous()
        b._sel = b._mass = b._row = b._logZ = None  # (they described the slots as they were)
        self.n_resamples += 1

    @torch.no_grad()
    def run(self):
        while self.t < self.max_bytes:
            go = self.step()
            if go is None and (self.t % self.CHECK_EVERY == 0):
                go = bool(self._open().any().item())
            if go is False:
                break
        return self

    def results(self):
        """(texts, log_weights, finished): the prefix and the drawn bytes of every particle (one copy to the host), float32
        [n] on the device with -inf for every particle that is not finished, bool [n] on the device."""
        finished = self.beam.ended != 0
        lw = torch.where(finished, self.beam.log_weights, torch.full_like(self.beam.log_weights, float("-inf")))
        host = self.bytes.cpu().numpy()
        return [self.prefix + bytes(int(v) for v in row if 0 <= v < 256) for row in host], lw, finished

    def log_evidence(self):
        """logsumexp(the finished particles' log-weights) - log n: a 0-dim device tensor."""
        lw = self.beam.log_weights
        return torch.logsumexp(torch.where(self.beam.ended != 0, lw, torch.full_like(lw, float("-inf"))), 0) - math.log(self.n)
