"""A byte-level language model out of a token model: next-byte distributions from a beam over tokenisations.

`p(next byte | byte prefix)` of a token model sums over every token sequence that spells the prefix (Vieira et al. 2024, "From
Language Models over Tokens to Language Models over Characters").  `ByteBeam` keeps, per prefix, the `width` heaviest
candidates (token context x, trie node n, u = log p(x)): the tokens committed so far and the bytes read since, as a node of
the token -> byte trie.  A candidate's weight is w = u + log M_x[n], M_x the trie masses (`TokenByteTrie.masses_from_logits`)
of x's next-token distribution.  One byte costs two selections' masses, three small kernels (glb_bytelm_children /
_extend / _next) and a forward over the candidates that just committed a token - the others keep their logits row.

Not here: more than one device, LoRA names, `constraints` (the row is [n, 257]: a byte constraint is a 257-wide mask - a
follow-up), and pruning by a threshold relative to the best weight."""
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

    State per slot (group g owns slots g * width .. g * width + width - 1; a candidate never moves): `node`, `alive` int32,
    `u`, `w` float32, `contexts` int32 [n * width, cap] and `lengths`, the logits row store [n * width, V] in the model's
    logits dtype with `lse`; `logp` float32 [n] per group."""

    def __init__(self, llm, byte_vocab, eos_ids, width=16, n=1, prompt_ids=None, temperature=1.0, max_bytes=256, ignore_ids=()):
        check_width(width)
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
    def next_byte_logprobs(self):
        """float32 [n, 257] on the device: log p(next byte | the bytes so far) for the 256 bytes and, in column 256, EOS.  A
        group without a live candidate (ended, or advanced by a byte no tokenisation spells) has a row of -inf.  The same
        tensor until the next `advance`."""
        if self._row is None:
            self._prepare()
            self._row, self._logZ = self.eng.bytelm_next(self._trie, self.node, self.u, self.w, self.alive, self._sel, self._mass, self.width)
        return self._row

    def advance(self, byte):
        """Read one byte per group: an int32 [n] device tensor or a list of ints - 0..255, 256 to end the group with EOS, -1 to
        leave it where it is.  `logp` grows by the row's entry."""
        if not torch.is_tensor(byte):
            byte = torch.tensor([int(b) for b in byte], dtype=torch.int32, device=self.dev)
        if byte.dtype != torch.int32 or byte.shape != (self.n,) or byte.device != self.dev:
            raise ValueError(f"byte must be an int32 [{self.n}] tensor on {self.dev}, or a list of {self.n} ints")
        if self.t >= self.max_bytes:
            raise ValueError(f"max_bytes = {self.max_bytes} bytes have been read")
        self._prepare()
        self.eng.bytelm_next(self._trie, self.node, self.u, self.w, self.alive, self._sel, self._mass, self.width,
                             byte=byte.contiguous(), logp=self.logp, fresh=self.fresh)
        self.t += 1
        self._sel = self._mass = self._row = self._logZ = None

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
        the most probable entry), stopping a group at EOS.  Returns one bytes object per group."""
        gen = torch.Generator(device=self.dev)
        gen.manual_seed(int(seed))
        done = torch.zeros(self.n, dtype=torch.bool, device=self.dev)
        picked = []
        for _ in range(min(max_bytes, self.max_bytes - self.t)):
            row = self.next_byte_logprobs()
            done = done | ~torch.isfinite(row.max(dim=1).values)
            p = torch.where(done[:, None], torch.ones_like(row), row.exp())  # (a finished group's draw is not used)
            choice = p.argmax(dim=1) if greedy else torch.multinomial(p, 1, generator=gen)[:, 0]
            byte = torch.where(done, torch.full_like(choice, -1), choice).to(torch.int32)
            picked.append(byte)
            self.advance(byte)
            done = done | (byte == EOS)
        if not picked:
            return [b""] * self.n
        host = torch.stack(picked, dim=1).cpu().numpy()
        return [bytes(int(b) for b in host[g] if 0 <= b < 256) for g in range(self.n)]
