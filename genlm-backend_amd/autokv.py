"""KV rows that follow the contexts of a stateless API.

`AsyncAmdLM.batch_next_token_step` is handed plain token lists, step after step; a population that grows by one token
per step asks for contexts whose first L - 1 tokens were evaluated the step before.  The reference re-encodes them in
full unless the caller pinned a prompt with `cache_kv` (hf.py:155-164); its MLX backend keeps per-token KV on the
trie's nodes instead (mlx.py:177-318, cache.py:103-191).  `AutoKV` is that idea on slab rows: R rows of `cap` positions
(`kv.SharedSlabKV`), a device table of the context every row holds (tokens, length, hash), and per call

  * a lookup of every distinct context - the row that holds exactly it, else the row that holds its first L - 1 tokens
    (glb_match_rows: hashes select candidates, every candidate's tokens are compared: a hash never decides alone);
  * contexts with a row feed ONE token (the first to claim a row keeps it, the others get a copy of the prefix in a row
    nobody used for the longest time: copy-on-append); contexts without one are encoded from their tokens and their
    KV kept if a row is to be had;
  * the table rows of everything that now holds a context are rewritten.

With `chunk` = K > 1 (AsyncAmdLM's auto_kv_chunk) a context is served by ANY row it shares a prefix with,
as long as the tokens behind the shared prefix are at most K: glb_match_prefix_rows finds the row with the longest shared
prefix (`keep` tokens), glb_kv_plan_chunk feeds the context its last L - keep tokens in one forward
(glb_slab_attention_chunk) - a context that grew by several tokens, shrank and grew again, or forks off a longer one.  A
row that holds more than keep + 1 tokens is never truncated: the context takes a copy of the shared prefix.  K = 1 is the
lookup and the plan above, unchanged.

Lookup and block table run on the device (glb_match_rows, glb_kv_plan: one launch each), like `DeviceSIS._step_shared_kv`;
the host reads the numbers of rows of each kind from the call's one D2H copy and launches the forwards (kv.SlabRunner).
"""
import torch

from .kv import SlabRunner


class AutoKV:
    def __init__(self, llm, rows, cap=64, in_place=0.75, graph=True, chunk=1):
        self.llm, self.eng, self.dev = llm, llm.engine, llm.device
        self.R, self.cap, self.chunk = int(rows), int(cap), int(chunk)
        self.kv = SlabRunner(llm, rows, cap, in_place, graph)  # the slabs (they outlive a reset) and the forwards over them
        self.reset()

    pkv = property(lambda self: self.kv.pkv)
    _slab_fwd = property(lambda self: self.kv._slab_fwd)
    in_place = property(lambda self: self.kv.in_place, lambda self, v: setattr(self.kv, "in_place", v))

    def reset(self):
        dev, R, cap = self.dev, self.R, self.cap
        self.row_tok = torch.zeros((R, cap), dtype=torch.int32, device=dev)
        self.row_len = torch.zeros(R, dtype=torch.int32, device=dev)       # 0: the row holds nothing
        self.row_hash = torch.zeros(R, dtype=torch.int64, device=dev)
        self.stamp = torch.zeros(R, dtype=torch.int64, device=dev)          # call in which the row was last used
        self.t = 0
        self.last = None  # (plan, counts, (chunk rows, most tokens fed)) of the latest call: tests and tools read it
        self.stats = dict(calls=0, forward_rows=0, one_token_rows=0, encoded_rows=0, copied_rows=0, unkept_rows=0,
                          in_place_calls=0, chunk_rows=0, chunk_tokens=0)

    @torch.no_grad()
    def logits(self, tok_d, st_d, ln_d, group_of, rep, ng, extra_head=()):
        """Next-token logits rows of the call's distinct contexts.  tok_d / st_d / ln_d: the ragged batch on the device;
        group_of, rep, ng: glb_group_contexts' output.  Returns (logits [U, V], row_of_group int32 [n] device: the
        logits row of dedup group g, group_of_row int64 [U]: its inverse, U, extra: the host values of `extra_head`'s
        device scalars - they ride on the call's one D2H copy)."""
        eng, dev, R, cap = self.eng, self.dev, self.R, self.cap
        # the row that holds every distinct context, or its first L - 1 tokens (every candidate's tokens are compared:
        # a hash never decides alone), then the block table - both on the device, one launch each
        self.t += 1
        if self.chunk > 1:
            return self._logits_chunk(tok_d, st_d, ln_d, group_of, rep, ng, extra_head)
        old, gh = eng.match_rows(tok_d, st_d, ln_d, rep, ng, self.row_tok, self.row_len, self.row_hash)
        plan = eng.kv_plan(group_of, rep, ng, old, ln_d, R, cap, stamps=self.stamp, call_no=self.t,
                           table=(self.row_tok, self.row_len, self.row_hash, gh, tok_d, st_d))
        head = torch.cat([plan["head"][:6], *[e.to(torch.int32).view(1) for e in extra_head]]).cpu().tolist()  # the one D2H copy
        counts, extra = head[:6], head[6:]
        return self._forwards(plan, counts, (0, 0), 0, extra, tok_d, st_d, ln_d)

    def _logits_chunk(self, tok_d, st_d, ln_d, group_of, rep, ng, extra_head):
        """`logits` with auto_kv_chunk > 1: the row with the longest shared prefix, up to `chunk` tokens fed per row."""
        eng, R, cap = self.eng, self.R, self.cap
        old, keep, gh = eng.match_prefix_rows(tok_d, st_d, ln_d, rep, ng, self.row_tok, self.row_len, self.row_hash, self.chunk)
        plan = eng.kv_plan_chunk(group_of, rep, ng, old, keep, ln_d, R, cap, stamps=self.stamp, call_no=self.t,
                                 table=(self.row_tok, self.row_len, self.row_hash, gh, tok_d, st_d))
        fed = plan["n_new_of_row"]
        chunk_tokens = (fed * (fed > 1)).sum().to(torch.int32).view(1)  # tokens fed to the rows that are fed more than one
        head = torch.cat([plan["head"], chunk_tokens, *[e.to(torch.int32).view(1) for e in extra_head]]).cpu().tolist()  # the one D2H copy
        return self._forwards(plan, head[:6], (head[8], head[9]), head[10], head[11:], tok_d, st_d, ln_d)

    def _forwards(self, plan, counts, chunk, chunk_tokens, extra, tok_d, st_d, ln_d):
        dev = self.dev
        U, nA, nB, n_copied, n_unkept, _ = counts
        self.last = (plan, tuple(counts), tuple(chunk))
        st = self.stats
        st["calls"] += 1
        st["forward_rows"] += U
        st["one_token_rows"] += nA - chunk[0]
        st["chunk_rows"] += chunk[0]
        st["chunk_tokens"] += chunk_tokens
        st["encoded_rows"] += nB
        st["copied_rows"] += n_copied
        st["unkept_rows"] += n_unkept
        # rows outside an in-place forward still hold contexts the table knows: hence row_len (SlabRunner.run)
        logits, _, in_place = self.kv.run(plan, counts, lambda ctx, pos: tok_d[st_d[ctx] + pos], (tok_d, st_d, ln_d),
                                          pad_id=self.llm._pad_id, row_len=self.row_len, chunk=chunk)
        st["in_place_calls"] += int(in_place)
        row_of_group = plan["logits_row"]
        group_of_row = torch.empty(U, dtype=torch.int64, device=dev)
        group_of_row[row_of_group[:U].long()] = torch.arange(U, device=dev)
        return logits, row_of_group, group_of_row, U, extra
