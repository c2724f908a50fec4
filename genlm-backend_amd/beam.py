"""Beam search on the device, under any constraint: the deterministic twin of `sis.DeviceSIS`.

Every prompt is a group of `width` beams.  A step runs one forward over the live beams' contexts (the pipeline of
`AsyncAmdLM.batch_next_token_step_device`), takes every beam's k best continuations under its constraint state's mask row
(glb_topk_rows), keeps each group's `width` best of them and of its finished hypotheses (glb_beam_select), moves token rows
and constraint states to their parents' slots (glb_gather_rows_i32) and appends the tokens (glb_particles_advance).  A
hypothesis's score is the sum of its tokens' log-probabilities under the model - plus, over a `constraints.ByteWFSA`, its
weights - as float32 additions in step order; there is no length normalisation.  Nothing is drawn: no rng, no proposal, and
one device."""
import numpy as np
import torch


class DeviceBeam:
    """width beams (1..64) over each prompt of `prompt_ids` (one prompt, or a list of prompts: one group each), at most
    `max_tokens` tokens a hypothesis, ended by `eos_id`.

    constraint   any constraint of `constraints` (`mask_rows` / `step_masks` / `advance`): a beam's candidates are the tokens
                 its state's row allows; a hypothesis that has `max_tokens` tokens may only end (EOS if its state accepts,
                 else it dies), as in `DeviceSIS`.  Over weighted rows the candidates' values carry the weights, a hypothesis
                 made to end takes its state's final weight after the selection, and the scores start at
                 `constraint.start_logw`.  Without a constraint a hypothesis that reaches `max_tokens` stays as it is: alive.
    k            candidates a beam offers a step (default min(width, 64): no beam can place more than `width`).
    temperature  the log-probabilities are those of softmax(logits / temperature).

    State, as `DeviceSIS` keeps it, beam b of group g in slot g * width + b: `contexts` int32 [G * width, cap], `lengths`,
    `prompt_len`, `active` (int32: still generating), `scores` float32 (-inf: an empty slot), `states`.  After every step a
    group's slots are in score order, best first."""

    def __init__(self, llm, width, prompt_ids, max_tokens, eos_id, constraint=None, k=None, temperature=1.0):
        if not isinstance(width, int) or not 1 <= width <= 64:
            raise ValueError(f"width must be an integer in 1..64, got {width!r}")
        k = min(width, 64) if k is None else k
        if not isinstance(k, int) or not 1 <= k <= 64:
            raise ValueError(f"k must be an integer in 1..64, got {k!r}")
        if not isinstance(max_tokens, int) or max_tokens < 1:
            raise ValueError(f"max_tokens must be a positive integer, got {max_tokens!r}")
        if not float(temperature) > 0.0:
            raise ValueError(f"temperature must be > 0, got {temperature!r}")
        if len(prompt_ids) == 0:
            raise ValueError("no prompt")
        prompts = [list(p) for p in prompt_ids] if isinstance(prompt_ids[0], (list, tuple)) else [list(prompt_ids)]
        if any(len(p) == 0 for p in prompts):
            raise ValueError("a prompt needs at least one token")
        self.llm, self.eng, self.dev = llm, llm.engine, llm.device
        self.width, self.k, self.max_tokens, self.eos_id = width, k, max_tokens, int(eos_id)
        self.temperature, self.constraint = float(temperature), constraint
        self.G, self.N = len(prompts), len(prompts) * width
        self.cap = max(len(p) for p in prompts) + max_tokens + 1
        ctx = np.zeros((self.N, self.cap), np.int32)
        for g, p in enumerate(prompts):
            ctx[g * width:(g + 1) * width, :len(p)] = p
        self._ctx0 = torch.from_numpy(ctx).to(self.dev)
        self._prompt_len0 = torch.tensor([len(p) for p in prompts for _ in range(width)], dtype=torch.int32, device=self.dev)
        slot = torch.arange(self.N, device=self.dev)
        self._base = (slot // width * width).to(torch.int32)  # a slot's group's first slot
        self._first = slot % width == 0
        self._zeros = torch.zeros(self.N, dtype=torch.float32, device=self.dev)
        self.reset()

    def reset(self):
        """One live beam per group - the prompt, at score `constraint.start_logw` (else 0) - and width - 1 empty slots."""
        start = float(getattr(self.constraint, "start_logw", 0.0))
        self.contexts = self._ctx0.clone()
        self.prompt_len = self._prompt_len0.clone()
        self.lengths = self.prompt_len.clone()
        self.active = self._first.to(torch.int32)
        self.scores = torch.where(self._first, torch.full_like(self._zeros, start), torch.full_like(self._zeros, float("-inf")))
        self.states = self.constraint.states0(self.N) if self.constraint is not None else None
        self.t = 0
        self._checked = False

    def n_alive(self):
        """Beams still generating (one small D2H copy)."""
        return int(((self.active > 0) & torch.isfinite(self.scores)).sum().item())

    @torch.no_grad()
    def step(self):
        """One step for every group.  Returns the number of beams that were alive before it (0: the step changed nothing)."""
        eng, con, B = self.eng, self.constraint, self.width
        live = (self.active > 0) & torch.isfinite(self.scores)
        n_live = int(live.sum().item())
        if n_live == 0:
            return 0
        # finished and empty slots still occupy a row: their 1-token stub dedups to one forward row, their candidates are not read
        lengths_eff = torch.where(live, self.lengths, torch.ones_like(self.lengths))
        done = ((self.lengths - self.prompt_len) >= self.max_tokens).to(torch.int32)
        mid = None
        if con is not None:
            mid = con.mask_rows(self.states, done=done)
            mid = torch.where(live, mid, torch.zeros_like(mid))  # (row 0 allows nothing)
        cand_tok, cand_logp = self.llm.batch_next_token_topk_device(self.contexts, lengths_eff, self.k, constraint=con, mask_rows=mid,
                                                                    temperature=self.temperature)
        parent, token, score = eng.beam_select(self.scores, live.to(torch.int32), cand_tok.contiguous(), cand_logp.contiguous(), B)
        empty = parent < 0
        src = self._base + parent.clamp(min=0)  # (an empty slot reads its group's first row: it is dead)
        srcl = src.long()
        self.contexts = eng.gather_rows_i32(self.contexts, src)
        self.lengths = self.lengths[srcl].contiguous()
        self.active = (live[srcl] & ~empty).to(torch.int32)
        self.scores = score  # as computed by the selection: nothing is added again
        if con is not None:
            self.states = self.states[srcl].contiguous()
            if con.weighted:  # a hypothesis made to end was served the EOS-only row (weight 0): its state's final weight
                forced = (done[srcl] > 0) & (self.active > 0) & (token == self.eos_id)
                self.scores = self.scores + con.forced_final_logw(self.states, forced)
        len_was = self.lengths.clone() if con is not None else None
        # appends the token; EOS or a token < 0 (a finished hypothesis carried over, an empty slot) deactivates
        eng.particles_advance(self.contexts, self.lengths, self.active, self.scores, self._zeros, token, self.eos_id, self.cap)
        if con is not None:
            con.advance(self.states, self.contexts, len_was, self.lengths, out=self.states)
        self.t += 1
        return n_live

    def run(self, max_steps=None):
        """Steps until no beam is alive or `max_tokens` tokens are out (one more step under a constraint: the one in which
        hypotheses of `max_tokens` tokens may only end).  Returns the number of steps taken."""
        limit = self.max_tokens + (1 if self.constraint is not None else 0) - self.t
        if max_steps is not None:
            limit = min(limit, max_steps)
        steps = 0
        while steps < limit and self.step():
            steps += 1
        return steps

    def results(self):
        """Per group (contexts, scores): the generated tokens of its `width` slots as lists, best first, and their scores as
        a float32 device tensor [width] (-inf: an empty slot, its token list is meaningless).  A hypothesis has ended when its
        `active` entry is 0; its EOS is not stored."""
        if self.constraint is not None and not self._checked:
            self.constraint.check()
            self._checked = True
        # (a weighted constraint's final weights are added after the selection: order the slots by what they score now)
        order = torch.argsort(self.scores.view(self.G, self.width), dim=1, descending=True, stable=True)
        idx = (order + self._base.view(self.G, self.width)[:, :1].long()).view(-1)
        ctx, ln, pl = self.contexts[idx].cpu().numpy(), self.lengths[idx].cpu().numpy(), self.prompt_len[idx].cpu().numpy()
        scores = self.scores[idx]
        self.result_slots = idx  # slot of every returned hypothesis (for `active`, `states`, ...)
        B = self.width
        return [([[int(t) for t in ctx[i, pl[i]:ln[i]]] for i in range(g * B, (g + 1) * B)], scores[g * B:(g + 1) * B]) for g in range(self.G)]
