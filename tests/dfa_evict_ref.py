"""The contract of an evicting mask bank (include/glb.h glb_dfa_evict_serve), restated in NumPy: the bookkeeping only -
row_of_state, row_state, row_stamp and the epoch; a row's contents are tests/dfa_ref.py's and tests/wfsa_ref.py's business.
Which row a state gets depends on the order of the device's atomics, so `serve` does not predict row numbers: it says which
rows a call was ALLOWED to take and how many it HAD to, and the tests compare sets and contents.  Test infrastructure: the
product never imports it."""
import numpy as np


class EvictRef:
    def __init__(self, n_states, capacity):
        assert capacity >= 3
        self.S, self.capacity = int(n_states), int(capacity)
        self.row_of_state = np.full(self.S, -1, np.int64)
        self.row_state = np.full(self.capacity, -1, np.int64)
        self.row_stamp = np.zeros(self.capacity, np.int64)
        self.epoch = 1
        self.fills = self.evictions = 0
        self.overflow = False

    rows_in_use = property(lambda self: 2 + int((self.row_state >= 0).sum()))

    def serve(self, states):
        """One call.  Returns a dict:
        claimants  the distinct valid states without a row, ascending
        need       how many rows the call takes: min(claimants, rows not requested in this call)
        must       the rows every correct selection takes (stamp strictly below the need-th smallest)
        may        must plus the rows that tie at the need-th smallest stamp; need - len(must) of the ties are taken
        excess     how many claimants stay without a row (their ids are 0, the overflow word is raised)
        Its own state moves on by ONE correct selection (ties: lowest row first; claimants in ascending order)."""
        states = np.asarray(states, np.int64)
        valid = np.unique(states[(states >= 0) & (states < self.S)])
        have = valid[self.row_of_state[valid] >= 2]
        self.row_stamp[self.row_of_state[have]] = self.epoch  # touch
        claimants = valid[self.row_of_state[valid] < 0]
        cand = np.array([r for r in range(2, self.capacity) if self.row_stamp[r] != self.epoch], np.int64)
        need = min(len(claimants), len(cand))
        order = cand[np.argsort(self.row_stamp[cand], kind="stable")]  # ascending stamp; never-used rows (0) first
        must, may = set(), set()
        if need:
            kth = self.row_stamp[order[need - 1]]
            must = {int(r) for r in cand if self.row_stamp[r] < kth}
            may = must | {int(r) for r in cand if self.row_stamp[r] == kth}
        for s, r in zip(claimants[:need], order[:need]):  # reassign
            old = self.row_state[r]
            if old >= 0:
                self.row_of_state[old] = -1
                self.evictions += 1
            self.row_state[r], self.row_of_state[s], self.row_stamp[r] = s, r, self.epoch
            self.fills += 1
        excess = len(claimants) - need
        self.overflow |= excess > 0
        self.epoch += 1
        return dict(claimants=[int(s) for s in claimants], need=need, must=must, may=may, excess=excess)

    def ids(self, states, done=None, accepting=None):
        """The ids of glb_dfa_mask_ids for this restatement's own assignment."""
        out = []
        for i, s in enumerate(np.asarray(states, np.int64)):
            ok = 0 <= s < self.S
            if done is not None and done[i]:
                out.append(1 if ok and accepting[s] else 0)
            else:
                out.append(int(self.row_of_state[s]) if ok and self.row_of_state[s] >= 2 else 0)
        return out
