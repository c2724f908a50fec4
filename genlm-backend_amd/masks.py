"""Where the fused step's masks come from.  `RegisteredMasks` (the backend's shared log-masks), `ParticleMasks` (a caller's
bit row per particle) and `constraints.DeviceConstraint` (rows made on the device from an automaton) answer one question
through one method,

    step_masks(logits, ids, by_row, n_particles, parity) -> (mask keyword arguments of `HipEngine.step`, handed over raw?)

logits: the step's [rows, V] (a source reads their element type, `ParticleMasks` also V; a constraint neither); ids: int32 per
unit - per logits row when `by_row`, else per particle; parity: the draw is the two-launch parity race.  A caller picks its
source once and never asks which kind it holds.
"""
import torch

from ._lib import MASK_BITS, MASK_F32, MASK_NONE


class RegisteredMasks:
    """The log-masks given to `AsyncAmdLM.register_masks`: {0, -inf} tables packed to bit rows on the device and brought into
    the kernels' layout once per element width (glb_mask_prepare), anything else kept as float."""

    def __init__(self, engine):
        self.engine, self.kind, self.table, self.vocab, self._prepared = engine, MASK_NONE, None, None, {}

    def register(self, masks):
        bits, flag = self.engine.mask_to_bits(masks)
        self._prepared = {}
        if int(flag.item()) == 0:
            self.kind, self.table, self.vocab = MASK_BITS, bits, masks.shape[1]
        else:
            self.kind, self.table = MASK_F32, masks

    def tables(self, dtype):
        """The table arguments alone (no ids): {} with nothing registered."""
        if self.kind == MASK_NONE:
            return {}
        if self.kind == MASK_F32:
            return dict(mask_kind=MASK_F32, mask=self.table)
        wide = dtype == torch.float32
        if wide not in self._prepared:
            self._prepared[wide] = self.engine.prepare_masks(self.table, self.vocab, dtype)
        return dict(mask=self._prepared[wide])

    def step_masks(self, logits, ids, by_row, n_particles=None, parity=False):
        kw = self.tables(logits.dtype)
        if kw:
            kw["row_mask_id" if by_row else "mask_id"] = ids
        return kw, self.kind == MASK_F32


class ParticleMasks:
    """int32 bit rows [n + 1, ceil(V / 32)] on the device, `masks`: particle i's own mask, row n for one that may only end.
    Two ways to hand the bit rows over.  RAW: the fused launch's stats waves read the caller's rows themselves
    (kMaskRaw: + 2 us a step on float32 rows, + 5 us on 16-bit ones, nothing to prepare).  PREPARED: the rows
    transposed into the kernels' layout (glb_mask_prepare: 11 us for 1025 rows of 50257), afterwards only the rows
    `update` named again (glb_mask_prepare_rows).  A grammar that moves every particle's mask every
    token is served raw; masks that stand still, or of which a few move a step, prepared.  A step goes raw
     * when more than `raw_above` of the rows changed since the prepared form was last brought up to date and
       some did since the last step (their names are kept: a step before which nothing moved brings it up to date);
     * when the tensor is in a state this object has not seen - rebound, or written in place by anyone but
       `update` (its version counter moves); seen twice in a row, that state is prepared.
    The parity draw is two launches (no raw form): always prepared."""

    def __init__(self, engine, n, masks):
        self.engine, self.n, self.masks = engine, n, masks
        self.raw_above = None  # fraction of changed rows above which a step hands the bit rows over raw (None: by dtype)
        self.raw_steps = 0
        self.reset()

    def reset(self):
        self._prepared, self._dirty, self._seen, self._moved = None, None, None, False

    def update(self, rows, bit_rows):
        """Particles `rows` (int32 device tensor) get new masks `bit_rows` (int32 [len(rows), ceil(V / 32)]): only these are
        brought into the kernels' layout again before the next step."""
        pm = self.masks
        known = self._prepared is not None and self._prepared[1][:2] == (pm.data_ptr(), pm._version)
        pm[rows.long()] = bit_rows
        if known:  # the prepared form follows this write row by row; any other write makes the next step prepare everything
            self._prepared = (self._prepared[0], (pm.data_ptr(), pm._version, self._prepared[1][2]))
            self._dirty = rows if self._dirty is None else torch.unique(torch.cat([self._dirty, rows]))
            self._moved = True

    def step_masks(self, logits, ids, by_row=False, n_particles=None, parity=False):
        eng, pm, dtype, key = self.engine, self.masks, logits.dtype, "row_mask_id" if by_row else "mask_id"
        state = (pm.data_ptr(), pm._version, dtype)
        frac = self.raw_above if self.raw_above is not None else (0.25 if dtype == torch.float32 else 0.5)
        raw = False
        if self._prepared is None or self._prepared[1] != state:
            if not parity and frac < 1.0 and self._seen != state:
                raw, self._prepared, self._dirty = True, None, None
            else:
                self._prepared, self._dirty = (eng.prepare_masks(pm, logits.shape[-1], dtype), state), None
        elif self._dirty is not None:
            if not parity and self._moved and self._dirty.numel() > frac * self.n:
                raw = True  # (the prepared form stays behind by the rows named in _dirty, until the masks stand still)
            else:
                eng.update_prepared_masks(self._prepared[0], pm, self._dirty)
                self._dirty = None
        self._seen, self._moved = state, False
        self.raw_steps += int(raw)
        return ({"mask_kind": MASK_BITS, "mask": pm, key: ids} if raw else {"mask": self._prepared[0], key: ids}), raw
