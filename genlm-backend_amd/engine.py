"""Tensor-level front-end of the HIP library: torch tensors in, torch tensors out, raw pointers and
the current HIP stream across the C ABI (include/glb.h).  PyTorch only provides device memory and
streams here.  Nothing in this module computes on the CPU; constructing `HipEngine` without a GPU
raises.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import GLB_EHIP, GlbError
from ._lib import (F32, BF16, F16, MASK_NONE, MASK_BITS, MASK_F32, MASK_PREPARED, RNG_NONE, RNG_PHILOX, RNG_NOISE,
                   STEP_HW_EXP, KvPlanArgs, KvPlanChunkArgs, MtRowsArgs, StepArgs, TrieArgs, TriePlan, TrieRowsArgs, MT19937, MT_POLY_WORDS, check)

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class LoraRowsTable:
    """The uploaded adapter table of glb_lora_rows (HipEngine.lora_rows_table): device bytes, its shape, the largest rank,
    and the adapter tensors it points into."""

    def __init__(self, dev, n_slots, n_modules, r_max, keep):
        self.dev, self.n_slots, self.n_modules, self.r_max, self.keep = dev, n_slots, n_modules, r_max, keep


class HostRng:
    """torch-CPU-compatible MT19937 stream for GLB_RNG_NOISE (parity mode).

    `exponential(n)` returns the float32 values `torch.empty(n).exponential_(1, generator=g)` yields
    for a generator seeded with `seed` (README.md:87 / base.py:125-141 draw through it)."""

    def __init__(self, seed):
        self._lib = _lib.load()
        self.state = MT19937()
        self._lib.glb_mt19937_seed(C.byref(self.state), C.c_uint64(seed))

    def exponential(self, n, out=None):
        if out is None:
            out = torch.empty(n, dtype=torch.float32, pin_memory=torch.cuda.is_available())
        assert out.dtype == torch.float32 and out.is_contiguous() and out.device.type == "cpu"
        check(self._lib.glb_mt19937_exponential_f32(C.byref(self.state), _ptr(out), n))
        return out


def _low_priority_stream(device):
    """A stream of the LOWEST priority HIP has (torch offers normal and high only): work queued on it fills what the
    caller's stream leaves idle instead of competing with it.  Falls back to an ordinary torch stream."""
    try:
        hip = C.CDLL("libamdhip64.so")
        least, greatest = C.c_int(0), C.c_int(0)
        if hip.hipDeviceGetStreamPriorityRange(C.byref(least), C.byref(greatest)) == 0 and least.value > 0:
            h = C.c_void_p()
            with torch.cuda.device(device):
                if hip.hipStreamCreateWithPriority(C.byref(h), C.c_uint(1), C.c_int(least.value)) == 0 and h.value:  # (1: hipStreamNonBlocking)
                    return torch.cuda.ExternalStream(h.value, device=device)
    except OSError:
        pass
    return torch.cuda.Stream(device=device)


class DeviceRng:
    """torch's CPU generator for the parity draw, ON THE DEVICE (glb_mt19937_exponential_rows): the MT19937 stream of
    `torch.Generator().manual_seed(seed)` entered at every particle's row at once - no serial host loop, no noise tensor
    over PCIe.  `rows(...)` returns float32 [n_out, V] Exp(1) rows exactly as `torch.empty(V).exponential_(1, generator)`
    would yield them one after the other, and moves the stream on by the rows consumed.

    The stream's position is a 624-word window on the device; the jump polynomials for stride 2 V are computed on the host
    once per vocabulary (about 0.1 s) and cached on the engine.

    `ahead=True` (what `DeviceSIS` uses): the rows of the NEXT call depend on nothing but where the stream stands after this
    one, so `prefetch()` - called once the step that consumed the rows has been queued - generates them in stream order on a
    side stream while the caller's stream runs the next forward; the next `rows(...)` then only copies the rows its
    `row_slot` names into place and moves the position (the same rows, bit for bit: the same kernels made them)."""

    SMALL = 32

    def __init__(self, engine, seed, vocab, ahead=False):
        self.eng, self.seed, self.vocab, self.ahead = engine, int(seed), int(vocab), bool(ahead)
        self._side = None   # the side stream
        self._pre = None    # (max_draw, rows buffer, done event): what prefetch() has queued
        self._ws = None     # this stream's own windows (the engine's scratch is shared by every caller)
        self._last = None   # max_draw of the last rows() call
        self.reset()

    def reset(self):
        if self._pre is not None:  # (let the side stream finish with the window before it is replaced)
            self._pre[2].synchronize()
            self._pre = None
        w = np.zeros(624, np.uint32)
        check(self.eng.lib.glb_mt19937_window(C.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF), C.c_void_p(w.ctypes.data)))
        self.window = torch.from_numpy(w.view(np.int32)).to(self.eng.device)
        self.rows_drawn = 0  # host-side tally when the counts are known here (diagnostic)

    def _args(self, max_draw, n_big, polys):
        eng = self.eng
        need = eng.lib.glb_mt19937_rows_workspace(max_draw, self.SMALL)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=eng.device)
        a = MtRowsArgs()
        a.struct_size = C.sizeof(MtRowsArgs)
        a.window = self.window.data_ptr()
        a.polys = polys.data_ptr()
        a.n_small, a.n_big = self.SMALL, n_big
        a.vocab, a.max_draw_rows = self.vocab, max_draw
        a.workspace, a.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        return a

    def rows(self, n_out, row_slot=None, n_draw=None, max_draw=None, out=None):
        """n_out rows; row_slot: int32 [n_out] device - the stream row every output row takes (negative: a row of ones),
        None: identity; n_draw: int32 device scalar tensor - rows the stream moves on by (None: max_draw); max_draw: host
        upper bound of it (default n_out)."""
        eng, V = self.eng, self.vocab
        max_draw = int(n_out if max_draw is None else max_draw)
        polys, n_big = eng.mt_polys(V, max_draw + 1)
        if out is None:
            out = torch.empty((n_out, V), dtype=torch.float32, device=eng.device)
        eng._check_dev(row_slot, n_draw, out)
        if row_slot is not None and (row_slot.dtype != torch.int32 or row_slot.numel() != n_out):
            raise ValueError("row_slot must be int32 [n_out]")
        if n_draw is not None and n_draw.dtype != torch.int32:
            raise TypeError("n_draw must be an int32 device scalar")
        pre, self._pre = self._pre, None
        if pre is not None and pre[0] != max_draw:  # (made for another shape: wait it out - it reads the window - and drop it)
            pre[2].synchronize()
            pre = None
        a = self._args(max_draw, n_big, polys)
        a.window_out = self.window.data_ptr()
        a.n_draw = None if n_draw is None else n_draw.data_ptr()
        a.n_out_rows = n_out
        a.row_slot = None if row_slot is None else row_slot.data_ptr()
        a.out, a.out_ld = out.data_ptr(), out.stride(0) if n_out > 1 else max(V, out.stride(0))
        if pre is not None:  # the rows stand in pre[1], the windows in the workspace: copy and move on
            torch.cuda.current_stream(eng.device).wait_event(pre[2])
            a.reuse_windows = 1
            a.rows_from, a.rows_from_ld = pre[1].data_ptr(), pre[1].stride(0)
        check(eng.lib.glb_mt19937_exponential_rows(C.byref(a), eng._stream()))
        if n_draw is None:
            self.rows_drawn += max_draw
        self._last = max_draw
        return out

    def prefetch(self):
        """Queue the generation of the next call's rows (as many as the last call could draw, in stream order) on the side
        stream; it starts when everything queued on the current stream so far is done - call it after the step that reads
        the last rows() has been queued.  No-op unless `ahead`."""
        if not self.ahead or self._last is None or self._pre is not None:
            return
        eng, V, max_draw = self.eng, self.vocab, self._last
        if self._side is None:
            self._side = _low_priority_stream(eng.device)
            self._rows_buf = None
        if self._rows_buf is None or self._rows_buf.shape[0] < max_draw:
            self._rows_buf = torch.empty((max_draw, V), dtype=torch.float32, device=eng.device)
        polys, n_big = eng.mt_polys(V, max_draw + 1)
        a = self._args(max_draw, n_big, polys)
        a.n_out_rows = max_draw
        a.out, a.out_ld = self._rows_buf.data_ptr(), self._rows_buf.stride(0)
        self._side.wait_stream(torch.cuda.current_stream(eng.device))
        with torch.cuda.stream(self._side):
            check(eng.lib.glb_mt19937_exponential_rows(C.byref(a), eng._stream()))
            done = torch.cuda.Event()
            done.record(self._side)
        self._pre = (max_draw, self._rows_buf, done)


class PreparedMasks:
    """Bit masks in the kernels' own layout (glb_mask_prepare): built once for masks that do not change."""

    def __init__(self, blob, n_masks, vocab, dtype):
        self.blob, self.n_masks, self.vocab, self.dtype = blob, n_masks, vocab, dtype


class StepPlan:
    """A fused step whose argument block is already filled (HipEngine.step_plan)."""

    __slots__ = ("eng", "args", "keep", "out", "_ref")

    def __init__(self, eng, args, keep, out):
        self.eng, self.args, self.keep, self.out = eng, args, keep, out
        self._ref = C.byref(args)

    def run(self, offset=None, seed=None):
        a = self.args
        if offset is not None:
            a.offset = offset
        if seed is not None:
            a.seed = seed
        if self.eng._step_ws is not self.keep[-1]:
            raise RuntimeError("the engine's scratch buffer was reallocated since this plan was made: make a new plan")
        check(self.eng.lib.glb_logprob_mask_sample(self._ref, self.eng._stream()))
        return self.out

    def run_timed(self, events, offset=None, seed=None):
        """run() whose launch(es) carry `events` = (start, stop) - two recorded-once torch.cuda.Event(enable_timing=True)
        - as their own start / stop stamps (glb_logprob_mask_sample_timed): start.elapsed_time(stop) is the duration of
        the step's launches on the device."""
        a = self.args
        if offset is not None:
            a.offset = offset
        if seed is not None:
            a.seed = seed
        if self.eng._step_ws is not self.keep[-1]:
            raise RuntimeError("the engine's scratch buffer was reallocated since this plan was made: make a new plan")
        check(self.eng.lib.glb_logprob_mask_sample_timed(self._ref, self.eng._stream(), C.c_void_p(events[0].cuda_event),
                                                         C.c_void_p(events[1].cuda_event)))
        return self.out


class _OnDevice:
    """The library's entry points, each run with the engine's device current.  HIP launches go to the calling thread's
    current device; the engine's tensors and stream belong to `self.device`, so a caller that has another device
    current (one process driving several GPUs) must not be able to send a launch to the wrong one."""

    def __init__(self, lib, index):
        self._lib, self._index = lib, index

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        index = self._index

        def call(*args):
            if torch.cuda.current_device() == index:
                return fn(*args)
            with torch.cuda.device(index):
                return fn(*args)

        setattr(self, name, call)  # resolved once per entry point
        return call


def check_truncation(top_k, top_p, min_p):
    """(top_k, top_p, log_min_p) as glb_truncate_rows takes them, from the sampling options top_k (0: off), top_p (1: off) and
    min_p (0: off); a ValueError names the offending value.  log_min_p is the float32 log(min_p), so key_max + log_min_p is one
    rounded add on the host and on the device."""
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
        raise ValueError(f"top_k must be a non-negative integer (0: off), got {top_k!r}")
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0.0 < top_p <= 1.0:  # (NaN fails both)
        raise ValueError(f"top_p must lie in (0, 1] (1: off), got {top_p!r}")
    if isinstance(min_p, bool) or not isinstance(min_p, (int, float)) or not 0.0 <= min_p <= 1.0:
        raise ValueError(f"min_p must lie in [0, 1] (0: off), got {min_p!r}")
    with np.errstate(divide="ignore"):
        log_min_p = float(np.log(np.float32(min_p)))
    return top_k, float(top_p), log_min_p


class HipEngine:
    """All device work of the hot path for one GPU."""

    CONTRACTS = ("poly", "hw", "auto")

    def __init__(self, device=None, contract="auto"):
        """contract: the arithmetic of the fused step's terms (include/glb.h, GLB_STEP_HW_EXP) - "poly":
        the polynomial exponential, restated bit for bit by the oracle; "hw": the hardware's v_exp_f32 - within one ulp of
        2^y, deterministic and independent of launch geometry on gfx950, checked against the oracle by tolerance and
        against torch's ids in parity mode (tests/test_step_hw_gpu.py); "auto" (the default): "hw" for 16-bit logits (a
        sixth less time on rows bound by instruction issue), "poly" for float32 rows (bound by memory: 4 % to gain, and
        their results stay the oracle's bit for bit).  `step(contract=...)` overrides it per call."""
        if contract not in self.CONTRACTS:
            raise ValueError(f"contract must be one of {self.CONTRACTS}, got {contract!r}")
        self.contract = contract
        lib = _lib.load()
        if not torch.cuda.is_available() or lib.glb_device_count() <= 0:
            raise RuntimeError(
                "HipEngine needs a HIP device (MI355X / gfx950); none is visible and there is no CPU fallback"
            )
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.type != "cuda":
            raise RuntimeError(f"HipEngine device must be a HIP device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _OnDevice(lib, self.device.index)
        self._ws = None
        self._step_ws = None
        self._imp_ws = None
        self._trie_ws = None
        self._lora_rows_ws = None
        self._mt_polys = {}
        self._ptr_tables = {}

    def __del__(self):
        try:
            if self._step_ws is not None:
                self.lib.glb_workspace_release(_ptr(self._step_ws))
        except Exception:  # interpreter shutdown
            pass

    # ------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _i32(self, n):
        return torch.empty(n, dtype=torch.int32, device=self.device)

    def _f32(self, n):
        return torch.empty(n, dtype=torch.float32, device=self.device)

    def _check_dev(self, *ts):
        for t in ts:
            if t is not None and (t.device != self.device or not t.is_contiguous()):
                if t.device != self.device:
                    raise ValueError(f"tensor on {t.device}, engine on {self.device}")
                raise ValueError("tensor must be contiguous")

    # ------------------------------------------------------------------------------------------
    def _scratch(self, need):
        """The step's scratch buffer, zeroed and registered with the library (glb_workspace_init): calls that find their
        workspace registered run as ONE launch."""
        if self._step_ws is None or self._step_ws.numel() < need:
            if self._step_ws is not None:
                self.lib.glb_workspace_release(_ptr(self._step_ws))
            self._step_ws = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=self.device)
            check(self.lib.glb_workspace_init(_ptr(self._step_ws), self._step_ws.numel(), self._stream()))
        return self._step_ws

    def step(self, logits, vocab=None, row_of=None, mask_kind=MASK_NONE, mask=None, mask_id=None,
             rng_mode=RNG_NONE, noise=None, seed=0, offset=0, particle_base=0, logit_scale=1.0,
             want_lse=True, out=None, row_mask_id=None, out_margin=None, _plan=False, timing_events=None,
             contract=None):
        """Fused particle step (glb_logprob_mask_sample).  Returns (logZ, lse, token) device tensors.

        logits: [n_rows, ld] (last dim contiguous; rows may be strided), vocab <= ld.
        mask: int32 bit rows / float rows, or a `PreparedMasks` (prepare_masks).  `row_mask_id` gives the mask per
        logits row (the mask is a function of the context): shared rows are then reduced once.
        A launch whose waves gave up waiting shows as token -2 / NaN and in `error_word()`: `raise_if_failed`.
        contract: "poly" / "hw" / "auto" (None: the engine's) - see __init__.
        """
        if logits.dim() != 2 or logits.stride(1) != 1:
            raise ValueError("logits must be 2-D with unit inner stride")
        if logits.dtype not in _DT:
            raise TypeError(f"unsupported logits dtype {logits.dtype}")
        n_rows, width = logits.shape
        ld = logits.stride(0) if n_rows > 1 else max(width, logits.stride(0))
        V = width if vocab is None else vocab
        n = n_rows if row_of is None else row_of.numel()
        self._check_dev(row_of, mask_id, row_mask_id, noise)
        if out is None:
            logZ, lse, tok = self._f32(n), (self._f32(n) if want_lse else None), None
            if rng_mode != RNG_NONE:
                tok = self._i32(n)
        else:
            logZ, lse, tok = out
        a = StepArgs()
        a.struct_size = C.sizeof(StepArgs)
        a.logits = logits.data_ptr()
        a.dtype = _DT[logits.dtype]
        a.n_rows, a.vocab, a.ld = n_rows, V, ld
        a.logit_scale = logit_scale
        a.n_particles = n
        a.row_of = None if row_of is None else row_of.data_ptr()
        n_masks = 0
        if isinstance(mask, PreparedMasks):
            if mask.vocab != V or (mask.dtype == F32) != (_DT[logits.dtype] == F32):
                raise ValueError("prepared masks were built for another vocabulary / element width")
            a.mask_kind = MASK_PREPARED
            a.mask = mask.blob.data_ptr()
            a.mask_ld = 0
            a.n_masks = mask.n_masks
        else:
            a.mask_kind = mask_kind
            if mask_kind != MASK_NONE:
                self._check_dev(mask)
                if mask.dim() != 2 or mask.stride(1) != 1:
                    raise ValueError("mask must be 2-D")
                want = torch.float32 if mask_kind == MASK_F32 else torch.int32
                if mask.dtype != want:
                    raise TypeError(f"mask dtype {mask.dtype}, expected {want}")
                a.mask = mask.data_ptr()
                a.mask_ld = mask.stride(0) if mask.shape[0] > 1 else mask.shape[1]
                a.n_masks = mask.shape[0]
                n_masks = mask.shape[0] if mask_kind == MASK_BITS else 0
        if a.mask_kind != MASK_NONE:
            a.mask_id = None if mask_id is None else mask_id.data_ptr()
            a.row_mask_id = None if row_mask_id is None else row_mask_id.data_ptr()
        a.rng_mode = rng_mode
        if rng_mode == RNG_NOISE:
            if noise.dim() != 2 or noise.dtype != torch.float32:
                raise ValueError("noise must be float32 [n_particles, >=vocab]")
            a.noise = noise.data_ptr()
            # one row for everybody (batch_sample seeds every sequence alike): pitch 0
            a.noise_ld = noise.stride(0) if noise.shape[0] > 1 else (0 if n > 1 else noise.shape[1])
        a.seed, a.offset, a.particle_base = seed, offset, particle_base
        a.out_logZ = None if logZ is None else logZ.data_ptr()
        a.out_lse = None if lse is None else lse.data_ptr()
        a.out_token = None if tok is None else tok.data_ptr()
        a.out_margin = None if out_margin is None else out_margin.data_ptr()  # parity mode: tie margin of every draw
        contract = self.contract if contract is None else contract
        if contract not in self.CONTRACTS:
            raise ValueError(f"contract must be one of {self.CONTRACTS}, got {contract!r}")
        a.flags = STEP_HW_EXP if contract == "hw" or (contract == "auto" and a.dtype != F32) else 0
        ws = self._scratch(self.lib.glb_step_workspace_bytes(n, n_rows, V, n_masks))
        a.workspace = ws.data_ptr()
        a.workspace_bytes = ws.numel()
        if _plan:  # step_plan(): the filled argument block, the tensors it points into, the outputs
            return StepPlan(self, a, (logits, row_of, mask, mask_id, row_mask_id, noise, out_margin, ws),
                            (logZ, lse, tok))
        if timing_events is not None:  # (start, stop) from timing_events(): the launches' own start / stop stamps
            check(self.lib.glb_logprob_mask_sample_timed(C.byref(a), self._stream(), C.c_void_p(timing_events[0].cuda_event),
                                                         C.c_void_p(timing_events[1].cuda_event)))
        else:
            check(self.lib.glb_logprob_mask_sample(C.byref(a), self._stream()))
        return logZ, lse, tok

    def importance_step(self, target, proposal=None, *, proposal_scale=1.0, vocab=None, row_of=None, mask_kind=MASK_NONE,
                        mask=None, mask_id=None, row_mask_id=None, seed=0, offset=0, particle_base=0, want_lse=False,
                        want_logZ_proposal=False, out=None):
        """Importance-weighted particle step (glb_importance_step): the token drawn from
        softmax(proposal * proposal_scale + mask), dlogw = log[softmax(target)_tok e^{mask_tok}] - log of the probability
        it was drawn with.  Returns (dlogw, token, lse_target or None) - with `want_logZ_proposal` a fourth tensor,
        lse(y + m) - lse(y).

        target, proposal: [n_rows, ld] logits of the same contexts under two models (last dim contiguous, any of float32 /
        bfloat16 / float16 each); proposal None: the target's own rows.  mask: int32 bit rows (MASK_BITS) or float rows
        (MASK_F32) as they lie - not a `PreparedMasks`; `mask_id` per particle or `row_mask_id` per logits row.
        out: (dlogw, token, lse or None) to write into.  The records live in a scratch buffer of their own: the fused
        step's is registered with the library and carries its tags."""
        if isinstance(mask, PreparedMasks):
            raise TypeError("importance_step reads bit rows or float rows as they lie, not prepared masks")
        mats = [("target", target)] + ([("proposal", proposal)] if proposal is not None else [])
        for name, t in mats:
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{name} must be 2-D with unit inner stride")
            if t.dtype not in _DT:
                raise TypeError(f"unsupported {name} dtype {t.dtype}")
            if t.device != self.device:
                raise ValueError(f"{name} on {t.device}, engine on {self.device}")
        n_rows, width = target.shape
        if proposal is not None and tuple(proposal.shape) != (n_rows, width):
            raise ValueError(f"proposal is {tuple(proposal.shape)}, target {tuple(target.shape)}: row r of one pairs with row r "
                             "of the other")
        V = width if vocab is None else vocab
        n = n_rows if row_of is None else row_of.numel()
        self._check_dev(row_of, mask_id, row_mask_id)
        if out is None:
            dlogw, tok, lse = self._f32(n), self._i32(n), (self._f32(n) if want_lse else None)
        else:
            dlogw, tok, lse = out
        logZq = self._f32(n) if want_logZ_proposal else None
        a = _lib.ImportanceArgs()
        a.struct_size = C.sizeof(_lib.ImportanceArgs)
        a.target, a.target_dtype = target.data_ptr(), _DT[target.dtype]
        a.ld_p = target.stride(0) if n_rows > 1 else max(width, target.stride(0))
        if proposal is not None:
            a.proposal, a.proposal_dtype = proposal.data_ptr(), _DT[proposal.dtype]
            a.ld_q = proposal.stride(0) if n_rows > 1 else max(width, proposal.stride(0))
        a.n_rows, a.vocab, a.proposal_scale, a.n_particles = n_rows, V, proposal_scale, n
        a.row_of = None if row_of is None else row_of.data_ptr()
        a.mask_kind = mask_kind
        if mask_kind != MASK_NONE:
            self._mask_block(a, mask_kind, mask, V)
            a.mask_id = None if mask_id is None else mask_id.data_ptr()
            a.row_mask_id = None if row_mask_id is None else row_mask_id.data_ptr()
        a.seed, a.offset, a.particle_base = seed, offset, particle_base
        a.out_token = None if tok is None else tok.data_ptr()
        a.out_dlogw = None if dlogw is None else dlogw.data_ptr()
        a.out_lse_target = None if lse is None else lse.data_ptr()
        a.out_logZ_proposal = None if logZq is None else logZq.data_ptr()
        need = self.lib.glb_importance_workspace_bytes(n, n_rows, V)
        if self._imp_ws is None or self._imp_ws.numel() < need:
            self._imp_ws = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=self.device)
        a.workspace, a.workspace_bytes = self._imp_ws.data_ptr(), self._imp_ws.numel()
        check(self.lib.glb_importance_step(C.byref(a), self._stream()))
        return (dlogw, tok, lse, logZq) if want_logZ_proposal else (dlogw, tok, lse)

    SCORE_OUTPUTS = ("logp", "lse", "logZ", "logp_masked")

    def score_rows(self, logits, tokens, *, vocab=None, logit_scale=1.0, mask_kind=MASK_NONE, mask=None, row_mask_id=None,
                   seq_start=None, want=("logp",)):
        """Scores of given tokens (glb_score_rows): per logits row r, with y = logits[r] * logit_scale and
        t = tokens[r], any of "logp" = y_t - lse(y), "lse" = lse(y), "logZ" = lse(y + m) - lse(y), "logp_masked" =
        y_t + m_t - lse(y + m) - the names in `want` -, as a dict of float32 [n_rows] device tensors.  No log-softmax is
        written.  logits: [n_rows, ld] (last dim contiguous; float32 / bfloat16 / float16); tokens int32 [n_rows]; mask:
        int32 bit rows (MASK_BITS) or float rows (MASK_F32) as they lie with `row_mask_id` int32 [n_rows] (None: one mask
        for all, or one per row) - the keywords a constraint's `step_masks(..., by_row=True, ...)` returns.  seq_start:
        int64 [n_seq + 1] ascending row offsets; the dict then also holds "seq_" + name, float32 [n_seq], for "logp",
        "logZ" and "logp_masked" where wanted: the sums over each sequence's rows."""
        if isinstance(mask, PreparedMasks) or mask_kind == MASK_PREPARED:
            raise TypeError("score_rows reads bit rows or float rows as they lie, not prepared masks")
        want = tuple(want)
        for w in want:
            if w not in self.SCORE_OUTPUTS:
                raise ValueError(f"want names {w!r}; the outputs are {self.SCORE_OUTPUTS}")
        a = _lib.ScoreArgs()
        a.struct_size = C.sizeof(_lib.ScoreArgs)
        n_rows, _ = self._row_block(a, logits, vocab, logit_scale, mask_kind, mask, row_mask_id, empty="no rows to score")
        self._check_dev(tokens, seq_start)
        if tokens.dtype != torch.int32 or tokens.shape != (n_rows,) or not tokens.is_contiguous():
            raise ValueError("tokens must be a contiguous int32 [n_rows] tensor")
        a.token = tokens.data_ptr()
        out = {w: self._f32(n_rows) for w in want}
        for w in want:
            setattr(a, "out_" + w, out[w].data_ptr())
        if seq_start is not None:
            if seq_start.dtype != torch.int64 or seq_start.dim() != 1 or seq_start.numel() < 1 or not seq_start.is_contiguous():
                raise ValueError("seq_start must be a contiguous int64 [n_seq + 1] tensor")
            a.seq_start, a.n_seq = seq_start.data_ptr(), seq_start.numel() - 1
            for w in want:
                if w != "lse":
                    out["seq_" + w] = self._f32(a.n_seq)
                    setattr(a, "out_seq_" + w, out["seq_" + w].data_ptr())
        check(self.lib.glb_score_rows(C.byref(a), self._stream()))
        return out

    def score_seq_sums(self, values, seq_start):
        """float32 [n_seq]: the sums of `values` (float32 [n_rows]) over rows seq_start[s] .. seq_start[s + 1] - 1, in row
        order, in double, rounded once (glb_score_seq_sums: the sums of `score_rows` for rows that were scored in chunks)."""
        self._check_dev(values, seq_start)
        if values.dtype != torch.float32 or values.dim() != 1:
            raise ValueError("values must be a float32 [n_rows] tensor")
        if seq_start.dtype != torch.int64 or seq_start.dim() != 1 or seq_start.numel() < 1:
            raise ValueError("seq_start must be an int64 [n_seq + 1] tensor")
        out = self._f32(seq_start.numel() - 1)
        if out.numel():
            # (an empty `values` has no storage to point at: any valid pointer serves, no row is read)
            src = values if values.numel() else out
            check(self.lib.glb_score_seq_sums(_ptr(src), values.numel(), _ptr(seq_start), out.numel(), _ptr(out), self._stream()))
        return out

    def _mask_block(self, a, mask_kind, mask, V):
        """The mask table's fields (mask, n_masks, mask_ld) of an argument block that reads bit rows or float rows as they
        lie, checked against `V` tokens and written into `a`; which row reads which mask is the caller's."""
        if mask is None:
            raise ValueError("mask_kind given without a mask table")
        if mask.device != self.device:
            raise ValueError(f"mask on {mask.device}, engine on {self.device}")
        if mask.dim() != 2 or mask.stride(1) != 1:
            raise ValueError("mask must be 2-D with unit inner stride (rows may be strided)")
        want_dt = torch.float32 if mask_kind == MASK_F32 else torch.int32
        if mask.dtype != want_dt:
            raise TypeError(f"mask dtype {mask.dtype}, expected {want_dt}")
        if mask.shape[1] < (V if mask_kind == MASK_F32 else (V + 31) // 32):
            raise ValueError(f"mask rows of {mask.shape[1]} elements are too short for {V} tokens")
        a.mask, a.n_masks = mask.data_ptr(), mask.shape[0]
        a.mask_ld = mask.stride(0) if mask.shape[0] > 1 else mask.shape[1]

    def _row_block(self, a, logits, vocab, logit_scale, mask_kind, mask, row_mask_id, empty="no rows to select from"):
        """The logits and mask fields that glb_score_args, glb_topk_args and glb_truncate_args share, checked and written
        into `a`; returns (n_rows, vocab).  `empty`: what to say of a logits tensor without rows."""
        if logits.dim() != 2 or logits.stride(1) != 1:
            raise ValueError("logits must be 2-D with unit inner stride")
        if logits.dtype not in _DT:
            raise TypeError(f"unsupported logits dtype {logits.dtype}")
        if logits.device != self.device:
            raise ValueError(f"logits on {logits.device}, engine on {self.device}")
        n_rows, width = logits.shape
        V = width if vocab is None else vocab
        if not 0 < V <= width:
            raise ValueError(f"vocab {V} outside (0, {width}]")
        if n_rows == 0:
            raise ValueError(empty)
        if not 0 < logit_scale < float("inf"):  # (NaN too; 0 or a negative scale would turn -inf logits into NaN / +inf)
            raise ValueError(f"logit_scale must be positive and finite, got {logit_scale!r}")
        self._check_dev(row_mask_id)
        if mask_kind not in (MASK_NONE, MASK_BITS, MASK_F32):
            raise ValueError(f"bad mask_kind {mask_kind}")
        a.logits, a.dtype = logits.data_ptr(), _DT[logits.dtype]
        a.n_rows, a.vocab, a.logit_scale = n_rows, V, logit_scale
        a.ld = logits.stride(0) if n_rows > 1 else max(width, logits.stride(0))
        a.mask_kind = mask_kind
        if mask_kind != MASK_NONE:
            self._mask_block(a, mask_kind, mask, V)
            if row_mask_id is not None and (row_mask_id.dtype != torch.int32 or row_mask_id.shape != (n_rows,)
                                            or not row_mask_id.is_contiguous()):
                raise ValueError("row_mask_id must be a contiguous int32 [n_rows] tensor")
            if row_mask_id is None and mask.shape[0] not in (1, n_rows):
                raise ValueError(f"no row_mask_id given but the table has {mask.shape[0]} rows: neither 1 nor {n_rows}")
            a.row_mask_id = None if row_mask_id is None else row_mask_id.data_ptr()
        elif mask is not None or row_mask_id is not None:
            raise ValueError("a mask table or row_mask_id given with MASK_NONE")
        return n_rows, V

    TOPK_OUTPUTS = ("logp", "logp_masked", "lse", "logZ")
    TOPK_MAX = 64

    def topk_rows(self, logits, k, *, vocab=None, logit_scale=1.0, mask_kind=MASK_NONE, mask=None, row_mask_id=None, want=("logp",)):
        """The k most probable tokens of every logits row (glb_topk_rows): with y = logits[r] * logit_scale,
        m the row's mask and key = y + m, a dict holding "token" int32 [n_rows, k] - the indices of the k largest keys, largest
        first, equal keys by lower index, -1 beyond the finite keys - and the names in `want`: "logp" = key - lse(y) and
        "logp_masked" = key - lse(y + m), float32 [n_rows, k] (-inf where the token is -1); "lse" = lse(y) and "logZ" =
        lse(y + m) - lse(y), float32 [n_rows].  No log-softmax is written.  logits, mask and row_mask_id as `score_rows`
        takes them - the keywords a constraint's `step_masks(..., by_row=True, ...)` returns."""
        if isinstance(mask, PreparedMasks) or mask_kind == MASK_PREPARED:
            raise TypeError("topk_rows reads bit rows or float rows as they lie, not prepared masks")
        want = tuple(want)
        for w in want:
            if w not in self.TOPK_OUTPUTS:
                raise ValueError(f"want names {w!r}; the outputs are {self.TOPK_OUTPUTS}")
        if not isinstance(k, int) or not 1 <= k <= self.TOPK_MAX:
            raise ValueError(f"k must be an integer in 1..{self.TOPK_MAX}, got {k!r}")
        a = _lib.TopkArgs()
        a.struct_size = C.sizeof(_lib.TopkArgs)
        n_rows, _ = self._row_block(a, logits, vocab, logit_scale, mask_kind, mask, row_mask_id)
        a.k = k
        out = {"token": torch.empty((n_rows, k), dtype=torch.int32, device=self.device)}
        a.out_token = out["token"].data_ptr()
        for w in want:
            out[w] = torch.empty((n_rows, k) if w.startswith("logp") else (n_rows,), dtype=torch.float32, device=self.device)
            setattr(a, "out_" + w, out[w].data_ptr())
        check(self.lib.glb_topk_rows(C.byref(a), self._stream()))
        return out

    TRUNCATE_OUTPUTS = ("threshold", "kept", "logmass")

    def truncate_rows(self, logits, *, top_k=0, top_p=1.0, min_p=0.0, vocab=None, logit_scale=1.0, mask_kind=MASK_NONE, mask=None,
                      row_mask_id=None, want=()):
        """The keep set of top-k, top-p (nucleus) and min-p truncation of every logits row (glb_truncate_rows):
        with y = logits[r] * logit_scale, m the row's mask and key = y + m, the row keeps {key > -inf, key >= tau}, tau the
        largest of the top_k-th largest key (top_k = 0: off), the nucleus boundary of mass top_p among those (1: off) and
        key_max + log(min_p) (0: off); ties at tau are kept.  A dict holding "bits" int32 [n_rows, ceil(vocab / 32)] - raw
        MASK_BITS rows, one per logits row, as `step`, `score_rows` and `topk_rows` read them - and the names in `want`, each
        [n_rows]: "threshold" float32 (tau), "kept" int32, "logmass" float32 = log(kept mass / mass of the finite keys).
        logits, mask and row_mask_id as `topk_rows` takes them - the keywords a constraint's `step_masks(..., by_row=True, ...)`
        returns."""
        if isinstance(mask, PreparedMasks) or mask_kind == MASK_PREPARED:
            raise TypeError("truncate_rows reads bit rows or float rows as they lie, not prepared masks")
        want = tuple(want)
        for w in want:
            if w not in self.TRUNCATE_OUTPUTS:
                raise ValueError(f"want names {w!r}; the outputs are {self.TRUNCATE_OUTPUTS}")
        top_k, top_p, log_min_p = check_truncation(top_k, top_p, min_p)
        a = _lib.TruncateArgs()
        a.struct_size = C.sizeof(_lib.TruncateArgs)
        n_rows, V = self._row_block(a, logits, vocab, logit_scale, mask_kind, mask, row_mask_id)
        if V > 1 << 24:
            raise ValueError(f"vocab {V} above 2^24")
        a.top_k, a.top_p, a.log_min_p = top_k, top_p, log_min_p
        words = (V + 31) // 32
        out = {"bits": torch.empty((n_rows, words), dtype=torch.int32, device=self.device)}
        a.out_bits, a.out_ld = out["bits"].data_ptr(), words
        for w in want:
            out[w] = torch.empty(n_rows, dtype=torch.int32 if w == "kept" else torch.float32, device=self.device)
            setattr(a, "out_" + w, out[w].data_ptr())
        check(self.lib.glb_truncate_rows(C.byref(a), self._stream()))
        return out

    def beam_select(self, score, alive, cand_token, cand_logp, width):
        """A beam step's selection (glb_beam_select): groups of `width` beams - score float32 and alive int32
        [G * width], cand_token int32 and cand_logp float32 [G * width, k] as `topk_rows` writes them.  Returns (parent int32,
        token int32, score float32), each [G * width]: per group the `width` largest of score[b] + cand_logp[b, j] over the
        live beams' candidates and of score[b] over the finished beams (token -1), largest first, ties by lower (b, j);
        parent is the beam's index within its group; missing positions are (-1, -1, -inf)."""
        self._check_dev(score, alive, cand_token, cand_logp)
        if not isinstance(width, int) or not 1 <= width <= self.TOPK_MAX:
            raise ValueError(f"width must be an integer in 1..{self.TOPK_MAX}, got {width!r}")
        n = score.numel()
        if score.dtype != torch.float32 or score.dim() != 1 or n == 0 or n % width or not score.is_contiguous():
            raise ValueError("score must be a contiguous float32 [G * width] tensor, G >= 1")
        if alive.dtype != torch.int32 or alive.shape != (n,) or not alive.is_contiguous():
            raise ValueError("alive must be a contiguous int32 [G * width] tensor")
        if cand_token.dtype != torch.int32 or cand_token.dim() != 2 or cand_token.shape[0] != n or not cand_token.is_contiguous():
            raise ValueError("cand_token must be a contiguous int32 [G * width, k] tensor")
        k = cand_token.shape[1]
        if not 1 <= k <= self.TOPK_MAX:
            raise ValueError(f"k must be in 1..{self.TOPK_MAX}, got {k}")
        if cand_logp.dtype != torch.float32 or cand_logp.shape != (n, k) or not cand_logp.is_contiguous():
            raise ValueError("cand_logp must be a contiguous float32 tensor of cand_token's shape")
        parent = torch.empty(n, dtype=torch.int32, device=self.device)
        token = torch.empty(n, dtype=torch.int32, device=self.device)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        check(self.lib.glb_beam_select(_ptr(score), _ptr(alive), _ptr(cand_token), _ptr(cand_logp), n // width, width, k,
                                       _ptr(parent), _ptr(token), _ptr(out), self._stream()))
        return parent, token, out

    # ---- the byte-level beam's three calls (glb_bytelm_*) ------------------------------------------------------
    BYTELM_SEL, BYTELM_ROW, BYTELM_LEAVES = 260, 257, 4

    def _bytelm_block(self, trie, node, alive, width, **tensors):
        """glb_bytelm_args over a trie's device arrays (`bytelm.byte_trie_arrays`: child_ptr, child_idx, child_sym, leaf_token,
        n_nodes, root) and the slot state; `tensors`: further fields by name, each checked for device and contiguity."""
        if not isinstance(width, int) or not 1 <= width <= self.TOPK_MAX:
            raise ValueError(f"width must be an integer in 1..{self.TOPK_MAX}, got {width!r}")
        n = node.numel()
        if node.dtype != torch.int32 or node.dim() != 1 or n == 0 or n % width:
            raise ValueError("node must be an int32 [G * width] tensor, G >= 1")
        if alive.dtype != torch.int32 or alive.shape != (n,):
            raise ValueError("alive must be an int32 [G * width] tensor")
        want = {"u": (torch.float32, (n,)), "w": (torch.float32, (n,)), "sel": (torch.int32, (n, self.BYTELM_SEL)),
                "mass": (torch.float32, (n, self.BYTELM_SEL)), "fresh": (torch.int32, (n // width,)),
                "byte": (torch.int32, (n // width,)), "logp": (torch.float32, (n // width,))}
        a = _lib.ByteLmArgs()
        a.struct_size = C.sizeof(_lib.ByteLmArgs)
        a.width, a.n_groups, a.n_nodes, a.root = width, n // width, int(trie["n_nodes"]), int(trie["root"])
        for k in ("child_ptr", "child_idx", "child_sym", "leaf_token"):
            self._check_dev(trie[k])
            setattr(a, k, trie[k].data_ptr())
        self._check_dev(node, alive)
        a.node, a.alive = node.data_ptr(), alive.data_ptr()
        for k, t in tensors.items():
            if t is None:
                continue
            self._check_dev(t)
            if k in want and (t.dtype != want[k][0] or tuple(t.shape) != want[k][1]):
                raise ValueError(f"{k} must be a {want[k][0]} tensor of shape {list(want[k][1])}, got {t.dtype} {list(t.shape)}")
            setattr(a, k, t.data_ptr())
        return a, n

    def bytelm_children(self, trie, node, alive, width):
        """The selection rows of a byte beam's slots (glb_bytelm_children): int32 [G * width, 260] - columns 0..255 the byte
        children of every alive slot's node, 256..259 its leaf children, -1 where there is none and for dead slots - the
        `nodes` argument of `TokenByteTrie.masses_from_logits`."""
        sel = torch.empty((node.numel(), self.BYTELM_SEL), dtype=torch.int32, device=self.device)
        a, _ = self._bytelm_block(trie, node, alive, width, sel=sel)
        check(self.lib.glb_bytelm_children(C.byref(a), self._stream()))
        return sel

    def bytelm_extend(self, trie, node, u, w, alive, sel, mass, width, fresh=None):
        """A byte beam's token boundary (glb_bytelm_extend): per group the `width` largest of the alive candidates' `w` and of
        u + log(mass) of every leaf child of a candidate that is not at the root; ties by existing before spawned, lower
        slot, lower leaf.  Kept candidates stay in their slots, spawned survivors fill the lowest freed ones, best first.
        Returns a dict: parent (the slot itself / the offering slot / -1: empty) and token (the committed token of a spawned
        slot, else -1), the new state node, u, w, alive, and `spawned` int32 [G * width] (the spawned slots, ascending,
        then -1) with `n_spawned` int32 [1]."""
        n = node.numel()
        out = {k: torch.empty(n, dtype=torch.int32, device=self.device) for k in ("parent", "token", "node", "alive", "spawned")}
        out["u"], out["w"] = self._f32(n), self._f32(n)
        out["n_spawned"] = self._i32(1)
        a, _ = self._bytelm_block(trie, node, alive, width, u=u, w=w, sel=sel, mass=mass, fresh=fresh,
                                  **{"out_" + k: t for k, t in out.items()})
        check(self.lib.glb_bytelm_extend(C.byref(a), self._stream()))
        return out

    def bytelm_next(self, trie, node, u, w, alive, sel, mass, width, byte=None, logp=None, fresh=None):
        """A byte beam's next-byte rows, or its advance (glb_bytelm_next).  byte None: returns (next float32 [G, 257] - the
        log-probabilities of the 256 bytes and, in column 256, of EOS; -inf rows for groups without a live candidate - and
        logZ float32 [G]).  byte int32 [G]: moves every candidate of the groups whose byte is in 0..256 to its child under
        that byte (node, w, alive are written in place; 256 ends the group), adds the row's entry to `logp` (float32 [G]),
        marks the groups in `fresh`, and returns None."""
        if byte is None:
            G = node.numel() // max(width, 1) if isinstance(width, int) else 0
            nxt = torch.empty((max(G, 1), self.BYTELM_ROW), dtype=torch.float32, device=self.device)
            logZ = self._f32(max(G, 1))
            a, _ = self._bytelm_block(trie, node, alive, width, u=u, w=w, sel=sel, mass=mass, out_next=nxt, out_logZ=logZ)
            check(self.lib.glb_bytelm_next(C.byref(a), self._stream()))
            return nxt, logZ
        if logp is None:
            raise ValueError("an advance needs logp")
        a, _ = self._bytelm_block(trie, node, alive, width, u=u, w=w, sel=sel, mass=mass, byte=byte, logp=logp, fresh=fresh)
        check(self.lib.glb_bytelm_next(C.byref(a), self._stream()))
        return None

    def bytelm_step(self, trie, node, u, w, alive, sel, mass, width, tables, state, ended, log_weight, logp, byte=None, uniform=None,
                    seed=0, offset=0, fresh=None, want_row=False, peek=False):
        """One byte step of a byte beam under a byte automaton, one launch (glb_bytelm_step).  `tables`: a
        `constraints.tables.DeviceTables` on this device; state and ended int32 [G], log_weight and logp float32 [G].  The
        byte: `byte` int32 [G] given (-1 leaves a group alone), else the first column whose cumulative constrained
        probability exceeds `uniform` float32 [G], else that rule on one Philox uniform per group from (seed, offset, g).
        node, w, alive, fresh, logp, state, ended and log_weight are written in place.  Returns a dict: `byte` int32 [G]
        (the given tensor, or the bytes drawn: -1 for a group that died or had ended), `logZc` float32 [G], and with `want_row` `row` float32 [G, 257], the constrained and renormalised row.
        peek: only `logZc` and `row` are made, nothing moves and `byte` is None."""
        from .constraints.tables import DeviceTables

        if not isinstance(tables, DeviceTables):
            raise ValueError(f"tables must be a DeviceTables, got {type(tables).__name__}")
        if tables.live is None:
            raise ValueError("tables without `live` (as `minimized` returns them): upload a host automaton")
        if byte is not None and uniform is not None:
            raise ValueError("give byte or uniform, not both")
        p = _lib.ByteLmStepArgs()
        p.struct_size, p.peek = C.sizeof(_lib.ByteLmStepArgs), int(bool(peek))
        p.beam, n = self._bytelm_block(trie, node, alive, width, u=u, w=w, sel=sel, mass=mass, byte=None if peek else byte, logp=logp,
                                       fresh=fresh)
        G, S = n // width, int(tables.n_states)
        want = {"delta": (torch.int32, (S, 256)), "accepting": (torch.uint8, (S,)), "live": (torch.uint8, (S,)),
                "arc_logw": (torch.float32, (S, 256)), "final_logw": (torch.float32, (S,)), "state": (torch.int32, (G,)),
                "ended": (torch.int32, (G,)), "log_weight": (torch.float32, (G,)), "uniform": (torch.float32, (G,))}
        given = dict(delta=tables.delta, accepting=tables.accepting, live=tables.live, arc_logw=tables.arc_logw,
                     final_logw=tables.final_logw, state=state, ended=ended, log_weight=log_weight, uniform=None if peek else uniform)
        for k, t in given.items():
            if t is None:
                if k not in ("arc_logw", "final_logw", "uniform"):
                    raise ValueError(f"{k} is missing")
                continue
            self._check_dev(t)
            if t.dtype != want[k][0] or tuple(t.shape) != want[k][1]:
                raise ValueError(f"{k} must be a {want[k][0]} tensor of shape {list(want[k][1])}, got {t.dtype} {list(t.shape)}")
            setattr(p, k, t.data_ptr())
        if logp is None:
            raise ValueError("logp is missing")
        p.n_states, p.seed, p.offset = S, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
        out = {"byte": byte, "logZc": self._f32(G)}
        if peek:
            out["byte"] = None
        elif byte is None:
            out["byte"] = self._i32(G)
            p.out_byte = out["byte"].data_ptr()
        p.out_logZc = out["logZc"].data_ptr()
        if want_row:
            out["row"] = torch.empty((G, self.BYTELM_ROW), dtype=torch.float32, device=self.device)
            p.out_row = out["row"].data_ptr()
        check(self.lib.glb_bytelm_step(C.byref(p), self._stream()))
        return out

    # ---- failed one-launch calls (include/glb.h: glb_workspace_check) ---------------------------------------------
    def error_word(self):
        """int32 [1] device view of the scratch buffer's error word: nonzero after a one-launch call whose waves gave
        up waiting for their records (token -2 / NaN outputs).  Hosts that copy results back let it ride along and hand
        the value to `raise_if_failed`."""
        ws = self._step_ws
        if ws is None:
            return torch.zeros(1, dtype=torch.int32, device=self.device)
        return ws[ws.numel() - 64: ws.numel() - 60].view(torch.int32)

    def raise_if_failed(self, err_count=None, tokens=None, lse=None, what="glb_logprob_mask_sample"):
        """Raise when a one-launch call did not complete: `err_count` (the error word's value, already on the host),
        host `tokens` holding -2, or host `lse` / logZ values holding NaN.  Clears the error word."""
        bad = bool(err_count)
        if tokens is not None and not bad:
            bad = bool((np.asarray(tokens) == -2).any())
        if lse is not None and not bad:
            bad = bool(np.isnan(np.asarray(lse, dtype=np.float32)).any())
        if bad:
            if self._step_ws is not None:
                self.error_word().zero_()
            raise GlbError(GLB_EHIP, f"{what}: waves of the launch gave up waiting for their row's records (token -2 / "
                                     "NaN): the call did not complete and its results must not be used")

    def check(self):
        """Synchronising check of the scratch buffer's error word (glb_workspace_check): raises after a failed call."""
        if self._step_ws is not None:
            check(self.lib.glb_workspace_check(_ptr(self._step_ws), self._stream()))

    def set_spin_limit(self, microseconds):
        """Watchdog of the waits inside the one-launch calls (0: the default, 2 s; None: GLB_SPIN_NONE - a wave gives up
        at the first poll that finds a record missing, which forces the failure path)."""
        check(self.lib.glb_set_spin_limit(0xFFFFFFFFFFFFFFFF if microseconds is None else int(microseconds)))

    def timing_events(self, n):
        """n (start, stop) pairs of HIP events for `step(timing_events=...)` / `StepPlan.run_timed`: created and
        recorded once here (torch makes the hipEvent_t on first record), so that using them later puts nothing but the
        launch itself on the stream."""
        with torch.cuda.device(self.device):
            pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for a, b in pairs:
                a.record()
                b.record()
            torch.cuda.current_stream(self.device).synchronize()
        return pairs

    def step_plan(self, logits, **kw):
        """`step()` with the host work done once: validates and fills the argument block, returns a `StepPlan` whose
        `run(offset=..., seed=...)` only launches (a few microseconds of host time instead of a few tens - for loops
        that call the same configuration again and again, e.g. `bench.py --workload kernel`).  The tensors must keep
        their storage; the scratch buffer is the engine's, so a plan is valid until another, larger step reallocates
        it (run() checks)."""
        return self.step(logits, _plan=True, **kw)

    def noise_rng(self, seed, vocab, ahead=False):
        """The parity draw's noise source: torch's CPU generator seeded with `seed`, rows of `vocab` exponentials, on the
        device (DeviceRng; ahead: the next call's rows generated on a side stream once `prefetch()` is called)."""
        return DeviceRng(self, seed, vocab, ahead=ahead)

    def mt_polys(self, vocab, n_windows):
        """Device table of the MT19937 jump polynomials for rows of `vocab` exponentials (stride 2 * vocab words), enough
        for `n_windows` row windows per call (glb_mt19937_jump_polys; computed on the host once and cached).  Returns
        (int64 tensor [(SMALL + n_big), 312], n_big)."""
        small = DeviceRng.SMALL
        need_big = max(1, -(-int(n_windows) // small))
        ent = self._mt_polys.get(vocab)
        if ent is None or ent[1] < need_big:
            n_big = max(need_big, 2 * ent[1] if ent else 0)
            host = np.zeros((small + n_big, MT_POLY_WORDS), np.uint64)
            check(self.lib.glb_mt19937_jump_polys(2 * int(vocab), small, n_big, C.c_void_p(host.ctypes.data)))
            ent = self._mt_polys[vocab] = (torch.from_numpy(host.view(np.int64)).to(self.device), n_big)
        return ent

    def prepare_masks(self, bits, vocab, logits_dtype=torch.float32):
        """int32 bit rows [K, >= ceil(V/32)] -> `PreparedMasks` for logits of `logits_dtype` (glb_mask_prepare)."""
        if bits.dim() == 1:
            bits = bits[None]
        self._check_dev(bits)
        if bits.dtype != torch.int32:
            raise TypeError("bit masks must be int32 words")
        K = bits.shape[0]
        need = self.lib.glb_mask_prepared_bytes(K, vocab)
        blob = torch.empty(need, dtype=torch.uint8, device=self.device)
        dt = _DT[logits_dtype]
        check(self.lib.glb_mask_prepare(_ptr(bits), K, vocab, bits.stride(0) if K > 1 else bits.shape[1], dt,
                                        _ptr(blob), need, self._stream()))
        return PreparedMasks(blob, K, vocab, dt)

    def update_prepared_masks(self, prepared, bits, rows):
        """Re-prepare only the masks `rows` (int32 device tensor) of `prepared` (a `PreparedMasks` made from `bits` before)
        from their current bit rows (glb_mask_prepare_rows): masks that change a few at a time cost what changed."""
        if bits.dim() == 1:
            bits = bits[None]
        self._check_dev(bits, rows)
        if bits.dtype != torch.int32 or rows.dtype != torch.int32:
            raise TypeError("bit masks and row indices must be int32")
        if bits.shape[0] != prepared.n_masks:
            raise ValueError("the bit rows are not the ones these masks were prepared from")
        K = prepared.n_masks
        check(self.lib.glb_mask_prepare_rows(_ptr(bits), K, prepared.vocab, bits.stride(0) if K > 1 else bits.shape[1], prepared.dtype,
                                             _ptr(rows), rows.numel(), _ptr(prepared.blob), prepared.blob.numel(), self._stream()))
        return prepared

    def log_softmax_rows(self, logits, vocab=None, logit_scale=1.0, out=None, want_lse=False, workspace=None,
                         out_dtype=torch.float32):
        """out[r] = logits[r] - logsumexp(logits[r]) (glb_log_softmax_rows).  `out_dtype`: float32 (default) or the
        logits' own dtype - what the reference returns (cache.py:96 keeps the model's dtype): the float32 result rounded
        to nearest even.  `workspace`: a uint8 device tensor to lend instead of the engine's own scratch (one the
        library has not initialised takes the form that does not tag its records)."""
        if logits.dim() != 2 or logits.stride(1) != 1:
            raise ValueError("logits must be 2-D with unit inner stride")
        n_rows, width = logits.shape
        V = width if vocab is None else vocab
        ld = logits.stride(0) if n_rows > 1 else max(width, logits.stride(0))
        if out is None:
            out = torch.empty((n_rows, V), dtype=out_dtype, device=self.device)
        if out.dtype not in (torch.float32, logits.dtype):
            raise TypeError(f"log-probabilities leave as float32 or as {logits.dtype}, not {out.dtype}")
        lse = self._f32(n_rows) if want_lse else None
        out_ld = out.stride(0) if n_rows > 1 else max(V, out.stride(0))
        need = self.lib.glb_log_softmax_workspace_bytes(n_rows, V)
        ws = self._scratch(need) if workspace is None else workspace
        if ws.numel() < need:
            raise ValueError(f"workspace of {ws.numel()} bytes, {need} needed")
        check(self.lib.glb_log_softmax_rows(_ptr(logits), _DT[logits.dtype], n_rows, V, ld, logit_scale, _ptr(out),
                                            _DT[out.dtype], out_ld, _ptr(lse), _ptr(ws), ws.numel(), self._stream()))
        return (out, lse) if want_lse else out

    def row_lse(self, logits, vocab=None, logit_scale=1.0):
        """logsumexp(logits[r] * logit_scale) per row, float32 [n_rows] (glb_log_softmax_rows with no rows out: the rows are
        read once, nothing but n_rows floats is written) - the lse `trie_rows` / `trie_masses` take next to raw logits."""
        if logits.dim() != 2 or logits.stride(1) != 1:
            raise ValueError("logits must be 2-D with unit inner stride")
        n_rows, width = logits.shape
        V = width if vocab is None else vocab
        ld = logits.stride(0) if n_rows > 1 else max(width, logits.stride(0))
        lse = self._f32(n_rows)
        ws = self._scratch(self.lib.glb_log_softmax_workspace_bytes(n_rows, V))
        check(self.lib.glb_log_softmax_rows(_ptr(logits), _DT[logits.dtype], n_rows, V, ld, logit_scale, None, F32, 0,
                                            _ptr(lse), _ptr(ws), ws.numel(), self._stream()))
        return lse

    def mask_to_bits(self, mask):
        """{0,-inf} float log-masks [K, V] -> packed int32 bit rows [K, ceil(V/32)] + non-binary flag."""
        if mask.dim() == 1:
            mask = mask[None]
        mask = mask.to(self.device, torch.float32).contiguous()
        K, V = mask.shape
        W = (V + 31) // 32
        bits = torch.empty((K, W), dtype=torch.int32, device=self.device)
        flag = self._i32(1)
        check(self.lib.glb_mask_f32_to_bits(_ptr(mask), K, V, V, _ptr(bits), W, _ptr(flag), self._stream()))
        return bits, flag

    # ------------------------------------------------------------------------------------------
    def hash_contexts(self, tokens, starts, lengths):
        """The contexts' hashes (int64 tensor holding the 64-bit values) for `group_contexts(hashes=...)`; a context's
        hash extends token by token (`particles_advance(hashes=...)` keeps it up to date)."""
        n = lengths.numel()
        self._check_dev(tokens, starts, lengths)
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        check(self.lib.glb_hash_contexts(_ptr(tokens), _ptr(starts), _ptr(lengths), n, _ptr(out), self._stream()))
        return out

    def group_contexts(self, tokens, starts, lengths, hashes=None):
        """Exact dedup, first-appearance order.  Returns (group_of[n], rep[n], n_groups[1]) on device.  `hashes`: the
        contexts' hashes if the caller keeps them (hash_contexts); the tokens are then read only to confirm duplicates."""
        n = lengths.numel()
        self._check_dev(tokens, starts, lengths, hashes)
        need = self.lib.glb_group_contexts_workspace(n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=self.device)
        group_of, rep, ng = self._i32(n), self._i32(n), self._i32(1)
        check(self.lib.glb_group_contexts(_ptr(tokens), _ptr(starts), _ptr(lengths), n, _ptr(hashes), _ptr(group_of),
                                          _ptr(rep), _ptr(ng), _ptr(self._ws), self._ws.numel(), self._stream()))
        return group_of, rep, ng

    def match_prefixes(self, tokens, starts, lengths, prefix_tokens, prefix_starts, prefix_lengths):
        n = lengths.numel()
        npre = 0 if prefix_lengths is None else prefix_lengths.numel()
        pref, base = self._i32(n), self._i32(n)
        check(self.lib.glb_match_prefixes(_ptr(tokens), _ptr(starts), _ptr(lengths), n, _ptr(prefix_tokens),
                                          _ptr(prefix_starts), _ptr(prefix_lengths), npre, _ptr(pref), _ptr(base),
                                          self._stream()))
        return pref, base

    def gather_padded(self, tokens, starts, lengths, sel, n_sel, base, pad_id, p_max, l_max):
        dev = self.device
        ids = torch.empty((n_sel, l_max), dtype=torch.int64, device=dev)
        am = torch.empty((n_sel, p_max + l_max), dtype=torch.int64, device=dev)
        pos = torch.empty((n_sel, l_max), dtype=torch.int64, device=dev)
        last = self._i32(n_sel)
        check(self.lib.glb_gather_padded(_ptr(tokens), _ptr(starts), _ptr(lengths), _ptr(sel), n_sel, _ptr(base),
                                         pad_id, p_max, l_max, _ptr(ids), _ptr(am), _ptr(pos), _ptr(last),
                                         self._stream()))
        return ids, am, pos, last

    def gather_kv_padded(self, slab_ptrs, slab_len, prefix_of, heads, head_dim, p_max, dtype):
        """slab_ptrs: int64 device tensor of raw pointers to [heads, len_k, head_dim] slabs."""
        n_rows = prefix_of.numel()
        out = torch.empty((n_rows, heads, p_max, head_dim), dtype=dtype, device=self.device)
        check(self.lib.glb_gather_kv_padded(_ptr(slab_ptrs), _ptr(slab_len), slab_len.numel(), _ptr(prefix_of),
                                            n_rows, heads, head_dim, p_max, out.element_size(), _ptr(out),
                                            self._stream()))
        return out

    def particles_advance(self, contexts, lengths, active, log_weights, logZ, token, eos_id, max_len, hashes=None):
        n, ld = contexts.shape
        check(self.lib.glb_particles_advance(_ptr(contexts), ld, _ptr(lengths), _ptr(active), _ptr(log_weights),
                                             _ptr(logZ), _ptr(token), n, eos_id, max_len, _ptr(hashes), self._stream()))

    def normalize_weights(self, log_weights):
        n = log_weights.numel()
        probs, stats = self._f32(n), self._f32(2)
        check(self.lib.glb_normalize_weights(_ptr(log_weights), n, _ptr(probs), _ptr(stats), self._stream()))
        return probs, stats

    # ---- fp32 projections on bf16 MFMA (glb_gemm_*: DESIGN.md §12) ------------------------------------------------
    def gemm_split_supports(self, k, n):
        return self.lib.glb_gemm_split_bytes(k, n) > 0

    def gemm_split_blocks_per_cu(self, gelu=False, form=None):
        """Blocks of the split GEMM's kernel (with the GELU epilogue when `gelu`) resident on one CU of this device; `form`:
        _lib.GEMM_FORM_LARGE (the default) or _lib.GEMM_FORM_SMALL."""
        blocks = C.c_int(0)
        with torch.cuda.device(self.device):
            if form is None:
                check(self.lib.glb_gemm_split_blocks_per_cu(int(bool(gelu)), C.byref(blocks)))
            else:
                check(self.lib.glb_gemm_split_form_blocks_per_cu(int(form), int(bool(gelu)), C.byref(blocks)))
        return blocks.value

    def gemm_split_pick(self, m, n, k, n_cus=None):
        """The tile form glb_gemm_f32_split runs for an [m, k] x [k, n] call on a device of `n_cus` CUs (this one's by
        default): _lib.GEMM_FORM_LARGE or _lib.GEMM_FORM_SMALL (glb_gemm_split_pick: host arithmetic only)."""
        if n_cus is None:
            n_cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        form = C.c_int(0)
        check(self.lib.glb_gemm_split_pick(m, n, k, n_cus, C.byref(form)))
        return form.value

    def gemm_split_weights(self, w):
        """The packed hi / mid / lo bf16 image of a float32 weight w [K, N] (glb_gemm_split_weights: 6 bytes per element),
        or None when the kernel does not serve its shape."""
        k, n = w.shape
        nbytes = self.lib.glb_gemm_split_bytes(k, n)
        if nbytes == 0 or w.dtype != torch.float32 or w.stride(1) != 1:
            return None
        if w.device != self.device:
            raise ValueError(f"tensor on {w.device}, engine on {self.device}")
        out =torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        check(self.lib.glb_gemm_split_weights(_ptr(w), k, n, w.stride(0), _ptr(out), nbytes, self._stream()))
        return out

    def gemm_split(self, x, w_split, n, bias=None, gelu=False, out=None, form=None, residual=None):
        """x [..., K] float32 (rows of unit inner stride) times the weight whose image is `w_split`, plus bias [N], then the
        tanh GELU when `gelu` (glb_gemm_f32_split).  Returns [..., N] float32, or None when the kernel does not serve the
        call (alignment, shape, a bias that is not contiguous float32): the caller then runs its library GEMM.  `out`: a
        float32 [M, N] tensor on the engine's device with unit inner stride (rows may be padded); ValueError otherwise, and
        for a bias of the wrong length or device.  `form`: None lets the library pick the tile form from the shape;
        _lib.GEMM_FORM_LARGE / _lib.GEMM_FORM_SMALL force one (glb_gemm_f32_split_form) - the result's bits are the same.
        `residual`: float32 [..., N] (M rows of unit inner stride) added to the result in the kernel's epilogue, after the bias
        (glb_gemm_f32_split_residual): the bits of `gemm_split(x, ...) + residual`.  `out` may be `residual` itself; with
        `gelu`, on another device or of another shape it is a ValueError, overlapping `out` in part a GlbError: no launch.
        Non-finite and out-of-range operands: include/glb.h."""
        k = x.shape[-1]
        x2 = x.reshape(-1, k)
        m = x2.shape[0]
        if m == 0 or x2.stride(1) != 1:
            return None
        if bias is not None:
            if bias.device != self.device:
                raise ValueError(f"bias on {bias.device}, engine on {self.device}")
            if bias.dim() != 1 or bias.numel() != n:
                raise ValueError(f"bias of shape {tuple(bias.shape)}, expected ({n},)")
            if bias.dtype != torch.float32 or bias.stride(0) != 1:
                return None
        if out is None:
            out = torch.empty((m, n), dtype=torch.float32, device=self.device)
        else:
            if out.device != self.device:
                raise ValueError(f"out on {out.device}, engine on {self.device}")
            if out.dtype != torch.float32 or tuple(out.shape) != (m, n):
                raise ValueError(f"out is {out.dtype} {tuple(out.shape)}, expected torch.float32 {(m, n)}")
            if out.stride(1) != 1 or (m > 1 and out.stride(0) < n):
                raise ValueError(f"out has strides {out.stride()}: rows of unit inner stride, at least {n} apart, are needed")
        a = _lib.GemmArgs()
        a.struct_size = C.sizeof(_lib.GemmArgs)
        a.m, a.n, a.k = m, n, k
        a.a, a.lda = x2.data_ptr(), x2.stride(0)
        a.w_split = w_split.data_ptr()
        a.bias = bias.data_ptr() if bias is not None else None
        a.c, a.ldc = out.data_ptr(), max(out.stride(0), n)  # (a one-row tensor's stride is arbitrary)
        a.epilogue = _lib.GEMM_BIAS_GELU_TANH if gelu else _lib.GEMM_BIAS
        if residual is not None:
            if gelu:
                raise ValueError("gemm_split: the residual epilogue does not follow the GELU")
            if residual.device != self.device:
                raise ValueError(f"residual on {residual.device}, engine on {self.device}")
            r2 = residual.view(-1, n) if residual.dim() != 2 else residual
            if residual.dtype != torch.float32 or tuple(r2.shape) != (m, n) or r2.stride(1) != 1 or (m > 1 and r2.stride(0) < n):
                raise ValueError(f"residual is {residual.dtype} {tuple(residual.shape)} with strides {residual.stride()}: "
                                 f"torch.float32 {(m, n)} rows of unit inner stride are needed")
            rc = self.lib.glb_gemm_f32_split_residual(C.byref(a), r2.data_ptr(), max(r2.stride(0), n), int(form or 0),
                                                      self._stream())  # (a partial overlap with out: GlbError below)
        elif form is None:
            rc = self.lib.glb_gemm_f32_split(C.byref(a), self._stream())
        else:
            rc = self.lib.glb_gemm_f32_split_form(C.byref(a), int(form), self._stream())
        if rc == _lib.GLB_EUNSUPPORTED:
            return None
        check(rc)
        return out.view(*x.shape[:-1], n)

    # ---- the plan of a row-packed encoding (glb_packed_plan: DESIGN.md §27) -----------------------------------------
    def packed_plan(self, batch, sel, n_sel, grp, groups, n_tail_rows, pos_cap):
        """The four arrays of kv.encode_packed's plan in two launches: (segments int32 [G + n_sel, 4], ids int64 [M], pos
        int64 [M], last int64 [n_sel]) for the ragged `batch` = (tokens int32, starts int64, lengths int32), `sel` / `grp`
        int32 (their first n_sel entries) and `groups` (kv.PromptGroups); M = groups.n_rows + n_tail_rows.  Nothing is read
        back; hostile lengths are clamped as the torch-op plan clamps them (include/glb.h)."""
        tokens, starts, lengths = batch
        G, n_pre = len(groups.lens), groups.n_rows
        ins = (tokens, starts, lengths, sel, grp, groups.starts_d, groups.lens_d, groups.segments, groups.ids, groups.pos)
        self._check_dev(*ins)
        want = (torch.int32, torch.int64, torch.int32, torch.int32, torch.int32, torch.int32, torch.int32, torch.int32,
                torch.int64, torch.int64)
        if any(t.dtype != d for t, d in zip(ins, want)):
            raise ValueError(f"packed_plan: dtypes {[t.dtype for t in ins]}, expected {list(want)}")
        if sel.numel() < n_sel or grp.numel() < n_sel or starts.numel() != lengths.numel() or groups.ids.numel() != n_pre:
            raise ValueError("packed_plan: sel / grp shorter than n_sel, or starts / lengths / the prompts' rows disagree")
        M = n_pre + int(n_tail_rows)
        seg = torch.empty((G + n_sel, 4), dtype=torch.int32, device=self.device)
        ids = torch.empty(M, dtype=torch.int64, device=self.device)
        pos = torch.empty(M, dtype=torch.int64, device=self.device)
        last = torch.empty(n_sel, dtype=torch.int64, device=self.device)
        ends = self._i32(n_sel)
        a = _lib.PackedPlanArgs()
        a.struct_size = C.sizeof(_lib.PackedPlanArgs)
        a.n_tokens, a.n_contexts, a.n_sel, a.n_groups = tokens.numel(), lengths.numel(), n_sel, G
        a.n_pre, a.n_tail_rows, a.pos_cap = n_pre, int(n_tail_rows), int(pos_cap)
        (a.tokens, a.starts, a.lengths, a.sel, a.grp, a.group_starts, a.group_lens, a.group_segments, a.group_ids,
         a.group_pos) = (t.data_ptr() for t in ins)
        a.segments, a.ids, a.pos, a.last, a.ends = (t.data_ptr() for t in (seg, ids, pos, last, ends))
        check(self.lib.glb_packed_plan(C.byref(a), self._stream()))
        return seg, ids, pos, last

    # ---- LoRA merge (glb_lora_merge: DESIGN.md §13) ------------------------------------------------------------------
    def lora_merge(self, jobs):
        """out = w + scale * b @ a for every job, in ONE library call (one launch per weight dtype among the jobs).  A job is
        a dict: `w` [n_out, k_in] (or [k_in, n_out] with `transposed`: GPT-2's Conv1D), `a` = lora_A [r, k_in], `b` = lora_B
        [n_out, r], `scale` (float), `transposed` (bool), `out` (w's dtype and layout; must not overlap w, a or b).  Every
        matrix has unit inner stride; rows may be padded.  Arithmetic: include/glb.h glb_lora_merge (bit-exact contract)."""
        n = len(jobs)
        if n == 0:
            return
        table = (_lib.LoraJob * n)()
        for q, j in zip(table, jobs):
            w, a, b, out = j["w"], j["a"], j["b"], j["out"]
            for t in (w, a, b, out):
                if t.device != self.device:
                    raise ValueError(f"tensor on {t.device}, engine on {self.device}")
                if t.dim() != 2 or t.stride(1) != 1:
                    raise ValueError("lora_merge: every matrix must be 2-D with unit inner stride")
                if t.dtype not in _DT:
                    raise ValueError(f"lora_merge: unsupported dtype {t.dtype}")
            if a.dtype != b.dtype or out.dtype != w.dtype or out.shape != w.shape:
                raise ValueError("lora_merge: a / b must share a dtype, out must match w's dtype and shape")
            tr = bool(j.get("transposed", False))
            q.struct_size = C.sizeof(_lib.LoraJob)
            q.w_dtype, q.ab_dtype, q.w_transposed = _DT[w.dtype], _DT[a.dtype], int(tr)
            q.k_in, q.n_out = (w.shape[0], w.shape[1]) if tr else (w.shape[1], w.shape[0])
            q.r = a.shape[0]
            if tuple(a.shape) != (q.r, q.k_in) or tuple(b.shape) != (q.n_out, q.r):
                raise ValueError(f"lora_merge: a {tuple(a.shape)} / b {tuple(b.shape)} do not fit w {tuple(w.shape)}")
            q.w, q.ldw = w.data_ptr(), w.stride(0)
            q.a, q.lda = a.data_ptr(), a.stride(0)
            q.b, q.ldb = b.data_ptr(), b.stride(0)
            q.scale = float(j["scale"])
            q.out, q.ldo = out.data_ptr(), out.stride(0)
        nbytes = self.lib.glb_lora_merge_workspace_bytes(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)  # (freed in stream order: the launch reads it first)
        check(self.lib.glb_lora_merge(table, n, _ptr(ws), nbytes, self._stream()))

    # ---- LoRA per row (glb_lora_rows: DESIGN.md §15) -----------------------------------------------------------------
    def lora_rows_table(self, slots):
        """The device table of glb_lora_rows for `slots`: a list (one item per adapter slot) of equally long lists (one item
        per module index) holding None - the adapter does not target the module - or a dict `a` = lora_A [r, k_in], `b` =
        lora_B [n_out, r] (2-D, unit inner stride, one dtype), `scale`.  Uploaded once; the returned object keeps the
        tensors alive and goes to `lora_rows`."""
        n_slots = len(slots)
        n_modules = len(slots[0]) if n_slots else 0
        nbytes = self.lib.glb_lora_rows_table_bytes(n_slots, n_modules)
        if nbytes == 0:
            raise ValueError(f"lora_rows_table: {n_slots} slots x {n_modules} modules is not served")
        host = (_lib.LoraRowsEntry * (n_slots * n_modules))()
        keep, r_max = [], 0
        for si, mods in enumerate(slots):
            if len(mods) != n_modules:
                raise ValueError("lora_rows_table: every slot lists every module")
            for mi, j in enumerate(mods):
                q = host[si * n_modules + mi]
                q.struct_size = C.sizeof(_lib.LoraRowsEntry)
                if j is None:
                    continue
                a, b = j["a"], j["b"]
                for t in (a, b):
                    if t.device != self.device:
                        raise ValueError(f"tensor on {t.device}, engine on {self.device}")
                    if t.dim() != 2 or t.stride(1) != 1 or t.dtype not in _DT:
                        raise ValueError("lora_rows_table: a / b must be 2-D float32 / bfloat16 / float16 with unit inner stride")
                if a.dtype != b.dtype or a.shape[0] != b.shape[1]:
                    raise ValueError("lora_rows_table: a / b must share a dtype and the rank")
                q.ab_dtype = _DT[a.dtype]
                q.n_out, q.k_in, q.r = b.shape[0], a.shape[1], a.shape[0]
                q.a, q.lda = a.data_ptr(), a.stride(0)
                q.b, q.ldb = b.data_ptr(), b.stride(0)
                q.scale = float(j["scale"])
                keep += [a, b]
                r_max = max(r_max, int(a.shape[0]))
        dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        check(self.lib.glb_lora_rows_table_upload(host, n_slots, n_modules, _ptr(dev), nbytes, self._stream()))
        return LoraRowsTable(dev, n_slots, n_modules, max(r_max, 1), keep)

    @staticmethod
    def _rows_2d(t, what):
        """(rows, row pitch) of a tensor [..., C] read as a matrix of rows with one pitch (a column slice of a contiguous
        tensor qualifies).  The pitch is the stride of the innermost row dimension of size > 1 (the stride of a dimension
        of size 1 means nothing); with one row it is C."""
        if t.dim() < 1 or t.stride(-1) != 1:
            raise ValueError(f"lora_rows: {what} must have unit inner stride")
        rows, pitch = 1, None
        for d in range(t.dim() - 2, -1, -1):
            if t.shape[d] == 1:
                continue
            if pitch is None:  # (rows == 1 so far)
                pitch = t.stride(d)
            elif t.stride(d) != pitch * rows:
                raise ValueError(f"lora_rows: {what} is not a matrix of rows with one pitch")
            rows *= t.shape[d]
        return rows, (t.shape[-1] if pitch is None else pitch)

    def lora_rows(self, x, y, row_slot, table, module_index):
        """In place on y [..., N], the output of a projection whose input was x [..., K] (same dtype, same rows): for every
        row with row_slot >= 0 (int32, device, one per row) y += scale * (x A^T) B^T with that slot's entry of module
        `module_index`; other rows, and rows whose slot has no entry for the module, are not written (glb_lora_rows)."""
        if x.dtype != y.dtype or x.dtype not in _DT:
            raise ValueError(f"lora_rows: x {x.dtype} / y {y.dtype} must be one of float32, bfloat16, float16")
        for t in (x, y, row_slot, table.dev):  # (y may be a column slice: not contiguous)
            if t.device != self.device:
                raise ValueError(f"tensor on {t.device}, engine on {self.device}")
        try:
            m, ldx = self._rows_2d(x, "x")
        except ValueError:  # (x is only read: an input that is no matrix of rows is COPIED, on every such call)
            x = x.contiguous()
            m, ldx = self._rows_2d(x, "x")
        my, ldy = self._rows_2d(y, "y")
        if m != my or m == 0 or row_slot.dtype != torch.int32 or row_slot.numel() != m or not row_slot.is_contiguous():
            raise ValueError(f"lora_rows: x has {m} rows, y {my}, row_slot {tuple(row_slot.shape)} {row_slot.dtype}")
        need = self.lib.glb_lora_rows_workspace_bytes(m, table.r_max)
        ws = self._lora_rows_ws
        if ws is None or ws.numel() < need:  # (grown, never shrunk)
            if torch.cuda.is_current_stream_capturing():
                # the buffer it replaces may be held by a captured graph, and one made now would belong to this capture
                raise RuntimeError(f"lora_rows: the workspace must grow to {need} bytes while a stream is capturing; run the "
                                   "call once at this size before the capture")
            ws = self._lora_rows_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        a = _lib.LoraRowsArgs()
        a.struct_size = C.sizeof(_lib.LoraRowsArgs)
        a.dtype = _DT[x.dtype]
        a.m, a.n, a.k = m, y.shape[-1], x.shape[-1]
        a.x, a.ldx = x.data_ptr(), ldx
        a.y, a.ldy = y.data_ptr(), ldy
        a.row_slot, a.table = row_slot.data_ptr(), table.dev.data_ptr()
        a.n_slots, a.n_modules, a.module, a.r_max = table.n_slots, table.n_modules, int(module_index), table.r_max
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        check(self.lib.glb_lora_rows(C.byref(a), self._stream()))
        return y

    # ---- 4-bit block-quantised weights (glb_w4_*: DESIGN.md §14) --------------------------------------------------------
    @staticmethod
    def _codebook(codebook):
        cb = (C.c_float * 16)(*[float(v) for v in codebook])
        if len(codebook) != 16:
            raise ValueError("a 4-bit codebook has 16 entries")
        return cb

    def w4_bytes(self, n, k):
        return self.lib.glb_w4_bytes(n, k)

    def w4_gemm_max_rows(self):
        return self.lib.glb_w4_gemm_max_rows()

    def _w4_args(self, w, n, k, transposed, codebook, image):
        if w.device != self.device or image.device != self.device:
            raise ValueError(f"tensor on {w.device} / {image.device}, engine on {self.device}")
        if w.dim() != 2 or w.stride(1) != 1 or w.dtype not in _DT:
            raise ValueError("w4: the weight must be 2-D float32 / bfloat16 / float16 with unit inner stride")
        if tuple(w.shape) != ((k, n) if transposed else (n, k)):
            raise ValueError(f"w4: weight {tuple(w.shape)} does not fit n {n}, k {k}, transposed {transposed}")
        a = _lib.W4Args()
        a.struct_size = C.sizeof(_lib.W4Args)
        a.dtype, a.transposed = _DT[w.dtype], int(bool(transposed))
        a.n, a.k = n, k
        a.w, a.ldw = w.data_ptr(), w.stride(0)
        a.codebook = self._codebook(codebook)
        a.image, a.image_bytes = image.data_ptr(), image.numel()
        return a

    def w4_quantize(self, w, codebook, transposed=False, out=None):
        """The packed 4-bit image (uint8 [glb_w4_bytes(n, k)]) of a weight w [n, k] (or [k, n] with `transposed`: GPT-2's
        Conv1D) in float32 / bfloat16 / float16, rows of unit inner stride (glb_w4_quantize: one pass over w), or None
        when the shape is not served (k % 64 != 0)."""
        n, k = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
        nbytes = self.lib.glb_w4_bytes(n, k)
        if nbytes == 0:
            return None
        if out is None:
            out = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        a = self._w4_args(w, n, k, transposed, codebook, out)
        check(self.lib.glb_w4_quantize(C.byref(a), self._stream()))
        return out

    def w4_dequantize(self, image, n, k, codebook, dtype=torch.float32, transposed=False, out=None):
        """W' [n, k] (or [k, n] with `transposed`) of a packed image, in `dtype` (glb_w4_dequantize); `out`: a 2-D tensor of
        that shape with unit inner stride (rows may be padded).  None when the shape is not served."""
        if self.lib.glb_w4_bytes(n, k) == 0:
            return None
        if out is None:
            out = torch.empty((k, n) if transposed else (n, k), dtype=dtype, device=self.device)
        a = self._w4_args(out, n, k, transposed, codebook, image)
        check(self.lib.glb_w4_dequantize(C.byref(a), self._stream()))
        return out

    def w4_gemm(self, x, image, n, codebook, bias=None, out=None):
        """x [..., K] bfloat16 / float16 (rows of unit inner stride) times the dequantised weight of `image`, transposed,
        plus bias [N] of x's dtype (glb_w4_gemm: codes expanded in registers).  Returns [..., N] in x's dtype, or None
        when the kernel does not serve the call (more rows than glb_w4_gemm_max_rows(), shape, alignment): the caller then
        dequantises and runs its library GEMM."""
        k = x.shape[-1]
        x2 = x.reshape(-1, k)
        m = x2.shape[0]
        if m == 0 or x2.stride(1) != 1 or x.dtype not in (torch.bfloat16, torch.float16):
            return None
        if bias is not None and bias.dtype != x.dtype:
            return None
        ws_bytes = self.lib.glb_w4_gemm_workspace_bytes(m, n, k)
        if ws_bytes == 0:
            return None
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)  # (freed in stream order)
        y = out if out is not None else torch.empty((m, n), dtype=x.dtype, device=self.device)
        a = _lib.W4GemmArgs()
        a.struct_size = C.sizeof(_lib.W4GemmArgs)
        a.dtype = _DT[x.dtype]
        a.m, a.n, a.k = m, n, k
        a.x, a.ldx = x2.data_ptr(), x2.stride(0)
        a.image = image.data_ptr()
        a.codebook = self._codebook(codebook)
        a.bias = bias.data_ptr() if bias is not None else None
        a.y, a.ldy = y.data_ptr(), y.stride(0)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
        rc = self.lib.glb_w4_gemm(C.byref(a), self._stream())
        if rc == _lib.GLB_EUNSUPPORTED:
            return None
        check(rc)
        return y if out is not None else y.view(*x.shape[:-1], n)

    # ---- byte-level DFA constraints (glb_dfa_*: DESIGN.md §17; constraints.DeviceConstraint fills the argument block) ---------
    # the glb_dfa_* entries of `_lib.SYMBOLS` that take (argument block, stream)
    DFA_CALLS = frozenset(name for name, (_, argtypes) in _lib.SYMBOLS.items()
                          if name.startswith("glb_dfa_") and argtypes and issubclass(argtypes[0], C._Pointer))

    def dfa_call(self, name, args):
        """One of `DFA_CALLS` with its block (`_lib.SYMBOLS` names it), on the current stream."""
        if name not in HipEngine.DFA_CALLS:
            raise ValueError(name)
        check(getattr(self.lib, name)(C.byref(args), self._stream()))

    # the glb_fsa_* entries (products of automata) that take (argument block, stream)
    FSA_CALLS = frozenset(name for name, (_, argtypes) in _lib.SYMBOLS.items()
                          if name.startswith("glb_fsa_") and argtypes and issubclass(argtypes[0], C._Pointer))

    def fsa_call(self, name, args):
        """One of `FSA_CALLS` with its block, on the current stream."""
        if name not in HipEngine.FSA_CALLS:
            raise ValueError(name)
        check(getattr(self.lib, name)(C.byref(args), self._stream()))

    # the glb_nfa_* entries (determinisation) that take (argument block, stream)
    NFA_CALLS = frozenset(name for name, (_, argtypes) in _lib.SYMBOLS.items()
                          if name.startswith("glb_nfa_") and argtypes and issubclass(argtypes[0], C._Pointer))

    def nfa_call(self, name, args):
        """One of `NFA_CALLS` with its block, on the current stream."""
        if name not in HipEngine.NFA_CALLS:
            raise ValueError(name)
        check(getattr(self.lib, name)(C.byref(args), self._stream()))

    # the glb_lazy_* entries (subsets made while decoding) that take (argument block, stream)
    LAZY_CALLS = frozenset(name for name, (_, argtypes) in _lib.SYMBOLS.items()
                           if name.startswith("glb_lazy_") and argtypes and issubclass(argtypes[0], C._Pointer))

    def lazy_call(self, name, args):
        """One of `LAZY_CALLS` with its block, on the current stream."""
        if name not in HipEngine.LAZY_CALLS:
            raise ValueError(name)
        check(getattr(self.lib, name)(C.byref(args), self._stream()))

    # the glb_pda_* entries (pushdown configurations made while decoding) that take (argument block, stream)
    PDA_CALLS = frozenset(name for name, (_, argtypes) in _lib.SYMBOLS.items()
                          if name.startswith("glb_pda_") and argtypes and issubclass(argtypes[0], C._Pointer))

    def pda_call(self, name, args):
        """One of `PDA_CALLS` with its block, on the current stream."""
        if name not in HipEngine.PDA_CALLS:
            raise ValueError(name)
        check(getattr(self.lib, name)(C.byref(args), self._stream()))

    # the glb_conj_* entries (conjunctions of constraints, tuples of part states numbered while decoding) that
    # take (argument block, stream)
    CONJ_CALLS = frozenset(name for name, (_, argtypes) in _lib.SYMBOLS.items()
                           if name.startswith("glb_conj_") and argtypes and issubclass(argtypes[0], C._Pointer))

    def conj_call(self, name, args):
        """One of `CONJ_CALLS` with its block, on the current stream."""
        if name not in HipEngine.CONJ_CALLS:
            raise ValueError(name)
        check(getattr(self.lib, name)(C.byref(args), self._stream()))

    # ---- device-resident particle state ------------------------------------------------------------------
    def kv_append(self, slab, new_rows, pos, rows=None):
        """slab[rows[i] (or i), h, pos[i], :] = new_rows[i, h, 0, :] (glb_kv_append).  slab [R, H, cap, Dh] contiguous;
        new_rows [n, H, 1, Dh] with unit inner stride (usually a transposed view of the projection output); rows: int32
        [n] slab row of every forward row (shared KV rows), None: row i."""
        R, H, cap, Dh = slab.shape
        n = new_rows.shape[0]
        assert new_rows.shape == (n, H, 1, Dh) and new_rows.stride(3) == 1 and slab.is_contiguous()
        assert rows is not None or n == R
        check(self.lib.glb_kv_append(_ptr(slab), _ptr(new_rows), _ptr(pos), _ptr(rows), n, H, cap, Dh, new_rows.stride(0),
                                     new_rows.stride(1), slab.element_size(), self._stream()))

    def slab_attention(self, query, k_new, v_new, k_slab, v_slab, pos, scale):
        """Attention of a one-token forward over slab rows where they lie, the new token's K / V appended on the way
        (glb_slab_attention).  query [R, H, 1, Dh], k_new / v_new [R, H_kv, 1, Dh] (unit inner stride; usually strided
        views of the projection output), slabs [R, H_kv, cap, Dh] contiguous, pos int32 [R].  Returns [R, 1, H, Dh]."""
        R, H, _, Dh = query.shape
        Hkv, cap = k_slab.shape[1], k_slab.shape[2]
        assert query.stride(3) == 1 and k_new.stride(3) == 1 and v_new.stride(3) == 1 and k_slab.is_contiguous() and v_slab.is_contiguous()
        assert k_new.dtype == v_new.dtype == query.dtype == k_slab.dtype
        out = torch.empty((R, 1, H, Dh), dtype=query.dtype, device=self.device)
        check(self.lib.glb_slab_attention(_ptr(query), query.stride(0), query.stride(1), _ptr(k_new), k_new.stride(0),
                                          k_new.stride(1), _ptr(v_new), v_new.stride(0), v_new.stride(1), _ptr(k_slab),
                                          _ptr(v_slab), _ptr(pos), R, H, Hkv,
                                          cap, Dh, float(scale), _DT[query.dtype], _ptr(out), self._stream()))
        return out

    @staticmethod
    def slab_attention_supports(dtype, head_dim):
        return dtype in _DT and head_dim in (16, 32, 64, 128)

    def short_attention(self, query, key, value, mask, scale):
        """Masked attention of a padded batch of short contexts (glb_short_attention).  query [U, H, Lq, Dh], key / value
        [U, H_kv, Lk, Dh] (unit inner stride), mask: bool [U, 1, Lq, Lk] (true = attend) or None (causal).  Returns
        [U, Lq, H, Dh]."""
        U, H, Lq, Dh = query.shape
        Hkv, Lk = key.shape[1], key.shape[2]
        assert query.stride(3) == 1 and key.stride(3) == 1 and value.stride(3) == 1 and key.dtype == value.dtype == query.dtype
        out = torch.empty((U, Lq, H, Dh), dtype=query.dtype, device=self.device)
        i64x3 = C.c_int64 * 3
        m_ptr, m_sr, m_sq = None, 0, 0
        if mask is not None:
            assert mask.dtype == torch.bool and mask.dim() == 4 and mask.shape[-1] == Lk and mask.stride(3) == 1 and mask.shape[1] == 1
            m_ptr, m_sr, m_sq = _ptr(mask), (mask.stride(0) if mask.shape[0] > 1 else 0), (mask.stride(2) if mask.shape[2] > 1 else 0)
        check(self.lib.glb_short_attention(_ptr(query), i64x3(*query.stride()[:3]), _ptr(key), i64x3(*key.stride()[:3]), _ptr(value),
                                           i64x3(*value.stride()[:3]), m_ptr, m_sr, m_sq, U, H, Hkv, Lq, Lk, Dh, float(scale),
                                           _DT[query.dtype], _ptr(out), self._stream()))
        return out

    def short_attention_packed(self, query, key, value, plan, max_keys, scale, err=None, out=None):
        """Attention of a row-packed batch whose contexts share their prompt's rows (glb_short_attention_packed).  query
        [M, H, Dh], key / value [M, H_kv, Dh] (unit inner stride: views of the projection output), plan int32 [S, 4] on the
        device: (pre_start, pre_len, tail_start, tail_len) per segment, max_keys: the most keys of a segment (<= 32).
        Returns [M, H, Dh] (`out`, contiguous, when given); rows no segment names are left as they were.  A segment the kernel
        refuses (out of range) adds to `err` (int32 [1] device; default: `error_word()`, which `raise_if_failed` reports)."""
        M, H, Dh = query.shape
        Hkv = key.shape[1]
        assert key.shape == value.shape == (M, Hkv, Dh) and key.dtype == value.dtype == query.dtype
        assert query.stride(2) == 1 and key.stride(2) == 1 and value.stride(2) == 1
        assert plan.dtype == torch.int32 and plan.dim() == 2 and plan.shape[1] == 4 and plan.is_contiguous()
        self._check_dev(plan)
        err = self.error_word() if err is None else err
        assert err.dtype == torch.int32 and err.device == self.device
        if out is None:
            out = torch.empty((M, H, Dh), dtype=query.dtype, device=self.device)
        assert out.shape == (M, H, Dh) and out.dtype == query.dtype and out.device == self.device and out.is_contiguous()
        check(self.lib.glb_short_attention_packed(_ptr(query), query.stride(0), query.stride(1), _ptr(key), key.stride(0),
                                                  key.stride(1), _ptr(value), value.stride(0), value.stride(1), _ptr(plan),
                                                  plan.shape[0], M, H, Hkv, int(max_keys), Dh, float(scale),
                                                  _DT[query.dtype], _ptr(out), _ptr(err), self._stream()))
        return out

    def kv_gather_rows(self, srcs, dsts, src_row_of, len_of, srcs_stable=True):
        """dsts[t][i, h, p] = srcs[t][src_row_of[i], h, p] for p < len_of[i], for every tensor pair of the two lists
        (all [rows, heads, cap, head_dim], contiguous) in ONE launch through device pointer tables
        (glb_kv_gather_rows).  src_row_of[i] < 0 leaves row i untouched."""
        s0, d0 = srcs[0], dsts[0]
        assert all(t.is_contiguous() for t in srcs) and all(t.is_contiguous() for t in dsts)
        # (srcs_stable=False: the sources are a one-off - the KV a forward has just returned: their table is not kept)
        sp = self._ptr_table(srcs) if srcs_stable else torch.tensor([t.data_ptr() for t in srcs], dtype=torch.int64, device=self.device)
        dp = self._ptr_table(dsts)
        check(self.lib.glb_kv_gather_rows(_ptr(sp), _ptr(dp), len(srcs), d0.shape[0], d0.shape[1], d0.shape[3],
                                          s0.shape[2], d0.shape[2], _ptr(src_row_of), _ptr(len_of), d0.element_size(),
                                          self._stream()))

    def _ptr_table(self, tensors):
        """Device table of the tensors' addresses.  Slab sets are handed over again and again: the table of a set is made
        once (a host list -> device copy from pageable memory is a synchronous copy - one in every step kept the host from
        running ahead of the GPU).  An entry names its tensors by WEAK references: it never keeps a slab set alive (a set is
        gigabytes at the Llama-3-8B shape, and an engine outlives many DeviceSIS / SlabKV objects), and it is only valid
        while every one of them is the very object it was made for - an address the allocator hands out again after its
        owner died does not pass for the old tensor.  Entries whose tensors are gone leave at the next miss."""
        import weakref

        key = tuple(t.data_ptr() for t in tensors)
        ent = self._ptr_tables.get(key)
        if ent is not None and all(r() is t for r, t in zip(ent[1], tensors)):
            return ent[0]
        dead = [k for k, (_, refs) in self._ptr_tables.items() if any(r() is None for r in refs)]
        for k in dead:
            del self._ptr_tables[k]
        if len(self._ptr_tables) >= 64:
            self._ptr_tables.pop(next(iter(self._ptr_tables)))
        table = torch.tensor(key, dtype=torch.int64, device=self.device)
        self._ptr_tables[key] = (table, [weakref.ref(t) for t in tensors])
        return table

    def gather_rows_i32(self, src, row_of, out=None):
        """out[i] = src[row_of[i]] for an int32 matrix (glb_gather_rows_i32)."""
        n, width = row_of.numel(), src.shape[1]
        if out is None:
            out = torch.empty((n, width), dtype=torch.int32, device=self.device)
        check(self.lib.glb_gather_rows_i32(_ptr(src), src.stride(0), _ptr(row_of), n, width, _ptr(out), out.stride(0),
                                           self._stream()))
        return out

    # ---- KV rows shared between contexts: the block table on the device ------------------------------------------
    def match_rows(self, tokens, starts, lengths, rep, n_groups, row_tok, row_len, row_hash):
        """For every dedup group the table row that holds exactly its context, else the row that holds its first L - 1
        tokens, else -1 (glb_match_rows).  Returns (old_row int32 [n], group_hash int64 [n]); entries past the group
        count are unspecified."""
        n = lengths.numel()
        R, cap = row_tok.shape
        self._check_dev(tokens, starts, lengths, rep, n_groups, row_tok, row_len, row_hash)
        old = self._i32(n)
        gh = torch.empty(n, dtype=torch.int64, device=self.device)
        check(self.lib.glb_match_rows(_ptr(tokens), _ptr(starts), _ptr(lengths), _ptr(rep), _ptr(n_groups), n, _ptr(row_tok),
                                      _ptr(row_len), _ptr(row_hash), R, cap, _ptr(old), _ptr(gh), self._stream()))
        return old, gh

    def kv_plan(self, group_of, rep, n_groups, old_row, lengths, n_rows, cap, by_context=False, stamps=None, call_no=0,
                table=None, old_keep=None):
        """The block table of one step (glb_kv_plan).  `old_row`: the row every group's prefix sits in (match_rows'
        output), or with `by_context` every CONTEXT's row (the previous plan's `row_of_context`).  `stamps`: int64
        [n_rows], free rows are handed out longest unused first (and stamped `call_no`).  `table`: (row_tok, row_len,
        row_hash, group_hash, tokens, starts) - the rows' contents, rewritten for every group that holds a row.
        Returns a dict of int32 device tensors (include/glb.h names without the out_ prefix); `head` (8 words) is all
        the host has to read.  `old_keep`: see `kv_plan_chunk`."""
        n = group_of.numel()
        self._check_dev(group_of, rep, n_groups, old_row, lengths, stamps, old_keep)
        chunk = old_keep is not None
        buf = torch.empty(9 * n + 5 * n_rows + 10 if chunk else 8 * n + 4 * n_rows + 8, dtype=torch.int32, device=self.device)
        names_n = ("group_row", "logits_row", "rows_a", "ctx_a", "pos_a", "ctx_b", "rows_b", "row_of_context")
        names_r = ("copy_src", "copy_len", "ctx_of_row", "pos_of_row")
        out, o = {}, 0
        if chunk:
            out["n_new_a"], out["n_new_of_row"], o = buf[:n], buf[n:n + n_rows], n + n_rows
        for k in names_n:
            out[k] = buf[o:o + n]
            o += n
        for k in names_r:
            out[k] = buf[o:o + n_rows]
            o += n_rows
        out["head"] = buf[o:o + (10 if chunk else 8)]
        need = self.lib.glb_kv_plan_workspace(n, n_rows)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=self.device)
        if chunk:
            c = KvPlanChunkArgs()
            c.struct_size = C.sizeof(KvPlanChunkArgs)
            c.old_keep, c.out_n_new_a, c.out_n_new_of_row = old_keep.data_ptr(), out["n_new_a"].data_ptr(), out["n_new_of_row"].data_ptr()
            a = c.plan
        else:
            a = KvPlanArgs()
        a.struct_size = C.sizeof(KvPlanArgs)
        a.n, a.n_rows, a.cap = n, n_rows, cap
        a.group_of, a.rep, a.n_groups = group_of.data_ptr(), rep.data_ptr(), n_groups.data_ptr()
        a.old_row, a.old_row_by_context = old_row.data_ptr(), 1 if by_context else 0
        a.lengths = lengths.data_ptr()
        a.row_stamps = None if stamps is None else stamps.data_ptr()
        a.call_no = int(call_no)
        if table is not None:
            row_tok, row_len, row_hash, group_hash, tokens, starts = table
            self._check_dev(row_tok, row_len, row_hash, group_hash, tokens, starts)
            a.row_tok, a.row_len, a.row_hash = row_tok.data_ptr(), row_len.data_ptr(), row_hash.data_ptr()
            a.group_hash, a.tokens, a.starts = group_hash.data_ptr(), tokens.data_ptr(), starts.data_ptr()
        for k in names_n + names_r + ("head",):
            setattr(a, "out_" + k, out[k].data_ptr())
        a.workspace, a.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        if chunk:
            check(self.lib.glb_kv_plan_chunk(C.byref(c), self._stream()))
        else:
            check(self.lib.glb_kv_plan(C.byref(a), self._stream()))
        return out

    def match_prefix_rows(self, tokens, starts, lengths, rep, n_groups, row_tok, row_len, row_hash, max_new):
        """For every dedup group the table row that shares the longest prefix with its context - `keep` tokens, at most
        L - 1, with the L - keep tokens behind them no more than `max_new` - else -1 (glb_match_prefix_rows; ties: a row that
        holds exactly the context, then the smallest row).  Returns (old_row int32 [n], keep int32 [n], group_hash int64
        [n]); entries past the group count are unspecified."""
        n = lengths.numel()
        R, cap = row_tok.shape
        self._check_dev(tokens, starts, lengths, rep, n_groups, row_tok, row_len, row_hash)
        old, keep = self._i32(n), self._i32(n)
        gh = torch.empty(n, dtype=torch.int64, device=self.device)
        check(self.lib.glb_match_prefix_rows(_ptr(tokens), _ptr(starts), _ptr(lengths), _ptr(rep), _ptr(n_groups), n,
                                             _ptr(row_tok), _ptr(row_len), _ptr(row_hash), R, cap, int(max_new), _ptr(old),
                                             _ptr(keep), _ptr(gh), self._stream()))
        return old, keep, gh

    def kv_plan_chunk(self, group_of, rep, n_groups, old_row, old_keep, lengths, n_rows, cap, stamps=None, call_no=0,
                      table=None):
        """The block table of one step whose rows with a prefix are fed the tokens keep .. L - 1 (glb_kv_plan_chunk):
        `kv_plan` with `old_keep` (match_prefix_rows' output) and the row table, which is required.  The dict has
        `kv_plan`'s entries - `pos_a` / `pos_of_row`: the first new position; forward rows: one-token rows, chunk rows,
        rows to encode - plus `n_new_a` [n], `n_new_of_row` [n_rows]; `head` has ten words (8: chunk rows, 9: the largest
        number of tokens fed to a row)."""
        if table is None:
            raise ValueError("kv_plan_chunk needs the row table: the rows' lengths decide who keeps a row in place")
        return self.kv_plan(group_of, rep, n_groups, old_row, lengths, n_rows, cap, stamps=stamps, call_no=call_no,
                            table=table, old_keep=old_keep)

    def slab_attention_chunk(self, query, k_new, v_new, k_slab, v_slab, pos, n_new, scale, rows=None):
        """Attention of a forward with up to 16 new tokens per row over slab rows where they lie, the new K / V appended on
        the way (glb_slab_attention_chunk).  query [n, H, T, Dh], k_new / v_new [n, H_kv, T, Dh] (unit inner stride), slabs
        [R, H_kv, cap, Dh] contiguous, pos / n_new int32 [n]: first new position and number of new tokens of every row,
        rows: int32 [n] slab row of forward row i (None: i).  Returns [n, T, H, Dh]; queries t >= n_new[i] give zeros."""
        n, H, T, Dh = query.shape
        R, Hkv, cap = k_slab.shape[0], k_slab.shape[1], k_slab.shape[2]
        assert query.stride(3) == 1 and k_new.stride(3) == 1 and v_new.stride(3) == 1 and k_slab.is_contiguous() and v_slab.is_contiguous()
        assert k_new.dtype == v_new.dtype == query.dtype == k_slab.dtype == v_slab.dtype
        assert k_new.shape == v_new.shape == (n, Hkv, T, Dh) and (rows is not None or n == R)
        out = torch.empty((n, T, H, Dh), dtype=query.dtype, device=self.device)
        i64x3 = C.c_int64 * 3
        check(self.lib.glb_slab_attention_chunk(_ptr(query), i64x3(*query.stride()[:3]), _ptr(k_new), i64x3(*k_new.stride()[:3]),
                                                _ptr(v_new), i64x3(*v_new.stride()[:3]), _ptr(k_slab), _ptr(v_slab), _ptr(pos),
                                                _ptr(n_new), _ptr(rows), n, R, H, Hkv, cap, Dh, T, float(scale), _DT[query.dtype],
                                                _ptr(out), self._stream()))
        return out

    @staticmethod
    def slab_attention_chunk_supports(dtype, head_dim):
        return dtype in _DT and head_dim in (16, 32, 64, 128)

    def resample_systematic(self, log_weights, seed, offset):
        """Ancestors of a systematic resampling step over `log_weights` (the gathered population), int32 [n]
        (glb_resample_systematic); also returns logsumexp of the weights as a 1-element tensor."""
        n = log_weights.numel()
        need = self.lib.glb_resample_workspace(n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=self.device)
        anc, stats = self._i32(n), self._f32(1)
        check(self.lib.glb_resample_systematic(_ptr(log_weights), n, seed, offset, _ptr(anc), _ptr(stats),
                                               _ptr(self._ws), self._ws.numel(), self._stream()))
        return anc, stats

    # ---- token -> byte trie masses ---------------------------------------------------------------------------
    def trie_masses(self, ws, flat, op=0, from_logprobs=False, lse=None, logit_scale=1.0, nodes=None, layout="rows"):
        """Token -> byte trie masses (glb_trie_masses).  ws: [B, >=V] rows of any supported element type - weights, or
        with from_logprobs log-probabilities, or with from_logprobs AND lse (float32 [B], the fused step's out_lse) raw
        LOGITS: the leaf weight is exp(x * logit_scale - lse[r]), no log-prob matrix in between.  Result:
          layout "rows"   float32 [B, n_nodes]                       (every node, row-major)
          nodes given     float32 [B, len(nodes)]                    (only the nodes asked for: int32 device tensor)
          layout "nodes"  float32 [n_nodes, pitch] view of the engine's scratch, pitch = B rounded up to 64: value of
                          node n for row r at [n, r]; valid until the next trie call (nothing is transposed back)."""
        if ws.dim() != 2 or ws.stride(1) != 1 or ws.dtype not in _DT:
            raise ValueError("weights must be [B, V] float32 / bfloat16 / float16 with unit inner stride")
        B = ws.shape[0]
        V, n_nodes = flat["vocab"], flat["n_nodes"]
        self._check_dev(lse, nodes)
        a = TrieArgs()
        a.struct_size = C.sizeof(TrieArgs)
        a.weights, a.dtype = ws.data_ptr(), _DT[ws.dtype]
        a.ld = ws.stride(0) if B > 1 else max(V, ws.stride(0))
        a.n_rows, a.vocab = B, V
        a.lse = None if lse is None else lse.data_ptr()
        a.logit_scale, a.from_logprobs, a.op = logit_scale, 1 if from_logprobs else 0, op
        a.n_nodes, a.n_levels = n_nodes, flat["n_levels"]
        ls = flat["level_start_host"]  # contiguous int32 NumPy array: it sizes the per-level launches
        a.leaf_node, a.level_start_host = flat["leaf_node"].data_ptr(), ls.ctypes.data
        a.level_nodes, a.child_ptr, a.child_idx = (flat[k].data_ptr() for k in ("level_nodes", "child_ptr", "child_idx"))
        need = self.lib.glb_trie_workspace_ex(B, n_nodes)
        if self._trie_ws is None or self._trie_ws.numel() < need:
            self._trie_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        a.workspace, a.workspace_bytes = self._trie_ws.data_ptr(), self._trie_ws.numel()
        out = None
        if nodes is not None:
            if nodes.dtype != torch.int32:
                raise TypeError("nodes must be int32")
            out = torch.empty((B, nodes.numel()), dtype=torch.float32, device=self.device)
            a.sel_nodes, a.n_sel, a.out_sel, a.out_sel_ld = nodes.data_ptr(), nodes.numel(), out.data_ptr(), out.stride(0)
        elif layout == "nodes":
            a.keep_node_major = 1
        elif layout == "rows":
            out = torch.empty((B, n_nodes), dtype=torch.float32, device=self.device)
            a.out, a.out_ld = out.data_ptr(), out.stride(0)
        else:
            raise ValueError(f"unknown layout {layout!r}")
        check(self.lib.glb_trie_masses(C.byref(a), self._stream()))
        if out is not None:
            return out
        pitch = (B + 63) // 64 * 64
        return self._trie_ws[: n_nodes * pitch * 4].view(torch.float32).view(n_nodes, pitch)

    def trie_rows(self, ws, plan, op=0, from_logprobs=False, lse=None, logit_scale=1.0, nodes=None, layout="rows", out=None,
                  out_slots=None):
        """Token -> byte trie masses with one row of a part of the trie resident in LDS (glb_trie_rows): the weights are
        read once, the result written once, row-major.  plan: `TokenByteTrie.plan_device_arrays()`.  ws as in
        `trie_masses`.  Result: layout "rows" float32 [B, n_nodes]; nodes given (int32 device tensor) [B, len(nodes)] - or,
        `nodes` int32 [B, K], every row's OWN nodes (negative: none, 0 out): only the parts of the trie that hold a row's
        nodes are read and reduced for that row;
        layout "slots" [B, n_slots] in the plan's slot numbering (plan["slot_of"]: node -> slot).  out_slots: float32
        [B, n_slots] to be filled with the slots IN ADDITION to the requested output (one call, the C entry point's several
        outputs at once)."""
        if ws.dim() != 2 or ws.stride(1) != 1 or ws.dtype not in _DT:
            raise ValueError("weights must be [B, V] float32 / bfloat16 / float16 with unit inner stride")
        B = ws.shape[0]
        V = plan["vocab"]
        self._check_dev(lse, nodes, out)
        pl = plan.get("_c")
        if pl is None:
            pl = TriePlan()
            pl.struct_size = C.sizeof(TriePlan)
            for k in ("n_parts", "n_top", "n_cut", "n_slots", "max_local", "top_base", "lds_bytes", "n_nodes"):
                setattr(pl, k, int(plan[k]))
            for k in ("desc", "idepth", "leaf_src", "leaf_local", "run_tab", "top_local", "slot_of", "cptr16", "inode16", "pn_local16"):
                setattr(pl, k, plan[k].data_ptr())
            if plan.get("sweep"):  # (the kernel that reads a row front to back: TokenByteTrie.plan(sweep=True))
                pl.tok_local16, pl.inode64 = plan["tok_local16"].data_ptr(), plan["inode64"].data_ptr()
                pl.lds_top_bytes, pl.vocab = int(plan["lds_top_bytes"]), int(plan["vocab"])
            plan["_c"] = pl
        a = TrieRowsArgs()
        a.struct_size = C.sizeof(TrieRowsArgs)
        a.weights, a.dtype = ws.data_ptr(), _DT[ws.dtype]
        a.ld = ws.stride(0) if B > 1 else max(V, ws.stride(0))
        a.n_rows, a.vocab = B, V
        a.lse = None if lse is None else lse.data_ptr()
        a.logit_scale, a.from_logprobs, a.op = logit_scale, 1 if from_logprobs else 0, op
        need = self.lib.glb_trie_rows_workspace(B, C.byref(pl))
        if need:
            if self._trie_ws is None or self._trie_ws.numel() < need:
                self._trie_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            a.workspace, a.workspace_bytes = self._trie_ws.data_ptr(), self._trie_ws.numel()
        per_row = nodes is not None and nodes.dim() == 2
        if nodes is not None:
            if nodes.dtype != torch.int32:
                raise TypeError("nodes must be int32")
            if per_row and (nodes.shape[0] != B or nodes.stride(1) != 1):
                raise ValueError(f"per-row nodes must be int32 [{B}, K] with unit inner stride")
            width = nodes.shape[1] if per_row else nodes.numel()
        elif layout == "rows":
            width = plan["n_nodes"]
        elif layout == "slots":
            width = plan["n_slots"]
        else:
            raise ValueError(f"unknown layout {layout!r}")
        if out is None:
            out = torch.empty((B, width), dtype=torch.float32, device=self.device)
        elif out.shape != (B, width) or out.dtype != torch.float32 or out.stride(1) != 1:
            raise ValueError(f"out must be float32 [{B}, {width}] with unit inner stride")
        if width == 0 or B == 0:
            return out
        if nodes is not None:
            a.sel_nodes, a.n_sel, a.out_sel, a.out_sel_ld = nodes.data_ptr(), width, out.data_ptr(), out.stride(0)
            a.sel_row_stride = max(nodes.stride(0), width) if per_row else 0
        elif layout == "rows":
            a.out_nodes, a.out_nodes_ld = out.data_ptr(), out.stride(0)
        else:
            a.out_slots, a.out_slots_ld = out.data_ptr(), out.stride(0)
        if out_slots is not None:
            if out_slots.shape != (B, plan["n_slots"]) or out_slots.dtype != torch.float32 or out_slots.stride(1) != 1:
                raise ValueError(f"out_slots must be float32 [{B}, {plan['n_slots']}] with unit inner stride")
            self._check_dev(out_slots)
            a.out_slots, a.out_slots_ld = out_slots.data_ptr(), out_slots.stride(0)
        check(self.lib.glb_trie_rows(C.byref(a), C.byref(pl), self._stream()))
        return out

    def trie_reduce(self, ws, flat, op=0, from_logprobs=False, out=None):
        """out[r, node] = sum / max of the weights of the tokens below `node` (glb_trie_reduce).  ws: float32 [B, >=V]
        device rows; flat: the trie's arrays (trie.TokenByteTrie.device_arrays: device tensors + the host level table)."""
        if ws.dim() != 2 or ws.stride(1) != 1 or ws.dtype != torch.float32:
            raise ValueError("weights must be float32 [B, V] with unit inner stride")
        B = ws.shape[0]
        V, n_nodes = flat["vocab"], flat["n_nodes"]
        if out is None:
            out = torch.empty((B, n_nodes), dtype=torch.float32, device=self.device)
        ls = flat["level_start_host"]  # contiguous int32 NumPy array: it sizes the per-level launches
        need = self.lib.glb_trie_workspace(B, n_nodes)  # node-major scratch for batches of 32 rows and more
        if need and (self._trie_ws is None or self._trie_ws.numel() < need):
            self._trie_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        check(self.lib.glb_trie_reduce(_ptr(ws), ws.stride(0) if B > 1 else max(V, ws.stride(0)), B, V, n_nodes,
                                       flat["n_levels"], _ptr(flat["leaf_node"]), C.c_void_p(ls.ctypes.data),
                                       _ptr(flat["level_nodes"]), _ptr(flat["child_ptr"]), _ptr(flat["child_idx"]), op,
                                       1 if from_logprobs else 0, _ptr(out), out.stride(0),
                                       _ptr(self._trie_ws) if need else None, need, self._stream()))
        return out
