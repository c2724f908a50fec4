"""HipEngine.lora_rows_table / lora_rows (include/glb.h glb_lora_rows) restated with torch on the CPU, on top of
the merge double of tests/lora_engine.py.  TEST INFRASTRUCTURE: lives under tests/, is never imported by the product.

    slot < 0 or no entry for the module: the row is not written
    else y[m] = round_to_y_dtype(y[m] + scale * (x[m] A^T) B^T)       (float64 here: the CPU tests compare within 1e-4)
"""
import torch

from tests.lora_engine import LoraOracleEngine


class _Table:
    def __init__(self, slots):
        self.slots = slots
        self.n_slots, self.n_modules = len(slots), len(slots[0])
        self.r_max = max([j["a"].shape[0] for row in slots for j in row if j is not None] + [1])


class LoraRowsOracleEngine(LoraOracleEngine):
    rows_calls = 0

    def lora_rows_table(self, slots):
        if not slots or any(len(row) != len(slots[0]) for row in slots):
            raise ValueError("lora_rows_table: every slot lists every module")
        return _Table(slots)

    def lora_rows(self, x, y, row_slot, table, module_index):
        if x.dtype != y.dtype:
            raise ValueError("lora_rows: x and y must share a dtype")
        k, n = x.shape[-1], y.shape[-1]
        x2 = x.reshape(-1, k)
        m = x2.shape[0]
        if y.numel() != m * n or row_slot.dtype != torch.int32 or row_slot.numel() != m:
            raise ValueError("lora_rows: rows of x, y and row_slot differ")
        if y.dim() > 1:
            lead = y.shape[:-1]
            y2 = y.as_strided((m, n), (y.stride(-2), 1)) if all(
                s == 1 or y.stride(d) == y.stride(-2) * int(torch.tensor(lead[d + 1:]).prod()) for d, s in enumerate(lead)
            ) else None
            if y2 is None:
                raise ValueError("lora_rows: y is not a matrix of rows with one pitch")
        else:
            y2 = y.view(1, n)
        for s in range(table.n_slots):
            ent = table.slots[s][module_index]
            rows = (row_slot == s).nonzero().flatten()
            if ent is None or rows.numel() == 0:
                continue
            a, b = ent["a"].double(), ent["b"].double()
            if tuple(a.shape) != (a.shape[0], k) or tuple(b.shape) != (n, a.shape[0]):
                continue
            delta = float(ent["scale"]) * ((x2[rows].double() @ a.T) @ b.T)
            y2[rows] = (y2[rows].double() + delta).to(y.dtype)
        self.rows_calls += 1
        return y
