"""Restatement of the 4-bit block format (include/glb.h glb_w4_quantize / glb_w4_dequantize) in numpy, on
LOGICAL codes and absmax: nothing here knows the order inside the library's packed image.  TEST INFRASTRUCTURE: lives under
tests/, is never imported by the product package.

  quantise:   blocks of 64 along k; absmax = max |w| (float32); sort the codebook, m_i = (c_i + c_{i+1}) * 0.5f; the code of
              w is the sorted entry whose index is the number of float32 products m_i * absmax strictly below w
  dequantise: w' = codebook[code] * absmax in float32, then one round-to-nearest-even to the output dtype
"""
import numpy as np
import torch

BLOCK = 64

NF4 = np.array([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635,
                -0.18477343022823334, -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725,
                0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0],
               dtype=np.float64)
_FP4_HALF = (np.array([0, 0.0625, 8, 12, 4, 6, 2, 3], dtype=np.float32) / np.float32(12)).astype(np.float32)
FP4 = np.concatenate([_FP4_HALF, -_FP4_HALF]).astype(np.float64)
TABLES = {"nf4": NF4, "fp4": FP4}


def codebook(name):
    """The table as float32 (every NF4 entry above is exactly a float32; test_quant4_cpu checks it)."""
    return TABLES[name].astype(np.float32)


def sorted_table(cb):
    """(sorted entries, their codes, the 15 float32 midpoints); ties keep the lower code first (+0 before -0 in FP4)."""
    cb = np.asarray(cb, np.float32)
    order = np.argsort(cb, kind="stable")
    srt = cb[order]
    mid = ((srt[:-1] + srt[1:]).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    return srt, order.astype(np.uint8), mid


def quantize(w, cb):
    """w: float32 array [n, k], k % 64 == 0 -> (codes uint8 [n, k], absmax float32 [n, k / 64])."""
    w = np.ascontiguousarray(w, np.float32)
    n, k = w.shape
    assert k % BLOCK == 0
    _, code_of, mid = sorted_table(cb)
    codes, absmax = np.empty((n, k), np.uint8), np.empty((n, k // BLOCK), np.float32)
    for r0 in range(0, n, 256):  # (row chunks: the comparison below is 15 times the chunk)
        blocks = w[r0:r0 + 256].reshape(-1, k // BLOCK, BLOCK)
        amax = np.abs(blocks).max(-1).astype(np.float32)
        with np.errstate(over="ignore", under="ignore"):
            prod = (mid[None, None, None, :] * amax[:, :, None, None]).astype(np.float32)  # one float32 product each
        cnt = (prod < blocks[..., None]).sum(-1)
        codes[r0:r0 + 256] = code_of[cnt].reshape(-1, k)
        absmax[r0:r0 + 256] = amax
    return codes, absmax


def dequantize_f32(codes, absmax, cb):
    """codebook[code] * absmax: one float32 multiplication."""
    cb = np.asarray(cb, np.float32)
    n, k = codes.shape
    vals = cb[codes].reshape(n, k // BLOCK, BLOCK)
    with np.errstate(under="ignore"):
        return (vals * absmax[:, :, None]).astype(np.float32).reshape(n, k)


def dequantize(codes, absmax, cb, dtype=torch.float32):
    """The dequantised weight as a torch tensor of `dtype` (torch rounds float32 -> bf16 / f16 to nearest even)."""
    return torch.from_numpy(dequantize_f32(codes, absmax, cb)).to(dtype)


def roundtrip(w, cb, dtype=torch.float32):
    """dequantize(quantize(w)) for a torch tensor w [n, k] of any served dtype (widening to float32 is exact)."""
    codes, absmax = quantize(w.detach().float().cpu().numpy(), cb)
    return dequantize(codes, absmax, cb, dtype)


class StubW4Engine:
    """The w4_* part of HipEngine on the CPU, by the restatement above (the image: codes two per byte in row-major order,
    then absmax).  Mixed into a CPU engine double for the host-logic tests; w4_gemm always answers "not served"."""

    device = torch.device("cpu")

    def w4_bytes(self, n, k):
        return n * k // 2 + 4 * (n * k // BLOCK) if n > 0 and k > 0 and k % BLOCK == 0 else 0

    def w4_gemm_max_rows(self):
        return 0

    def w4_quantize(self, w, cb, transposed=False, out=None):
        w = w.detach().float().cpu()
        w = w.T if transposed else w
        n, k = w.shape
        if self.w4_bytes(n, k) == 0:
            return None
        codes, absmax = quantize(w.numpy(), np.asarray(cb, np.float32))
        packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
        img = np.concatenate([packed.reshape(-1), absmax.reshape(-1).view(np.uint8)])
        assert img.size == self.w4_bytes(n, k)
        return torch.from_numpy(img.copy())

    def w4_dequantize(self, image, n, k, cb, dtype=torch.float32, transposed=False, out=None):
        img = image.numpy()
        packed = img[:n * k // 2].reshape(n, k // 2)
        codes = np.empty((n, k), np.uint8)
        codes[:, 0::2], codes[:, 1::2] = packed & 15, packed >> 4
        absmax = img[n * k // 2:].view(np.float32).reshape(n, k // BLOCK)
        w = dequantize(codes, absmax, np.asarray(cb, np.float32), dtype if out is None else out.dtype)
        w = w.T if transposed else w
        if out is None:
            return w.contiguous()
        out.copy_(w)
        return out

    def w4_gemm(self, x, image, n, cb, bias=None, out=None):
        return None
