"""Shared pieces of the tests of the fp8 encoder keys / values (tests/test_t5_cross_kv8_cpu.py,
tests/test_gpu_t5_cross_kv8.py): trlx_t5_cross_kv_quantize and trlx_t5_decode_attn_kv8 of
include/trlx_t5_amd.h.

  ref_quantize     the quantiser written from its definition, one (b, h) block at a time in Python
                   floats: amax over the live keys, frexp, the exponent rule, the clamp, then
                   torch's cast of the exactly scaled values.  The package's CPU fallback is
                   checked against it on the CPU; the kernel is checked against the fallback.
  EDGES            the scale rule at its edges: (name, amax, expected e)
  TIES             inputs whose scaled value sits on a tie or in the subnormals, with scale == 1
  special_case     one K / V / mask holding the ties, an all-zero head, both clamps, a fully masked
                   batch row
  layouts          the input layouts the quantiser reads in place

The attention cases are cross_case of tests/t5_decode_attn_checks.py, quantised; its float64 oracle
and eager route are used as they stand.  Test infrastructure only."""
import math

import torch

import t5_decode_attn_checks as A

B, NH = A.B, A.NH
D_KVS = (64, 128)
QUANT_S = A.CROSS_S          # (1, 9, 33, 200): 33 and 9 are no multiple of the 32 / 16 rows of one pass
E_MIN, E_MAX = -100, 119

# (name, amax, e): e is the smallest integer with amax * 2^-e <= 448, clamped to [E_MIN, E_MAX]
EDGES = (
    ("448", 448.0, 0),
    ("448*2^-3", 56.0, -3),
    ("448*2^5", 14336.0, 5),
    ("m=0.875 exactly, x=1", 1.75, -8),
    ("m just above 0.875", (1 + 97 / 128) * 1.0, -7),          # 1.7578125 * 2^8 = 450 > 448
    ("m just below 0.875", (1 + 95 / 128) * 1.0, -8),
    ("one", 1.0, -8),
    ("zero", 0.0, 0),
    ("tiny: the lower clamp", 2.0 ** -120, -100),
    ("at the lower clamp", 1.75 * 2.0 ** -92, -100),
    ("huge: the upper clamp", float(torch.finfo(torch.bfloat16).max), 119),
    ("at the upper clamp", 1.75 * 2.0 ** 127, 119),
)

# scale == 1 (amax 448): value -> what e4m3fn keeps (ties to even, subnormal spacing 2^-9)
TIES = ((17.0, 16.0), (19.0, 20.0), (21.0, 20.0), (23.0, 24.0), (432.0, 448.0),
        (2.0 ** -10, 0.0), (1.5 * 2.0 ** -9, 2.0 ** -8), (2.5 * 2.0 ** -9, 2.0 ** -8))


def exponent(amax):
    """The rule of the header, in Python floats."""
    if amax == 0.0:
        return 0
    m, x = math.frexp(amax)
    return max(E_MIN, min(E_MAX, x - 9 if m <= 0.875 else x - 8))


def ref_quantize(x, mask=None):
    """x: bf16 [B, nH, S, d] on the CPU, mask: int64 [B, S] or None -> (uint8 bytes, fp32 scales).
    A block with a live non-finite element: NaN scale, 0x7f in its live bytes."""
    Bx, nH, S, d = x.shape
    out = torch.zeros(Bx, nH, S, d, dtype=torch.uint8)
    scale = torch.empty(Bx, nH, dtype=torch.float32)
    for b in range(Bx):
        rows = torch.arange(S) if mask is None else torch.nonzero(mask[b] != 0).flatten()
        for h in range(nH):
            blk = x[b, h, rows].float()
            amax = float(blk.abs().max()) if len(rows) else 0.0
            if not math.isfinite(amax):
                scale[b, h] = float("nan")
                out[b, h, rows] = 0x7f
                continue
            e = exponent(amax)
            scale[b, h] = 2.0 ** e
            out[b, h, rows] = (blk * 2.0 ** -e).to(torch.float8_e4m3fn).view(torch.uint8)
    return out, scale


def same_scales(a, b):
    """fp32 equality of the raw bits (a NaN scale equals a NaN scale)."""
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def quantised_equal(got, k8, k_scale, v8, v_scale):
    return (torch.equal(got.k8.view(torch.uint8).cpu(), k8) and torch.equal(got.v8.view(torch.uint8).cpu(), v8)
            and same_scales(got.k_scale, k_scale) and same_scales(got.v_scale, v_scale))


def layouts(x):
    """name -> (tensor to pass, n_heads argument) for x = contiguous [B, nH, S, d]: the tensor itself,
    the projection output [B, S, nH*d] and HF's transposed view of it."""
    Bx, nH, S, d = x.shape
    proj = x.permute(0, 2, 1, 3).contiguous().reshape(Bx, S, nH * d)
    return {"bhsd": (x, None), "bsd": (proj, nH), "hf_view": (proj.view(Bx, S, nH, d).transpose(1, 2), None)}


def special_case(d, S=40):
    """K, V bf16 [B, NH, S, d] and an int64 mask [B, S].  Heads of K: 0 ties (amax 448, scale 1),
    1 all zero, 2 at the upper clamp, 3 at the lower clamp, 4 random.  V holds the same heads rotated by
    one.  Batch row 1 is fully masked and poisoned; row 2 has holes, its masked rows poisoned."""
    g = torch.Generator().manual_seed(9100 + d)
    K = torch.randn(B, NH, S, d, generator=g)
    vals = [v for v, _ in TIES]
    K[:, 0] = 0.0
    K[:, 0, :, :len(vals)] = torch.tensor(vals)
    K[:, 0, 1::2] *= -1.0                                   # both signs
    K[:, 0, 0, d - 1] = 448.0
    K[:, 0, S - 1, d - 1] = 448.0
    K[:, 1] = 0.0
    K[:, 2] = K[:, 2] * 2.0 ** 125
    K[:, 2, S // 2, 3] = float(torch.finfo(torch.bfloat16).max)
    K[:, 3] = K[:, 3] * 2.0 ** -125
    K = K.to(torch.bfloat16)
    V = torch.roll(K, 1, dims=1).contiguous()
    mask = torch.ones(B, S, dtype=torch.int64)
    mask[1] = 0
    mask[2, 1:S - 1:3] = 0
    return dict(K=A.poison(K, mask), V=A.poison(V, mask), mask=mask)
