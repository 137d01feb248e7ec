"""Shared pieces of the tests of the autoregressive decode step (tests/test_t5_decode_embed_cpu.py,
tests/test_gpu_t5_decode_embed.py, tests/test_gpu_t5_decode_live.py, tests/test_gpu_t5_rollout_graph.py):
trlx_t5_decode_embed and trlx_t5_decode_attn_live of include/trlx_t5_amd.h.

  bits, same        raw-bit equality: every GPU comparison built on these is exact
  with_margins      a guard-filled tensor inside a larger guard-filled allocation, so that a missing
                    guard in a kernel stays inside the test's own memory
  hf_layer_norm     HF's T5LayerNorm.forward restated in torch
  embed_reference   the decoder's input row of step t as torch expressions

Test infrastructure only."""
import torch
import torch.nn.functional as F

GUARD = -77.0
MARGIN = 4
ERR_SHAPE, ERR_STRIDE, ERR_DTYPE, ERR_ARG = 1, 2, 3, 5


def name(dt):
    return {torch.bfloat16: "bf16", torch.float32: "fp32"}[dt]


def bits(x):
    x = x.detach().contiguous()
    if x.dtype == torch.bfloat16:
        x = x.view(torch.int16)
    elif x.dtype == torch.float32:
        x = x.view(torch.int32)
    return x.cpu()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def with_margins(shape, dtype, device, row, ld=None, fill=GUARD):
    """A `fill`-ed [rows, cols] (or [n]) view inside a larger `fill`-ed allocation: MARGIN rows of
    `row` elements before and after; ld: the row stride of a 2-D view.  Returns (whole, view)."""
    if len(shape) == 1:
        n = shape[0]
        whole = torch.full((n + 2 * MARGIN * row,), fill, dtype=dtype, device=device)
        return whole, whole[MARGIN * row:MARGIN * row + n]
    rows, cols = shape
    ld = cols if ld is None else ld
    whole = torch.full((rows * ld + 2 * MARGIN * row,), fill, dtype=dtype, device=device)
    return whole, whole[MARGIN * row:MARGIN * row + rows * ld].view(rows, ld)[:, :cols]


def hf_layer_norm(h, weight, eps=1e-6):
    """transformers' T5LayerNorm.forward."""
    variance = h.to(torch.float32).pow(2).mean(-1, keepdim=True)
    h = h * torch.rsqrt(variance + eps)
    if weight.dtype in (torch.float16, torch.bfloat16):
        h = h.to(weight.dtype)
    return weight * h


def embed_reference(weight, tokens, t, start):
    """h of step t: weight[start] in every row at t == 0, else weight[tokens[:, t - 1]]; an id outside
    [0, V) gives a zero row."""
    B, V = tokens.shape[0], weight.shape[0]
    tok = torch.full((B,), start, dtype=torch.int64, device=tokens.device) if t == 0 else tokens[:, t - 1]
    ok = (tok >= 0) & (tok < V)
    h = F.embedding(tok.clamp(0, V - 1), weight)
    return torch.where(ok[:, None], h, torch.zeros_like(h))
