"""Multi-head self-attention over the T tokens of a cloud at head_dim 64: the core of PointViT's `Attention`
(openpoints/models/layers/attention.py:28-35).

`token_attention(qkv, heads)` takes the packed (B, T, 3*heads*64) tensor exactly as `nn.Linear(dim, 3*dim)` leaves it
(last axis [3][heads][64], the reference's `reshape(B, N, 3, H, C // H)`) and returns (B, T, heads*64) in the layout
`proj` consumes; the backward writes the packed gradient.  Any T >= 1; no (B,H,T,T) tensor, no permute, no cat
(csrc/token_attention.hip).  The autograd Function saves qkv, out and lse (B,H,T) -- nothing T x T.
"""
import torch

from . import _lib
from .fused import _call

HEAD_DIM = 64
MAX_GRID = 65535           # clouds and heads are grid dimensions z / y of every kernel (tok_check)
MAX_TOKENS = 1 << 24       # apn_token_attention_max_tokens()
MAX_ROWS = 16 * (2 ** 31 - 1)

# calls that ran the composition instead of the kernel, by reason
COMPOSED_CALLS = {}


def _why_composed(qkv, heads):
    """None if the kernel takes the call, else the reason it does not."""
    if not qkv.is_cuda:
        return "cpu tensor"
    if heads <= 0 or qkv.dim() != 3:
        return "heads %d, %d-d input" % (heads, qkv.dim())
    if qkv.shape[-1] != 3 * heads * HEAD_DIM:
        return "head dim %s" % (qkv.shape[-1] / (3.0 * heads))
    if qkv.dtype != torch.float32:
        return "dtype %s" % qkv.dtype
    B, T, _ = qkv.shape
    if not (0 < B <= MAX_GRID and heads <= MAX_GRID):
        return "batch %d / heads %d outside 1..%d" % (B, heads, MAX_GRID)
    if not (0 < T <= MAX_TOKENS and B * T * heads < MAX_ROWS):
        return "T=%d outside the grid bounds" % T
    return None


def supported(qkv, heads):
    return _why_composed(qkv, heads) is None


def composed(qkv, heads, attn_drop=None):
    """The reference's lines (attention.py:28-35) between `qkv` and `proj`: materialises (B,H,T,T) twice."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    qkv = qkv.reshape(B, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    attn = (q @ k.transpose(-2, -1)) * (C // heads) ** -0.5
    attn = attn.softmax(dim=-1)
    if attn_drop is not None:
        attn = attn_drop(attn)
    return (attn @ v).transpose(1, 2).reshape(B, N, C)


def fallback(qkv, heads, why, attn_drop=None):
    """The composition, counted under `why`."""
    COMPOSED_CALLS[why] = COMPOSED_CALLS.get(why, 0) + 1
    return composed(qkv, heads, attn_drop)


class _TokenAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads):
        qkv = qkv.contiguous()
        B, T, C3 = qkv.shape
        dev = qkv.device
        out = torch.empty(B, T, C3 // 3, dtype=torch.float32, device=dev)
        lse = torch.empty(B, heads, T, dtype=torch.float32, device=dev)
        _call("apn_token_attention_fwd", dev, B, T, heads, qkv.data_ptr(), out.data_ptr(), lse.data_ptr())
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, out, lse = ctx.saved_tensors
        B, T, _ = qkv.shape
        g = g.contiguous().float()
        delta = torch.empty_like(lse)
        dqkv = torch.empty_like(qkv)
        _call("apn_token_attention_bwd", qkv.device, B, T, ctx.heads, qkv.data_ptr(), out.data_ptr(), lse.data_ptr(),
              g.data_ptr(), delta.data_ptr(), dqkv.data_ptr())
        return dqkv, None


def token_attention(qkv, heads):
    """softmax(q k^T / 8) v per head; qkv (B, T, 3*heads*64) -> (B, T, heads*64).  What the kernel does not cover
    (CPU tensors, other head dims) runs the composition and is counted in COMPOSED_CALLS."""
    why = _why_composed(qkv, heads)
    if why is not None:
        return fallback(qkv, heads, why)
    _lib.load()
    return _TokenAttention.apply(qkv, heads)
