"""`attention()` operator seam of the reference (FlexAM/models/attention_utils.py:174-233), served by
the gfx950 flash-attention kernel.  Layout [B, L, N, D] like the reference; D must be 128.

The reference dispatches on VIDEOX_ATTENTION_TYPE to flash-attn / SageAttention / torch SDPA (attention_utils.py:195-233).
Here FLASH_ATTENTION and every other value map to the bf16 HIP kernel; SAGE_ATTENTION -- the reference's quantised attention --
maps to the MXFP8 kernel (csrc/attn_fp8.inc: e4m3 Q, K, P and V with E8M0 block scales, fp32 softmax) for self-attention shapes
(Lq == Lk, no key lengths) and to the bf16 kernel otherwise; with FLEXAM_SAGE_SMOOTH_K=1 it quantises K - mean_tokens(K) (smooth-K), with
FLEXAM_SAGE_SMOOTH_V=1 V - mean_tokens(V), the mean added back to the output in fp32 (smooth-V).  Unsupported options raise instead of silently changing semantics.

`causal` and `window_size` are flash-attn's (attention_utils.py:43-171 hands them to flash_attn_varlen_func): window_size = (left, right),
a negative side unbounded, query i sees key j iff j >= i - left and j <= i + right; causal=True sets right = 0.  They are served by the
windowed bf16 kernel (hip.attn_fwd_window) for Lq == Lk with q_lens / k_lens absent or all equal to that length.  Under SAGE_ATTENTION
a mask also runs that bf16 kernel unless FLEXAM_SAGE_WINDOW=1 (default 0, opt-in: quality on a real checkpoint is not measured), which
runs the windowed MXFP8 kernel (hip.attn_fwd_fp8 with a window) -- the reference's own `sageattn` call forwards is_causal only and
drops window_size (attention_utils.py:195-203), which this seam does not imitate."""
import os
import warnings

import torch

from . import hip
from .dit_layout import sage_window_asked, smooth_k_asked, smooth_v_asked


def attention(q, k, v, q_lens=None, k_lens=None, dropout_p=0.0, softmax_scale=None, q_scale=None, causal=False,
              window_size=(-1, -1), deterministic=False, dtype=torch.bfloat16, fa_version=None, attention_type=None, attn_mask=None):
    if attn_mask is not None or dropout_p != 0.0:
        raise NotImplementedError("flexam_amd.attention: attn_mask / dropout are not used on the FlexAM path")
    window = hip.attn_window(window_size, causal)
    if q_scale is not None:
        q = q * q_scale
    b, lq, n, d = q.shape
    lk = k.shape[1]
    out_dtype = q.dtype
    q, k, v = (u.to(torch.bfloat16).contiguous() for u in (q, k, v))
    if window != (-1, -1):
        # flash-attn aligns the mask of Lq != Lk (and of every sample's q_lens[i] != k_lens[i]) to the bottom-right corner, torch SDPA's
        # is_causal to the top-left one: the reference's answer depends on the backend it finds, so only the case both agree on is served
        lens = [int(x) for u in (q_lens, k_lens) if u is not None for x in u]
        if lq != lk or any(x != lq for x in lens):
            raise NotImplementedError("flexam_amd.attention: causal / window_size with Lq != Lk or with q_lens / k_lens other than the full "
                                      "length is not served: flash-attn aligns such a mask bottom-right, SDPA top-left")
        # FLEXAM_SAGE_WINDOW=1 (default 0) under SAGE_ATTENTION: the windowed MXFP8 launch, packed as the unmasked SAGE call below packs
        sage = (attention_type if attention_type is not None else os.environ.get("VIDEOX_ATTENTION_TYPE", "FLASH_ATTENTION")) == "SAGE_ATTENTION"
        if sage and sage_window_asked(os.environ) and not torch.is_grad_enabled() and d == hip.ATTN_HEAD_DIM:
            scale = (softmax_scale if softmax_scale is not None else d ** -0.5) * 1.4426950408889634
            mean = hip.k_mean(k.view(b * lk, n * d), None, None, None, lk) if smooth_k_asked(os.environ) else None
            v_mean = hip.k_mean(v.view(b * lk, n * d), None, None, None, lk) if smooth_v_asked(os.environ) else None
            bufs = hip.attn_fp8_pack((q.float() * scale).to(torch.bfloat16), k, v, k_shift=mean, v_shift=v_mean)
            return hip.attn_fwd_fp8(bufs, lq, o_shift=v_mean, window=window).to(out_dtype)
        return hip.attn_fwd_window(q, k, v, window, softmax_scale=softmax_scale).to(out_dtype)
    uniform = True
    if k_lens is not None:
        kl = [int(x) for x in k_lens]
        if any(x != kl[0] for x in kl):
            uniform = False
        lk_eff = kl
    if q_lens is not None and any(int(x) != lq for x in q_lens):
        warnings.warn("flexam_amd.attention: q_lens shorter than Lq are computed and left in place (rows past q_lens are not zeroed)")
    if attention_type is None:
        attention_type = os.environ.get("VIDEOX_ATTENTION_TYPE", "FLASH_ATTENTION")
    if attention_type == "SAGE_ATTENTION" and torch.is_grad_enabled():
        attention_type = "FLASH_ATTENTION"              # as the reference does (attention_utils.py:196-197)
    if attention_type == "SAGE_ATTENTION" and k_lens is None and lq == lk:
        scale = (softmax_scale if softmax_scale is not None else d ** -0.5) * 1.4426950408889634
        # FLEXAM_SAGE_SMOOTH_K=1 (default 0): K - mean_tokens(K) is quantised instead of K -- the same softmax, see csrc/attn_fp8.inc
        mean = hip.k_mean(k.view(b * lk, n * d), None, None, None, lk) if smooth_k_asked(os.environ) else None
        # FLEXAM_SAGE_SMOOTH_V=1 (default 0): V - mean_tokens(V) is quantised and the kernel adds the mean back before it rounds its output
        v_mean = hip.k_mean(v.view(b * lk, n * d), None, None, None, lk) if smooth_v_asked(os.environ) else None
        bufs = hip.attn_fp8_pack((q.float() * scale).to(torch.bfloat16), k, v, k_shift=mean, v_shift=v_mean)
        return hip.attn_fwd_fp8(bufs, lq, o_shift=v_mean).to(out_dtype)
    if k_lens is None:
        return hip.attn_fwd(q, k, v, softmax_scale=softmax_scale).to(out_dtype)
    if uniform:
        return hip.attn_fwd(q, k[:, :lk_eff[0]], v[:, :lk_eff[0]], softmax_scale=softmax_scale).to(out_dtype)
    out = torch.empty_like(q)
    for i in range(b):                                  # ragged key lengths: one launch per sample
        hip.attn_fwd(q[i:i + 1], k[i:i + 1, :lk_eff[i]], v[i:i + 1, :lk_eff[i]], out=out[i:i + 1], softmax_scale=softmax_scale)
    return out.to(out_dtype)
