"""Host side of the implicit-GEMM convolutions (the DiT's cnn-block, every convolution of the VAE): plain torch, allocation and index
arithmetic only.

A convolution runs as ONE flexam_gemm_bf16 launch over a zero-bordered channels-last bf16 image: K block kb of the GEMM reads, for
output position m, the 64 elements at buf[m * lda + a_koff[kb] ..] and multiplies them with columns kb * 64 .. kb * 64 + 63 of the
packed weight (include/flexam_hip.h, flexam_gemm_bf16).  The result is right only if the two agree block by block, so a convolution
states its K order ONCE -- as groups of taps, PackedConv -- and both the packed weight and the offset table are made from that.
"""
from typing import List, NamedTuple

import torch

from . import hip

BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def pad_k(w2d: torch.Tensor, device) -> torch.Tensor:
    """[N, K] -> bf16 [N, round_up(K, 64)], zero-padded: the GEMMs want K in 64-element blocks."""
    n, k = w2d.shape
    out = torch.zeros(n, round_up(k, 64), device=device, dtype=BF16)
    out[:, :k] = w2d.detach().to(device, BF16)
    return out


class Tap(NamedTuple):
    """Where a tap's weights apply: the contiguous image elements that start at channel `c` of the pixel (dt, dh, dw) away from the
    output position (frames, rows, columns of the padded image)."""
    dt: int
    dh: int
    dw: int
    c: int = 0


class PackedConv:
    """Packed bf16 weight [Cout, 64 * blocks], fp32 bias and the int64 a_koff table of one implicit-GEMM convolution.

    tap_w [Cout, taps, n] fp32: per tap, the weights of n contiguous image elements (the channels of one pixel; or a run of kw pixels);
    n is zero-padded to a multiple of 64 here.  groups: the same taps in the same order, as a list of lists of Tap.  The K order is
        for group: for 64-wide slice: for tap of the group
    -- every tap a group of its own is the tap-major order (tap, channel block); the taps of one image row as a group put the row's
    taps side by side on the same 64 channels (channel block, dw, 64)."""

    def __init__(self, tap_w: torch.Tensor, groups: List[List[Tap]], bias: torch.Tensor, device):
        co, nt, n = tap_w.shape
        taps = [t for g in groups for t in g]
        assert len(taps) == nt
        order, first = [], 0                                                     # K block -> (tap, 64-wide slice of it)
        for g in groups:
            order += [(first + j, s) for s in range(round_up(n, 64) // 64) for j in range(len(g))]
            first += len(g)
        self.blocks = [taps[i]._replace(c=taps[i].c + 64 * s) for i, s in order]
        wp = torch.zeros(co, nt, round_up(n, 64), device=device, dtype=F32)
        wp[..., :n] = tap_w
        ti, si = (torch.tensor(ix, device=device) for ix in zip(*order))
        self.weight = wp.view(co, nt, -1, 64)[:, ti, si].reshape(co, 64 * len(order)).to(BF16).contiguous()
        self.bias = bias.detach().to(device, F32).contiguous()
        self.co, self.device = co, device
        self._tables, self.a_koff = {}, None

    def at(self, hp: int, wp: int, cpix: int):
        """Sets a_koff for a padded image of hp x wp pixels of cpix elements each (one table per geometry, built once)."""
        key = (hp, wp, cpix)
        if key not in self._tables:
            offs = [((b.dt * hp + b.dh) * wp + b.dw) * cpix + b.c for b in self.blocks]
            self._tables[key] = torch.tensor(offs, dtype=I64, device=self.device)
        self.a_koff = self._tables[key]

    def launch(self, a, rows, out_dtype=F32, residual_into=None, out=None):
        """The convolution at the first `rows` positions of the 2-D image view `a`: -> [rows, Cout] (`out`, or new in out_dtype), or
        residual_into[rows, Cout] += bf16(conv) (fp32, in the GEMM epilogue)."""
        if residual_into is not None:
            return hip.gemm_gate_residual(a, self.weight, self.bias, residual_into, a_koff=self.a_koff)
        return hip.gemm(a, self.weight, self.bias, out=out, a_koff=self.a_koff, m=rows, k=self.weight.shape[1], out_dtype=out_dtype)


def reach(w: int, cp: int, overrun: int = 0) -> int:
    """Elements a 3x3 tap of the first or last padded position reaches outside a [.., w + 2, cp] image: one padded row and one pixel,
    plus what the last K block of a packed run reads past its run."""
    return round_up((w + 3) * cp + overrun, 8)


class GuardedImage:
    """Zero channels-last bf16 image [frames, h + 2, w + 2, cp] (`img`; `mat`: its rows as a 2-D view) inside one allocation `buf` with
    `front` and `back` guard elements, so that every tap offset of every padded position stays inside the allocation.  The border and
    the guards are zero and never written: they ARE the convolution's zero padding."""

    def __init__(self, frames, h, w, cp, device, front, back):
        n = frames * (h + 2) * (w + 2) * cp
        self.buf = torch.zeros(front + n + back, device=device, dtype=BF16)
        self.img = self.buf[front:front + n].view(frames, h + 2, w + 2, cp)
        self.mat = self.img.view(-1, cp)
