"""MI355X drop-in for `AutoencoderKLWan3_8` (Wan2.2 3D-VAE, z = 48, 4x16x16) -- decode and encode paths.

Reference: FlexAM/models/wan_vae3_8.py (:892-1079 wrapper, :739-870 chunked model, :621-728 decoder).
State-dict keys are the reference's (`model.encoder...`, `model.conv1...`, `model.decoder...`,
`model.conv2...`; a full Wan2.2_VAE.pth loads as VAE.py:1073-1077 does).  `decode(z).sample` and
`encode(x).latent_dist` run entirely in libflexam_hip.so:

  * activations are channels-last; every causal 3x3x3 / 3x3 convolution is ONE flexam_gemm_bf16
    launch over a zero-bordered bf16 image with a per-K-block tap-offset table (implicit GEMM, no
    im2col), 27 taps x Cin/64 K-blocks, fp32 accumulate on MFMA;
  * the chunk-causal cache of the reference (feat_cache/feat_idx, CACHE_T = 2) is a 2-frame history
    kept at the front of each conv's input image and rolled after the conv -- same arithmetic, see
    DESIGN.md "VAE chunk cache";
  * RMS_norm + SiLU, nearest-2x upsample (+ frame de-interleave), DupUp3D shortcut, the middle
    attention (head_dim = C, as three GEMMs + a row softmax) and unpatchify + clamp are one-pass
    bandwidth kernels (csrc/vae.hip); the residual stream between blocks stays fp32;
  * encode (VAE.py:788-818, Encoder3d :505-618): patchify writes the 12-channel conv1 image directly; the
    stride-2 spatial convs run as unit-stride implicit GEMMs over a space-to-depth image (the 9 taps address
    (row, col, sub-pixel channel group)); the stride-2 temporal conv is one GEMM per output frame over the
    same history image; AvgDown3D shortcuts are a fused gather-mean-add; the final 1x1 conv and the latent
    normalisation are folded into the head conv's weights (exact in fp32, one GEMM fewer).
"""
import math
import os
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import hip, vae_tiles
from .implicit_conv import GuardedImage, PackedConv, Tap, pad_k, reach, round_up
from .wan_transformer3d_FlexAM import ModelConfig

BF16, F32 = torch.bfloat16, torch.float32

# latent normalisation statistics of the Wan2.2 VAE (published constants; VAE.py:906-1010)
LATENT_MEAN = [-0.2289, -0.0052, -0.1323, -0.2339, -0.2799, 0.0174, 0.1838, 0.1557, -0.1382, 0.0542, 0.2813, 0.0891,
               0.1570, -0.0098, 0.0375, -0.1825, -0.2246, -0.1207, -0.0698, 0.5109, 0.2665, -0.2108, -0.2158, 0.2502,
               -0.2055, -0.0322, 0.1109, 0.1567, -0.0729, 0.0899, -0.2799, -0.1230, -0.0313, -0.1649, 0.0117, 0.0723,
               -0.2839, -0.2083, -0.0520, 0.3748, 0.0152, 0.1957, 0.1433, -0.2944, 0.3573, -0.0548, -0.1681, -0.0667]
LATENT_STD = [0.4765, 1.0364, 0.4514, 1.1677, 0.5313, 0.4990, 0.4818, 0.5013, 0.8158, 1.0344, 0.5894, 1.0901,
              0.6885, 0.6165, 0.8454, 0.4978, 0.5759, 0.3523, 0.7135, 0.6804, 0.5833, 1.4146, 0.8986, 0.5659,
              0.7069, 0.5338, 0.4889, 0.4917, 0.4069, 0.4999, 0.6866, 0.4093, 0.5709, 0.6065, 0.6415, 0.4944,
              0.5726, 1.2042, 0.5458, 1.6887, 0.3971, 1.0600, 0.3943, 0.5537, 0.5444, 0.4089, 0.7468, 0.7744]


class DecoderOutput:
    def __init__(self, sample):
        self.sample = sample


class DiagonalGaussianDistribution:
    """The posterior object `encode` returns (diffusers' class of the same name, used by VAE.py:1034):
    parameters = [mean | logvar] along dim 1, logvar clamped to [-30, 20]."""

    def __init__(self, parameters: torch.Tensor, deterministic: bool = False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if deterministic:
            self.var = self.std = torch.zeros_like(self.mean)

    def sample(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        noise = torch.randn(self.mean.shape, generator=generator, device=self.parameters.device, dtype=self.parameters.dtype)
        return self.mean + self.std * noise

    def mode(self) -> torch.Tensor:
        return self.mean


class AutoencoderKLOutput:
    def __init__(self, latent_dist):
        self.latent_dist = latent_dist

    def __getitem__(self, i):
        return (self.latent_dist,)[i]


def _shape_inventory():
    """-> (shapes, conv, res): an empty name -> shape dict and the two functions that enter a convolution / a ResidualBlock into it."""
    s: Dict[str, tuple] = {}

    def conv(name, co, ci, k):
        s[name + ".weight"], s[name + ".bias"] = (co, ci, *k), (co,)

    def res(name, ci, co):
        s[name + ".residual.0.gamma"] = (ci, 1, 1, 1)
        conv(name + ".residual.2", co, ci, (3, 3, 3))
        s[name + ".residual.3.gamma"] = (co, 1, 1, 1)
        conv(name + ".residual.6", co, co, (3, 3, 3))
        if ci != co:
            conv(name + ".shortcut", co, ci, (1, 1, 1))
    return s, conv, res


def decoder_param_shapes(z_dim=48, dec_dim=256, dim_mult=(1, 2, 4, 4), temporal_up=(True, True, False)) -> Dict[str, tuple]:
    """Parameter inventory of conv2 + Decoder3d under the reference's names (VAE.py:621-675)."""
    dims = [dec_dim * m for m in [dim_mult[-1]] + list(dim_mult[::-1])]
    s, conv, res = _shape_inventory()
    conv("conv2", z_dim, z_dim, (1, 1, 1))
    conv("decoder.conv1", dims[0], z_dim, (3, 3, 3))
    res("decoder.middle.0", dims[0], dims[0])
    s["decoder.middle.1.norm.gamma"] = (dims[0], 1, 1)
    conv("decoder.middle.1.to_qkv", dims[0] * 3, dims[0], (1, 1))
    conv("decoder.middle.1.proj", dims[0], dims[0], (1, 1))
    res("decoder.middle.2", dims[0], dims[0])
    for i, (ci, co) in enumerate(zip(dims[:-1], dims[1:])):
        c_in = ci
        for j in range(3):
            res(f"decoder.upsamples.{i}.upsamples.{j}", c_in, co)
            c_in = co
        if i != len(dims) - 2:
            conv(f"decoder.upsamples.{i}.upsamples.3.resample.1", co, co, (3, 3))
            if temporal_up[i]:
                conv(f"decoder.upsamples.{i}.upsamples.3.time_conv", co * 2, co, (3, 1, 1))
    s["decoder.head.0.gamma"] = (dims[-1], 1, 1, 1)
    conv("decoder.head.2", 12, dims[-1], (3, 3, 3))
    return s


def encoder_param_shapes(z_dim=48, dim=160, dim_mult=(1, 2, 4, 4), temporal_down=(False, True, True)) -> Dict[str, tuple]:
    """Parameter inventory of conv1 + Encoder3d under the reference's names (VAE.py:505-562, :757-758)."""
    dims = [dim * m for m in [1] + list(dim_mult)]
    s, conv, res = _shape_inventory()
    conv("conv1", z_dim * 2, z_dim * 2, (1, 1, 1))
    conv("encoder.conv1", dims[0], 12, (3, 3, 3))
    n_stage = len(dims) - 1
    for i, (ci, co) in enumerate(zip(dims[:-1], dims[1:])):
        q = f"encoder.downsamples.{i}.downsamples"
        res(f"{q}.0", ci, co)
        res(f"{q}.1", co, co)
        if i != n_stage - 1:
            conv(f"{q}.2.resample.1", co, co, (3, 3))
            if i < len(temporal_down) and temporal_down[i]:
                conv(f"{q}.2.time_conv", co, co, (3, 1, 1))
    res("encoder.middle.0", dims[-1], dims[-1])
    s["encoder.middle.1.norm.gamma"] = (dims[-1], 1, 1)
    conv("encoder.middle.1.to_qkv", dims[-1] * 3, dims[-1], (1, 1))
    conv("encoder.middle.1.proj", dims[-1], dims[-1], (1, 1))
    res("encoder.middle.2", dims[-1], dims[-1])
    s["encoder.head.0.gamma"] = (dims[-1], 1, 1, 1)
    conv("encoder.head.2", z_dim * 2, dims[-1], (3, 3, 3))
    return s


class _ParamTree(nn.Module):
    """Holds parameters under dotted names ('decoder.middle.0.residual.2.weight') as nested modules."""

    def add(self, dotted: str, shape):
        head, _, rest = dotted.partition(".")
        if not rest:
            self.register_parameter(head, nn.Parameter(torch.zeros(shape)))
            return
        if head not in self._modules:
            self.add_module(head, _ParamTree())
        self._modules[head].add(rest, shape)


def padded_rows(t, h, w):
    """GEMM rows of t frames of an h x w image with its zero border."""
    return t * (h + 2) * (w + 2)


class _CausalImage:
    """The input frames of a causal convolution: a zero-bordered channels-last bf16 image [hist + t_cap, h + 2, w + 2, cp] -- `hist`
    frames of history in front of the current chunk -- as a window into a ring of RING chunks.  The window [history | current chunk]
    slides forward by the chunk length after every run, so the last `hist` frames of a chunk ARE the history of the next one where they
    lie; only when the window reaches the end of the buffer are those frames copied to its start (every RING-th chunk instead of after
    every chunk: the copies were 3 % of a decode and 5 % of an encode).  Border positions are zero everywhere and never written."""
    RING = max(1, int(os.environ.get("FLEXAM_VAE_RING", "4")))

    def __init__(self, hist: int, t_cap: int, cp: int, device):
        self.hist, self.t_cap, self.cp, self.device, self.shape = hist, t_cap, cp, device, None

    def image(self, h, w):
        if self.shape != (h, w):
            ring = max(1, min(self.RING, 16 // max(self.t_cap, 1))) if self.hist else 1      # long chunks: fewer of them, and a short ring (memory)
            guard = reach(w, self.cp, 64)                        # + the overrun of a packed run's last K block
            self.all = GuardedImage(self.hist + self.t_cap * ring, h, w, self.cp, self.device, guard, guard).img
            self.cur = 0                                         # first frame of the window
            self.placed(h, w)
            self.shape = (h, w)
            self.img = self.all[:self.hist + self.t_cap]
        return self.img

    def placed(self, h, w):
        """The image has a new geometry: what depends on it follows here."""

    def reset(self):
        if self.shape is not None and self.hist:
            self.cur = 0
            self.img = self.all[:self.hist + self.t_cap]
            self.img[:self.hist].zero_()

    def roll(self, t):
        """The last `hist` frames of the chunk become the history of the next one: the window moves on by t frames."""
        if self.hist:
            win = self.hist + self.t_cap
            self.cur += t
            if self.cur + win > self.all.shape[0]:               # end of the ring: bring the history to the front
                src = self.all[self.cur:self.cur + self.hist]
                self.all[:self.hist].copy_(src.clone() if self.cur < self.hist else src)
                self.cur = 0
            self.img = self.all[self.cur:self.cur + win]


class _Conv(PackedConv, _CausalImage):
    """One (causal) convolution as an implicit GEMM: packed bf16 weight [Cout, taps*Cp], fp32 bias, tap-offset tables, over a
    _CausalImage with kt - 1 history frames."""

    def __init__(self, weight, bias, device, t_cap: int):
        w = weight.detach().to(device, F32)
        if w.dim() == 4:
            w = w.unsqueeze(2)
        co, ci, kt, kh, kw = w.shape
        self.ci, self.kt, self.kh, self.kw = ci, kt, kh, kw
        pix = w.permute(0, 2, 3, 4, 1)                                           # [co, kt, kh, kw, ci]
        rows = [(dt, dh - kh // 2) for dt in range(kt) for dh in range(kh)]      # the image rows under the window
        # Run packing (channel counts that are not multiples of 64: the encoder's 160-channel stage and its 12-channel input): the
        # image keeps `ci` channels per pixel (rounded to 8: 16-byte pixels) instead of padding each pixel to 64, and the kw taps of one
        # image row -- kw * cp CONTIGUOUS elements starting at pixel w - 1 -- are one K run, padded to 64 as a whole (3 * 160 = 480 ->
        # 512 instead of 3 * 192 = 576; 3 * 16 = 48 -> 64 instead of 192).  The run's last K block reads a few channels of pixel w + 2:
        # finite activations against zero weights.
        self.run_pack = kw == 3 and ci % 64 != 0
        if self.run_pack:
            cp = round_up(ci, 8)
            runs = torch.zeros(co, kt * kh, kw, cp, device=device, dtype=F32)
            runs[..., :ci] = pix.reshape(co, kt * kh, kw, ci)
            tap_w, groups = runs.view(co, kt * kh, kw * cp), [[Tap(dt, dh, -(kw // 2))] for dt, dh in rows]
        else:
            # K order (dt, dh, channel block, dw, 64 channels): the kw taps of one image row are consecutive K blocks, and they read
            # the same 64-channel slice of rows shifted by ONE position -- the second and third hit the L2 lines the first just
            # brought in.  (With the tap-major order (dt, dh, dw, channel block) a shifted re-read comes cp/64 K blocks later, after
            # the XCD's 32 workgroups have pulled 32 x cp/64 x 32 KiB through its 4 MiB L2: the 3x3x3 convs at 256 x 448 then fetch
            # every activation ~9 times over the fabric.)
            cp = round_up(ci, 64)
            tap_w, groups = pix.reshape(co, kt * kh * kw, ci), [[Tap(dt, dh, dw - kw // 2) for dw in range(kw)] for dt, dh in rows]
        PackedConv.__init__(self, tap_w, groups, bias, device)
        _CausalImage.__init__(self, kt - 1, t_cap, cp, device)

    def placed(self, h, w):
        self.at(h + 2, w + 2, self.cp)

    def weight_elems(self):
        """Weight elements the convolution multiplies per output position (_stage_cost)."""
        return self.weight.numel()

    def run(self, t, h, w, out_dtype=F32, residual_into=None):
        """Convolve the `t` current frames (window frames hist..hist+t); then slide the window."""
        out = self.launch(self.img.view(-1, self.cp), padded_rows(t, h, w), out_dtype, residual_into)
        self.roll(t)
        return out

    def run_time_stride2(self, t, h, w, out_dtype=F32):
        """(3,1,1) conv with temporal stride 2 and one cached frame (Resample downsample3d, VAE.py:162-174):
        output frame j reads [prev | x][2j .. 2j+2] = image frames 1+2j .. 3+2j; one GEMM per output frame."""
        if t % 2 or (self.kt, self.kh, self.kw) != (3, 1, 1):
            raise RuntimeError("run_time_stride2: needs an even frame count and a (3,1,1) kernel")
        rows = padded_rows(1, h, w)
        out = torch.empty(t // 2 * rows, self.co, device=self.device, dtype=out_dtype)
        for j in range(t // 2):
            self.launch(self.img[1 + 2 * j:].reshape(-1, self.cp), rows, out=out[j * rows:(j + 1) * rows])
        self.roll(t)
        return out


class _ConvFold(_CausalImage):
    """A causal convolution with few output channels (the decoder head, 256 -> 12) as a per-tap product + gather: ONE plain GEMM over
    the input pixels, Y[pixel, tap * Cout + o] = W[o, :, tap] . x[pixel, :] (K = Cin: every activation is read once; N = 27 * 12 = 324),
    then flexam_tapsum_cl adds, for every output pixel, the 27 products of its neighbours.  As an implicit GEMM the same convolution has
    K = 27 Cin -- every activation re-read 27 times -- for 12 useful columns of a 160-wide tile: 0.73 ms per 4 frames at 256 x 448, 2.4 %
    of a decode.  Y is recomputed for the two history frames of a chunk (they are the chunk before's last frames)."""

    def __init__(self, weight, bias, device, t_cap: int):
        w = weight.detach().to(device, F32)
        co, ci, kt, kh, kw = w.shape
        assert (kh, kw) == (3, 3)
        _CausalImage.__init__(self, kt - 1, t_cap, round_up(ci, 64), device)
        self.co, self.ci, self.kt = co, ci, kt
        # the taps lie along N, not K -- row (dt*9 + dh*3 + dw) * co + o, the order flexam_tapsum_cl gathers in -- and K is the channels
        # of one pixel: a plain GEMM with no offset table, so there is no K order to state
        self.weight = pad_k(w.permute(2, 3, 4, 0, 1).reshape(kt * 9 * co, ci), device)
        self.bias = bias.detach().to(device, F32).contiguous()
        self._y = None

    def run(self, t, h, w, out_dtype=F32, residual_into=None):
        assert out_dtype == F32 and residual_into is None
        rows_all = padded_rows(self.hist + t, h, w)
        if self._y is None or self._y.shape[0] < rows_all:
            self._y = torch.empty(padded_rows(self.hist + self.t_cap, h, w), self.weight.shape[0], device=self.device, dtype=F32)
        y = hip.gemm(self.img.view(-1, self.cp)[:rows_all], self.weight, None, out=self._y[:rows_all])
        out = torch.empty(padded_rows(t, h, w), self.co, device=self.device, dtype=F32)      # border rows: never read
        hip.tapsum_cl(y, t, h, w, self.kt, self.co, self.bias, out)
        self.roll(t)
        return out


class _ConvS2D(PackedConv):
    """ZeroPad2d((0,1,0,1)) + Conv2d(3x3, stride 2) (Resample downsample2d/3d, VAE.py:104-113) as a unit-stride
    implicit GEMM over a space-to-depth image [t, H/2+2, W/2+2, 4*Cs]: tap (dh, dw) of the strided conv is
    (row dh>>1, col dw>>1, channel group (dh&1)*2 + (dw&1)) of that image."""

    def __init__(self, weight, bias, device, t_cap: int):
        w = weight.detach().to(device, F32)
        co, ci, kh, kw = w.shape
        assert (kh, kw) == (3, 3)
        self.ci, self.cs = ci, round_up(ci, 64)
        # K order as in _Conv: (dh, channel block, dw, 64)
        groups = [[Tap(0, dh >> 1, dw >> 1, ((dh & 1) * 2 + (dw & 1)) * self.cs) for dw in range(3)] for dh in range(3)]
        super().__init__(w.permute(0, 2, 3, 1).reshape(co, 9, ci), groups, bias, device)
        self.t_cap, self.shape = t_cap, None

    def image(self, h2, w2):
        """h2, w2: OUTPUT resolution."""
        if self.shape != (h2, w2):
            c4 = 4 * self.cs
            self.img = GuardedImage(self.t_cap, h2, w2, c4, self.device, 0, (w2 + 4) * c4).img
            self.at(h2 + 2, w2 + 2, c4)
            self.shape = (h2, w2)
        return self.img

    def run(self, t, h2, w2, out_dtype=F32, residual_into=None):
        rows = padded_rows(t, h2, w2)
        return self.launch(self.img.view(-1, 4 * self.cs), rows, out_dtype, None if residual_into is None else residual_into[:rows])


class _ConvUp2x:
    """Nearest-exact 2x spatial upsample followed by Conv2d(3x3, padding 1) (Resample upsample2d / upsample3d, VAE.py:76-99) WITHOUT the
    upsampled image.  Output pixel (2y + a, 2x + b) sees, through the 3x3 window on the upsampled image, only the 2x2 block of
    LOW-resolution pixels (y - 1 + a + r, x - 1 + b + c), r, c in {0, 1}: rows 2y - 1 | 2y, 2y + 1 of the upsampled image are rows
    y - 1 | y, y of the input (a = 0) and rows 2y, 2y + 1 | 2y + 2 are rows y, y | y + 1 (a = 1).  So every parity (a, b) is a 2x2
    convolution of the low-resolution image with taps that are SUMS of the original ones (fp32 sums, rounded to bf16 once):
        W'[a][r] = { a=0: (W[-1], W[0] + W[1]);  a=1: (W[-1] + W[0], W[1]) }   (the same along x)
    -- four implicit GEMMs with K = 4 Cin over the low-resolution rows instead of one with K = 9 Cin over four times as many: 16
    instead of 36 tap products per low-resolution pixel (2.25x fewer FLOPs: these convolutions were 10 % of a decode), a quarter of the
    image bytes, and the zero border of the low-resolution image IS the convolution's zero padding (row 2H of the upsampled image
    does not exist, neither does row H of the input).  The four outputs [4, rows, Cout] fp32 are interleaved into the high-
    resolution residual stream by flexam_phase_dupup_cl together with the DupUp3D shortcut."""
    SETS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}        # (parity, r) -> original tap indices (dy + 1)

    def __init__(self, weight, bias, device, t_cap: int):
        w = weight.detach().to(device, F32)
        co, ci, kh, kw = w.shape
        assert (kh, kw) == (3, 3)
        self.co, self.ci, self.cp = co, ci, round_up(ci, 64)
        self.bias = bias.detach().to(device, F32).contiguous()
        self.phases = []
        for a in (0, 1):
            for b in (0, 1):
                sums = [sum(w[:, :, i, j] for i in self.SETS[(a, r)] for j in self.SETS[(b, c)]) for r in (0, 1) for c in (0, 1)]
                # K order (r, channel block, c, 64): the two column taps of a row are consecutive K blocks on the same 64 channels (see _Conv)
                groups = [[Tap(0, a + r - 1, b + c - 1) for c in (0, 1)] for r in (0, 1)]
                self.phases.append(PackedConv(torch.stack(sums, 1), groups, self.bias, device))
        self.weights = [p.weight for p in self.phases]
        self.t_cap, self.device, self.shape = t_cap, device, None

    def weight_elems(self):
        """Weight elements the four phases multiply per LOW-resolution position (_stage_cost)."""
        return sum(wt.numel() for wt in self.weights)

    def image(self, h, w):
        """h, w: INPUT (low) resolution.  Zero-bordered [t_cap, h + 2, w + 2, cp] with guard rows on both sides (the taps of the first
        and last padded rows reach one row past the image)."""
        if self.shape != (h, w):
            guard = reach(w, self.cp, 64)
            self.img = GuardedImage(self.t_cap, h, w, self.cp, self.device, guard, guard).img
            for p in self.phases:
                p.at(h + 2, w + 2, self.cp)
            self.shape = (h, w)
            self._ph = None
        return self.img

    def run(self, t, h, w):
        """-> phases [4, t*(h+2)*(w+2), Cout] fp32 (rows of the padded LOW-resolution image; border rows hold garbage, never read)."""
        rows = padded_rows(t, h, w)
        if self._ph is None or self._ph.shape[1] < rows:
            self._ph = torch.empty(4, padded_rows(self.t_cap, h, w), self.co, device=self.device, dtype=F32)
        a = self.img.view(-1, self.cp)
        for i, p in enumerate(self.phases):
            p.launch(a, rows, out=self._ph[i, :rows])
        return self._ph[:, :rows]


def _f32(t, dev):
    return t.detach().to(dev, F32).reshape(-1).contiguous()


class _ResBlock:
    """ResidualBlock (VAE.py:198-240): RMS_norm + SiLU + conv, twice, added to the input or to its 1x1x1 shortcut conv."""

    def __init__(self, g0, c1, g3, c2, short, plain_image):
        self.g0, self.c1, self.g3, self.c2, self.short = g0, c1, g3, c2, short
        self._plain_image = plain_image                    # the engine's: one shortcut image per (Cin, t, h, w, cp), not one per block

    def causal_convs(self):
        return [self.c1, self.c2]

    def weight_elems(self):
        return self.c1.weight_elems() + self.c2.weight_elems() + (self.short.weight_elems() if self.short is not None else 0)

    def run(self, x, t, h, w):
        """Rows x [t*(h+2)*(w+2), Cin] fp32 -> [.., Cout] fp32 (in place when there is no shortcut conv)."""
        c1, c2 = self.c1, self.c2
        hip.vae_prep_cl(x, c1.ci, t, h, w, c1.image(h, w), mode=2, gamma=self.g0, t0=c1.hist)
        t1 = c1.run(t, h, w, out_dtype=BF16)
        hip.vae_prep_cl(t1, c2.ci, t, h, w, c2.image(h, w), mode=2, gamma=self.g3, t0=c2.hist)
        if self.short is not None:
            sc = self.short
            xb = self._plain_image(("short", sc.ci), t, h, w, sc.cp)
            hip.vae_prep_cl(x, sc.ci, t, h, w, xb, mode=0)
            x = hip.gemm(xb.view(-1, sc.cp), sc.weight, sc.bias, out_dtype=F32)
        c2.run(t, h, w, residual_into=x)
        return x


class _AttnBlock:
    """AttentionBlock (VAE.py:243-282): per frame, one head with head_dim = C."""

    def __init__(self, sd, name, c, dev):
        wqkv = sd[name + ".to_qkv.weight"].detach().to(dev, F32).reshape(3 * c, c)
        self.bqkv = _f32(sd[name + ".to_qkv.bias"], dev)
        self.c, self.gamma, self.wqkv = c, _f32(sd[name + ".norm.gamma"], dev), wqkv.to(BF16).contiguous()
        self.wv, self.bv = wqkv[2 * c:].to(BF16).contiguous(), self.bqkv[2 * c:].contiguous()
        self.wproj = sd[name + ".proj.weight"].detach().to(dev, BF16).reshape(c, c).contiguous()
        self.bproj = _f32(sd[name + ".proj.bias"], dev)

    def causal_convs(self):
        return []

    def run(self, x, t, h, w):
        c, dev = self.c, self.gamma.device
        n = h * w
        n4, kp = round_up(n, 4), round_up(n, 64)                                         # GEMM N granularity / K granularity
        rows = padded_rows(1, h, w)
        for f in range(t):
            xf = x[f * rows:(f + 1) * rows]
            xn = torch.zeros(n4, c, device=dev, dtype=BF16)
            hip.vae_prep_cl(xf, c, 1, h, w, xn, mode=1, gamma=self.gamma, compact=True)
            qk = hip.gemm(xn, self.wqkv[:2 * c], self.bqkv[:2 * c])                       # [n4, 2c]
            s = hip.gemm(qk[:n, :c], qk[:, c:], out_dtype=F32)                             # q k^T  [n, n4]; softmax over the first n
            p = torch.empty(n, kp, device=dev, dtype=BF16)
            hip.softmax_rows(s, c ** -0.5, p, n)
            vt = torch.zeros(c, kp, device=dev, dtype=BF16)
            hip.gemm(self.wv, xn, out=vt[:, :n4])                                          # V^T (bias folded below: rows of P sum to 1)
            o = hip.gemm(p, vt, self.bv)                                                   # [n, c]
            y = hip.gemm(o, self.wproj, self.bproj)
            hip.scatter_add_cl(xf, y, c, 1, h, w)
        return x


class _Stage:
    """The residual blocks of one resolution; all stages but the last end in a resample (2x in space; with `time_conv` also in time)."""

    def __init__(self, res, cout, resample=None, time_conv=None):
        self.res, self.cout, self.resample, self.time_conv = res, cout, resample, time_conv
        self.temporal = time_conv is not None


class _UpStage(_Stage):
    up = property(lambda self: self.resample is not None)

    def __getitem__(self, key):                            # benchlib/vae_clip.py reads stages[i]["up"]
        return getattr(self, key)


class _DownStage(_Stage):
    down = property(lambda self: self.resample is not None)


class _EngineBase:
    """What the decoder and the encoder share: conv1, the stages, the middle [ResidualBlock, AttentionBlock, ResidualBlock], the head."""

    def _setup(self, vae):
        self.sd = sd = {k: v for k, v in vae.model.state_dict().items()}
        self.device = dev = next(vae.model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("flexam_amd: the VAE runs only on a GPU through libflexam_hip.so (no CPU fallback)")
        hip.device_check()
        self._scratch = {}
        return sd, dev

    def _mk_conv(self, name, t_cap=1):
        return _Conv(self.sd[name + ".weight"], self.sd[name + ".bias"], self.device, t_cap)

    def _mk_res(self, name, t_cap):
        sd, dev = self.sd, self.device
        return _ResBlock(_f32(sd[name + ".residual.0.gamma"], dev), self._mk_conv(name + ".residual.2", t_cap),
                         _f32(sd[name + ".residual.3.gamma"], dev), self._mk_conv(name + ".residual.6", t_cap),
                         self._mk_conv(name + ".shortcut", t_cap) if (name + ".shortcut.weight") in sd else None, self._plain_image)

    def _mk_mid(self, name, c, t_cap):
        r0, r2 = self._mk_res(name + ".0", t_cap), self._mk_res(name + ".2", t_cap)
        return [r0, _AttnBlock(self.sd, name + ".1", c, self.device), r2]

    def _plain_image(self, key, frames, h, w, cp):
        k = (key, frames, h, w, cp)
        if k not in self._scratch:
            self._scratch[k] = GuardedImage(frames, h, w, cp, self.device, 0, 0).img
        return self._scratch[k]

    def _all_convs(self):
        """Every convolution that carries frames from one chunk to the next."""
        blocks = self.mid + [r for st in self.stages for r in st.res]
        return ([self.conv1, self.head_conv] + [c for r in blocks for c in r.causal_convs()]
                + [st.time_conv for st in self.stages if st.time_conv is not None])

    def _run_mid(self, x, t, h, w):
        for blk in self.mid:
            x = blk.run(x, t, h, w)
        return x


class _DecoderEngine(_EngineBase):
    def __init__(self, vae):
        sd, dev = self._setup(vae)
        cfg = vae._arch
        self.z_dim, self.temporal_up = cfg["z_dim"], tuple(cfg["temporal_up"])
        dims = [cfg["dec_dim"] * m for m in [cfg["dim_mult"][-1]] + list(cfg["dim_mult"][::-1])]
        self.dims = dims
        # Latent frames per chunk after the first (1-frame) chunk.  The reference decodes one latent frame at a time (VAE.py:1046-1052) to
        # bound memory; the convolutions are causal over their own input history, so the output does not depend on the chunk length.
        # Several latent frames per chunk fill the 32 x 56 / 64 x 112 stages (1972 / 15048 GEMM rows per latent frame: pure split-K
        # launches at a third of the matrix rate) and cut the launch count.  FLEXAM_VAE_DEC_CHUNK=1 is the reference's walk.
        self.chunk = n = max(1, int(os.environ.get("FLEXAM_VAE_DEC_CHUNK", "2")))
        tmul = [n]
        for up in self.temporal_up:
            tmul.append(tmul[-1] * (2 if up else 1))                       # frames per chunk entering stage i
        conv, res = self._mk_conv, self._mk_res
        self.phase_up = os.environ.get("FLEXAM_VAE_UPCONV", "phase") != "image"
        self.conv2 = conv("conv2")
        self.conv1 = conv("decoder.conv1", n)
        self.mid = self._mk_mid("decoder.middle", dims[0], n)
        self.stages = []
        n_stage = len(dims) - 1
        for i in range(n_stage):
            p = f"decoder.upsamples.{i}.upsamples"
            blocks, resample, time_conv = [res(f"{p}.{j}", tmul[i]) for j in range(3)], None, None
            if i != n_stage - 1:
                t_rs = tmul[i] * (2 if self.temporal_up[i] else 1)
                # FLEXAM_VAE_UPCONV=image: the earlier form (upsampled image + one 3x3 convolution over it), A/B and cross-check only
                resample = (_ConvUp2x(sd[f"{p}.3.resample.1.weight"], sd[f"{p}.3.resample.1.bias"], dev, t_rs) if self.phase_up
                            else conv(f"{p}.3.resample.1", t_rs))
                time_conv = conv(f"{p}.3.time_conv", tmul[i]) if self.temporal_up[i] else None
            self.stages.append(_UpStage(blocks, dims[i + 1], resample, time_conv))
        self.head_gamma = _f32(sd["decoder.head.0.gamma"], dev)
        # FLEXAM_VAE_HEADCONV=implicit: the head as an implicit GEMM like every other convolution (A/B and cross-check)
        if os.environ.get("FLEXAM_VAE_HEADCONV", "fold") != "implicit" and sd["decoder.head.2.weight"].shape[0] % 4 == 0:
            self.head_conv = _ConvFold(sd["decoder.head.2.weight"], sd["decoder.head.2.bias"], dev, tmul[-1])
        else:
            self.head_conv = conv("decoder.head.2", tmul[-1])
        self.mean = torch.tensor(vae.latent_mean, device=dev, dtype=F32)
        self.std = torch.tensor(vae.latent_std, device=dev, dtype=F32)
        self._grid_cache = {}
        del self.sd

    def _chunk(self, src_rows, h, w, first, video, f0, stripe=None, t=1):
        """Decoder3d.forward on `t` latent frames (VAE.py:677-728; the first chunk is always the single first frame); writes 1 or 4 t
        frames into `video`.  stripe = {stage: (a, b, ca, cb)}: rows [a, b) x columns [ca, cb) (relative to what it holds at that point) of
        the activation ENTERING that stage are kept and everything after works on that tile (`video` is then the tile's buffer); see
        stripe_plan."""
        c1 = self.conv1
        hip.vae_prep_cl(src_rows, c1.ci, t, h, w, c1.image(h, w), mode=0, t0=c1.hist)
        x = c1.run(t, h, w, out_dtype=F32)
        x = self._run_mid(x, t, h, w)
        for si, st in enumerate(self.stages):
            if stripe is not None and si in stripe:
                a, b, ca, cb = stripe[si]
                band = torch.zeros(t, b - a + 2, cb - ca + 2, x.shape[1], device=self.device, dtype=F32)
                band[:, 1:-1, 1:-1] = x.view(t, h + 2, w + 2, -1)[:, a + 1:b + 1, ca + 1:cb + 1]
                x, h, w = band.view(-1, x.shape[1]), b - a, cb - ca
            x_in, cin = x, x.shape[1]
            # the residual blocks update their input in place unless the first one has a shortcut convolution (a new tensor): only then
            # does x_in survive without a copy for the DupUp3D shortcut below
            main = x.clone() if (st.up and st.res[0].short is None) else x
            for r in st.res:
                main = r.run(main, t, h, w)
            if not st.up:
                x = main
                continue
            co, rs = st.cout, st.resample
            ft = 2 if st.temporal else 1
            y = None
            if st.temporal and not first:
                tc = st.time_conv
                hip.vae_prep_cl(main, co, t, h, w, tc.image(h, w), mode=0, t0=tc.hist)
                y = tc.run(t, h, w, out_dtype=BF16)                                        # [rows, 2*co]: frames 2i | 2i + 1 side by side
            t2 = 2 * t if y is not None else t
            if self.phase_up:                     # 2x2 phase convolutions on the low-resolution frames (_ConvUp2x), then interleave + shortcut
                if y is not None:
                    hip.deinterleave_cl(y, co, t, h, w, rs.image(h, w))
                else:
                    hip.vae_prep_cl(main, co, t, h, w, rs.image(h, w), mode=0, t0=0)
                ph = rs.run(t2, h, w)
                out = torch.empty(padded_rows(t2, 2 * h, 2 * w), co, device=self.device, dtype=F32)      # border rows: never read
                hip.phase_dupup_cl(ph, out, co, t2, 2 * h, 2 * w, x_in, cin, ft, (ft - 1) if first else 0)
            else:
                if y is not None:
                    hip.upsample2x_cl(y, co, t, h, w, rs.image(2 * h, 2 * w), interleave=True)
                else:
                    hip.upsample2x_cl(main, co, t, h, w, rs.image(2 * h, 2 * w), interleave=False)
                out = rs.run(t2, 2 * h, 2 * w, out_dtype=F32)
                hip.dupup_add_cl(out, co, t2, 2 * h, 2 * w, x_in, cin, ft, (ft - 1) if first else 0)
            x, t, h, w = out, t2, 2 * h, 2 * w
        hc = self.head_conv
        hip.vae_prep_cl(x, hc.ci, t, h, w, hc.image(h, w), mode=2, gamma=self.head_gamma, t0=hc.hist)
        y = hc.run(t, h, w, out_dtype=F32)                                                 # [rows, 12]
        hip.vae_unpatchify_clamp(y, t, h, w, video, f0)
        return t

    def _stage_cost(self):
        """Relative matrix work of a stage per pixel of ITS resolution and latent frame (weights of its convolutions x the frames the
        temporal upsamples before it have made): what band_grid weighs the stages with."""
        out, frames = [], 1
        for st in self.stages:
            n = sum(r.weight_elems() for r in st.res)
            if st.up:
                n += st.resample.weight_elems() * (1 if self.phase_up else 4)        # the image form runs at the upsampled resolution
                if st.temporal:
                    n += st.time_conv.weight_elems()
            out.append(n * frames)
            if st.temporal:
                frames *= 2
        return out

    # The tile plan of the parallel decode is vae_tiles': these hand it the stages' shape and work
    def _tile_stages(self):
        return [(st.up, len(st.res)) for st in self.stages]

    def band_grid(self, h: int, w: int, world: int):
        """(rows, columns) of the tile grid the parallel decode cuts the output into (vae_tiles.band_grid), cached per (h, w, world)."""
        key = (h, w, world)
        if key not in self._grid_cache:
            self._grid_cache[key] = vae_tiles.band_grid(self._tile_stages(), self._stage_cost(), h, w, world)
        return self._grid_cache[key]

    def stripe_plan(self, h: int, w: int, rank: int, world: int):
        """Tiles of the parallel decode for `rank` of `world`: which rows x columns of the activation ENTERING each stage this
        rank keeps so that its tile of the output comes out EXACT with no exchange (vae_tiles.stripe_plan on band_grid's grid).
        Returns (crops, (lo, hi, clo, chi), (gr, gc)): crops = {stage: (a, b, ca, cb)} relative to what is held when entering that stage;
        the tile's video has its own pixels at [lo, hi) x [clo, chi); rank = row * gc + column of the grid."""
        grid = self.band_grid(h, w, world)
        return vae_tiles.stripe_plan(self._tile_stages(), grid, h, w, rank)[:2] + (grid,)

    assemble_tiles = staticmethod(vae_tiles.assemble_tiles)

    @torch.no_grad()
    def decode(self, z: torch.Tensor, stripe=None) -> torch.Tensor:
        """z [zc, T, H, W] -> video [3, 1 + 4(T-1), 16H, 16W] fp32 in [-1, 1].
        stripe = (rank, world): only this rank's tile of the output, [3, F, 16H/gr, 16W/gc] with (gr, gc) = band_grid(H, W, world)."""
        zc, tz, h, w = z.shape
        for c in self._all_convs():
            c.reset()
        zi = self._plain_image("z", tz, h, w, self.conv2.cp)
        hip.pack_affine_cl(z.to(self.device, F32), self.std, self.mean, zi)                # z / (1/std) + mean
        x0 = hip.gemm(zi.view(-1, self.conv2.cp), self.conv2.weight, self.conv2.bias, out_dtype=F32)
        rows = padded_rows(1, h, w)
        scale = 2 ** (len(self.stages) - 1)
        tfac = 2 ** sum(self.temporal_up)
        frames = 1 + tfac * (tz - 1)
        if stripe is None or stripe[1] == 1:
            video = torch.empty(3, frames, h * scale * 2, w * scale * 2, device=self.device, dtype=F32)
            self._walk(x0, rows, tz, h, w, video, None)
            return video
        rank, world = stripe
        crops, (lo, hi, clo, chi), held = vae_tiles.stripe_plan(self._tile_stages(), self.band_grid(h, w, world), h, w, rank)
        band = torch.empty(3, frames, *held, device=self.device, dtype=F32)
        self._walk(x0, rows, tz, h, w, band, crops)
        return band[:, :, lo:hi, clo:chi].contiguous()

    def _walk(self, x0, rows, tz, h, w, video, stripe):
        """The chunk walk over the latent frames: frame 0 alone, then `self.chunk` frames at a time."""
        f0, i = 0, 0
        while i < tz:
            t = 1 if i == 0 else min(self.chunk, tz - i)
            f0 += self._chunk(x0[i * rows:(i + t) * rows], h, w, i == 0, video, f0, stripe=stripe, t=t)
            i += t


class _EncoderEngine(_EngineBase):
    """Encoder3d + conv1 + latent normalisation (VAE.py:505-618, :788-818), chunked 1 + 4 + 4 + ... frames."""

    def __init__(self, vae):
        sd, dev = self._setup(vae)
        cfg = vae._arch
        z2 = 2 * cfg["z_dim"]
        self.z2 = z2
        self.temporal_down = tuple(cfg["temporal_down"])
        dims = [cfg["enc_dim"] * m for m in [1] + list(cfg["dim_mult"])]
        self.dims = dims
        # Frames per chunk after the first (1-frame) chunk.  The reference walks the clip in chunks of 4 frames (VAE.py:1029-1037) to bound
        # memory; every convolution here is causal over its own input history, so the result does not depend on where the chunks are cut
        # (only on their being multiples of 4, which keeps the stride-2 time convolutions' frame pairs together).  Long chunks fill the
        # GPU in the low-resolution stages -- at 4 frames the 64 x 112 stage launches 150 tiles and the 32 x 56 stage 24 on 256 CUs --
        # and cut the launch count; 288 GB of HBM hold a whole 97-frame clip's activations.  FLEXAM_VAE_ENC_CHUNK=4 is the reference's walk.
        self.chunk = max(4, int(os.environ.get("FLEXAM_VAE_ENC_CHUNK", "48")) // 4 * 4)
        tcap = [self.chunk]
        for down in self.temporal_down:
            tcap.append(max(1, tcap[-1] // (2 if down else 1)))             # frames per chunk entering stage i
        tcap += [tcap[-1]] * (len(dims) - len(tcap))
        conv, res = self._mk_conv, self._mk_res
        self.conv1 = conv("encoder.conv1", tcap[0])
        self.stages = []
        n_stage = len(dims) - 1
        for i in range(n_stage):
            p = f"encoder.downsamples.{i}.downsamples"
            blocks, resample, time_conv = [res(f"{p}.{j}", tcap[i]) for j in range(2)], None, None
            if i != n_stage - 1:
                resample = _ConvS2D(sd[f"{p}.2.resample.1.weight"], sd[f"{p}.2.resample.1.bias"], dev, tcap[i])
                time_conv = conv(f"{p}.2.time_conv", tcap[i]) if i < len(self.temporal_down) and self.temporal_down[i] else None
            self.stages.append(_DownStage(blocks, dims[i + 1], resample, time_conv))
        t_last = tcap[n_stage - 1] if n_stage - 1 < len(tcap) else 1
        self.mid = self._mk_mid("encoder.middle", dims[-1], t_last)
        self.head_gamma = _f32(sd["encoder.head.0.gamma"], dev)
        # head conv (C -> 2z) followed by conv1 (1x1x1, 2z -> 2z) and (mu - mean) / std: one linear map, folded in fp32
        w1 = sd["conv1.weight"].detach().to(dev, F32).reshape(z2, z2)
        b1 = sd["conv1.bias"].detach().to(dev, F32)
        wh = sd["encoder.head.2.weight"].detach().to(dev, F32)
        bh = sd["encoder.head.2.bias"].detach().to(dev, F32)
        inv_std = torch.ones(z2, device=dev, dtype=F32)
        mean = torch.zeros(z2, device=dev, dtype=F32)
        inv_std[:z2 // 2] = 1.0 / torch.tensor(vae.latent_std, device=dev, dtype=F32)
        mean[:z2 // 2] = torch.tensor(vae.latent_mean, device=dev, dtype=F32)
        wf = torch.einsum("oc,cikhw->oikhw", w1, wh) * inv_std.view(-1, 1, 1, 1, 1)
        bf = (w1 @ bh + b1 - mean) * inv_std
        self.head_conv = _Conv(wf, bf, dev, t_last)
        del self.sd

    def _chunk(self, video, f0, t, h, w, first):
        """Encoder3d.forward (VAE.py:564-618) on frames f0..f0+t of `video`; returns rows [t'*(h'+2)*(w'+2), 2z] fp32."""
        c1 = self.conv1
        hip.vae_patchify_cl(video, f0, t, c1.image(h, w), t0=c1.hist)
        x = c1.run(t, h, w, out_dtype=F32)
        for st in self.stages:
            x_in, cin, t_in = x, x.shape[1], t
            co = st.cout
            # Stage 0 (same width in and out, spatial downsample only): the AvgDown3D shortcut is taken FIRST, into the buffer the
            # stride-2 convolution then adds its result to (fp32 residual epilogue) -- the residual blocks can overwrite x in place, and
            # neither a copy of x (0.3 GB per 4 frames at 256 x 448) nor a second pass over the downsampled rows is needed
            fold = st.down and not st.temporal and st.res[0].short is None and cin == co
            if fold:
                short = torch.zeros(padded_rows(t, h // 2, w // 2), co, device=self.device, dtype=F32)
                hip.avgdown_add_cl(short, co, t, h // 2, w // 2, x_in, cin, t_in, 1, 2)
                main = x
            else:
                main = x.clone() if st.res[0].short is None else x
            for r in st.res:
                main = r.run(main, t, h, w)
            if st.down:
                ds = st.resample
                h, w = h // 2, w // 2
                hip.space_to_depth_cl(main, co, t, 2 * h, 2 * w, ds.image(h, w), ds.cs)
                if fold:
                    x = ds.run(t, h, w, residual_into=short)
                    continue
                main = ds.run(t, h, w, out_dtype=F32)
                if st.temporal:
                    tc = st.time_conv
                    hip.vae_prep_cl(main, co, t, h, w, tc.image(h, w), mode=0, t0=tc.hist)
                    if first:
                        tc.roll(t)                                          # first chunk: the frame is only cached (VAE.py:165-166)
                    else:
                        main = tc.run_time_stride2(t, h, w, out_dtype=F32)
                        t //= 2
            hip.avgdown_add_cl(main, co, t, h, w, x_in, cin, t_in, 2 if st.temporal else 1, 2 if st.down else 1)
            x = main
        x = self._run_mid(x, t, h, w)
        hc = self.head_conv
        hip.vae_prep_cl(x, hc.ci, t, h, w, hc.image(h, w), mode=2, gamma=self.head_gamma, t0=hc.hist)
        return hc.run(t, h, w, out_dtype=F32), t, h, w

    @torch.no_grad()
    def encode(self, x: torch.Tensor) -> torch.Tensor:
        """x [3, 1 + 4k, H, W] in [-1, 1] -> [2z, 1 + k, H/16, W/16] fp32: normalised mu | log_var."""
        c, frames, hh, ww = x.shape
        n_down = sum(1 for st in self.stages if st.down)
        if c != 3 or hh % (2 << n_down) or ww % (2 << n_down):
            raise ValueError(f"encode: expected [3, F, H, W] with H, W multiples of {2 << n_down}, got {tuple(x.shape)}")
        for cv in self._all_convs():
            cv.reset()
        video = x.to(self.device, F32).contiguous()
        h, w = hh // 2, ww // 2
        frames = 1 + (frames - 1) // 4 * 4                 # trailing frames past 1 + 4k are not encoded (VAE.py:1029: iter_ = 1 + (t - 1) // 4)
        outs, t_out, f0 = [], 0, 0
        while f0 < frames:
            t = 1 if f0 == 0 else min(self.chunk, frames - f0)
            rows, to, ho, wo = self._chunk(video, f0, t, h, w, f0 == 0)
            outs.append(rows)
            t_out += to
            f0 += t
        return hip.unpack_cl(torch.cat(outs) if len(outs) > 1 else outs[0], self.z2, t_out, ho, wo)


class AutoencoderKLWan3_8(nn.Module):
    def __init__(self, latent_channels=48, c_dim=160, vae_pth=None, dim_mult=[1, 2, 4, 4], temperal_downsample=[False, True, True],
                 temporal_compression_ratio=4, spatial_compression_ratio=8, dec_dim=256):
        super().__init__()
        self.config = ModelConfig(latent_channels=latent_channels, c_dim=c_dim, vae_pth=vae_pth, dim_mult=list(dim_mult),
                                  temperal_downsample=list(temperal_downsample), temporal_compression_ratio=temporal_compression_ratio,
                                  spatial_compression_ratio=spatial_compression_ratio)
        self.latent_channels = latent_channels
        self.temporal_compression_ratio = temporal_compression_ratio
        self.spatial_compression_ratio = spatial_compression_ratio
        self.latent_mean, self.latent_std = LATENT_MEAN[:latent_channels], LATENT_STD[:latent_channels]
        if latent_channels != len(LATENT_MEAN):
            self.latent_mean, self.latent_std = [0.0] * latent_channels, [1.0] * latent_channels
        temporal_up = list(temperal_downsample)[::-1]
        self._arch = dict(z_dim=latent_channels, dec_dim=dec_dim, enc_dim=c_dim, dim_mult=tuple(dim_mult), temporal_up=tuple(temporal_up),
                          temporal_down=tuple(temperal_downsample))
        self.model = _ParamTree()
        for name, shape in encoder_param_shapes(latent_channels, c_dim, tuple(dim_mult), tuple(temperal_downsample)).items():
            self.model.add(name, shape)
        for name, shape in decoder_param_shapes(latent_channels, dec_dim, tuple(dim_mult), tuple(temporal_up)).items():
            self.model.add(name, shape)
        self.supports_encode = True
        self._engine: Optional[_DecoderEngine] = None
        self._enc_engine: Optional[_EncoderEngine] = None
        self._parallel_group, self._parallel = None, False

    def _apply(self, fn, *a, **k):
        self._engine = self._enc_engine = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._engine = self._enc_engine = None
        return super().load_state_dict(*a, **k)

    @property
    def dtype(self):
        return next(self.model.parameters()).dtype

    @property
    def device(self):
        return next(self.model.parameters()).device

    def engine(self) -> _DecoderEngine:
        if self._engine is None:
            self._engine = _DecoderEngine(self)
        return self._engine

    def enable_parallel_decode(self, group=None):
        """Tiled decode over the ranks of `group` (replaces the reference's missing `parallel_magvit_vae`,
        FlexAM/models/__init__.py:36-38): every rank decodes 1/N of the output pixels -- a tile of a rows x columns grid -- exactly
        (see vae_tiles) and one all-gather assembles the clip."""
        self._parallel_group, self._parallel = group, True

    def disable_parallel_decode(self):
        self._parallel_group, self._parallel = None, False

    def _decode_one(self, eng, u):
        import torch.distributed as dist
        world = dist.get_world_size(self._parallel_group) if (self._parallel and dist.is_initialized()) else 1
        if world == 1:
            return eng.decode(u)
        band = eng.decode(u, stripe=(dist.get_rank(self._parallel_group), world))
        bands = [torch.empty_like(band) for _ in range(world)]
        dist.all_gather(bands, band, group=self._parallel_group)
        return vae_tiles.assemble_tiles(bands, eng.band_grid(u.shape[-2], u.shape[-1], world))

    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = True):
        """VAE.py:1041-1056: per sample chunked decode, clamp(-1, 1)."""
        eng = self.engine()
        out = torch.stack([self._decode_one(eng, u) for u in z])
        if z.dtype == BF16:
            out = out.to(BF16)
        return DecoderOutput(out) if return_dict else (out,)

    def encoder_engine(self) -> _EncoderEngine:
        if self._enc_engine is None:
            self._enc_engine = _EncoderEngine(self)
        return self._enc_engine

    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """VAE.py:1021-1039: per sample chunked encode -> DiagonalGaussianDistribution([normalised mu | log_var])."""
        eng = self.encoder_engine()
        h = torch.stack([eng.encode(u) for u in x])
        if x.dtype == BF16:
            h = h.to(BF16)
        posterior = DiagonalGaussianDistribution(h)
        return AutoencoderKLOutput(latent_dist=posterior) if return_dict else (posterior,)

    @classmethod
    def from_pretrained(cls, pretrained_model_path, additional_kwargs={}):
        """VAE.py:1059-1079: raw Wan2.2_VAE.pth keys are prefixed with 'model.'; strict=False."""
        import inspect
        allowed = set(inspect.signature(cls.__init__).parameters) - {"self"}
        model = cls(**{k: v for k, v in additional_kwargs.items() if k in allowed})
        if pretrained_model_path.endswith(".safetensors"):
            from safetensors.torch import load_file
            state = load_file(pretrained_model_path)
        else:
            state = torch.load(pretrained_model_path, map_location="cpu")
        m, u = model.load_state_dict({"model." + k: v for k, v in state.items()}, strict=False)
        print(f"### missing keys: {len(m)}; \n### unexpected keys: {len(u)};")
        return model
