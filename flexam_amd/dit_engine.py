"""HIP execution engine of the FlexAM DiT (Wan2.2-Fun-5B-FLEXAM) on one MI355X, optionally one
shard of a sequence-parallel group.

What the reference does per denoise step in wan_transformer3d_FlexAM.py:817-1123 is split here by
how often it changes:

  per clip   (`set_conditioning`)  cnn-block over the control/depth/cos latents (:869-881), the
             100 step-invariant input channels of the patch embedding (:883-885), ref_conv tokens
             (:895-899), text embedding (:958-964) and every block's cross-attention K/V
             (:364-365), density embedding (:950-955), RoPE rows (:137-164)
  per step   (`run`)  48-channel patchify + patch GEMM, the time-embedding MLP on the DISTINCT
             timesteps only (two rows in the sampler: frame-0 tokens have t = 0, PIPE.py:891-898),
             one AdaLN table for all blocks, 30 blocks, head

Data layout in HBM (per rank): residual stream x fp32 [B*Lc, C] (token-major, rows of 12 KiB);
GEMM operands bf16 row-major with K contiguous; q|k|v of a block in one [B*Lc, 3C] buffer (heads
packed along the row, so attention addresses head h at column h*128); AdaLN rows are looked up per
token through an int32 row index instead of the reference's materialised [B, L, 6, C] fp32 tensor.
All arithmetic runs in libflexam_hip.so (flexam_amd/hip.py); torch only allocates and slices.
"""
import math
import os
from contextlib import nullcontext
from typing import List, Optional

import torch

from . import hip
from .dit_layout import (SINGLE_RANK, halo_plan, resolve_mode, resolve_parallel, sage_asked, sage_window_asked, smooth_k_asked, smooth_v_asked,
                         sp_halo_asked, sp_sage_window_asked, sp_window_asked)
from .dit_sp import HeadAllToAll, KVGather, KVHalo, RecordGather
from .implicit_conv import GuardedImage, PackedConv, Tap, pad_k, reach, round_up
from .rope import rope_angle_table, rope_tables

BF16, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
F8 = torch.float8_e4m3fn


def _conv_cl(weight: torch.Tensor, bias: torch.Tensor, device) -> PackedConv:
    """A (1,kh,kw) convolution of the cnn-block as an implicit GEMM over a padded channels-last image (GuardedImage).  K order
    (dh, dw, channel block): tap-major, every tap a group of its own."""
    co, ci = weight.shape[0], weight.shape[1]
    kh, kw = weight.shape[-2], weight.shape[-1]
    groups = [[Tap(0, dh - kh // 2, dw - kw // 2)] for dh in range(kh) for dw in range(kw)]
    return PackedConv(weight.detach().to(device, F32).reshape(co, ci, kh * kw).permute(0, 2, 1), groups, bias, device)


def _fp8_weight(pk: dict, name: str):
    """(e4m3 bytes, per-output-channel scales) of pack entry `name`, quantised once per pack (the pack is rebuilt when a parameter
    changes): the one store behind DiTEngine.enable_fp8 and the blocks called as modules."""
    key = "_f8_" + name
    if key not in pk:
        w = pk[name]
        pk[key] = hip.quantize_rows_fp8(w.to(BF16) if w.dtype == F8 else w)     # (qfloat8 storage: one matrix upcast at a time)
    return pk[key]


# the pack that owns each fp8 weight: the self- / cross-attention module's (a block pack's "sa" / "ca", which those modules ask when the
# block is called as a module) or the block's own (None)
_FP8_OWNER = dict(wqkv="sa", wo="sa", cwq="ca", cwo="ca", w1=None, w2=None)


def _proj_fp8(h: torch.Tensor, pk: dict, wname: str, bias, epilogue: int = 0) -> torch.Tensor:
    """h [M, K] bf16 -> bf16 [M, N] on the fp8 (OCP e4m3) MFMA path: rows of h quantised per call (absmax / 448), weights per output channel,
    fp32 accumulation, scales / bias / activation in the epilogue (csrc/gemm_fp8.hip) -- the module-seam form of DiTEngine.enable_fp8."""
    a8, sa = hip.quantize_rows_fp8(h)
    w8, sw = _fp8_weight(pk, wname)
    return hip.gemm_fp8(a8, sa, w8, sw, bias, epilogue=epilogue)


class DiTEngine:
    _sage_warned = False
    _smooth_k_warned = False
    _smooth_v_warned = False
    _sage_window_warned = False
    _sp_window_overlap_warned = False
    _sp_halo_warned = False

    def __init__(self, model):
        self.model = model
        c = model.config
        self.dim, self.ffn, self.nh, self.nl = c["dim"], c["ffn_dim"], c["num_heads"], c["num_layers"]
        self.hd = self.dim // self.nh
        self.eps = c["eps"]
        self.patch = tuple(c["patch_size"])
        self.out_dim, self.in_dim = c["out_dim"], c["in_dim"]
        self.text_len, self.freq_dim = c["text_len"], c["freq_dim"]
        # flash-attn's (left, right) window of the self-attention in tokens, (-1, -1) = none (the model's window_size, as the reference's
        # WanSelfAttention hands it to its kernel); kept beside the mode like smooth-K / smooth-V, and part of a launch plan's key
        self.window = hip.attn_window(c["window_size"])
        # under a window: the first window_sink tokens stay visible to every query (the model's window_sink); in the plan's key too
        self.window_sink = int(c["window_sink"])
        # the window counted in frames of the clip's token grid instead (the model's window_frames; never together with window_size): served
        # by the same windowed kernel, refused and warned about like a token window; with the frame's tokens part of a launch plan's key
        self.window_frames = hip.attn_window(c["window_frames"])
        if self.hd != hip.ATTN_HEAD_DIM:
            raise RuntimeError(f"flexam_amd: head_dim {self.hd} unsupported by the HIP attention kernel ({hip.ATTN_HEAD_DIM} only)")
        if self.patch != (1, 2, 2):
            raise RuntimeError("flexam_amd: only patch_size (1,2,2) is implemented")
        self.device = model.patch_embedding.weight.device
        if self.device.type != "cuda":
            raise RuntimeError("flexam_amd: the DiT runs only on a GPU through libflexam_hip.so "
                               "(no CPU or eager fallback); move the model to cuda first")
        hip.device_check()
        self.sp_group = None
        self.sp_rank, self.sp_size = 0, 1
        self.sp_mode, self.sp_overlap_level, self.sp_pieces, self.sp_fused_qkv = SINGLE_RANK
        self.sp_overlap = False
        self.world_group, self.world_size = None, 1
        self.cfg_size, self.cfg_row = 1, 0          # cfg_size 2: this rank computes only CFG row `cfg_row`
        self._ws = {}
        self._attn8 = {}                            # MXFP8 operand buffers of the quantised self-attention (_attn8_buffers)
        self._kmean = {}                            # smooth-K: K's token mean and the scratch of its parts (_k_mean_buffers)
        self._vmean = {}                            # smooth-V: the same pair for V's token mean
        self._smooth_k = self.sage_smooth_taken = False
        self._smooth_v = self.sage_smooth_v_taken = False
        self._ws_gen = 0                            # bumped whenever the activation buffers are dropped: recorded launch plans name their addresses
        self._angles = None
        self.cond = None
        self.n_conditioning = 0                     # set_conditioning runs so far (tests: the per-clip work is hoisted)
        # AdaLN tables of all layers are built in one launch per step ([layers, R, 6, C] fp32, R = distinct timesteps x batch);
        # beyond this many bytes (masks with fractional edges: hundreds of distinct timesteps) ONE [R, 6, C] table is rebuilt
        # per layer instead -- the reference's own footprint is [B, L, 6, C] per step (wan_transformer3d_FlexAM.py:944)
        self.table_limit = 1 << 30
        self.fp8 = False                            # BASELINE configs[4]: QKV / FFN GEMMs on fp8 MFMA (enable_fp8)
        self._fp8_w = None
        self.fp8_modules = False                    # fp8 GEMMs inside blocks that are called as modules (not the fused path): enable_fp8
        self._pack()

    # ------------------------------------------------------------------ weights
    def _pack(self):
        m, dev, d = self.model, self.device, self.dim
        bf = lambda t: t.detach().to(dev, BF16).contiguous()
        f32 = lambda t: t.detach().to(dev, F32).contiguous()
        # (qfloat8 storage, fp8_optimization.py: the e4m3 parameters outside the blocks -- embeddings, head, conv taps, biases and
        # norm rows -- are upcast here once, exactly; the block GEMM weights stay e4m3 in their packs, _Block.packed)
        small = lambda t: t.detach().to(dev).contiguous() if t.dtype in (BF16, F32) else (bf(t) if t.dtype == F8 else f32(t))
        self.pe_w, self.pe_b = pad_k(m.patch_embedding.weight.flatten(1), dev), f32(m.patch_embedding.bias)
        self.ref_w = self.ref_b = None
        if m.ref_conv is not None:
            self.ref_w, self.ref_b = pad_k(m.ref_conv.weight.flatten(1), dev), f32(m.ref_conv.bias)
        self.head_w, self.head_b = bf(m.head.head.weight), f32(m.head.head.bias)
        self.txt = [(pad_k(m.text_embedding[0].weight, dev), f32(m.text_embedding[0].bias)),
                    (bf(m.text_embedding[2].weight), f32(m.text_embedding[2].bias))]
        self.time = [(small(l.weight), f32(l.bias)) for l in (m.time_embedding[0], m.time_embedding[2], m.time_projection[1])]
        self.dens = [(small(l.weight), f32(l.bias)) for l in (m.density_embedding[0], m.density_embedding[2], m.density_projection[1])]
        # per-layer parameter packs live on the block modules (`_Block.packed()`: fused q|k|v and cross k|v buffers that the
        # parameters alias, softmax_scale * log2(e) folded into norm_q for the FLEXAM_ATTN_PRESCALED attention form); a block that
        # was replaced (`transformer.blocks[i] = wrapper`, comfyui_nodes.py:67-71) or whose forward / attention forward was
        # re-bound (wan_transformer3d_FlexAM.py:807-815) has no pack here and is CALLED as a module by run()
        self.blocks, self.block_modules = [], list(m.blocks)
        for blk in m.blocks:
            blk = getattr(blk, "_orig_mod", blk)          # torch.compile(block) wraps the same module: nothing to compile in a HIP-call block
            native = hasattr(blk, "packed") and hasattr(blk, "pristine") and blk.pristine()
            self.blocks.append(blk.packed() if native else None)
        self.fused = all(p is not None for p in self.blocks)
        nat = [p for p in self.blocks if p is not None]
        self.mod = torch.stack([p["mod"] for p in nat]) if self.fused else None                # [nl, 6, d]
        self.mdens = torch.stack([p["mdens"] for p in nat]) if self.fused else None           # [nl, 2, d]
        self.hmod, self.hmdens = f32(m.head.modulation), f32(m.head.modulation_density)       # [1,2,d], [1,1,d]
        self.cnn = None
        if m.cnn_conv1 is not None:
            cin = [round_up(m.cnn_conv1[0].weight.shape[1], 64), 192, 192, 128, 128]         # pixel widths of conv1..5's input images
            self.cnn = dict(
                convs=[_conv_cl(getattr(m, f"cnn_conv{i}")[0].weight, getattr(m, f"cnn_conv{i}")[0].bias, dev) for i in range(1, 5)],
                gn=[(f32(getattr(m, f"cnn_conv{i}")[1].weight), f32(getattr(m, f"cnn_conv{i}")[1].bias)) for i in range(1, 5)],
                conv5=_conv_cl(m.cnn_conv5.weight, m.cnn_conv5.bias, dev), groups=[24, 24, 12, 12], cp=cin)

    def set_parallel(self, sp_group, sp_rank: int, sp_size: int, world_group=None, world_size: int = None, cfg_size: int = 1,
                     cfg_row: int = 0):
        """Parallel layout of this rank: token chunk `sp_rank` of `sp_size` inside `sp_group`; with cfg_size = 2 the
        world is two such groups, one per CFG row (world rank = cfg_row * sp_size + sp_rank)."""
        self.sp_group, self.sp_rank, self.sp_size = sp_group, sp_rank, sp_size
        self.sp_mode, self.sp_overlap_level, self.sp_pieces, self.sp_fused_qkv = resolve_parallel(os.environ, self.nh, sp_size)
        self.sp_overlap = self.sp_overlap_level != 0
        # FLEXAM_CU_BUDGET=<n>: plan the persistent grids for n CUs (a multiple of 8) while this layout runs collectives beside compute --
        # a kernel that owns every CU leaves a collective's own kernels nowhere to run until it ends.  Not set by default: on one GPU
        # the emulation's stand-in (a single delay wave) finds room beside the GEMMs, and 8 CUs cost 3 % of a rank's step
        # (profiles/r6s_*); what RCCL's kernels need on a real node is the first thing to measure there.
        if os.environ.get("FLEXAM_CU_BUDGET"):
            hip.set_cu_budget(int(os.environ["FLEXAM_CU_BUDGET"]) if sp_size > 1 else 0)
        self.world_group = world_group if cfg_size > 1 else sp_group
        self.world_size = world_size if world_size is not None else sp_size
        self.cfg_size, self.cfg_row = cfg_size, cfg_row
        self._ws.clear()
        self._ws_gen += 1

    def enable_fp8(self, on: bool = True):
        """QKV (self-attention q|k|v, cross-attention q) and FFN projections on the fp8 (OCP e4m3) MFMA path: weights quantised once per output channel, activations per
        row and per call (flexam_quantize_rows_fp8), fp32 accumulation, the same fused epilogues.  Attention, the output / cross
        projections, norms, modulation and the residual stream are unchanged.  BASELINE.json configs[4] ("fp8 MFMA QKV/FFN
        variant"); the reference's own fp8 mode only stores weights in fp8 (FlexAM/utils/fp8_optimization.py:1-57)."""
        if not self.fused:
            # some block is replaced / wrapped / re-bound: every block is CALLED as a module and carries the switch itself
            # (_Block.set_fp8, set by model.enable_fp8_gemm on every native block, also inside wrappers) -- the same GEMMs on the fp8 pipe
            # with absmax row scales; the engine only has to keep its own fused-path state out of the way
            for blk in self.model.modules():
                if hasattr(blk, "set_fp8"):
                    blk.set_fp8(on)
            self.fp8 = False
            self.fp8_modules = bool(on)
            return
        # wo / cwo are quantised too: FLEXAM_FP8_OPROJ=1 (read per forward; an experiment, not part of configs[4]'s "QKV/FFN") runs the
        # self-attention and cross-attention output projections on the fp8 pipe as well -- the attention output is row-quantised by one
        # more pass (flexam_quantize_rows_fp8)
        if on and self._fp8_w is None:
            self._fp8_w = []
            for p in self.blocks:
                q = {}
                for name in ("wqkv", "cwq", "w1", "w2", "wo", "cwo"):
                    q[name], q["s_" + name] = _fp8_weight(p[_FP8_OWNER[name]] if _FP8_OWNER[name] else p, name)
                # bounds for the a-priori scale of FFN1's e4m3 output (flexam_ln_modulate_fp8, next_scale): the largest L2 norm of a
                # DEQUANTISED w1 row (what the MFMA multiplies) and the largest |bias|; two floats per layer, read back once
                deq = q["w1"].view(torch.float8_e4m3fn).float() * q["s_w1"][:, None]
                q["w1_norm"] = float(deq.norm(dim=1).max()) * 1.001
                q["b1_max"] = float(p["b1"].abs().max()) if p["b1"] is not None else 0.0
                del deq
                self._fp8_w.append(q)
        self.fp8 = bool(on)
        self._ws.clear()
        self._ws_gen += 1

    def _ln_fp8(self, xres, ws, hbuf, nxt=None, **kw):
        """LN + modulate as the fp8 GEMMs' A operand: one launch at widths the wave-per-row kernel covers (multiples of 512, the 5B
        model's 3072), the bf16 row kernel followed by the row quantiser otherwise.  nxt = (w_norm_max, bias_max) of the GEMM the
        rows feed: the launch then also writes the a-priori output scales of that GEMM into ws["so"] (fused form only; returns
        whether it did)."""
        d, m = self.dim, xres.shape[0]
        if d % 512 == 0 and d <= 4096:
            if nxt is not None:
                hip.ln_modulate_fp8(xres, ws["a8d"][:m], ws["sa"][:m], eps=self.eps, next_scale=ws["so"][:m], next_wnorm=nxt[0], next_bias=nxt[1], **kw)
                return ws["a8d"][:m], ws["sa"][:m], True
            a8, sa = hip.ln_modulate_fp8(xres, ws["a8d"][:m], ws["sa"][:m], eps=self.eps, **kw)
            return a8, sa, False
        hip.ln_modulate(xres, out=hbuf, eps=self.eps, **kw)
        a8, sa = hip.quantize_rows_fp8(hbuf, ws["a8d"][:m], ws["sa"][:m])
        return a8, sa, False

    def set_sequence_parallel(self, group, rank: int, size: int):
        self.set_parallel(group, rank, size)

    # ------------------------------------------------------------------ per-clip state
    def _cnn_block(self, control: torch.Tensor, additional: torch.Tensor) -> torch.Tensor:
        """control [Cc,F,H,W], additional [Ca,F,H,W] -> cnn output [Co,F,H,W] fp32 (FX.py:869-880)."""
        dev = self.device
        _, f, h, w = control.shape
        cn = self.cnn
        rows = f * (h + 2) * (w + 2)
        image = lambda cp: GuardedImage(f, h, w, cp, dev, reach(w, cp), reach(w, cp))

        def conv(c, img):
            c.at(h + 2, w + 2, img.img.shape[-1])
            return c.launch(img.mat, rows)
        img = image(cn["cp"][0])
        hip.pack_cl(control.contiguous(), img.img, 0)
        hip.pack_cl(additional.contiguous(), img.img, control.shape[0])
        for i, c in enumerate(cn["convs"]):
            y = conv(c, img)
            nxt = image(cn["cp"][i + 1])
            gamma, beta = cn["gn"][i]
            residual = img.img if i in (1, 3) else None                   # x2 = conv2(x1) + x1, x4 = conv4(x3) + x3
            hip.groupnorm_silu_cl(y, c.co, f, h, w, cn["groups"][i], gamma, beta, nxt.img, residual=residual)
            img = nxt
        return hip.unpack_cl(conv(cn["conv5"], img), cn["conv5"].co, f, h, w)

    def set_conditioning(self, context: List[torch.Tensor], y: Optional[torch.Tensor], full_ref: Optional[torch.Tensor],
                         additional_control: Optional[torch.Tensor], density: Optional[torch.Tensor], latent_shape,
                         shared: bool = False):
        """Computes everything that does not depend on the noisy latent or the timestep.
        context: list of B tensors [len_i, text_dim]; y [By, 100, F, H, W]; full_ref [By, 48, H, W];
        additional_control [By, 240, F, H, W]; density [B].  shared=True: conditioning tensors have
        batch 1 and are shared by all B rows (the sampler's CFG pair differs only in `context`)."""
        dev, d = self.device, self.dim
        B = len(context)
        cx, f, h, w = latent_shape
        lvid = f * (h // 2) * (w // 2)
        ref_len = (h // 2) * (w // 2) if (full_ref is not None and self.ref_w is not None) else 0
        L = lvid + ref_len
        nb = 1 if shared else B
        kpe = self.pe_w.shape[1]
        patch_a = torch.zeros(nb, lvid, kpe, device=dev, dtype=BF16)
        ref_tok = torch.empty(nb, ref_len, d, device=dev, dtype=F32) if ref_len else None
        if y is not None:
            for b in range(nb):
                yb = y[b].to(dev)
                if self.cnn is not None and additional_control is not None:
                    cnn_out = self._cnn_block(yb[:cx].float(), additional_control[b].to(dev).float())
                    hip.patchify(cnn_out, patch_a[b], col0=cx * 4)
                    rest = yb[cx:].float().contiguous()
                    hip.patchify(rest, patch_a[b], col0=(cx + cnn_out.shape[0]) * 4)
                else:
                    hip.patchify(yb.float().contiguous(), patch_a[b], col0=cx * 4)
        if ref_len:
            kr = self.ref_w.shape[1]
            for b in range(nb):
                ra = torch.zeros(ref_len, kr, device=dev, dtype=BF16)
                hip.patchify(full_ref[b].to(dev).float().unsqueeze(1).contiguous(), ra)
                # the reference's conv output is bf16 (autocast); keep that rounding for the tokens
                hip.gemm(ra, self.ref_w, self.ref_b, out=ref_tok[b], out_dtype=F32)
        # text -> context embedding -> per-block cross K (normalised) and V
        tdim = self.txt[0][0].shape[1]
        ctx_in = torch.zeros(B * self.text_len, tdim, device=dev, dtype=BF16)
        n_max = 0
        for b, u in enumerate(context):
            n = min(u.shape[0], self.text_len)
            n_max = max(n_max, n)
            ctx_in[b * self.text_len:b * self.text_len + n, :u.shape[1]] = u[:n].to(dev, BF16)
        # Rows n_max .. text_len - 1 of EVERY sample are zero before the text MLP (the reference pads the same way, FX.py:958-964),
        # so behind it they are one and the same context row and, per block, one and the same K / V row: cross-attention keeps the
        # first of them and counts it text_len - n_max times (flexam_attn_fwd_lastkey) instead of attending to 386 copies
        cross_lk, cross_mult = None, 1.0
        if n_max + 1 < self.text_len and os.environ.get("FLEXAM_CROSS_DEDUP", "1") != "0":
            cross_lk, cross_mult = n_max + 1, float(self.text_len - n_max)
        hmid = hip.gemm(ctx_in, self.txt[0][0], self.txt[0][1], epilogue=hip.EPI_GELU_TANH)
        ctx = hip.gemm(hmid, self.txt[1][0], self.txt[1][1])
        cross_kv = []
        for p in (self.blocks if self.fused else ()):
            kv = hip.gemm(ctx, p["cwkv"], p["cbkv"])
            hip.rmsnorm_rope(kv[:, :d], p["cnk"], eps=self.eps)
            cross_kv.append(kv.view(B, self.text_len, 2 * d))
        # density embedding
        dens_emb = dens0 = None
        if density is not None:
            s = hip.sinusoid_embed(density.to(dev, F32).reshape(-1), self.freq_dim)
            e1 = hip.small_linear(s, *self.dens[0])
            dens_emb = hip.small_linear(e1, *self.dens[1], silu_in=True)
            dens0 = hip.small_linear(dens_emb, *self.dens[2], silu_in=True).view(B, 2, d)
        # all samples carry the same density (the sampler's CFG pair does): part of what lets block 0 share its self-attention half
        dens_same = dens0 is None or B == 1 or bool((dens0 == dens0[:1]).all())
        grid = (f + (1 if ref_len else 0), h // 2, w // 2)
        if self._angles is None:
            self._angles = self.model._rope_angles()
        cos, sin = rope_tables(grid, L, self.hd, self._angles)
        self.cond = dict(B=B, nb=nb, L=L, lvid=lvid, ref_len=ref_len, latent_shape=(cx, f, h, w), patch_a=patch_a, ref_tok=ref_tok,
                         cross_kv=cross_kv, dens_emb=dens_emb, dens0=dens0, cos=cos.to(dev), sin=sin.to(dev),
                         ctx=ctx.view(B, self.text_len, d), grid=grid, dens_same=dens_same, cross_lk=cross_lk, cross_mult=cross_mult)
        self.n_conditioning += 1
        return self.cond

    # ------------------------------------------------------------------ workspace
    def _workspace(self, B, lc):
        """Activation buffers of one run.  Buffers of other shapes are dropped when a new shape arrives."""
        key = (B, lc)
        if key not in self._ws:
            dev, d, m = self.device, self.dim, B * lc
            self._ws = {}
            self._ws_gen += 1
            self._ws[key] = dict(
                x=torch.empty(m, d, device=dev, dtype=F32), h=torch.empty(m, d, device=dev, dtype=BF16),
                qkv=torch.empty(m, 3 * d, device=dev, dtype=BF16), ao=torch.empty(m, d, device=dev, dtype=BF16),
                ffn=torch.empty(m, self.ffn, device=dev, dtype=BF16),
                head=torch.empty(m, self.head_w.shape[0], device=dev, dtype=F32))
            if self.fp8:
                self._ws[key].update(a8=torch.empty(m, self.ffn, device=dev, dtype=torch.uint8), sa=torch.empty(m, device=dev, dtype=F32),
                                     a8d=torch.empty(m, d, device=dev, dtype=torch.uint8), so=torch.empty(m, device=dev, dtype=F32))
        return self._ws[key]

    def _attn8_buffers(self, nb, lc, heads=None):
        """MXFP8 operand buffers of the quantised self-attention (one set per (samples, tokens, heads) shape, reused by every block)."""
        cache = self._attn8
        heads = self.nh if heads is None else heads
        if (nb, lc, heads) not in cache:
            if any(k[1:] != (lc, heads) for k in cache):          # another token / head count: drop the old sets (as _workspace does)
                cache.clear()
            cache[(nb, lc, heads)] = hip.attn_fp8_buffers(nb, heads, lc, self.device)      # (block 0 may run one sample: its own set, not a re-allocation per step)
        return cache[(nb, lc, heads)]

    def _k_mean_buffers(self, nb, lc, of_v=False):
        """(mean fp32 [nb, dim], scratch fp32 [nb, parts, dim]) of hip.k_mean under FLEXAM_SAGE_SMOOTH_K (of_v: FLEXAM_SAGE_SMOOTH_V, a
        pair of its own: V's mean lives until the attention has added it back), cached as _attn8_buffers caches the operands: one set
        per (samples, heads), block 0's one-sample run under share0 its own."""
        cache = self._vmean if of_v else self._kmean
        if (nb, lc, self.nh) not in cache:
            if any(k[1:] != (lc, self.nh) for k in cache):
                cache.clear()
            cache[(nb, lc, self.nh)] = (torch.empty(nb, self.dim, device=self.device, dtype=F32),
                                        torch.empty(nb, hip.k_mean_parts(lc), self.dim, device=self.device, dtype=F32))
        return cache[(nb, lc, self.nh)]

    # ------------------------------------------------------------------ per-step
    def embed_time(self, t_rows: torch.Tensor):
        """t_rows [R] fp32 distinct timesteps -> e [R, d], e0 [R, 6, d] (fp32, FX.py:928-944)."""
        R, d = t_rows.numel(), self.dim
        s = hip.sinusoid_embed(t_rows.to(self.device, F32), self.freq_dim)
        e = torch.empty(R, d, device=self.device, dtype=F32)
        e0 = torch.empty(R, 6 * d, device=self.device, dtype=F32)
        step = 8 if R <= 8 else 32                 # rows per pass over the 113 MB projection weight (results do not depend on it)
        for i in range(0, R, step):
            sl = slice(i, min(i + step, R))
            e1 = hip.small_linear(s[sl], *self.time[0])
            hip.small_linear(e1, *self.time[1], silu_in=True, out=e[sl])
            hip.small_linear(e[sl], *self.time[2], silu_in=True, out=e0[sl])
        return e, e0.view(R, 6, d)

    def _mode(self, bx, R, rows_per_batch, only_row, rows_shared, teacache):
        """The mode of one forward (see _Mode).  Every environment switch a forward reads is read here, once per forward: tests and
        benchlib flip them between forwards."""
        cd, env = self.cond, os.environ
        window = getattr(self, "window", (-1, -1))         # (tests/test_smooth_k_mode_cpu.py resolves modes on a bare namespace)
        frames = getattr(self, "window_frames", (-1, -1))
        windowed = window != (-1, -1) or frames != (-1, -1)
        # FLEXAM_SP_WINDOW=1 (default 0): a windowed model under sequence parallelism runs the windowed kernel at each rank's query offset
        # (flexam_attn_fwd_window_at; flexam_amd/dit_sp.py).  Without the switch:
        sp_window = windowed and self.sp_size > 1
        if sp_window and not sp_window_asked(env):
            raise NotImplementedError(f"flexam_amd: {'window_size' if frames == (-1, -1) else 'window_frames'} under sequence parallelism is not "
                                      "served: a rank's queries and the keys it gathers carry global token indices, which the windowed "
                                      "kernel does not take")
        overlap = self.sp_overlap_level
        if sp_window and self.fused and self.sp_mode == "allgather" and overlap >= 1:
            # the overlapped K|V gather (local chunk first, partial softmaxes + merge) has no windowed form: the gather is waited for, piece
            # by piece, and one windowed call per piece follows.  The mode says so (sp_overlap_level 0), and with it a launch plan's key
            overlap = 0
            if not DiTEngine._sp_window_overlap_warned:    # said once per process
                DiTEngine._sp_window_overlap_warned = True
                import warnings
                warnings.warn("flexam_amd: FLEXAM_SP_OVERLAP is ignored with window_size / window_frames under the K|V all-gather: each "
                              "piece of the gather is waited for and one windowed attention call follows", RuntimeWarning, stacklevel=3)
        # (record_gather: under a window the ranks gather bf16 K|V and pad to the ranks alone, whatever FLEXAM_SAGE_WINDOW says -- unless
        #  FLEXAM_SP_SAGE_WINDOW=1 (default 0; with FLEXAM_SP_WINDOW=1, SAGE_ATTENTION and FLEXAM_SAGE_WINDOW=1 only) asks for the MXFP8
        #  records, which flexam_attn_fwd_fp8_window_at reads under the mask at the rank's query offset: resolve_mode then decides
        #  sage_gather as it does for an unmasked model, and where it does not resolve the replacement below runs as ever)
        sp_sage_window = sp_window and sp_sage_window_asked(env)
        m = resolve_mode(env, fused=self.fused, nl=self.nl, nh=self.nh, hd=self.hd, dim=self.dim, table_limit=self.table_limit, fp8=self.fp8,
                         sp=self.sp_size, rank=self.sp_rank,
                         parallel=(self.sp_mode, overlap, self.sp_pieces, self.sp_fused_qkv),
                         B=cd["B"], L=cd["L"], dens_same=cd.get("dens_same", False), bx=bx, R=R, rows_per_batch=rows_per_batch,
                         only_row=only_row, rows_shared=rows_shared, teacache=teacache is not None, record_gather=not sp_window or sp_sage_window)
        if sage_asked(env) and not m.sage and not sp_window and not DiTEngine._sage_warned:          # said once per process
            DiTEngine._sage_warned = True
            import warnings
            warnings.warn("flexam_amd: VIDEOX_ATTENTION_TYPE=SAGE_ATTENTION is ignored " +
                          "under sequence parallelism with the OVERLAPPED K|V all-gather (FLEXAM_SP_OVERLAP=1 / head-group pieces) or an all-to-all "
                          "over a padded sequence: self-attention runs the bf16 kernel", RuntimeWarning, stacklevel=3)
        # FLEXAM_SAGE_SMOOTH_K=1 (default 0): the quantised self-attention quantises K - mean_tokens(K) (csrc/attn_fp8.inc).  Kept beside
        # the mode, not in it, and part of a launch plan's key.  One rank only: under the record gather each rank would shift ITS keys by
        # ITS mean, which is not exact (the all-to-all over heads could do it exactly and does not yet)
        asked = smooth_k_asked(env)
        self._smooth_k = bool(m.sage and m.sp == 1 and asked)
        if asked and m.sage and m.sp > 1 and not DiTEngine._smooth_k_warned:       # said once per process
            DiTEngine._smooth_k_warned = True
            import warnings
            warnings.warn("flexam_amd: FLEXAM_SAGE_SMOOTH_K=1 is ignored under sequence parallelism: K is quantised as it is",
                          RuntimeWarning, stacklevel=3)
        # FLEXAM_SAGE_SMOOTH_V=1 (default 0): V - mean_tokens(V) is quantised and the mean added back to the attention's output in fp32.
        # Kept like smooth-K and independent of it.  One rank only: under the record gather each rank's own mean would not be exact
        asked = smooth_v_asked(env)
        self._smooth_v = bool(m.sage and m.sp == 1 and asked)
        if asked and m.sage and m.sp > 1 and not DiTEngine._smooth_v_warned:       # said once per process
            DiTEngine._smooth_v_warned = True
            import warnings
            warnings.warn("flexam_amd: FLEXAM_SAGE_SMOOTH_V=1 is ignored under sequence parallelism: V is quantised as it is",
                          RuntimeWarning, stacklevel=3)
        # FLEXAM_SAGE_WINDOW=1 (default 0): a windowed model under SAGE runs the windowed MXFP8 kernel (flexam_attn_fwd_fp8_window); the mode
        # keeps `sage` then, which tells a launch plan of it from one of the replacement below.  Without the switch:
        # (under sequence parallelism, FLEXAM_SP_WINDOW=1: the same, and with the switch the all-to-all over heads alone keeps `sage` --
        #  resolve_mode never asked for the record gather above, which is said here as well; with FLEXAM_SP_SAGE_WINDOW=1 on top it was
        #  asked for, and where it resolved `sage` stands)
        if windowed and ((m.sage and not sage_window_asked(env)) or (sp_window and self.fused and sage_asked(env) and not m.sage)):      # the windowed bf16 kernel runs
            m = m._replace(sage=False, sage_gather=False, sage_fused=False)
            self._smooth_k = self._smooth_v = False
            if not DiTEngine._sage_window_warned:          # said once per process
                DiTEngine._sage_window_warned = True
                import warnings
                warnings.warn("flexam_amd: VIDEOX_ATTENTION_TYPE=SAGE_ATTENTION is ignored with window_size / window_frames: self-attention "
                              "runs the windowed bf16 kernel", RuntimeWarning, stacklevel=3)
        # FLEXAM_SP_HALO=1 (default 0): under FLEXAM_SP_WINDOW=1, the K|V gather and the bf16 kernel a rank fetches only the key rows its
        # windowed call visits (dit_layout.halo_plan; dit_sp.KVHalo).  Kept beside the mode and part of a launch plan's key.  halo_rows /
        # halo_gather_rows: the rows of this rank's compact buffer and of the gathered buffer it replaces (None when the switch does not act)
        self._sp_halo, self.halo_rows, self.halo_gather_rows = False, None, None
        if sp_halo_asked(env) and self.sp_size > 1 and self.fused:
            why = None
            if not sp_window:
                why = "the model has no window_size / window_frames"
            elif m.sage_gather:                            # (FLEXAM_SP_SAGE_WINDOW=1)
                why = "the MXFP8 record gather moves whole chunks"
            elif m.sp_mode != "allgather" or m.sage:
                why = "the all-to-all over heads hands a rank every token of its heads"
            else:
                mask = self._window_mask()
                plans = [halo_plan(cd["L"], m.sp, r, mask[0], mask[1], mask[2]) for r in range(m.sp)]
                if all(pl.gap == 0 and pl.rows == cd["L"] for pl in plans):
                    why = "every rank's window reaches the whole sequence"
                else:
                    self._sp_halo, self.halo_rows, self.halo_gather_rows = True, plans[m.rank].rows, m.sp * m.lc
            if why is not None and not DiTEngine._sp_halo_warned:      # said once per process
                DiTEngine._sp_halo_warned = True
                import warnings
                warnings.warn(f"flexam_amd: FLEXAM_SP_HALO=1 is ignored ({why}): the exchange runs as it does without the switch",
                              RuntimeWarning, stacklevel=3)
        return m

    def run(self, x: torch.Tensor, t_rows: torch.Tensor, row_index: Optional[torch.Tensor], rows_per_batch: int,
            only_row: Optional[int] = None, teacache=None, cond_flag: bool = True, rows_shared: bool = False) -> torch.Tensor:
        """x [Bx, 48, F, H, W] (Bx = B, or 1 when all rows share the latent); t_rows [R] distinct
        timesteps with R = B * rows_per_batch table rows (rows of batch b are b*rows_per_batch ..);
        row_index int32 [B * L] global table row per token, or None (then token (b, l) uses row b).
        Returns the head output tokens fp32 [B, Lc, 4*out_dim] of this rank's token chunk."""
        cd, dev, d = self.cond, self.device, self.dim
        m = self._mode(x.shape[0], t_rows.numel(), rows_per_batch, only_row, rows_shared, teacache)
        B, L, ref_len, lc, R = m.B, cd["L"], cd["ref_len"], m.lc, m.R
        # only_row: run a single conditioning row (cfg_skip: the unconditional row is dropped, cfg_optimization.py:5-37);
        # t_rows / row_index then describe that one row
        rsel = slice(None) if only_row is None else slice(only_row, only_row + 1)
        dens0 = cd["dens0"][rsel] if cd["dens0"] is not None else None
        dens_emb = cd["dens_emb"][rsel] if cd["dens_emb"] is not None else None
        if m.Lp > L and cd["cos"].shape[0] < m.Lp:         # RoPE rows of the pad tokens: the identity, like every token beyond the grid
            extra = m.Lp - cd["cos"].shape[0]
            cd["cos"] = torch.cat([cd["cos"], torch.ones(extra, cd["cos"].shape[1], device=dev)])
            cd["sin"] = torch.cat([cd["sin"], torch.zeros(extra, cd["sin"].shape[1], device=dev)])
        ws = self._workspace(B, lc)
        xres = ws["x"]
        xr = xres.view(B, lc, d)

        # ---- stem: patch embedding of the noisy latent (+ cached static channels), ref tokens
        bx = x.shape[0]
        full = torch.empty(m.Lp, d, device=dev, dtype=F32) if m.sp > 1 else None
        if m.Lp > L:
            full[L:].zero_()
        for b in range(bx):
            pa = cd["patch_a"][b if cd["nb"] > 1 else 0]
            hip.patchify(x[b].to(dev).contiguous(), pa, col0=0)
            dst = full if m.sp > 1 else xr[b]
            hip.gemm(pa, self.pe_w, self.pe_b, out=dst[ref_len:L], out_dtype=F32)
            if ref_len:
                dst[:ref_len].copy_(cd["ref_tok"][b if cd["nb"] > 1 else 0])
            if m.sp > 1:
                xr[b].copy_(full[m.tok0:m.tok0 + lc])
        self.share0_taken, self.sage_taken = m.share0, m.sage          # what this forward DID (bench.py labels its line from them)
        self.sage_smooth_taken, self.sage_smooth_v_taken = self._smooth_k, self._smooth_v
        if not m.share0:
            for b in range(bx, B):
                xr[b].copy_(xr[0])

        # ---- timestep embedding on the distinct rows + AdaLN tables of all blocks and the head
        if rows_shared and R > rows_per_batch:     # every sample carries the same timestep rows (the sampler's CFG pair): embed once
            e1, e01 = self.embed_time(t_rows[:rows_per_batch])
            reps = R // rows_per_batch
            e, e0 = e1.repeat(reps, 1), e01.repeat(reps, 1, 1)
        else:
            e, e0 = self.embed_time(t_rows)
        dens0c = dens0.contiguous() if dens0 is not None else None
        # the tables live in the workspace (one set per row count): the blocks' launches name their addresses, and a recorded launch plan
        # (below) is only valid while they stay put
        tabs = ws.setdefault(("tabs", R, m.per_layer), {})
        if not tabs:
            tabs["blk"] = torch.empty(1 if m.per_layer else self.nl, R, 6, d, device=dev, dtype=F32)
            tabs["head"] = torch.empty(1, R, 2, d, device=dev, dtype=F32)
        if not m.per_layer:
            hip.mod_table(self.mod, e0, tabs["blk"], rows_per_batch, hip.MOD_BLOCK_SLOTS.scale_mask, self.mdens, dens0c,
                          hip.MOD_BLOCK_SLOTS.dens_slots if dens0 is not None else -1)
        e2 = e.unsqueeze(1).expand(R, 2, d).contiguous()
        hd_dens = dens_emb.reshape(B, 1, d).contiguous() if dens_emb is not None else None
        hip.mod_table(self.hmod, e2, tabs["head"], rows_per_batch, hip.MOD_HEAD_SLOTS.scale_mask, self.hmdens if hd_dens is not None else None, hd_dens,
                      hip.MOD_HEAD_SLOTS.dens_slots if hd_dens is not None else -1)
        calc = self._teacache_decide(teacache, e0, row_index, B, L, cond_flag) if teacache is not None else True
        if row_index is not None:
            # the per-token row index of THIS rank's rows, copied (47 KB) into a buffer of the workspace: the blocks' launches then see ONE
            # address from step to step whoever built the index (the sampler keeps one tensor per clip, the reference-style forward()
            # builds a new one per call) -- what a recorded launch plan (below) needs
            if m.sp > 1:
                from .dist import shard_rows
                row_index = shard_rows(row_index, B, L, m.rank, m.sp, chunk=lc)
            buf = ws.get("row_index_buf")
            if buf is None or buf.numel() != row_index.numel():
                buf = ws["row_index_buf"] = torch.empty(row_index.numel(), device=dev, dtype=I32)
            buf.copy_(row_index.reshape(-1))
            row_index = buf
        ws["row_index"] = row_index                        # this forward's (the stages read it here), or None
        if teacache is not None:
            key = "previous_residual_cond" if cond_flag else "previous_residual_uncond"
            if not calc:                                   # skipped step: x += residual of the last computed step (FX.py:1003-1006)
                res = getattr(teacache, key)
                n = xres.shape[0]                          # `previous_residual[-x.size(0):]`: a cfg-skipped (B = 1) forward takes the
                res = res[-n:] if res.shape[0] >= n else res.repeat(n // res.shape[0], 1)      # conditional row of a B = 2 residual
                hip.axpby(xres, 1.0, res.contiguous(), 1.0)
            else:
                ori = xres.clone()

        self.replay_taken = False
        if m.use_plan:
            self._record_or_replay(m, ws, e0, dens0c)
            return ws["head"].view(B, lc, -1)
        if calc and self.fused:
            self._blocks(m, ws, e0, dens0c)
        elif calc:
            self._run_block_modules(xres, B, lc, e0, row_index, rows_per_batch, dens0, t_rows, rsel)
        if teacache is not None and calc:                  # residual = x_after_blocks - x_before (FX.py:1048-1051), kept on the GPU
            hip.axpby(ori, 1.0, xres, -1.0)
            setattr(teacache, key, ori)
        self._head(m, ws)
        return ws["head"].view(B, lc, -1)

    def _window_frames(self):
        """((a, b), T) of the self-attention's frame window for this clip, T = the tokens of one frame of its grid; ((-1, -1), 0) without one."""
        frames = getattr(self, "window_frames", (-1, -1))
        if frames == (-1, -1):
            return frames, 0
        from .wan_transformer3d_FlexAM import frame_tokens
        return frames, frame_tokens(self.cond["grid"], self.cond["L"])

    def _window_mask(self):
        """None without a window, else (window, sink, frame_tokens) as hip.attn_fwd_window takes them: the token window with frame_tokens
        0, or the frame window with the tokens of one frame of this clip's grid (whole frames of the REAL length, never of a chunk)."""
        if self.window != (-1, -1):
            return self.window, self.window_sink, 0
        if self.window_frames != (-1, -1):
            frames, T = self._window_frames()
            return frames, self.window_sink, T
        return None

    def _record_or_replay(self, m, ws, e0, dens0):
        """The blocks and the head through a launch plan: they issue the same ~420 launches on the same buffers every step (only buffer
        CONTENTS change), so the first step records them (hip.record: executed and appended to command lists) and every later step
        re-issues the lists from C (flexam_replay, csrc/replay.hip: ~1 us per launch instead of 20-30 us of Python + ctypes).  Collectives,
        waits and torch copies between them are host steps of the plan (hip.host_op).  The key is the mode and the addresses and context
        the launches name; plans live in the per-clip state (new conditioning = new plans) and hold references to every tensor whose
        address they carry.  Not with TeaCache (data-dependent skipping), per-layer tables or blocks called as modules (_Mode.use_plan)."""
        cd, ri, tabs = self.cond, ws["row_index"], ws["tabs", m.R, m.per_layer]
        key = (m, self._ws_gen, ri.data_ptr() if ri is not None else 0, tabs["blk"].data_ptr(), tabs["head"].data_ptr(), cd["cos"].data_ptr(),
               torch.cuda.current_stream().cuda_stream, hip.num_cus(), id(self.sp_group), getattr(self, "window", (-1, -1)), getattr(self, "window_sink", 0),
               DiTEngine._window_frames(self), self._sp_halo, self._smooth_v, self._smooth_k)      # (unbound: the mode tests hand a bare namespace)
        plans = cd.setdefault("_plans", {})
        plan = plans.get(key)
        if plan is None:
            for k in [k for k in plans if k[1] != self._ws_gen]:      # plans of dropped activation buffers would keep those buffers alive
                del plans[k]
            with hip.record() as plan:
                self._blocks(m, ws, e0, dens0)
                self._head(m, ws)
            while len(plans) >= 6:                         # (cond / uncond rows of cfg_skip, the shared-block-0 form, ...: a handful per clip)
                plans.pop(next(iter(plans)))
            plans[key] = plan
        else:
            plan.run()
            self.replay_taken = True
        self.plan_launches = plan.launches

    # ------------------------------------------------------------------ stages of a forward (fused blocks)
    def _blocks(self, m, ws, e0, dens0):
        tab = ws["tabs", m.R, m.per_layer]["blk"]
        ex = self._exchange(m, ws) if m.sp > 1 else None
        for i, p in enumerate(self.blocks):
            if m.per_layer:                                # one table, rebuilt per layer (bounded memory, see table_limit)
                hip.mod_table(self.mod[i:i + 1], e0, tab, m.rows_per_batch, hip.MOD_BLOCK_SLOTS.scale_mask, self.mdens[i:i + 1], dens0,
                              hip.MOD_BLOCK_SLOTS.dens_slots if dens0 is not None else -1)
            T = tab[0 if m.per_layer else i]
            self._self_attention(i, p, T, m, ws, ex)
            self._cross_attention(i, p, m, ws)
            self._ffn(i, p, T, m, ws)

    def _heads(self, m, ws):
        """q, k, v [B, lc, heads, 128] of ws["qkv"] and the attention output ws["ao"] as the same views."""
        q4, k4, v4 = ws["qkv"].view(m.B, m.lc, 3, self.nh, self.hd).unbind(2)
        return q4, k4, v4, ws["ao"].view(m.B, m.lc, self.nh, self.hd)

    def _ln_a(self, m, ws, rows, nxt=None, **kw):
        """LN + modulate of the first `rows` rows of the residual stream as the A operand of the next GEMM: bf16 rows of ws["h"]
        (returns (None, False)), or with fp8 on ((e4m3 rows, row scales), whether FFN1's output scales were written) (_ln_fp8)."""
        x, h = ws["x"][:rows], ws["h"][:rows]
        if m.fp8:
            a8, sa, bound = self._ln_fp8(x, ws, h, nxt, **kw)
            return (a8, sa), bound
        hip.ln_modulate(x, out=h, eps=self.eps, **kw)
        return None, False

    def _out_proj(self, i, p, wname, bname, a, ws, rows, fp8, **kw):
        """ws["x"][:rows] += (a @ W^T + b) [* gate]: bf16 MFMA, or (FLEXAM_FP8_OPROJ) fp8 MFMA on `a` row-quantised by one more pass."""
        x = ws["x"][:rows]
        if fp8:
            a8, sa = hip.quantize_rows_fp8(a, ws["a8d"][:rows], ws["sa"][:rows])
            w8 = self._fp8_w[i]
            hip.gemm_fp8_gate_residual(a8, sa, w8[wname], w8["s_" + wname], p[bname], x, **kw)
        else:
            hip.gemm_gate_residual(a, p[wname], p[bname], x, **kw)

    def _norm_rope_qk(self, p, m, ws, nb, bufs=None):
        """RMSNorm + RoPE of q and k of the first nb samples at this chunk's token offset.  With bufs (SAGE_ATTENTION) q, k and v become
        the MXFP8 operands of the quantised attention (csrc/attn_fp8.inc): at the 5B model's 24 heads (sage_fused) the RMSNorm + RoPE
        launch writes Q and K as operands directly and V is packed on its own; otherwise q and k are normed in bf16 and all three packed.
        Smooth-K (FLEXAM_SAGE_SMOOTH_K, _mode): one more pass over k, the token mean of the normed and rotated K (hip.k_mean: computed
        from the raw k in the fused form, which never writes that K), is what the producer subtracts before it quantises K.
        Smooth-V (FLEXAM_SAGE_SMOOTH_V): the token mean of the V columns, taken as given, is what both pack forms subtract from V; it is
        returned (else None) for the attention to add back (hip.attn_fwd_fp8's o_shift)."""
        d, rows, cd = self.dim, nb * m.lc, self.cond
        q, k = ws["qkv"][:rows, 0:d], ws["qkv"][:rows, d:2 * d]
        q4, k4, v4, _ = self._heads(m, ws)
        smooth = bufs is not None and self._smooth_k
        mean, scratch = self._k_mean_buffers(nb, m.lc) if smooth else (None, None)
        v_mean = None
        if bufs is not None and self._smooth_v:
            v_mean, v_scratch = self._k_mean_buffers(nb, m.lc, of_v=True)
            hip.k_mean(ws["qkv"][:rows, 2 * d:3 * d], None, None, None, m.lc, out=v_mean, scratch=v_scratch)
        if bufs is not None and m.sage_fused:
            if smooth:
                hip.k_mean(k, p["nk"], cd["cos"], cd["sin"], m.lc, m.tok0, eps=self.eps, head_dim=self.hd, out=mean, scratch=scratch)
            hip.rmsnorm_rope_mx(q, p["nq"], k, p["nk"], bufs, cd["cos"], cd["sin"], m.lc, m.tok0, eps=self.eps, k_shift=mean)
            hip.attn_fp8_pack(None, None, v4[:nb], bufs, v_shift=v_mean)
            return v_mean
        hip.rmsnorm_rope(q, p["nq"], k, p["nk"], eps=self.eps, rope_cos=cd["cos"], rope_sin=cd["sin"], tokens_per_batch=m.lc,
                         token_offset=m.tok0, head_dim=self.hd)
        if smooth:
            hip.k_mean(k, None, None, None, m.lc, out=mean, scratch=scratch)
        if bufs is not None:
            hip.attn_fp8_pack(q4[:nb], k4[:nb], v4[:nb], bufs, k_shift=mean, v_shift=v_mean)
        return v_mean

    def _self_attention(self, i, p, T, m, ws, ex=None):
        """LN + modulate -> q|k|v -> self-attention in this forward's layout (one rank, all-to-all over heads or K|V all-gather) ->
        output projection + gated residual."""
        d = self.dim
        nb = 1 if (m.share0 and i == 0) else m.B          # samples that run the self-attention half of this block (share0: _mode)
        mb = nb * m.lc
        ri = ws["row_index"][:mb] if ws["row_index"] is not None else None
        a8sa, _ = self._ln_a(m, ws, mb, shift=T[:, 0], scale=T[:, 1], row_index=ri, rows_per_batch=m.lc)
        gate = dict(gate=T[:, 2], gate_row=ri, rows_per_batch=m.lc)
        if m.sp > 1 and m.sp_mode == "ulysses":
            # all tokens of H/sp heads per rank: q|k|v all-to-all -> attention -> all-to-all back; the o-projection reads the
            # returned blocks in place (flexam_amd/dist.py)
            a_o, koff_o = ex.run(self, ws, a8sa, i, p, m)
            self._out_proj(i, p, "wo", "bo", a_o, ws, mb, False, a_koff=koff_o, **gate)
            return
        qkv, h = ws["qkv"], ws["h"]
        if m.sp > 1:
            # K|V projection + K norm/RoPE first, written straight into the send buffer; their all-gather (RCCL over xGMI)
            # runs under the Q projection, the Q norm/RoPE and the attention to the LOCAL chunk
            # (FLEXAM_SP_FUSED_QKV=1, default: ONE q|k|v launch instead -- at a rank's few thousand rows two launches of 24 and 12 tile
            #  columns quantise worse on 256 CUs than one of 36 (emulated rank of 8, profiles/r5*: 119 + 80 us against ~135), and the
            #  gather starts ~15 us later, not ~80; sage_gather: the MXFP8 records travel, always one q|k|v launch)
            whole = m.sp_fused_qkv or m.sage
            self._proj(h, a8sa, i, p, "wqkv", "bqkv", slice(None) if whole else slice(d, None), qkv if whole else qkv[:, d:])
            ex.run(self, ws, a8sa, i, p, m)
            self._out_proj(i, p, "wo", "bo", ws["ao"], ws, mb, False, **gate)
            return
        self._proj(h[:mb], a8sa, i, p, "wqkv", "bqkv", slice(None), qkv[:mb])
        q4, k4, v4, ao4 = self._heads(m, ws)
        if m.sage:
            bufs = self._attn8_buffers(nb, m.lc)
            v_mean = self._norm_rope_qk(p, m, ws, nb, bufs)
            # (a window here: FLEXAM_SAGE_WINDOW=1, else _mode cleared `sage`; without one the call is the one it has always been)
            window, frame_t = (self.window, 0) if self.window_frames == (-1, -1) else self._window_frames()
            hip.attn_fwd_fp8(bufs, m.lc, out=ao4[:nb], o_shift=v_mean, window=window, sink=self.window_sink, frame_tokens=frame_t)
        else:
            self._norm_rope_qk(p, m, ws, nb)
            if self.window != (-1, -1):
                hip.attn_fwd_window(q4[:nb], k4[:nb], v4[:nb], self.window, out=ao4[:nb], prescaled=True, sink=self.window_sink)
            elif self.window_frames != (-1, -1):
                frames, T = self._window_frames()
                hip.attn_fwd_window(q4[:nb], k4[:nb], v4[:nb], frames, out=ao4[:nb], prescaled=True, sink=self.window_sink, frame_tokens=T)
            else:
                hip.attn_fwd(q4[:nb], k4[:nb], v4[:nb], out=ao4[:nb], prescaled=True)
        self._out_proj(i, p, "wo", "bo", ws["ao"][:mb], ws, mb, m.fp8_oproj, **gate)
        if nb < m.B:
            xr = ws["x"].view(m.B, m.lc, d)
            hip.host_op(lambda: xr[1].copy_(xr[0]))         # (a torch copy, not a library call: a host step of a recorded plan)

    def _cross_attention(self, i, p, m, ws):
        """Cross-attention on the text context (K/V precomputed per clip): LN -> Q (on the fp8 pipe as well with fp8 on) -> attention
        -> output projection + residual."""
        d, cd, o = self.dim, self.cond, m.only_row
        qc = ws["qkv"][:, 0:d]
        a8sa, _ = self._ln_a(m, ws, m.B * m.lc, ln_w=p["n3w"], ln_b=p["n3b"])
        self._proj(ws["h"], a8sa, i, p, "cwq", "cbq", slice(None), qc)
        hip.rmsnorm_rope(qc, p["cnq"], eps=self.eps)
        kv = cd["cross_kv"][i][slice(None) if o is None else slice(o, o + 1)]
        heads = lambda t: t.unflatten(2, (self.nh, self.hd))
        q4, _, _, ao4 = self._heads(m, ws)
        if cd.get("cross_lk"):                             # the identical padded text rows as ONE weighted key
            lk = cd["cross_lk"]
            hip.attn_fwd_lastkey(q4, heads(kv[:, :lk, 0:d]), heads(kv[:, :lk, d:]), cd["cross_mult"], out=ao4, prescaled=True)
        else:
            hip.attn_fwd(q4, heads(kv[:, :, 0:d]), heads(kv[:, :, d:]), out=ao4, prescaled=True)
        self._out_proj(i, p, "cwo", "cbo", ws["ao"], ws, m.B * m.lc, m.fp8_oproj)

    def _ffn(self, i, p, T, m, ws):
        """LN + modulate -> FFN1 + GELU -> FFN2 + gated residual."""
        ri = ws["row_index"]
        gate = dict(gate=T[:, 5], gate_row=ri, rows_per_batch=m.lc)
        if not m.fp8:
            self._ln_a(m, ws, m.B * m.lc, shift=T[:, 3], scale=T[:, 4], row_index=ri, rows_per_batch=m.lc)
            # (FFN1 -> FFN2 per row chunk, so that the [M, 14336] intermediate stays in the Infinity Cache: the clock rises with the
            #  saved HBM traffic, but tile quantisation and launch ramps cost more: +0.5 / +1.6 / +7.1 % of a step at 2 / 4 / 7 chunks,
            #  profiles/r4p_ffn_row_chunks.txt)
            hip.gemm(ws["h"], p["w1"], p["b1"], out=ws["ffn"], epilogue=hip.EPI_GELU_TANH)
            hip.gemm_gate_residual(ws["ffn"], p["w2"], p["b2"], ws["x"], **gate)
            return
        w8 = self._fp8_w[i]
        # FFN1 writes FFN2's e4m3 operand itself: its output row scales are known before it runs (a bound from the row's L2 norm, written
        # by the LN launch), so there is no absmax / quantise pass over the [M, 14336] intermediate
        # (FLEXAM_FP8_FFN_APRIORI=0: the earlier form -- bf16 intermediate + an absmax row quantiser pass -- for checkpoints whose w1
        #  has a few very large rows: the bound is set by the LARGEST row norm, so every ordinary row's outputs then sit lower in
        #  e4m3's range.  One scale per output row has to cover all 14336 columns, so a per-tile bound cannot be used by FFN2.)
        (a8, sa), bound = self._ln_a(m, ws, m.B * m.lc, nxt=(w8["w1_norm"], w8["b1_max"]) if m.ffn_apriori else None, shift=T[:, 3],
                                     scale=T[:, 4], row_index=ri, rows_per_batch=m.lc)
        if bound:
            hip.gemm_fp8_gelu_q(a8, sa, w8["w1"], w8["s_w1"], p["b1"], ws["so"], ws["a8"])
            a8, sa = ws["a8"], ws["so"]
        else:                                              # widths the fused LN launch does not cover: bf16 intermediate + row quantiser
            hip.gemm_fp8(a8, sa, w8["w1"], w8["s_w1"], p["b1"], out=ws["ffn"], epilogue=hip.EPI_GELU_TANH)
            a8, sa = hip.quantize_rows_fp8(ws["ffn"], ws["a8"], ws["sa"])
        hip.gemm_fp8_gate_residual(a8, sa, w8["w2"], w8["s_w2"], p["b2"], ws["x"], **gate)

    def _head(self, m, ws):
        H = ws["tabs", m.R, m.per_layer]["head"][0]
        hip.ln_modulate(ws["x"], out=ws["h"], eps=self.eps, shift=H[:, 0], scale=H[:, 1], row_index=ws["row_index"], rows_per_batch=m.lc)
        hip.gemm(ws["h"], self.head_w, self.head_b, out=ws["head"])

    # ------------------------------------------------------------------ block-level seam
    def _run_block_modules(self, xres, B, lc, e0, row_index, rows_per_batch, dens0, t_rows, rsel):
        """Some block is not a pristine native block (replaced, wrapped, or with a re-bound forward): every block is CALLED
        with the reference's block signature (wan_transformer3d_FlexAM.py:1053-1089) on [B, L, C] fp32 tensors.  The AdaLN
        input is materialised per token like the reference's e0 ([B, L, 6, C]); native blocks find its compact form in the
        `_flexam_rows` attribute."""
        cd, d = self.cond, self.dim
        if row_index is not None:
            e_full = e0[row_index.long()].view(B, lc, 6, d)
        else:
            e_full = e0.view(B, 6, d)
        e_full._flexam_rows = (e0, row_index, rows_per_batch)
        grid_sizes = torch.tensor([list(cd["grid"])] * B, dtype=torch.long)
        # Under sequence parallelism the blocks get this rank's token chunk and the GLOBAL lengths / grid, as the reference hands them
        # over (wan_transformer3d_FlexAM.py:970-975, 1075-1086); the exchange around self-attention belongs to `self_attn.forward`
        # (the reference re-binds it to a USP forward, :807-815): the native _SelfAttn.forward reads the context below and gathers K|V
        # itself, a caller's re-bound forward finds group / rank / token offset / RoPE tables in flexam_amd.dist.current_sp_context()
        from .dist import sequence_parallel_context
        sp = self.sp_size
        seq_lens = torch.tensor([cd["L"]] * B, dtype=torch.long)      # the REAL lengths (FX.py:917): under sequence parallelism lc * sp may be padded
        x3 = xres.view(B, lc, d)
        ctx = cd["ctx"][rsel]
        with sequence_parallel_context(self.sp_group, self.sp_rank, sp, self.sp_rank * lc, cd["L"], cd["cos"], cd["sin"]) if sp > 1 else nullcontext():
            for blk in self.block_modules:
                out = blk(x3, e=e_full, density_emb=dens0, seq_lens=seq_lens, grid_sizes=grid_sizes, freqs=self.model.freqs, context=ctx,
                          context_lens=None, dtype=BF16, t=t_rows)
                x3.copy_(out.view(B, lc, d))

    # ------------------------------------------------------------------ TeaCache
    @staticmethod
    def _teacache_decide(tc, e0, row_index, B, L, cond_flag: bool) -> bool:
        """Step-skipping decision of wan_transformer3d_FlexAM.py:977-1000 (host logic on the tiny AdaLN input).
        e0 [R, 6, C]; the reference looks at the LAST token's row (`e0[:, -1, :]`) or at e0 itself for 1-D t."""
        if not cond_flag:
            return tc.should_calc
        if row_index is not None:
            mod_inp = e0[row_index.view(B, L)[:, -1].long()]
        else:
            mod_inp = e0
        if tc.cnt < tc.num_skip_start_steps:
            calc = True
            tc.accumulated_rel_l1_distance = 0
        else:
            prev = tc.previous_modulated_input
            rel = ((mod_inp - prev).abs().mean() / prev.abs().mean()).item()
            tc.accumulated_rel_l1_distance += tc.rescale_func(rel)
            if tc.accumulated_rel_l1_distance < tc.rel_l1_thresh:
                calc = False
            else:
                calc = True
                tc.accumulated_rel_l1_distance = 0
        tc.previous_modulated_input = mod_inp.clone()
        tc.should_calc = calc
        return calc

    # ------------------------------------------------------------------ sequence parallel
    def _exchange(self, m, ws):
        """The exchange object of sequence-parallel self-attention in this forward's layout (flexam_amd/dit_sp.py): one per workspace and
        layout, made by the first forward that needs it."""
        cls = HeadAllToAll if m.sp_mode == "ulysses" else (RecordGather if m.sage else KVGather)      # (the all-to-all serves bf16 and SAGE)
        if self._sp_halo:                                  # (DiTEngine._mode: the bf16 K|V gather of a windowed model, FLEXAM_SP_HALO=1)
            cls = KVHalo
        ex = ws.get(("exchange", cls.__name__))
        if ex is None:
            ex = ws["exchange", cls.__name__] = cls(self, m, ws)
        return ex

    def _proj(self, hbuf, a8sa, layer, p, wname, bname, rows, out):
        """out = h @ W[rows]^T + b[rows]: bf16 MFMA, or fp8 MFMA on the row-quantised h (`a8sa` = (bytes, row scales)) with the
        per-channel scales of the same weight rows."""
        if a8sa:
            w8 = self._fp8_w[layer]
            return hip.gemm_fp8(a8sa[0], a8sa[1], w8[wname][rows], w8["s_" + wname][rows], p[bname][rows], out=out)
        return hip.gemm(hbuf, p[wname][rows], p[bname][rows], out=out)

    def gather_tokens(self, head_local: torch.Tensor) -> torch.Tensor:
        """All-gather of the head output [B, Lc, 192] -> [B, L, 192] (the reference's one collective,
        wan_transformer3d_FlexAM.py:1103-1104)."""
        if self.world_size == 1:
            return head_local
        from .dist import all_gather_seq
        Lr = self.cond["L"]                            # the pad tokens of a sequence that does not divide over the ranks end here
        if self.cfg_size == 1:
            return all_gather_seq(head_local, self.sp_group)[:, :Lr]
        # world rank = cfg_row * sp + sp_rank, one local row each: the rank-major gather IS [2, sp, Lc, n]
        from .dist import all_gather_into_tensor
        bl, lc, n = head_local.shape
        if bl != 1:
            raise RuntimeError("cfg-parallel ranks carry exactly one CFG row")
        out = torch.empty(self.world_size * lc, n, device=head_local.device, dtype=head_local.dtype)   # rank-major concat
        all_gather_into_tensor(out, head_local.reshape(lc, n).contiguous(), group=self.world_group)
        return out.view(self.cfg_size, self.sp_size * lc, n)[:, :Lr]
