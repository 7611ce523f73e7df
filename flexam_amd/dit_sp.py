"""The exchanges of sequence-parallel self-attention in the DiT engine: the all-to-all over heads, the K|V all-gather in bf16, its
halo form for a windowed model (only the key rows a rank's window reaches travel) and the all-gather of MXFP8 key / value records.
One object per (workspace, layout) (DiTEngine._exchange): it owns the exchange's buffers, planned splits, per-peer view lists and the Work handles between the host step that issues a collective and the one that
waits for it.  It keeps no reference to the engine or the workspace that holds it (both are arguments of `run`), so dropping a
workspace frees its buffers at once.  Buffers that code outside the engine reads are placed in the workspace under their names
(a2a_recv, a2a_out, kv_cat, kv_halo).
Collectives, waits and torch copies are host steps (hip.host_op): run in place, and again in that place by every replay of a
recorded launch plan.  The arithmetic of the layouts is flexam_amd/dit_layout.py."""
import torch

from . import hip
from .dist import all_gather_into_tensor, all_to_all_blocks, exchange_rows, group_backend
from .dit_layout import a2a_koff, gather_key_ranges, halo_plan, key_range_sizes

BF16, I64 = torch.bfloat16, torch.int64


class HeadAllToAll:
    """h [B*lc, C] (LayerNorm output of this rank's tokens) -> q|k|v projection -> exchange -> attention -> exchange back ->
    (A base view, per-K-block A offsets) of the attention output for the o-projection.  Head group j = heads j*H/sp .. goes
    to rank j.
    Send layout [B, sp, lc, 3*G] (G = H/sp * head_dim): written by the RMSNorm+RoPE launch itself (q, k normed + rotated, v
    copied), block (b, j) goes to rank j.  Receive layout [B, sp, lc, 3*G] = [B, L, 3*G]: rank-major blocks ARE the token
    order, so attention addresses it with plain strides.  Its output [B, L, G] is cut into the sp token chunks that go back;
    rank j's block returns to [j, B, lc, G], which the o-projection reads as A[m, j*G + c] through its K-block offsets.
    With several samples per rank (the CFG pair batched: pure N-way chunks) the samples are stages of the outbound exchange
    (FLEXAM_SP_OVERLAP=1, default): sample b's q|k|v leave as soon as ITS projection and norm are done and travel under the
    projection of sample b + 1; ONE attention call for the pair follows the last arrival (two calls of half the work units fill
    256 CUs a quarter worse than one), then the outputs return.  FLEXAM_SP_OVERLAP=2 pipelines the attention too: sample b's
    call runs while sample b + 1's blocks arrive and sample b - 1's output returns -- only the last return is not under compute;
    it pays when a link is slower than the ~0.1 ms the two smaller attention calls cost (about 35 GB/s at 8 GPUs)."""

    def __init__(self, eng, m, ws):
        self.group = eng.sp_group
        sp, B, lc, dev = m.sp, m.B, m.lc, eng.device
        hg = eng.nh // sp
        self.G = G = hg * eng.hd
        self.send = torch.empty(B, sp, lc, 3 * G, device=dev, dtype=BF16)
        self.recv = ws["a2a_recv"] = torch.empty(B, sp, lc, 3 * G, device=dev, dtype=BF16)
        self.out = ws["a2a_out"] = torch.empty(B, sp * lc, hg, eng.hd, device=dev, dtype=BF16)
        self.recv2 = torch.empty(sp, B, lc, G, device=dev, dtype=BF16)
        self.koff = torch.tensor(a2a_koff(eng.dim, G, B * lc), dtype=I64, device=dev)
        self.full = self.recv.view(B, sp * lc, 3, hg, eng.hd)
        self.chunks = self.out.view(B, sp, lc, G)
        # the per-peer block views, made once (a replayed step must not rebuild 32 views per block)
        self.lists = [([self.recv[b, i] for i in range(sp)], [self.send[b, j] for j in range(sp)],
                       [self.recv2[j, b] for j in range(sp)], [self.chunks[b, i] for i in range(sp)]) for b in range(B)]
        self.works = {"there": [None] * B, "back": [None] * B}

    def _go_there(self, b, async_op):              # packed = the same blocks as ONE tensor pair (a backend that copies can do it in one go)
        self.works["there"][b] = all_to_all_blocks(self.lists[b][0], self.lists[b][1], self.group, async_op=async_op,
                                                   packed=(self.recv[b], self.send[b]))

    def _go_back(self, b, async_op):
        self.works["back"][b] = all_to_all_blocks(self.lists[b][2], self.lists[b][3], self.group, async_op=async_op,
                                                  packed=(self.recv2[:, b], self.chunks[b]))

    def _wait(self, which, bs):
        for b in bs:
            if self.works[which][b] is not None:
                self.works[which][b].wait()

    def _attend(self, eng, m, b0, nb):
        """Attention of samples b0 .. b0 + nb - 1 on this rank's heads over all tokens; SAGE_ATTENTION: the received bf16 q|k|v are
        packed into MXFP8 operands first (flexam_attn_fp8_pack) and the quantised kernel runs (resolve_mode only asks for it when
        nk = sp * lc)."""
        nk = eng.cond["L"]                    # keys: the real tokens (rows nk .. sp*lc - 1 are the reference's zero pads, FX.py:919-925)
        full, out = self.full, self.out
        q_, k_, v_ = full[b0:b0 + nb, :, 0], full[b0:b0 + nb, :nk, 1], full[b0:b0 + nb, :nk, 2]
        # a windowed model (FLEXAM_SP_WINDOW=1, DiTEngine._mode): the rank holds every padded row of its heads from token 0 on, so the
        # mask sits at offset 0 -- with Lq = sp * lc >= Lk = nk rows, the pad rows behind the keys.  SAGE (FLEXAM_SAGE_WINDOW=1; asked for
        # on an unpadded sequence only): the windowed MXFP8 launch, one length
        mask = eng._window_mask()
        if m.sage:
            bufs = eng._attn8_buffers(nb, m.sp * m.lc, eng.nh // m.sp)
            hip.attn_fp8_pack(q_, k_, v_, bufs)
            kw = {} if mask is None else dict(window=mask[0], sink=mask[1], frame_tokens=mask[2])
            hip.attn_fwd_fp8(bufs, m.sp * m.lc, out=out[b0:b0 + nb], **kw)
        elif mask is not None:
            hip.attn_fwd_window(q_, k_, v_, mask[0], out=out[b0:b0 + nb], prescaled=True, sink=mask[1], frame_tokens=mask[2], q_offset=0)
        else:
            hip.attn_fwd(q_, k_, v_, out=out[b0:b0 + nb], prescaled=True)

    def _project_and_pack(self, eng, ws, a8sa, layer, p, m, rows, b0, nb):
        """Samples b0 .. b0 + nb - 1: rows of h -> q|k|v -> normed / rotated send blocks."""
        G, d, cd = self.G, eng.dim, eng.cond
        qkv = ws["qkv"]
        a8 = a8sa and (a8sa[0][rows], a8sa[1][rows])
        eng._proj(ws["h"][rows], a8, layer, p, "wqkv", "bqkv", slice(None), qkv[rows])
        flat = self.send[b0:b0 + nb].view(-1)
        hip.rmsnorm_rope_scatter(qkv[rows, 0:d], p["nq"], qkv[rows, d:2 * d], p["nk"], qkv[rows, 2 * d:], flat, flat[G:], flat[2 * G:],
                                 ld_out=3 * G, out_bs=m.sp * m.lc * 3 * G, col_block=G, block_stride=m.lc * 3 * G, eps=eng.eps,
                                 rope_cos=cd["cos"], rope_sin=cd["sin"], tokens_per_batch=m.lc, token_offset=m.tok0, head_dim=eng.hd)

    def run(self, eng, ws, a8sa, layer, p, m):
        B, lc = m.B, m.lc
        a_o = self.recv2.view(m.sp * B * lc, self.G)
        if B == 1 or m.sp_overlap_level == 0:
            self._project_and_pack(eng, ws, a8sa, layer, p, m, slice(None), 0, B)
            hip.host_op(lambda: [self._go_there(b, False) for b in range(B)])
            self._attend(eng, m, 0, B)
            hip.host_op(lambda: [self._go_back(b, False) for b in range(B)])
            return a_o, self.koff
        for b in range(B):
            self._project_and_pack(eng, ws, a8sa, layer, p, m, slice(b * lc, (b + 1) * lc), b, 1)
            hip.host_op(lambda b=b: self._go_there(b, True))
        if m.sp_overlap_level < 2:
            hip.host_op(lambda: self._wait("there", range(B)))
            self._attend(eng, m, 0, B)
            hip.host_op(lambda: ([self._go_back(b, True) for b in range(B)], self._wait("back", range(B))))
            return a_o, self.koff
        for b in range(B):
            hip.host_op(lambda b=b: self._wait("there", [b]))
            self._attend(eng, m, b, 1)
            hip.host_op(lambda b=b: self._go_back(b, True))
        hip.host_op(lambda: self._wait("back", range(B)))
        return a_o, self.koff


class KVGather:
    """K|V of this rank's tokens are in qkv[:, C:] (projected, not yet normed).  The RMSNorm+RoPE launch writes K (normed,
    rotated) and V into the send buffer, cut into `sp_pieces` groups of heads: [G, B, lc, 2*C/G].  One all-gather per group
    and CFG row assembles [G, B, L, 2*C/G] in token order (the rank-major concatenation IS the token order: no re-layout
    pass), all of them issued at once.  DEFAULT (r6: FLEXAM_SP_OVERLAP=0, one piece): the gather is waited for and ONE ordinary
    attention call of the local queries over all L real keys follows -- the fastest form on compute.  FLEXAM_SP_OVERLAP=1
    (r2-r5's default, a layout-probe candidate): underneath the gather: Q projection, Q norm/RoPE, then the heads of group 0 attend to the LOCAL
    chunk (partial softmax, straight from the send buffer), to the chunks before / after it once piece 0 has landed, one
    merge; the heads of group g > 0 run one ordinary attention call on their gathered piece, which travelled while group
    g - 1 computed.  A peer chunk cannot arrive faster than its one xGMI link delivers it, and the chunks of one gather all
    land together; cutting along the heads gives pieces that are complete work for part of the kernel, so all links stay
    busy in every phase (reference call sites of the missing exchange: wan_transformer3d_FlexAM.py:801-815, 970-975)."""

    def __init__(self, eng, m, ws):
        self.group = eng.sp_group
        sp, B, lc, dev = m.sp, m.B, m.lc, eng.device
        G = m.sp_pieces
        self.cb, self.hg = cb, hg = eng.dim // G, eng.nh // G
        self.send = torch.empty(G, B, lc, 2 * cb, device=dev, dtype=BF16)
        self.cat = ws["kv_cat"] = torch.empty(G, B, sp * lc, 2 * cb, device=dev, dtype=BF16)      # rows: the padded sequence
        # keys are the real tokens; rows L .. sp * lc - 1 of `cat` are zero pads (FX.py:919-925) and end every key range.  The splits
        # and the merge workspace are planned here, for the clip this workspace first sees; `run` takes the range sizes from its own clip
        ranges = gather_key_ranges(eng.cond["L"], sp, m.rank, B * hg)
        self.splits, self.sizes, self.sizes_of = ranges.splits, ranges.sizes, eng.cond["L"]
        self.part = hip.attn_partial_workspace(B, hg, lc, ranges.total, dev)
        # RCCL runs the pieces one after the other on its own stream, in the order they are issued here.  The host-staged backends of the
        # test runs (gloo) execute several in-flight collectives of one group on concurrent worker threads, which is not what is being
        # modelled (and delivered wrong chunks intermittently with 8 ranks on one device): there each gather completes before the next.
        self.overlapped = group_backend(self.group) in ("nccl", "loopback")
        self.works = None

    def _issue(self):
        send, cat, grp = self.send, self.cat, self.group
        self.works = [[all_gather_into_tensor(cat[g, b], send[g, b], group=grp, async_op=self.overlapped) for b in range(send.shape[1])]
                      for g in range(send.shape[0])]

    def _wait(self, g):
        for w in self.works[g]:
            if w is not None:
                w.wait()

    def run(self, eng, ws, a8sa, layer, p, m):
        cd, send, cat, cb, hg, part = eng.cond, self.send, self.cat, self.cb, self.hg, self.part
        d, hd, B, lc, tok0, qkv, Lr = eng.dim, eng.hd, m.B, m.lc, m.tok0, ws["qkv"], cd["L"]
        q4, _, _, ao4 = eng._heads(m, ws)
        flat = send.view(-1)
        hip.rmsnorm_rope_scatter(None, None, qkv[:, d:2 * d], p["nk"], qkv[:, 2 * d:], None, flat, flat[cb:], ld_out=2 * cb, out_bs=lc * 2 * cb,
                                 col_block=cb, block_stride=B * lc * 2 * cb, eps=eng.eps, rope_cos=cd["cos"], rope_sin=cd["sin"],
                                 tokens_per_batch=lc, token_offset=tok0, head_dim=hd)
        hip.host_op(self._issue)
        if not m.sp_fused_qkv:
            eng._proj(ws["h"], a8sa, layer, p, "wqkv", "bqkv", slice(0, d), qkv[:, 0:d])
        hip.rmsnorm_rope(qkv[:, 0:d], p["nq"], eps=eng.eps, rope_cos=cd["cos"], rope_sin=cd["sin"], tokens_per_batch=lc, token_offset=tok0,
                         head_dim=hd)
        heads = lambda t: t.unflatten(2, (hg, hd))
        # a windowed model (FLEXAM_SP_WINDOW=1): the local queries are the global tokens tok0 .. tok0 + lc - 1, the gathered rows the keys
        # 0 .. Lr - 1: one windowed call per piece at that offset, once the piece has landed (DiTEngine._mode resolves the overlap level to
        # 0 under a window: the local-chunk-first form below has no mask)
        mask = eng._window_mask()
        for g in range(m.sp_pieces):
            qg, og = q4[:, :, g * hg:(g + 1) * hg], ao4[:, :, g * hg:(g + 1) * hg]
            kc, vc = cat[g, :, :, 0:cb], cat[g, :, :, cb:]
            if g > 0 or m.sp_overlap_level == 0:
                hip.host_op(lambda g=g: self._wait(g))
                if mask is not None:
                    hip.attn_fwd_window(qg, heads(kc[:, :Lr]), heads(vc[:, :Lr]), mask[0], out=og, prescaled=True, sink=mask[1],
                                        frame_tokens=mask[2], q_offset=tok0)
                else:
                    hip.attn_fwd(qg, heads(kc[:, :Lr]), heads(vc[:, :Lr]), out=og, prescaled=True)
                continue
            assert mask is None, "a window under the overlapped K|V gather is not served"
            if Lr != self.sizes_of:                    # another clip under the same chunk size: its own key ranges
                self.sizes, self.sizes_of = key_range_sizes(Lr, m.sp, m.rank), Lr
            (n_loc, n_before, n_after), (s_loc, s_before, s_after) = self.sizes, self.splits
            n = 0
            if n_loc:
                n = hip.attn_fwd_partial(qg, heads(send[0, :, :n_loc, 0:cb]), heads(send[0, :, :n_loc, cb:]), part, 0, s_loc, prescaled=True)
            hip.host_op(lambda: self._wait(0))
            if n_before:
                n += hip.attn_fwd_partial(qg, heads(kc[:, :n_before]), heads(vc[:, :n_before]), part, n, s_before, prescaled=True)
            if n_after:
                n += hip.attn_fwd_partial(qg, heads(kc[:, tok0 + lc:Lr]), heads(vc[:, tok0 + lc:Lr]), part, n, s_after, prescaled=True)
            hip.attn_merge(og, part, n, prescaled=True)


class KVHalo:
    """The K|V gather of a windowed model that moves only the halo (FLEXAM_SP_HALO=1 under FLEXAM_SP_WINDOW=1, bf16; DiTEngine._mode):
    a rank's windowed call visits the sink tiles and one run of window tiles, so it receives those rows alone, from the peers that hold
    them, into a compact buffer [G, B, rows, 2*C/G] (dit_layout.halo_plan states rows, ranges and peers; `rows` instead of sp * lc).  The
    same RMSNorm+RoPE launch fills the same send buffer [G, B, lc, 2*C/G]; a row range of one head group and CFG row is contiguous in
    both buffers, so the ranges travel as they lie (dist.exchange_rows: one grouped send / receive for all of them) and the rank's own
    rows are one device copy.  The exchange is waited for, then one flexam_attn_fwd_window_halo call per head group runs at the rank's
    query offset on the buffer.  Every row of the buffer below `rows` is written by each exchange: a visited tile never holds stale bytes."""

    def __init__(self, eng, m, ws):
        self.group = eng.sp_group
        G = m.sp_pieces
        self.cb, self.hg = cb, hg = eng.dim // G, eng.nh // G
        self.send = torch.empty(G, m.B, m.lc, 2 * cb, device=eng.device, dtype=BF16)
        self.overlapped = group_backend(self.group) in ("nccl", "loopback")
        self.plan = self.plan_of = self.halo = self.work = None

    def _layout(self, eng, m, ws):
        """The plan and the buffer for this clip's length and mask (another clip under the same chunk size: its own)."""
        mask = eng._window_mask()
        key = (eng.cond["L"], mask)
        if key != self.plan_of:
            plan = halo_plan(eng.cond["L"], m.sp, m.rank, mask[0], mask[1], mask[2])
            send = self.send
            halo = ws["kv_halo"] = torch.empty(send.shape[0], send.shape[1], max(plan.rows, 1), send.shape[3], device=send.device, dtype=BF16)
            pairs = [(g, b) for g in range(send.shape[0]) for b in range(send.shape[1])]
            # the per-range views, made once: head group and CFG row outermost on both sides, so a peer's k-th send is my k-th receive
            self.recvs = [(peer, halo[g, b, d:d + n]) for g, b in pairs for peer, _, d, n in plan.recvs]
            self.sends = [(peer, send[g, b, s:s + n]) for g, b in pairs for peer, s, _, n in plan.sends]
            self.plan, self.plan_of, self.halo = plan, key, halo
        return self.plan, self.halo, self.recvs, self.sends

    def run(self, eng, ws, a8sa, layer, p, m):
        cd, send, cb, hg = eng.cond, self.send, self.cb, self.hg
        d, hd, lc, tok0, qkv, Lr = eng.dim, eng.hd, m.lc, m.tok0, ws["qkv"], cd["L"]
        plan, halo, recvs, sends = self._layout(eng, m, ws)
        q4, _, _, ao4 = eng._heads(m, ws)
        flat = send.view(-1)
        hip.rmsnorm_rope_scatter(None, None, qkv[:, d:2 * d], p["nk"], qkv[:, 2 * d:], None, flat, flat[cb:], ld_out=2 * cb, out_bs=lc * 2 * cb,
                                 col_block=cb, block_stride=m.B * lc * 2 * cb, eps=eng.eps, rope_cos=cd["cos"], rope_sin=cd["sin"],
                                 tokens_per_batch=lc, token_offset=tok0, head_dim=hd)

        def issue():
            self.work = exchange_rows(recvs, sends, self.group, async_op=self.overlapped, like=send)
            for s, dst, n in plan.local:
                halo[:, :, dst:dst + n].copy_(send[:, :, s:s + n])
        hip.host_op(issue)
        if not m.sp_fused_qkv:
            eng._proj(ws["h"], a8sa, layer, p, "wqkv", "bqkv", slice(0, d), qkv[:, 0:d])
        hip.rmsnorm_rope(qkv[:, 0:d], p["nq"], eps=eng.eps, rope_cos=cd["cos"], rope_sin=cd["sin"], tokens_per_batch=lc, token_offset=tok0,
                         head_dim=hd)
        hip.host_op(lambda: self.work is not None and self.work.wait())
        window, sink, T = eng._window_mask()
        heads = lambda t: t.unflatten(2, (hg, hd))
        for g in range(m.sp_pieces):
            hip.attn_fwd_window(q4[:, :, g * hg:(g + 1) * hg], heads(halo[g, :, :, 0:cb]), heads(halo[g, :, :, cb:]), window,
                                out=ao4[:, :, g * hg:(g + 1) * hg], prescaled=True, sink=sink, frame_tokens=T, q_offset=tok0,
                                key_gap_tiles=plan.gap, Lk=Lr, k_rows=plan.rows)


class RecordGather:
    """SAGE_ATTENTION under the K|V all-gather (r6; the reference's `sageattn` switch, attention_utils.py:195-203, with the exchange of
    the missing FlexAM/dist, wan_transformer3d_FlexAM.py:801-815): this rank's q, k (RMSNorm + RoPE at the chunk's global offset) and
    v become MXFP8 operands (DiTEngine._norm_rope_qk), ONE all-gather moves the key / value RECORDS ([B, H, lc / 64] x 18 KiB per rank:
    288 bytes per key and head instead of 512 in bf16; the rank-major result is the chunk layout flexam_attn_fwd_fp8_chunked reads),
    and one attention call of the local queries over all L real keys follows.  lc is a multiple of 64 (resolve_mode pads to 64 x ranks)."""

    def __init__(self, eng, m, ws):
        self.group = eng.sp_group
        records = eng._attn8_buffers(m.B, m.lc)[2]                   # (the operand buffers themselves are the engine's, shared by every block)
        self.kv8_all = torch.empty(m.sp, *records.shape, device=eng.device, dtype=torch.uint8)

    def run(self, eng, ws, a8sa, layer, p, m):
        kv8_all, group = self.kv8_all, self.group
        bufs = eng._attn8_buffers(m.B, m.lc)
        eng._norm_rope_qk(p, m, ws, m.B, bufs)
        hip.host_op(lambda: all_gather_into_tensor(kv8_all.view(m.sp * m.B, *bufs[2].shape[1:]), bufs[2], group=group))
        # a windowed model (FLEXAM_SP_SAGE_WINDOW=1): the mask at this rank's query offset, on the same records
        window, sink, T = eng._window_mask() or ((-1, -1), 0, 0)
        hip.attn_fwd_fp8_chunked(bufs[0], bufs[1], kv8_all, m.lc, eng.cond["L"], out=eng._heads(m, ws)[3], window=window, sink=sink,
                                 frame_tokens=T, q_offset=m.tok0)
