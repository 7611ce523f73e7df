// flexam_amd/csrc/attn_fp8.inc -- self-attention with MXFP8 operands (OCP e4m3 + one E8M0 scale per 32 elements), the quantised
// variant behind VIDEOX_ATTENTION_TYPE=SAGE_ATTENTION (FlexAM/models/attention_utils.py:195-203 calls the third-party `sageattn`,
// which quantises Q, K and P.V the same way; what is kept here is its contract -- softmax attention within a stated tolerance --
// not its int8 / per-block format).  Included by attn.hip inside its namespace: shares AttnParams, the work-unit walk
// (unit_of_workgroup), the epilogue (store_partial / store_output), the split-KV workspace and attn_merge_kernel with the bf16 kernel.
//
// Both products run on v_mfma_scale_f32_32x32x64_f8f6f4 (2 x the bf16 MFMA rate).  Operand maps of that instruction with e4m3 data,
// found with exact integers (tools/probes/mfma_scale32_map.hip, mfma_scale32_probe.hip): lane (r = l & 31, h = l >> 5) holds, in
// byte j = 0..31 of its 8 operand registers, k = 32 (j / 16) + 16 h + j % 16 of row (A) / column (B) r -- 16 bytes of each of the
// instruction's two 32-deep MX blocks -- and the E8M0 byte that op_sel picks from the scale register of lane (r, h) scales MX block h
// (k = 32 h .. 32 h + 31) of that row / column.  C/D as every 32x32 form.
//
//  * S^T = K.Q^T: A = 32 keys x 64 channels of the K tile, B = the wave's 32 queries; two MFMAs per 32-key half tile (bf16: 8).
//    A lane reads the 16-byte chunks 4m + h and 4m + 2 + h of its key row; the scale byte of channel block 2m + h is its own.
//  * a lane then holds 16 scores of one query per half tile, as in the bf16 kernel; the exponentials of BOTH halves of a 64-key tile,
//    packed to e4m3 (v_cvt_pk_fp8_f32), are the 32 bytes of the B operand of O^T += V^T.P^T, one MFMA per 32 channels of V and tile
//    (bf16: 4).  Byte j of lane half h is key 32 (j / 16) + 8 ((j % 16) / 4) + 4 h + j % 4 of the tile, so the V^T operand must carry
//    the keys in that order: flexam_attn_fp8_pack writes V transposed, [128 channels][64 key positions], with exactly that order
//    inside a row, and one scale per channel and 32-key half tile (= MX block).
//  * P is at most 2^8.5 = 362 < 448: the row reference of the online softmax is set 2^6 below the row maximum and raised when a
//    score exceeds it by more than 2^8.5; e4m3 then resolves weights down to 2^-15 ... 2^-17.5 of the row maximum.  The row sums
//    are taken from the unrounded fp32 exponentials.
//  * The reference only moves by WHOLE powers of two, and a move rescales nothing but the row sum: the E8M0 scale that the P.V MFMA
//    applies to its B operand for free carries 2^(ref - ref0), so every tile's product lands in the units of the FIRST reference
//    (lane half h supplies the scale of MX block h = the tile's half h, i.e. the reference in force when that half was
//    exponentiated).  O and the packed P are never touched -- the rescale branch of the bf16 kernel (64 + 12 registers rewritten,
//    and hipcc's copies of all of them on the not-taken path) is three instructions here.  ref - ref0 is capped at 96 (fp32 O):
//    scores more than 2^96 above the first half tile's maximum saturate at the cap (66 nats; the bf16 kernel has no such limit).
//  * K, V and their scales of one (batch, head, 64-key tile) are ONE 18 KiB record, written by the pack kernel as the LDS image
//    (XOR swizzles included): a tile arrives by lane-linear LDS-DMA pieces, no source-side address arithmetic -- per wave 1 KiB of K,
//    1 KiB of V and 256 B of the scale area (every wave issues the same three instructions: a branch around the scale piece of a
//    single wave would be a basic-block boundary in the loop, see the steps).
constexpr int REC_V = 8192, REC_KS = 16384, REC_VS = 16640, REC_BYTES = 18432;   // [K image 8 KiB][V^T image 8 KiB][K scales 256 B][V scales 256 B][unused 1.5 KiB]
constexpr float F8_REF_HEAD = 6.0f, F8_RESCALE_THR = 8.5f, F8_RD_MAX = 96.0f;

typedef int i32x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ i32x8 join8(u32x4 lo, u32x4 hi) {
  return (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// The mask of the windowed instances (attn8_window_kernel, attn8_window_oshift_kernel; flexam_attn_fwd_fp8_window), a kernel argument of
// their own: in AttnParams the window words of the bf16 kernel ARE the MXFP8 words (qs, lq_pad, the two chunk words), which this kernel
// reads, and a longer AttnParams would move the kernarg loads of every other instance.  Lq == Lk = L; row i sees key j iff j < sink or
// lo(i) <= j <= hi(i), with lo = i - left, hi = i + right in tokens (frame = 0), or lo = (i / T - left) T, hi = (i / T + right + 1) T - 1
// with frame = T > 0; a negative side is unbounded.  The rule of the bf16 kernel's WIN / FRAMES instances (attn.hip).
struct Attn8Window { int left, right, sink, frame; };
// ... and that of the instances at a query offset (attn8_window_at_kernel, attn8_window_at_oshift_kernel; flexam_attn_fwd_fp8_window_at): a
// sibling, so that the two kernels above keep their argument.  Row i of the call is global token g = q_offset + i and sees key j
// (0 <= j < Lk) iff j < sink or lo(g) <= j <= hi(g): a rank's lc queries against the records of every rank's chunk, Lq and Lk two lengths
struct Attn8WindowAt { Attn8Window w; int q_offset; };

// The kernel's body, inlined into its __global__ wrappers below (KIND: the profiler symbol, as attn_fwd_kernel's).  OSHIFT: the
// epilogue adds p.o_shift (smooth-V) to O / l in fp32 in front of the rounding to bf16 -- loaded behind the key loop, nothing of it inside.
// p by value, as the kernel had it: by reference hipcc allocates the loop differently (186 instead of 188 VGPRs, another schedule).
// WIN (whole units only): the unit walks the sink tiles and the key tiles that hold a key one of its 256 rows sees, as the bf16 kernel's
// WIN instance does and by its arithmetic (local tile indices in the loop and the ring; issue_tile maps them to global tiles).  Tiles in
// which every row sees every key run the step as it is; in the others -- the ragged last tile among them -- ONE uniform branch in front of
// the row maxima sets the scores of the keys the lane's row does not see to -inf (mask_window; keys past L lie past every row's hi).
// A row's reference cannot come from half tile 0, in which the row may see no key: it stays 0 and the row `unstarted` (gate = -inf: any
// finite score passes the test of the rescale branch) until the first half tile in which it sees one, whose maximum sets the first
// reference the way the prologue does for every row of the other instances -- O = l = 0 until then, so nothing is rescaled, and rd
// counts from there.  A half tile in which a row sees nothing is all -inf: its maximum moves no reference (-inf passes no test; the
// factors are selected, never computed from it) and its exponentials are exactly 0.  Every row sees its own key: l > 0 at the end.
// AT (on top of WIN; g0 = the global token of the call's row 0): the unit's bounds and the lane's row are taken at g0 + ..., the keys are
// the first Lk tokens and their records come in chunks ([chunk][B][H][chunk_tiles], as the unwindowed kernel reads them).  Rows from
// global token Lk on are pad rows: queries, never keys.  A unit none of whose rows sees a key issues no tile and writes zeros
// (attn_fwd_body's arithmetic for it, attn.hip); a row that sees no key in a unit that walks some stays unstarted to the end -- O = l = 0,
// reference 0 -- and is written as zeros (with OSHIFT too), not as 0 / 0.
template <int KIND, bool OSHIFT, bool WIN = false, bool AT = false>
__device__ __forceinline__ void attn8_fwd_body(const AttnParams p, const Attn8Window w = {}, const int g0 = 0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // ring of 4 records
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r_ = lane & 31, h_ = lane >> 5;

  int split = 0, ul, unit, tps = p.tiles_per_split, partial = p.partial;
  if (!unit_of_workgroup(p, split, ul, unit, tps, partial)) return;
  int qb = unit % p.q_blocks;
  if constexpr (WIN) qb = w.left < 0 ? p.q_blocks - 1 - qb : qb;      // units of a window without a left bound grow with the q block: longest first
  const int bh = unit / p.q_blocks;
  const int head = bh % p.H, b = bh / p.H;

  // ---- Q operand (B of S^T = K.Q^T) in registers: rows are padded to whole 256-row blocks by the pack kernel, so no clamp
  const int q0 = qb * QBLK + wave * 32;
  const int64_t qidx = (int64_t)bh * p.lq_pad + q0 + r_;
  i32x8 qf[2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
    qf[m] = join8(*(const u32x4*)(p.q8 + qidx * 128 + 16 * (4 * m + h_)), *(const u32x4*)(p.q8 + qidx * 128 + 16 * (4 * m + 2 + h_)));
  auto q_read = [&](int m) -> i32x8 { return qf[m]; };
  const int qsc = (int)(p.qs[qidx] >> (8 * h_));      // byte 0: channel block h, byte 2: block 2 + h

  // ---- LDS read addresses inside a record (slot, half tile and channel block are immediates)
  const char* kaddr[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int x = 0; x < 2; ++x) kaddr[m][x] = smem + r_ * 128 + 16 * ((4 * m + 2 * x + h_) ^ ((r_ >> 1) & 7));
  const char* ksaddr = smem + REC_KS + 4 * r_;
  int sh8 = 8 * h_;                                   // the one lane-half value the loop keeps (the tail's key mask derives 4 h from it)
  asm volatile("" : "+v"(sh8));
  const char* vaddr[2];
#pragma unroll
  for (int x = 0; x < 2; ++x) vaddr[x] = smem + REC_V + r_ * 64 + 16 * ((2 * x + h_) ^ ((r_ >> 2) & 3));
  const char* vsaddr = smem + REC_VS + 2 * r_ + h_;

  const int tiles_all = (p.Lk + KVBLK - 1) / KVBLK;
  // WIN: the unit's w_n tiles = the sink tiles [0, s_n), then (behind `gap` tiles no row sees) the window's; [ti_lo, ti_hi] (local) are the
  // window tiles every row sees whole, s_full the tiles wholly below the sink.  attn_fwd_body's arithmetic, word for word (restated, not
  // shared: the bf16 windowed instances keep the parent's machine code, and FRAMES is a template argument there, w.frame > 0 a test here)
  int w_n = 0, ti_lo = 0, ti_hi = 0, s_n = 0, s_full = 0, gap = 0;
  if constexpr (WIN) {
    const int qa = g0 + qb * QBLK, qz = g0 + min(qb * QBLK + QBLK, p.Lq) - 1;      // first and last row of the unit (AT: as global tokens)
    int fa = 0, fz = 0;
    if (w.frame > 0) { fa = (int)((unsigned)qa / (unsigned)w.frame); fz = (int)((unsigned)qz / (unsigned)w.frame); }
    const int lo_a = w.frame > 0 ? (fa - w.left) * w.frame : qa - w.left;
    const int hi_z = w.frame > 0 ? (fz + w.right + 1) * w.frame - 1 : qz + w.right;
    const int k_first = w.left < 0 ? 0 : max(0, lo_a);
    const int k_last = w.right < 0 ? p.Lk - 1 : min(p.Lk - 1, hi_z);
    s_n = (min(w.sink, p.Lk) + KVBLK - 1) / KVBLK;
    s_full = w.sink / KVBLK;
    gap = max(0, k_first / KVBLK - s_n);
    w_n = max(k_last / KVBLK, s_n - 1) + 1 - gap;
    if constexpr (AT) if (k_first > k_last) { gap = 0; w_n = s_n; }      // every row's window lies behind the last key: the sink tiles alone, or none
    const int lo_z = w.frame > 0 ? (fz - w.left) * w.frame : qz - w.left;
    ti_lo = w.left < 0 ? 0 : (max(0, lo_z) + KVBLK - 1) / KVBLK;
    const int hi_a = w.frame > 0 ? (fa + w.right + 1) * w.frame - 1 : qa + w.right;
    const int top_key = hi_a - (KVBLK - 1);
    ti_hi = min(w.right < 0 ? tiles_all : top_key >= 0 ? top_key / KVBLK : -1, p.Lk / KVBLK - 1);      // (whole tiles only)
    ti_lo -= gap;
    ti_hi -= gap;
  }
  const int t0 = WIN ? 0 : split * tps;
  const int ntiles = WIN ? w_n : min(tps, tiles_all - t0);
  if constexpr (AT) {
    if (ntiles == 0) {                       // no row of the unit sees a key: zeros, and no record read (uniform over the workgroup)
      f32x16 z[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) z[dt][e] = 0.f;
      store_output(p, z, 0.f, b, head, q0 + r_, h_);
      return;
    }
  }
  // records: [chunk][B][H][chunk_tiles]; one chunk holds all tiles unless the records came out of a sequence-parallel all-gather
  // (flexam_attn_fwd_fp8_chunked).  Tile g = t0 + t -> chunk g / chunk_tiles by one scalar multiply-high (uniform: scalar registers)
  const unsigned ct = (unsigned)p.kv8_chunk_tiles, cmagic = p.kv8_chunk_magic;
  const int64_t chunk_recs = (int64_t)p.B * p.H * ct;
  const char* rec0 = (const char*)p.kv8 + (int64_t)bh * ct * REC_BYTES;
  const unsigned lds0 = (unsigned)(size_t)LDS_PTR(smem);
  const unsigned voff16 = (unsigned)tid * 16u;
  auto issue_tile = [&](int t, int parts, int tslot = -1) {      // parts: 1 = K (+ the scales of both), 2 = V; tslot: the ring position (default t)
    const unsigned slot = lds0 + (unsigned)(((tslot < 0 ? t : tslot) & (NSLOT - 1)) * REC_BYTES);
    const unsigned gt = WIN ? (unsigned)(t < s_n ? t : t + gap) : (unsigned)(t0 + t);      // (WIN: one chunk holds all tiles)
    const unsigned chunk = WIN && !AT ? 0u : ct > 1 ? __umulhi(gt, cmagic) : gt;      // (AT: the global tile through the chunk table)
    const char* src = rec0 + (chunk * chunk_recs + (gt - chunk * ct)) * REC_BYTES;
    if (parts & 1) {
      lds_dma16_sbase(src, voff16, slot + wave * 1024);
      const unsigned voff4 = voff16 >> 2;          // rebuilt per tile: one register less across the loop
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff4), "s"(src + REC_KS), "s"(slot + REC_KS + wave * 256) : "memory");
    }
    if (parts & 2) lds_dma16_sbase(src + REC_V, voff16, slot + REC_V + wave * 1024);
  };

  // The row reference is subtracted from the scores in front of the exponentials (packed fp32 adds).  (As the C operand of the first
  // MFMA of every chain, as in the bf16 kernel, it costs a 16-register tuple this loop does not have: 316 bytes of scratch.)
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float ref = 0.f;
  auto k_read = [&](auto ghalf_c, auto m_c) -> i32x8 {
    constexpr int ghalf = decltype(ghalf_c)::value, m = decltype(m_c)::value;
    constexpr int imm = ((ghalf >> 1) & (NSLOT - 1)) * REC_BYTES + (ghalf & 1) * 4096;
    return join8(*(const u32x4*)(kaddr[m][0] + imm), *(const u32x4*)(kaddr[m][1] + imm));
  };
  auto ks_read = [&](auto ghalf_c) -> int {
    constexpr int ghalf = decltype(ghalf_c)::value;
    constexpr int imm = ((ghalf >> 1) & (NSLOT - 1)) * REC_BYTES + (ghalf & 1) * 128;
    return (int)(*(const unsigned*)(ksaddr + imm) >> sh8);
  };
  // keys past Lk (or past this split's range) -> -inf.  No branch: the tail tiles keep the one-block shape of the main loop's steps.
  auto mask_half = [&](int g, f32x16& sacc) {
    const int gg = 2 * t0 + g;
    const int lim = g >= 2 * ntiles ? 0 : p.Lk - gg * 32 - (sh8 >> 1);      // keys of this half with (e & 3) + 8 (e >> 2) < lim are valid
#pragma unroll
    for (int e = 0; e < 16; ++e) sacc[e] = (e & 3) + 8 * (e >> 2) < lim ? sacc[e] : -INFINITY;
  };
  // WIN: keys the lane's row does not see -> -inf.  Element e is key 32 gg + 4 h + (e & 3) + 8 (e >> 2) of global half gg; the row's bounds
  // (hi clipped to the last key: this is the mask of the ragged tile too) and the sink less 4 h are the three per-lane values, the
  // half's base is uniform.  The visible in-half positions as ONE bit mask, as attn_fwd_body's mask_window has them and for its reason.
  int w_lo = 0, w_hi = 0, w_sk = 0;
  if constexpr (WIN) {
    const int row = g0 + q0 + r_, h4 = 4 * h_;      // (AT: the lane's row as a global token)
    const int f = w.frame > 0 ? (int)((unsigned)row / (unsigned)w.frame) : 0;
    w_lo = w.left < 0 ? -(1 << 30) : (w.frame > 0 ? (f - w.left) * w.frame : row - w.left) - h4;
    w_hi = (w.right < 0 ? p.Lk - 1 : min(p.Lk - 1, w.frame > 0 ? (f + w.right + 1) * w.frame - 1 : row + w.right)) - h4;
    w_sk = w.sink - h4;
  }
  auto mask_window = [&](int g, f32x16& sacc) {
    const int tl = g >> 1;
    const int base = (2 * (tl < s_n ? tl : tl + gap) + (g & 1)) * 32;
    const int lo = w_lo - base, hi = w_hi - base, sk = w_sk - base;
    const unsigned below_sk = (1u << min(max(sk, 0), 28)) - 1u, below_lo = (1u << min(max(lo, 0), 28)) - 1u, to_hi = (1u << min(max(hi + 1, 0), 28)) - 1u;
    const unsigned seen = below_sk | (to_hi & ~below_lo);
#pragma unroll
    for (int e = 0; e < 16; ++e) sacc[e] = seen & (1u << ((e & 3) + 8 * (e >> 2))) ? sacc[e] : -INFINITY;
  };
  float gate = WIN ? -INFINITY : F8_RESCALE_THR;      // WIN: what a row's maximum less its reference must exceed for the reference to move; -inf = unstarted
  f32x16 o_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o_acc[dt][e] = 0.f;
  // packed P of two consecutive tiles, ping-ponged by tile parity: while tile t is exponentiated into one, the PV of tile t - 1 reads the other
  i32x8 pk[2];
#pragma unroll
  for (int w = 0; w < 8; ++w) { pk[0][w] = 0; pk[1][w] = 0; }
  auto v_read = [&](auto tslot_c, auto dt_c, i32x8& vf, int& vs) __attribute__((always_inline)) {
    constexpr int slot = decltype(tslot_c)::value & (NSLOT - 1), dt = decltype(dt_c)::value;
    constexpr int imm = slot * REC_BYTES + dt * 2048;
    vf = join8(*(const u32x4*)(vaddr[0] + imm), *(const u32x4*)(vaddr[1] + imm));
    vs = (int)*(const unsigned char*)(vsaddr + slot * REC_BYTES + dt * 64);
  };
  float l_run = 0.f;
  float rd = 0.f;            // ref - ref0, a whole number; psc_now = its E8M0 byte; psc[tile parity] = the byte each lane hands the P.V MFMA
  int psc_now = 127, psc[2] = {127, 127};

  // ---- prologue: tiles 0 and 1 on their way; the V image and V scales that PV(-1) multiplies by P = 0 must hold finite numbers
  *(u32x4*)(smem + (NSLOT - 1) * REC_BYTES + REC_V + tid * 16) = (u32x4){0u, 0u, 0u, 0u};
  if (tid < 16) *(u32x4*)(smem + (NSLOT - 1) * REC_BYTES + REC_VS + tid * 16) = (u32x4){0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu};
  issue_tile(0, 3);
  if (ntiles > 1) issue_tile(1, 3);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  f32x16 s_a, s_b;
  {
    const int ks = ks_read(IC<0>{});
    s_a = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(k_read(IC<0>{}, IC<0>{}), q_read(0), zero16, 0, 0, 0, ks, 0, qsc);
    s_a = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(k_read(IC<0>{}, IC<1>{}), q_read(1), s_a, 0, 0, 2, ks, 2, qsc);
  }
  i32x8 kf_pre = k_read(IC<1>{}, IC<0>{});
  int ks_nxt = ks_read(IC<1>{});
  if constexpr (!WIN) {   // the first reference (= ref0): a whole number 2^6 ... 2^7 below the row maximum of half tile 0's VALID keys -- a range whose
      // only tile holds fewer than 32 keys has padding here (zero rows: score 0), which would otherwise set ref0 and flush P to zero
    mask_half(0, s_a);
    float mx = s_a[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) mx = fmaxf(mx, s_a[e]);
    ref = floorf(pair_max(mx)) - F8_REF_HEAD;
  }

  // A half-tile step g (tile t = g >> 1) in two parts, as in the bf16 kernel.
  //  part A: first MFMA of S(g+1) | row maximum of S(g), the (rare) move of the reference
  //  part B: second MFMA of S(g+1), two of the four MFMAs of PV(t-1) | exp2, row sum, e4m3 pack of S(g) into its half of P(t)
  // The common path of the main loop is ONE basic block per step apart from the rescale branch (no key mask: MASK = false; the
  // LDS-DMA of a tile past the end re-reads the last tile into a free slot instead of branching): across block boundaries hipcc
  // sinks every MFMA down to the block of its first use, i.e. S(g+1) to just in front of its row maxima and the PVs into the next
  // step, and the matrix pipe then runs serially with the softmax.  The rescale branch uses the accumulators and (empty asm)
  // S(g+1), which keeps their MFMAs in front of it.
  auto stepA = [&](int g, auto g8_c, auto mask_c, f32x16& s_cur, f32x16& s_nxt) __attribute__((always_inline)) {
    constexpr bool MASK = decltype(mask_c)::value;
    constexpr int g8 = decltype(g8_c)::value;
    constexpr int cur = (g8 >> 1) & 1;                   // pk[cur]: this tile's P, pk[cur ^ 1]: the previous tile's
    if constexpr (MASK) mask_half(g, s_cur);
    if constexpr (WIN) {
      const int tl = g >> 1;               // (local: a tile below s_full is its own global index)
      if (tl >= s_full && (tl < ti_lo || tl > ti_hi)) mask_window(g, s_cur);
    }
    // first K fragment and the scales of the next half tile: read here, used behind the row maxima (held across part B of the
    // previous step instead, they are 8 registers the loop does not have)
    const i32x8 kf0 = kf_pre;                         // read behind the last MFMA of the previous step (part B, block 3)
    const i32x8 qf0 = q_read(0);                      // (its Q partner here, under the row maxima: 8 registers less across the step boundary)
    const float m0 = vmax8(s_cur[0], s_cur[1], s_cur[2], s_cur[3], s_cur[4], s_cur[5], s_cur[6], s_cur[7]);
    const float m1 = vmax8(s_cur[8], s_cur[9], s_cur[10], s_cur[11], s_cur[12], s_cur[13], s_cur[14], s_cur[15]);
    const float mloc = vmax(m0, m1) - ref;            // relative to the row reference
    s_nxt = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf0, qf0, zero16, 0, 0, 0, ks_nxt, 0, qsc);
    if (WIN ? __any(mloc > gate) : __any(mloc > F8_RESCALE_THR)) {
      // rows whose maximum stays below the threshold keep their reference; the others move it by a whole number to 2^6 ... 2^7
      // below the maximum (as far as the cap allows).  Only the row sum is rescaled (see the file header).
      const float mx = pair_max(mloc);
      float delta = fminf(mx > F8_RESCALE_THR ? floorf(mx - F8_REF_HEAD) : 0.f, F8_RD_MAX - rd);
      if constexpr (WIN) {
        // an unstarted row (reference 0, O = l = 0, rd = 0) takes floor(its first maximum) - 6 as its FIRST reference: rd stays 0, the
        // cap counts from here, nothing is rescaled; while that maximum is -inf the row stays unstarted
        const bool started = gate > -INFINITY, live = mx > -INFINITY;
        const float first = live ? floorf(mx) - F8_REF_HEAD : 0.f;
        ref += started ? 0.f : first;
        delta = started ? delta : 0.f;
        gate = started || live ? F8_RESCALE_THR : -INFINITY;
      }
      ref += delta;
      rd += delta;
      l_run *= __builtin_amdgcn_exp2f(-delta);
      psc_now = 127 + (int)rd;
#pragma unroll
      for (int e = 0; e < 16; ++e) s_cur[e] = fminf(s_cur[e], ref + F8_RESCALE_THR);      // only bites at the cap
      // empty asm: the accumulators and S(g+1) count as used here, which keeps their MFMAs in front of this branch -- hipcc sinks an
      // MFMA whose result nothing in the step reads down to the end of the 4-tile loop body (and spills the fragments it waits with)
      asm volatile("" : "+v"(s_nxt), "+v"(o_acc[0]), "+v"(o_acc[1]), "+v"(o_acc[2]), "+v"(o_acc[3]));
    }
    psc[cur] = h_ == (g8 & 1) ? psc_now : psc[cur];      // lane half h answers for the tile's half h
  };
  // Part B is written as three fenced blocks (sched_barrier): left to itself hipcc hoists all eleven LDS reads to the top, runs the
  // three MFMAs first and the softmax behind them with every fragment live -- and spills 80 registers.
  auto stepB = [&](auto g8_c, f32x16& s_cur, f32x16& s_nxt) __attribute__((always_inline)) {
    constexpr int g8 = decltype(g8_c)::value;            // g mod 8
    constexpr int odd = g8 & 1;
    constexpr int cur = (g8 >> 1) & 1;
    constexpr int ps = (g8 >> 1) + 3;                    // PV of the previous tile: its record sits in slot (t - 1) & 3
    float psum;
    const f32x2 ref2 = {ref, ref};
    auto exp4 = [&](int w) __attribute__((always_inline)) {
      const f32x2 a = (f32x2){s_cur[4 * w], s_cur[4 * w + 1]} - ref2, b = (f32x2){s_cur[4 * w + 2], s_cur[4 * w + 3]} - ref2;
      const float p0 = __builtin_amdgcn_exp2f(a[0]), p1 = __builtin_amdgcn_exp2f(a[1]);
      const float p2 = __builtin_amdgcn_exp2f(b[0]), p3 = __builtin_amdgcn_exp2f(b[1]);
      psum = w == 0 ? (p0 + p1) + (p2 + p3) : psum + ((p0 + p1) + (p2 + p3));
      int o = pk[cur][4 * odd + w];
      o = __builtin_amdgcn_cvt_pk_fp8_f32(p0, p1, o, false);
      o = __builtin_amdgcn_cvt_pk_fp8_f32(p2, p3, o, true);
      pk[cur][4 * odd + w] = o;
    };
    // block 1: fragments of the first two MFMAs on their way | half of the exponentials
    __builtin_amdgcn_sched_barrier(0);
    const i32x8 kf1 = k_read(IC<((g8 + 1) & 7)>{}, IC<1>{});
    const i32x8 qf1 = q_read(1);
    i32x8 vf0, vf1;
    int vs0, vs1;
    v_read(IC<ps>{}, IC<2 * odd>{}, vf0, vs0);
    exp4(0);
    exp4(1);
    __builtin_amdgcn_sched_barrier(0);
    // block 2: second MFMA of S(g+1), first PV | the other fragments, the other half of the exponentials
    s_nxt = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf1, qf1, s_nxt, 0, 0, 2, ks_nxt, 2, qsc);
    o_acc[2 * odd] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf0, pk[cur ^ 1], o_acc[2 * odd], 0, 0, 0, vs0, 0, psc[cur ^ 1]);
    exp4(2);
    __builtin_amdgcn_sched_barrier(0);
    v_read(IC<ps>{}, IC<2 * odd + 1>{}, vf1, vs1);
    exp4(3);
    __builtin_amdgcn_sched_barrier(0);
    // block 3: second PV
    o_acc[2 * odd + 1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf1, pk[cur ^ 1], o_acc[2 * odd + 1], 0, 0, 0, vs1, 0, psc[cur ^ 1]);
    l_run += psum;
    asm volatile("" : "+v"(pk[cur]), "+v"(l_run));
    // first fragments and K scales of S(g+2) for the next step's part A: the registers of this step's fragments are free from here
    kf_pre = k_read(IC<((g8 + 2) & 7)>{}, IC<0>{});
    ks_nxt = ks_read(IC<((g8 + 2) & 7)>{});
    __builtin_amdgcn_sched_barrier(0);
  };
  auto tile = [&](int t, auto t4_c, auto mask_c) __attribute__((always_inline)) {
    constexpr int t4 = decltype(t4_c)::value;
    // top of tile t: tile t + 1 (issued one tile ago) has landed and becomes visible; the slot of tile t - 2 is free again
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    const int tn = min(t + 2, ntiles - 1);               // past the end: the last tile once more, into a slot nobody reads
    issue_tile(tn, 1, t + 2);
    stepA(2 * t, IC<2 * t4>{}, mask_c, s_a, s_b);
    stepB(IC<2 * t4>{}, s_a, s_b);
    issue_tile(tn, 2, t + 2);
    stepA(2 * t + 1, IC<2 * t4 + 1>{}, mask_c, s_b, s_a);
    stepB(IC<2 * t4 + 1>{}, s_b, s_a);
  };
  using T_ = std::integral_constant<bool, true>;
  using F_ = std::integral_constant<bool, false>;
  int t = 0;
  using M_ = F_;
  for (; t + 4 < ntiles; t += 4) {                       // whole tiles that are not the last one: no key mask
    tile(t, IC<0>{}, M_{});
    tile(t + 1, IC<1>{}, M_{});
    tile(t + 2, IC<2>{}, M_{});
    tile(t + 3, IC<3>{}, M_{});
  }
  const int rem = ntiles - t;               // 1..4 tail tiles (the last one may be partial), same code with static slots and the mask
  using TM_ = std::integral_constant<bool, !WIN>;      // (WIN: mask_window masks the keys past the end as well)
  tile(t, IC<0>{}, TM_{});
  if (rem > 1) tile(t + 1, IC<1>{}, TM_{});
  if (rem > 2) tile(t + 2, IC<2>{}, TM_{});
  if (rem > 3) tile(t + 3, IC<3>{}, TM_{});
  // pending PV of the last tile: slot (ntiles - 1) & 3, operand pk[(ntiles - 1) & 1]
  auto pv_last = [&](auto slot_c) {
    constexpr int sl = decltype(slot_c)::value;
    i32x8 vf[4];
    int vs[4];
    v_read(slot_c, IC<0>{}, vf[0], vs[0]);
    v_read(slot_c, IC<1>{}, vf[1], vs[1]);
    v_read(slot_c, IC<2>{}, vf[2], vs[2]);
    v_read(slot_c, IC<3>{}, vf[3], vs[3]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      o_acc[dt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf[dt], pk[sl & 1], o_acc[dt], 0, 0, 0, vs[dt], 0, psc[sl & 1]);
  };
  switch ((ntiles - 1) & 3) {
    case 0: pv_last(IC<0>{}); break;
    case 1: pv_last(IC<1>{}); break;
    case 2: pv_last(IC<2>{}); break;
    default: pv_last(IC<3>{}); break;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue (store_partial / store_output of attn.hip).  Lane-derived values are rebuilt from a fresh lane id: kept alive across
  // the loop they are registers it does not have (spill slots)
  const float l_tot = pair_sum(l_run);
  const float osc = __builtin_amdgcn_exp2f(-rd);       // O is in the units of the first reference, the row sum in those of the last
  const int le = fresh_lane(), r = le & 31, h = le >> 5;
  if (partial) {
    store_partial<true>(p, o_acc, osc, ref, l_tot, split, ul, wave, r, h, q0 + r);      // reference in exp2 units (the merge runs in its prescaled form)
    return;
  }
  if constexpr (AT) store_output<OSHIFT, true>(p, o_acc, l_tot > 0.f ? osc / l_tot : 0.f, b, head, q0 + r, h);      // (a row that saw no key is zeros)
  else store_output<OSHIFT>(p, o_acc, osc / l_tot, b, head, q0 + r, h);
}

template <int KIND>
__global__ __launch_bounds__(NT, 2) void attn8_fwd_kernel(AttnParams p) { attn8_fwd_body<KIND, false>(p); }
// the same kernel with the output shift: a symbol of its own (flexam_attn_fwd_fp8_oshift)
__global__ __launch_bounds__(NT, 2) void attn8_oshift_kernel(AttnParams p) { attn8_fwd_body<0, true>(p); }
// The windowed instances (flexam_attn_fwd_fp8_window), without and with the output shift.  Templates for the order of emission alone:
// hipcc emits a template's instances in the order of their first use, and attn8_window_instance at the end of attn.hip is theirs -- a
// listing of that file then differs from one without them by the two kernels alone (tools/isa_diff.py), the labels of the others included
template <int KIND>
__global__ __launch_bounds__(NT, 2) void attn8_window_kernel(AttnParams p, Attn8Window w) { attn8_fwd_body<KIND, false, true>(p, w); }
template <int KIND>
__global__ __launch_bounds__(NT, 2) void attn8_window_oshift_kernel(AttnParams p, Attn8Window w) { attn8_fwd_body<KIND, true, true>(p, w); }
// ... and the windowed instances at a query offset on chunked records (flexam_attn_fwd_fp8_window_at), emitted behind those by
// attn8_window_at_instance at the end of attn.hip
template <int KIND>
__global__ __launch_bounds__(NT, 2) void attn8_window_at_kernel(AttnParams p, Attn8WindowAt a) { attn8_fwd_body<KIND, false, true, true>(p, a.w, a.q_offset); }
template <int KIND>
__global__ __launch_bounds__(NT, 2) void attn8_window_at_oshift_kernel(AttnParams p, Attn8WindowAt a) { attn8_fwd_body<KIND, true, true, true>(p, a.w, a.q_offset); }

// ---- the pack kernel: q, k (after RMSNorm + RoPE; q carrying softmax_scale * log2 e) and v, bf16 [B, L, H, 128] -> MXFP8 operands.
// One workgroup per (64-token tile, head, batch).  K and Q: thread = (token row, 32-channel block); V: thread = (channel, 32-key half
// tile) reading its column from an LDS copy of the V tile.
struct Attn8Pack {
  const bf16 *q, *k, *v;
  int64_t q_bs, q_rs, k_bs, k_rs, v_bs, v_rs;
  unsigned char* q8;
  unsigned char* qs;      // [B][H][lq_pad][4] E8M0 bytes (read as one dword per row by the attention kernel)
  unsigned char* kv8;
  int H, L, lq_pad, tiles;
  const float* k_shift;   // SHIFT instances only (flexam_attn_fp8_pack_shift): fp32 [B][H * 128], subtracted from K before it is quantised
  const float* v_shift;   // VSHIFT instances only (flexam_attn_fp8_pack_shift_kv): fp32 [B][H * 128], subtracted from V before it is quantised
};

// smallest power of two 2^e with amax * 2^-e <= 448 (the largest e4m3 number): returns the E8M0 byte e + 127 and 2^-e
__device__ __forceinline__ unsigned mx_scale(float amax, float& inv) {
  const unsigned bits = __float_as_uint(amax * (1.0f / 448.0f));
  int e = (int)((bits >> 23) & 255u) + ((bits & 0x7FFFFFu) ? 1 : 0);      // biased exponent of the power of two >= amax / 448
  e = e < 1 ? 1 : (e > 253 ? 253 : e);
  inv = __uint_as_float((unsigned)(254 - e) << 23);
  return (unsigned)e;
}

template <bool SHIFT, bool VSHIFT = false>
__global__ __launch_bounds__(256) void attn8_pack_kernel(Attn8Pack a) {
  __shared__ __attribute__((aligned(16))) bf16 vt[64 * 128];
  const int tid = threadIdx.x, tile = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int64_t bh = (int64_t)b * a.H + head;
  unsigned char* rec = a.kv8 + (bh * a.tiles + tile) * REC_BYTES;
  const bool has_kv = tile < a.tiles;
  // V tile -> LDS (rows past L: zeros)
  if (has_kv) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + 256 * i, row = idx >> 4, ch = idx & 15, tok = tile * 64 + row;
      u32x4 x = {0u, 0u, 0u, 0u};
      if (tok < a.L) x = *(const u32x4*)(a.v + (int64_t)b * a.v_bs + (int64_t)tok * a.v_rs + head * HD + ch * 8);
      *(u32x4*)(vt + row * 128 + ch * 8) = x;
    }
  }
  // K and Q rows
  {
    const int row = tid >> 2, blk = tid & 3, tok = tile * 64 + row;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      if (which == 0 && !has_kv) continue;
      if (!a.q) continue;                                // V-only call: Q and K rows come from flexam_rmsnorm_rope_mx
      const bf16* src = which == 0 ? a.k + (int64_t)b * a.k_bs + (int64_t)tok * a.k_rs : a.q + (int64_t)b * a.q_bs + (int64_t)tok * a.q_rs;
      float x[32];
      if (tok < a.L) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bf16x8 v8 = *(const bf16x8*)(src + head * HD + 32 * blk + 8 * c);
#pragma unroll
          for (int j = 0; j < 8; ++j) x[8 * c + j] = bf2f(v8[j]);
        }
        if constexpr (SHIFT) {
          if (which == 0) {                              // smooth-K: k - shift in fp32, one rounding; rows past L stay zero rows
            const float* sh = a.k_shift + bh * HD + 32 * blk;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
              const f32x4 s4 = *(const f32x4*)(sh + 4 * c);
#pragma unroll
              for (int j = 0; j < 4; ++j) x[4 * c + j] -= s4[j];
            }
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 32; ++j) x[j] = 0.f;
      }
      float amax = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(x[j]));
      float inv;
      const unsigned sb = mx_scale(amax, inv);
      unsigned w[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int o = 0;
        o = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * j] * inv, x[4 * j + 1] * inv, o, false);
        o = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * j + 2] * inv, x[4 * j + 3] * inv, o, true);
        w[j] = (unsigned)o;
      }
      if (which == 0) {
#pragma unroll
        for (int xh = 0; xh < 2; ++xh)
          *(u32x4*)(rec + row * 128 + 16 * ((2 * blk + xh) ^ ((row >> 1) & 7))) = (u32x4){w[4 * xh], w[4 * xh + 1], w[4 * xh + 2], w[4 * xh + 3]};
        rec[REC_KS + 4 * row + blk] = (unsigned char)sb;
      } else {
        unsigned char* dst = a.q8 + (bh * a.lq_pad + tok) * 128 + 32 * blk;
        *(u32x4*)dst = (u32x4){w[0], w[1], w[2], w[3]};
        *(u32x4*)(dst + 16) = (u32x4){w[4], w[5], w[6], w[7]};
        a.qs[(bh * a.lq_pad + tok) * 4 + blk] = (unsigned char)sb;
      }
    }
  }
  if (!has_kv) return;
  __syncthreads();
  {
    const int d = tid >> 1, bb = tid & 1;
    float x[32];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int e = 0; e < 16; ++e) x[16 * hh + e] = bf2f(vt[(32 * bb + (e & 3) + 8 * (e >> 2) + 4 * hh) * 128 + d]);
    if constexpr (VSHIFT) {                                // smooth-V: v - shift in fp32, one rounding; keys past L stay zero, not -shift
      const float sh = a.v_shift[bh * HD + d];
      const int key0 = tile * 64 + 32 * bb;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (key0 + (e & 3) + 8 * (e >> 2) + 4 * hh < a.L) x[16 * hh + e] -= sh;
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(x[j]));
    float inv;
    const unsigned sb = mx_scale(amax, inv);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      unsigned w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int o = 0;
        o = __builtin_amdgcn_cvt_pk_fp8_f32(x[16 * hh + 4 * j] * inv, x[16 * hh + 4 * j + 1] * inv, o, false);
        o = __builtin_amdgcn_cvt_pk_fp8_f32(x[16 * hh + 4 * j + 2] * inv, x[16 * hh + 4 * j + 3] * inv, o, true);
        w[j] = (unsigned)o;
      }
      *(u32x4*)(rec + REC_V + d * 64 + 16 * ((2 * bb + hh) ^ ((d >> 2) & 3))) = (u32x4){w[0], w[1], w[2], w[3]};
    }
    rec[REC_VS + 2 * d + bb] = (unsigned char)sb;
  }
}

// ---- RMSNorm (full width) + RoPE of q and k, written as the MXFP8 operands directly (the quantised self-attention's producer):
// what flexam_rmsnorm_rope followed by the Q / K half of flexam_attn_fp8_pack does, without the bf16 round trip -- the values are
// quantised from fp32 (so the bytes differ from the two-step path by bf16's rounding).  One 128-thread workgroup per (token, q | k);
// thread t holds channels 8 (t + 128 i) .. +7, i < 3: four consecutive lanes hold one 32-channel MX block.
struct RmsRopeMx {
  const bf16 *q, *k;
  int64_t ldq, ldk;
  const float *wq, *wk, *cs, *sn;
  unsigned char *q8, *qs, *kv8;
  int64_t tokens_per_batch, token_offset;
  int H, L, lq_pad, tiles;
  float eps;
  const float* k_shift;   // SHIFT instance only (flexam_rmsnorm_rope_mx_shift): fp32 [B][3072], subtracted from the rotated K in fp32.  That
                          // instance writes the K half alone; the Q half of a shifted call is a launch of the plain instance: the same bytes
};

template <bool SHIFT>
__global__ __launch_bounds__(128) void rmsnorm_rope_mx_kernel(RmsRopeMx a) {
  __shared__ float red[8];
  constexpr int VPT = 3, C = 24 * HD;                 // 3072 channels = 24 heads
  const int which = SHIFT ? 1 : blockIdx.y;           // 0: q, 1: k (the SHIFT instance is launched for k alone)
  const int64_t m = blockIdx.x;
  const bf16* xr = which == 0 ? a.q + m * a.ldq : a.k + m * a.ldk;
  const float* w = which == 0 ? a.wq : a.wk;
  bf16x8 v[VPT];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    v[i] = *(const bf16x8*)(xr + (threadIdx.x + i * 128) * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = bf2f(v[i][j]);
      ss += f * f;
    }
  }
  const float rn = __builtin_amdgcn_rsqf(block_sum<128>(ss, red) / (float)C + a.eps);
  const int b = (int)(m / a.tokens_per_batch), tl = (int)(m % a.tokens_per_batch);
  const int64_t tok = a.token_offset + tl;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int c = (threadIdx.x + i * 128) * 8, head = c >> 7, ch = c & 127;
    const f32x4 w0 = *(const f32x4*)(w + c), w1 = *(const f32x4*)(w + c + 4);
    float y[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      y[j] = bf2f(v[i][j]) * rn * w0[j];
      y[4 + j] = bf2f(v[i][4 + j]) * rn * w1[j];
    }
    const f32x4 co = *(const f32x4*)(a.cs + tok * 64 + (ch >> 1)), si = *(const f32x4*)(a.sn + tok * 64 + (ch >> 1));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float re = y[2 * j], im = y[2 * j + 1];
      y[2 * j] = re * co[j] - im * si[j];
      y[2 * j + 1] = re * si[j] + im * co[j];
    }
    if constexpr (SHIFT) {                              // smooth-K: behind the rotation, in front of the block amax
      const f32x4 s0 = *(const f32x4*)(a.k_shift + (int64_t)b * C + c), s1 = *(const f32x4*)(a.k_shift + (int64_t)b * C + c + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        y[j] -= s0[j];
        y[4 + j] -= s1[j];
      }
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(y[j]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));      // the 32-channel block = 4 consecutive lanes
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    float inv;
    const unsigned sb = mx_scale(amax, inv);
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0] * inv, y[1] * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2] * inv, y[3] * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4] * inv, y[5] * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6] * inv, y[7] * inv, hi, true);
    const int64_t bh = (int64_t)b * a.H + head;
    const int blk = ch >> 5;
    if (which == 0) {
      *(u32x2*)(a.q8 + (bh * a.lq_pad + tl) * 128 + ch) = (u32x2){(unsigned)lo, (unsigned)hi};
      if ((threadIdx.x & 3) == 0) a.qs[(bh * a.lq_pad + tl) * 4 + blk] = (unsigned char)sb;
    } else {
      const int tile = tl >> 6, row = tl & 63;
      unsigned char* rec = a.kv8 + (bh * a.tiles + tile) * REC_BYTES;
      *(u32x2*)(rec + row * 128 + 16 * ((ch >> 4) ^ ((row >> 1) & 7)) + (ch & 8)) = (u32x2){(unsigned)lo, (unsigned)hi};
      if ((threadIdx.x & 3) == 0) rec[REC_KS + 4 * row + blk] = (unsigned char)sb;
    }
  }
}

// ---- smooth-K (SageAttention's preprocessing of K): the mean over the tokens of K as the attention will see it, per (batch, channel).
// softmax(q.(k_j - c)) = softmax(q.k_j - q.c) = softmax(q.k_j) for ANY c, since q.c is one number per query row: subtracting the mean
// changes no output, only what e4m3 has to resolve -- a channel offset shared by all keys otherwise costs every score its relative error.
// NORM: k is the projection's output and RMSNorm over the full row + RoPE come first (flexam_rmsnorm_rope's arithmetic: the fused
// producer above never materialises that K); otherwise k is taken as given.
// Deterministic, whatever the device: no atomics, no CU count.  ONE wave per (part, batch) sums the rows of ceil(L / parts) consecutive
// tokens in token order in fp32 -- lane l holds channels 8 (l + 64 i) .. +7, i < VPT, so the sum of squares of a row is a wave
// reduction (no LDS, no barrier) -- into partial[b][part][:]; k_mean_finish_kernel adds the parts in index order and multiplies by 1 / L.
// The next token's row is loaded in front of the work on this one (past the end: the last row once more).
struct KMean {
  const bf16* k;
  int64_t ldk, token_offset;
  const float *wk, *cs, *sn;
  float *partial, *mean;
  int C, L, parts, tpp;      // tpp = ceil(L / parts) tokens per part
  float eps, inv_l;
};

template <int VPT, bool NORM>
__global__ __launch_bounds__(64) void k_mean_part_kernel(KMean a) {
  const int lane = threadIdx.x, part = blockIdx.x, b = blockIdx.y;
  const int nvec = a.C >> 3;
  const int t0 = min(part * a.tpp, a.L), t1 = min(t0 + a.tpp, a.L);
  const bf16* rows = a.k + (int64_t)b * a.L * a.ldk;
  float acc[VPT][8];
  float w[NORM ? VPT : 1][8];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    if constexpr (NORM) {
      const int vec = min(lane + 64 * i, nvec - 1);
      const f32x4 w0 = *(const f32x4*)(a.wk + vec * 8), w1 = *(const f32x4*)(a.wk + vec * 8 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[i][j] = w0[j];
        w[i][4 + j] = w1[j];
      }
    }
  }
  auto load_row = [&](int t, bf16x8 (&v)[VPT]) {
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int vec = lane + 64 * i;
      v[i] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
      if (vec < nvec) v[i] = *(const bf16x8*)(rows + (int64_t)t * a.ldk + vec * 8);
    }
  };
  bf16x8 cur[VPT], nxt[VPT];
  if (t0 < t1) load_row(t0, cur);
  for (int t = t0; t < t1; ++t) {
    load_row(min(t + 1, t1 - 1), nxt);
    if constexpr (NORM) {
      const int64_t tok = a.token_offset + t;
      const int pair0 = (lane * 8 & (HD - 1)) >> 1;     // 64 lanes x 8 channels = 4 heads: the same 4 pairs of a head for every i
      const f32x4 co = *(const f32x4*)(a.cs + tok * (HD / 2) + pair0), si = *(const f32x4*)(a.sn + tok * (HD / 2) + pair0);
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < VPT; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = bf2f(cur[i][j]);
          ss += f * f;
        }
      const float rn = __builtin_amdgcn_rsqf(wave_sum(ss) / (float)a.C + a.eps);
#pragma unroll
      for (int i = 0; i < VPT; ++i) {
        float y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = bf2f(cur[i][j]) * rn * w[i][j];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float re = y[2 * j], im = y[2 * j + 1];
          acc[i][2 * j] += re * co[j] - im * si[j];
          acc[i][2 * j + 1] += re * si[j] + im * co[j];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < VPT; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] += bf2f(cur[i][j]);
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) cur[i] = nxt[i];
  }
  float* dst = a.partial + ((int64_t)b * a.parts + part) * a.C;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int vec = lane + 64 * i;
    if (vec < nvec) {
      *(f32x4*)(dst + vec * 8) = (f32x4){acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
      *(f32x4*)(dst + vec * 8 + 4) = (f32x4){acc[i][4], acc[i][5], acc[i][6], acc[i][7]};
    }
  }
}

// thread = (batch, channel): the parts in index order (the loads do not depend on the sum: unrolled, they are all in flight together)
__global__ __launch_bounds__(256) void k_mean_finish_kernel(KMean a, int B) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * a.C) return;
  const int b = idx / a.C, c = idx - b * a.C;
  const float* src = a.partial + (int64_t)b * a.parts * a.C + c;
  float s = 0.f;
#pragma unroll 16
  for (int p = 0; p < a.parts; ++p) s += src[(int64_t)p * a.C];
  a.mean[idx] = s * a.inv_l;
}
