// flexam_amd/csrc/attn.hip -- flash attention forward, head_dim 128, bf16 in/out, fp32 softmax
// and accumulation; non-causal with a key-length bound.  Used for the DiT's full 3-D
// spatiotemporal self-attention (Lq = Lk = 11648 at 97x512x896) and the text cross-attention
// (Lk = 512).  Replaces flash_attn / sageattn / SDPA behind attention():
// FlexAM/models/attention_utils.py:43-233, called from wan_transformer3d_FlexAM.py:251-256,367.
//
// Structure (cdna_hip_programming.md, "Fused attention prefill"; everything derived from the
// MFMA lane maps in section 3 of that guide):
//  * one workgroup = 8 waves = 256 query rows of one (batch, head); each wave owns 32 rows and
//    keeps its Q fragment (32 VGPRs) and the O^T accumulator (64 VGPRs) in registers;
//  * K/V tiles of 64 keys go global -> LDS by LDS-DMA into two 4-slot rings (details at the kernel); the LDS
//    image is the dual-use XOR-swizzled image "(b)" of the guide: the K tile is read row-wise with
//    ds_read_b128, the V tile column-wise with ds_read_b64_tr_b16, both conflict-free (tools/lds_sim.py);
//  * QK^T is computed swapped, S^T = K.Q^T (v_mfma_f32_32x32x16_bf16, K fragment in the A slot)
//    so a lane holds 32 scores of ONE query row: the row max / sum are in-register plus one
//    v_permlane32_swap, and the bf16-packed P registers are directly the B operand of
//    O^T += V^T.P^T (accumulator-as-operand with the permuted-k order of the guide);
//  * softmax scale and log2(e) are folded into one FMA in front of v_exp_f32, or (PRE) into q by its producer.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "flexam_hip.h"

namespace {

constexpr int QBLK = 256;     // query rows per workgroup
constexpr int KVBLK = 64;     // keys per tile
constexpr int HD = 128;       // head dim (fixed)
constexpr int KV_TILE_BYTES = KVBLK * HD * 2;   // 16 KiB

struct AttnParams {
  const bf16* q;
  const bf16* k;
  const bf16* v;
  bf16* o;
  int64_t q_bs, q_rs;   // batch stride, row stride (elements); head h at column h*128
  int64_t k_bs, k_rs;
  int64_t v_bs, v_rs;
  int64_t o_bs, o_rs;
  int B, H, Lq, Lk;
  float scale_log2e;    // softmax_scale * log2(e)
  int prescaled;        // q already carries that factor (see flexam_hip.h): the kernel instance with PRE = true runs
  int q_blocks;
  // split-KV (kv_splits > 1): workgroup (q block, head, split) covers key tiles [split*tiles_per_split, ..) and writes its
  // un-normalised O (fp32) and (running max, row sum) to the workspace; attn_merge_kernel combines the splits
  int kv_splits, tiles_per_split;
  int unit0, n_units;   // this launch covers work units (q block, head, batch) unit0 .. unit0 + n_units - 1
  // whole_units > 0: ONE launch for a split-KV call.  Units 0 .. whole_units - 1 (= unit0) run all keys in one workgroup each and
  // write O; the n_units units behind them run as kv_splits workgroups each and write partials.  Every XCD gets an eighth of both
  // kinds, its whole units first: the short workgroups start as the CUs of that XCD finish their last whole unit, without a launch
  // boundary (and its drain) in between.
  int whole_units;
  float* ws_o;          // [slots][n_units][256 rows][128]
  float* ws_ml;         // [slots][n_units][256 rows][2]
  // partial: write un-normalised O and (reference, row sum) to workspace slot slot0 + split even with one key range (the keys of
  // this call are only PART of the softmax: local-chunk-first attention under a sequence-parallel K|V all-gather);
  // n_slots: slots the merge kernel adds up
  // (the attn_window_at_kernel instances, whole units that no merge follows, read n_slots as win_q0: the global token of the call's row 0
  //  (flexam_attn_fwd_window_at).  The struct, and with it the kernarg loads of every other instance, stay as they are)
  int partial, slot0;
  union { int n_slots; int win_q0; };
  float last_key_bias;  // added to the score of key Lk - 1 in exp2 units (log2 of its multiplicity), 0 = none: see flexam_attn_fwd_lastkey
  // MXFP8 operands (attn_fp8.inc; q8 != nullptr selects that kernel): written by flexam_attn_fp8_pack
  const unsigned char* q8;   // [B][H][lq_pad][128] e4m3
  // (attn_window_frames_kernel, which has no MXFP8 operands, reads the low word of this pointer as win_frame = T > 0
  //  (flexam_attn_fwd_window_frames): win_left / win_right count frames of T tokens from token 0, see below.  attn_window_kernel, whose
  //  window counts tokens, does not read it: attn_run leaves it 0 there, the null qs)
  union { const unsigned* qs; int win_frame; };        // [B][H][lq_pad] four E8M0 bytes per row
  // kv8: [B][H][ceil(Lk / 64)] records of REC_BYTES -- or, in chunks of kv8_chunk_tiles key tiles, [chunk][B][H][kv8_chunk_tiles]
  // (attn_window_halo_kernel, which has no MXFP8 operands, reads the low word of this pointer as win_key_gap: the key tiles its compact
  //  k / v leave out between the sink tiles and the window tiles (flexam_attn_fwd_window_halo).  No other instance reads the word so)
  union { const unsigned char* kv8; int win_key_gap; };
  // (attn_window_kernel reads this word as its sink, the way it reads the two chunk words below as its window: the first win_sink keys
  //  are visible to EVERY row, whatever win_right says -- the model is not causal.  Row i sees key j iff j < win_sink or j is in its window)
  union { int lq_pad; int win_sink; };
  // key tile g lives in chunk g / kv8_chunk_tiles (flexam_attn_fwd_fp8_chunked: the rank-major result of a sequence-parallel all-gather of
  // every rank's records; one chunk = all tiles for the plain call); kv8_chunk_magic = ceil(2^32 / kv8_chunk_tiles) turns the division
  // into one s_mul_hi_u32 (exact for g, tiles < 2^16)
  // (attn_window_kernel, which has no MXFP8 operands, reads the two words as its window: the struct, and with it the kernarg loads of
  //  every other instance, stay as they are.)  Sliding window, Lq == Lk: row i sees key j iff (win_left < 0 or j >= i - win_left) and
  //  (win_right < 0 or j <= i + win_right); with win_frame = T > 0 the same two words count frames: j / T >= i / T - win_left and
  //  j / T <= i / T + win_right, i.e. row i sees the keys [(i / T - win_left) T, (i / T + win_right + 1) T - 1] -- whole frames
  union { int kv8_chunk_tiles; int win_left; };
  union { unsigned kv8_chunk_magic; int win_right; };
  // smooth-V (flexam_attn_fwd_fp8_oshift): fp32 [B][H * 128] added to O / l in fp32 in front of the one rounding to bf16, by the OSHIFT
  // instances of the two final writers (store_output, attn_merge_kernel); nullptr = none.  Partials never carry it: their weights sum to 1
  const float* o_shift;
};

// byte offset of 16-byte chunk `ch` (0..15) of key row `row` in a [64][128] bf16 tile, image (b)
__device__ __forceinline__ int kv_off(int row, int ch) {
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// Exchange between lane l and lane l^32 (the two halves of a query row).  Inline asm on purpose:
// hipcc (ROCm 7.2) folds __builtin_amdgcn_permlane32_swap(x, x) as if both results were equal
// (observed: v_add v1, v1, v1), which silently drops the other half's value.  The s_nop covers the
// VALU-write -> v_permlane read hazard (2 wait states) inside the asm string.
__device__ __forceinline__ void half_swap(float& a, float& b) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void half_swap_u32(unsigned& a, unsigned& b) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
// 16-byte-per-lane LDS-DMA issued from inline asm: hipcc then does not know an LDS write is in flight and does
// not put s_waitcnt vmcnt(0) in front of every ds_read_b64_tr_b16 intrinsic (it does for the builtin form,
// which would drain the DMA in the middle of a tile).  Completion is tracked by hand: vmcnt(0) + s_barrier
// at the top of each 64-key tile.  M0 (LDS base of the DMA) is saved / restored inside the statement.
__device__ __forceinline__ void lds_dma16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}

// max of MFMA outputs as single instructions: fmaxf() makes hipcc put a canonicalising v_max_f32 x, x in front of every operand it
// cannot prove quiet (each MFMA result), 4-5 extra vector instructions per half tile in a loop that is bound by vector issue
__device__ __forceinline__ float vmax3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// max of 8 values in ONE statement: between separate asm statements that feed each other hipcc pads an s_nop per dependency
__device__ __forceinline__ float vmax8(float a, float b, float c, float d, float e, float f, float g, float h) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3\n\tv_max3_f32 %0, %0, %4, %5\n\tv_max3_f32 %0, %0, %6, %7\n\tv_max_f32 %0, %0, %8"
      : "=&v"(r)
      : "v"(a), "v"(b), "v"(c), "v"(d), "v"(e), "v"(f), "v"(g), "v"(h));
  return r;
}
// max(a, b) combined across the two lanes (l, l ^ 32) that hold one query row, one statement (wait states inside)
__device__ __forceinline__ float pair_max2(float a, float b) {
  float r, t;
  asm("v_max_f32 %0, %2, %3\n\tv_mov_b32 %1, %0\n\ts_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 0\n\tv_max_f32 %0, %0, %1"
      : "=&v"(r), "=&v"(t)
      : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float vmax(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// scalar-base form of the same DMA: uniform 64-bit base in SGPRs + one loop-invariant 32-bit per-lane offset, so a full tile's four
// pieces cost no vector address arithmetic; M0 is written and not restored (nothing else in this kernel reads it: LDS instructions
// on gfx9+ do not)
__device__ __forceinline__ void lds_dma16_sbase(const char* sbase, unsigned voff, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

__device__ __forceinline__ float pair_max(float x) {
  float a = x, b = x;
  half_swap(a, b);
  return vmax(a, b);
}
__device__ __forceinline__ float pair_sum(float x) {
  float a = x, b = x;
  half_swap(a, b);
  return a + b;
}

// ------------------------------------------------------------------------------------------------
// Structure: 8 waves x 32 query rows = 256 rows per workgroup, two waves per SIMD.
//  * K/V tiles of 64 keys go HBM/L2 -> LDS by LDS-DMA (global_load_lds, 16 B/lane, swizzle applied to
//    the source address) into a ring of 4 slots: no staging registers, no ds_write; ONE s_barrier per
//    64 keys, and the DMA of tile t+2 is in flight for two tiles before the vmcnt(0) that precedes it;
//  * the softmax pipeline runs on 32-key HALF tiles g.  Step g issues on the matrix pipe
//        S(g+1) = K(g+1).Q^T          8 MFMA   (scores of the next half; S double-buffered: 32 VGPRs)
//        O^T   += V(g-1)^T.P(g-1)^T   8 MFMA   (PV of the previous half; P kept packed in 8 VGPRs)
//    in the same basic blocks as the VALU work of half g (row max, exp2, row sum, bf16 pack), so the
//    wave overlaps its own MFMAs with its own softmax, and its SIMD partner fills the remaining gaps;
//  * deferred rescale: the running max is raised (O, l and the pending P rescaled) only when a row max
//    grew by more than 2^THR; P <= 2^THR is harmless in bf16 / fp32 floating point.
// (A 4-wave x 64-row variant -- each K/V fragment feeding two MFMAs -- was tried in r1: hipcc cannot keep
//  Q in the accumulator file and spills 150+ VGPRs; see DESIGN.md.)
// ------------------------------------------------------------------------------------------------
constexpr int NT = 512;
constexpr int NSLOT = 4;
constexpr int V_RING = NSLOT * KV_TILE_BYTES;   // LDS: [4 K slots][4 V slots]
template <int V>
using IC = std::integral_constant<int, V>;
// Deferred-rescale threshold in exp2 units.  A trade, measured in r6 (profiles/r6zb_*): every deferral leaves the row's dominant key at a
// P that is not exactly 1, i.e. with a bf16 rounding error the exact-maximum form does not have -- attention error against fp64 on
// peaked rows (logit std 6, L = 11648) 1.51e-3 rms at 2^0, 1.77e-3 at 2^8, 2.10e-3 at 2^24 -- while the rescale branch costs
// +1.2 % of a denoise step at 2^4 and -0.5 / -0.9 / -1.3 ... -2.1 % at 2^12 / 2^16 / 2^24 on such rows (nothing on N(0, 1) logits).
// 8 stays: parity before speed.
constexpr float RESCALE_THR_LOG2 = 8.0f;

// workgroups bid = 8 * local + xcd go to XCD `xcd` in the order of `local`: an XCD walks a contiguous eighth of the work list
__device__ __forceinline__ int eighth(int n, int xcd, int local) {      // index into a list of n items, -1 past this XCD's share
  const int q = n >> 3, rr = n & 7;
  if (local >= q + (xcd < rr ? 1 : 0)) return -1;
  return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + local;
}
// The work unit of this workgroup (not SHORT: a walk of its own): a whole unit -- all keys, writes O -- or key range `split` of unit `ul` of the
// launch's split part.  The caller presets split = 0, tps = p.tiles_per_split and partial = p.partial; false = this workgroup has no work.
__device__ __forceinline__ bool unit_of_workgroup(const AttnParams& p, int& split, int& ul, int& unit, int& tps, int& partial) {
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  const int wmax = (p.whole_units + 7) >> 3;
  if (local < wmax) {                              // (whole_units = 0: wmax = 0)
    unit = eighth(p.whole_units, xcd, local);
    if (unit < 0) return false;
    ul = unit;
    tps = (p.Lk + KVBLK - 1) / KVBLK;
    partial = 0;
  } else {
    // consecutive workgroups: the units of one split, i.e. q blocks of one head first -> same K/V range in L2
    const int j = eighth(p.n_units * p.kv_splits, xcd, local - wmax);
    if (j < 0) return false;
    split = j / p.n_units;
    ul = j - split * p.n_units;                    // unit index inside the launch's split (or only) part
    unit = p.unit0 + ul;
  }
  return true;
}
// ---- epilogue of both kernels: O[q][32dt + 8i + 4h + (0..3)] = o_acc[dt][4i + (0..3)] / l, lane (r, h) of `wave` holding row qi.  Partial result
// of one key range: un-normalised O (SCALE: times osc) and (reference, row sum) to the workspace; attn_merge_kernel finishes the softmax.
template <bool SCALE>
__device__ __forceinline__ void store_partial(const AttnParams& p, const f32x16 (&o_acc)[4], float osc, float ref, float l_tot, int split,
                                              int ul, int wave, int r, int h, int qi) {
  if (qi >= p.Lq) return;
  const int64_t row = ((int64_t)(p.slot0 + split) * p.n_units + ul) * QBLK + wave * 32 + r;
  float* orow = p.ws_o + row * HD;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) ov[e] = SCALE ? o_acc[dt][4 * i + e] * osc : o_acc[dt][4 * i + e];
      *(f32x4*)(orow + 32 * dt + 8 * i + 4 * h) = ov;
    }
  if (h == 0) *(f32x2*)(p.ws_ml + row * 2) = (f32x2){ref, l_tot};
}
// A lane holds 4 of the 8 columns of each 8-column group of its row, its partner (lane ^ 32) the other 4.  One half exchange
// per dword between the groups of a pair (lower lanes give their part of the odd group, upper lanes their part of the even
// one) leaves 16 contiguous bytes in every lane: 8 stores of 16 B instead of 16 of 8 B (the tail is store-issue bound).
// OSHIFT: p.o_shift[b][head * 128 + column] is added to O / l in fp32, loaded here (behind the key loop) in the accumulator's column order.
// EMPTY (the attn8_window_at instances with OSHIFT): inv_l = 0 marks a row that saw no key, which is written as zeros, not as the shift.
template <bool OSHIFT = false, bool EMPTY = false>
__device__ __forceinline__ void store_output(const AttnParams& p, const f32x16 (&o_acc)[4], float inv_l, int b, int head, int qi, int h) {
  bf16* orow = p.o + (int64_t)b * p.o_bs + (int64_t)min(qi, p.Lq - 1) * p.o_rs + head * HD + 8 * h;
  const float* srow = OSHIFT ? p.o_shift + ((int64_t)b * p.H + head) * HD + 4 * h : nullptr;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
      bf16x4 even, odd;
      f32x4 se = {0.f, 0.f, 0.f, 0.f}, so = {0.f, 0.f, 0.f, 0.f};
      if constexpr (OSHIFT) {
        se = *(const f32x4*)(srow + 32 * dt + 8 * i);
        so = *(const f32x4*)(srow + 32 * dt + 8 * i + 8);
        if constexpr (EMPTY) if (inv_l == 0.f) { se = (f32x4){0.f, 0.f, 0.f, 0.f}; so = se; }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        even[e] = f2bf(OSHIFT ? o_acc[dt][4 * i + e] * inv_l + se[e] : o_acc[dt][4 * i + e] * inv_l);
        odd[e] = f2bf(OSHIFT ? o_acc[dt][4 * i + 4 + e] * inv_l + so[e] : o_acc[dt][4 * i + 4 + e] * inv_l);
      }
      const u32x2 ev = __builtin_bit_cast(u32x2, even), od = __builtin_bit_cast(u32x2, odd);
      unsigned a0 = ev[0], a1 = ev[1], c0 = od[0], c1 = od[1];
      half_swap_u32(a0, c0);
      half_swap_u32(a1, c1);
      if (qi < p.Lq) *(u32x4*)(orow + 32 * dt + 8 * i) = (u32x4){a0, a1, c0, c1};
    }
}

// KIND: 0 = self-attention, 1 = short-context (text) attention: distinct profiler symbols.
// PRE: q was multiplied by softmax_scale * log2(e) by its producer, BEFORE its one rounding to bf16 (in the DiT: folded into the
// RMSNorm weight of q).  The scores then leave the MFMA chain in exp2 units, and with the row reference of the online softmax as
// the chain's initial accumulator p = exp2(S') needs no FMA per score (16 of ~85 vector operations per 16 MFMAs).
// FULL (Lk >= 64, no weighted key; the DiT's self-attention): the common path of a half-tile step is ONE basic block apart from the
// rescale branch -- across block boundaries hipcc sinks MFMAs to the block of their first use, which serialises the pipeline
// (-0.9 % of a denoise step, profiles/r4ab_*).  To that end: the last tile of a key range that is not a multiple of 64 is the window
// [Lk - 64, Lk) instead of [64 (T - 1), 64 T) -- every tile is a whole in-bounds 64-row LDS-DMA with the same per-lane offsets, and
// its keys that the tile before already held are masked instead of keys past the end; the mask exists only in the 1-4 tail tiles
// of a work unit (branch-free there), the main loop has none; LDS-DMA past the end re-reads the last tile into a free slot; the
// barrier of tile 0 is kept.
// SHORT (at most 4 key tiles, i.e. the text cross-attention): one persistent workgroup per CU walks a contiguous range of work units
// (q blocks of one (batch, head), then of the next); the K/V tiles of a head stay in the ring while its q blocks last -- one LDS-DMA
// prologue and barrier per head change instead of per q block, none inside (the tiles are read-only), so the waves run through
// their rows of the blocks on their own.
// WIN (attn_window_kernel; the general form, whole units, Lq == Lk): flash-attn's sliding window.  A work unit walks the key tiles
// [first, last] that hold a key one of its 256 rows sees (hip.attn_window_tiles states the same rule) instead of all of them.  Tiles in
// which every row sees every key (`interior`) run the general step as it is; in the others -- the ragged last tile among them -- the
// one uniform branch the general step has in front of part A applies mask_half and the window mask, a per-lane range compare like
// mask_shift (a lane holds 32 scores of ONE row).  Rows of a wave may see no key at all in the first tiles of the unit (the unit's range
// is the union over its rows): a row's reference stays unset until its first finite score, and the rescale factors are guarded against
// inf - inf.  Units of a window without a left bound grow with the q block: the q blocks of a head are walked backwards, longest first.
// Sink (win_sink > 0, flexam_attn_fwd_window_sink): the first win_sink keys are visible to every row whatever the window says, the right
// side included -- the model is not causal.  The unit then walks the sink tiles and the window tiles (see global_tile below); a tile wholly
// below the sink is interior, the tile that holds key win_sink - 1 takes the per-lane mask `key < win_sink or in the window`.  Behind the
// sink tiles a row HAS started, and the first window tiles of the unit may again hold no key it sees: such a half tile is all -inf for the
// row, its maximum moves neither reference (PRE: delta = max(-inf, 0) = 0, alpha = 1; else m_new = m_run, alpha = exp2(0)) and its
// exp2(-inf) terms add exactly 0 -- the same guards, no new case.
// FRAMES (attn_window_frames_kernel; win_frame = T > 0, flexam_attn_fwd_window_frames): the window counts frames of T tokens from token 0 and row i sees the frames
// i / T - win_left .. i / T + win_right whole.  A row's keys are still ONE range [lo(i), hi(i)] and both ends are non-decreasing in i, which
// is all the walk, the interior test and the per-lane mask rest on: only the derivation of the bounds differs (one division by T per unit
// for the scalar bounds, one per row for the lane's), at kernel entry; the tile loop is the token window's.  Where T is a multiple of 64
// every frame boundary is a tile boundary: all window tiles are interior and the per-lane mask runs for the sink's edge and the ragged
// last tile only.
// (The one-block step of FULL for runs of interior tiles, next to the general step for the edges, was built and not kept: two step
//  bodies in one loop cost hipcc 70 (scale in kernel) to 330 (PRE) spilled VGPRs, and a loop for each does not fit the instruction cache.)
// AT (attn_window_at_kernel; flexam_attn_fwd_window_at, FRAMES with a token window as frames of one token): row i of the call is the global
// token win_q0 + i, its bounds are those of that token, and Lq and Lk are two lengths: a rank's chunk of queries against the gathered
// keys, pad rows (global tokens from Lk on) included.  The bounds stay non-decreasing in the row, so the walk, the interior test and the
// per-lane mask are the ones above on global rows.  New: a unit whose rows see no key at all (pad rows, no sink) walks no tile -- it
// reads no key and writes zeros --, and a row that sees no key in a unit that walks some ends with l = 0 and its reference never set
// (the guards above keep its O at 0): it is written as zeros, not as 0 * inf.
// HALO (attn_window_halo_kernel; flexam_attn_fwd_window_halo, on top of AT): k and v are a compact buffer that holds the sink tiles and, behind
// them, the key tiles from global tile s_n + win_key_gap on.  Every mask and bound stays in global indices; only the address of global
// tile tg moves: buffer tile tg below s_n, tg - win_key_gap from there on (the entry point has checked every unit's tiles against it).
template <int KIND, bool PRE, bool FULL, bool SHORT, bool WIN, bool FRAMES = false, bool AT = false, bool HALO = false>
__device__ __forceinline__ void attn_fwd_body(const AttnParams p) {      // (p by value, as attn8_fwd_body takes it and for its reason)
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [4 K tiles][4 V tiles], each a ring
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  // (Wave priorities: at equal priority the older half of the workgroup (waves 0-3) wins every arbitration against its SIMD partners,
  //  runs ahead and waits ~800 cycles per tile at the barrier; a static priority for waves 4-7 mirrors that, and every scheme that
  //  balances the halves -- priority in one part of the step only, turns by step or by tile -- is slower: while the leader waits its
  //  partner has the SIMD to itself.  profiles/r4u_attn_wave_priority_modes_and_barrier_wait.txt)

  int split = 0, ul, unit, tps = p.tiles_per_split, partial = p.partial;
  int unit_end;                              // SHORT: this workgroup walks units [unit, unit_end)
  if constexpr (SHORT) {
    const int64_t all = (int64_t)p.B * p.H * p.q_blocks;
    ul = unit = (int)(all * blockIdx.x / gridDim.x);
    unit_end = (int)(all * (blockIdx.x + 1) / gridDim.x);
    if (unit >= unit_end) return;
  } else if (!unit_of_workgroup(p, split, ul, unit, tps, partial)) {
    return;
  }
  if constexpr (!SHORT) unit_end = unit + 1;
  // (batch, head) of the unit being worked on: set at the top of every unit of the walk below
  int head = 0, b = 0, bh_loaded = -1;
  const bf16* qbase = nullptr;
  const char *kbase = nullptr, *vbase = nullptr;

  // ---- LDS read offsets (dual-use swizzled image, see kv_off)
  int koff[8];
  {
    const int sw = ((r & 3) << 2) | ((r >> 2) & 3);
#pragma unroll
    for (int ds = 0; ds < 8; ++ds) koff[ds] = 256 * r + 16 * ((2 * ds + h) ^ sw);
  }
  int voff[2][4];
  {
    const int g = lane >> 4, i = lane & 15, q_ = i >> 2, p_ = i & 3;
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        voff[half][dt] = kv_off(8 * half + 4 * h + q_, 4 * dt + 2 * (g & 1) + (p_ >> 1)) + 8 * (p_ & 1);
  }

  // ---- LDS-DMA staging: piece id = tid + 512*i (i < 2) lands at LDS byte id*16 of the tile, i.e. row id/16,
  //      slot id%16; it must carry chunk (slot ^ swizzle(row)) of that key row
  const int tiles_all = (p.Lk + KVBLK - 1) / KVBLK;
  // WIN: the unit's w_n key tiles and, of them, the window's interior tiles [ti_lo, ti_hi] (local indices) every row sees whole.
  // With a sink (the first win_sink keys, visible to every row) the walk is the union of the sink tiles [0, s_n) and the window tiles: ONE
  // run when they touch or overlap, else two runs with `gap` tiles between them that no row sees.  Tiles stay indexed locally (loop, ring,
  // 4-unroll); the global tile of local tile t is t below s_n and t + gap from there on (hip.attn_window_sink_tiles states the same rule).
  // Without a sink s_n = 0 and gap is the window's first tile.  s_full: the tiles wholly below win_sink, interior for every row.
  int w_n = 0, ti_lo = 0, ti_hi = 0, s_n = 0, s_full = 0, gap = 0;
  if constexpr (WIN) {
    int qb = unit % p.q_blocks;
    if (p.win_left < 0) qb = p.q_blocks - 1 - qb;
    const int g0 = AT ? p.win_q0 : 0;                             // (AT: rows as global tokens)
    const int qa = g0 + qb * QBLK, qz = g0 + min(qb * QBLK + QBLK, p.Lq) - 1;      // first and last row of the unit
    // the key ranges [lo, hi] of the first (_a) and the last (_z) row before clipping (an unbounded side's are not used): in tokens, or
    // FRAMES in whole frames of win_frame = T tokens counted from token 0 (fa, fz: the two rows' frames).  Non-decreasing in the row
    // either way
    int fa = 0, fz = 0;
    if constexpr (FRAMES) { fa = (int)((unsigned)qa / (unsigned)p.win_frame); fz = (int)((unsigned)qz / (unsigned)p.win_frame); }
    const int lo_a = FRAMES ? (fa - p.win_left) * p.win_frame : qa - p.win_left;
    const int hi_z = FRAMES ? (fz + p.win_right + 1) * p.win_frame - 1 : qz + p.win_right;
    const int k_first = p.win_left < 0 ? 0 : max(0, lo_a);
    const int k_last = p.win_right < 0 ? p.Lk - 1 : min(p.Lk - 1, hi_z);
    s_n = (min(p.win_sink, p.Lk) + KVBLK - 1) / KVBLK;
    s_full = p.win_sink / KVBLK;
    gap = max(0, k_first / KVBLK - s_n);
    w_n = max(k_last / KVBLK, s_n - 1) + 1 - gap;
    // AT: the window of every row of the unit may lie behind the last key (pad rows): the sink tiles alone, or no tile at all.  (The
    // interior test below is empty by itself then: lo_z lies behind every whole tile)
    if constexpr (AT) if (k_first > k_last) { gap = 0; w_n = s_n; }
    const int lo_z = FRAMES ? (fz - p.win_left) * p.win_frame : qz - p.win_left;
    ti_lo = p.win_left < 0 ? 0 : (max(0, lo_z) + KVBLK - 1) / KVBLK;      // its first key is the last row's first or later
    const int hi_a = FRAMES ? (fa + p.win_right + 1) * p.win_frame - 1 : qa + p.win_right;
    const int top_key = hi_a - (KVBLK - 1);                               // its last key is the first row's last or sooner
    ti_hi = min(p.win_right < 0 ? tiles_all : top_key >= 0 ? top_key / KVBLK : -1, p.Lk / KVBLK - 1);      // (whole tiles only)
    // as local indices, for the test in front of part A: the window's interior tiles lie at or behind its first tile, so behind the gap
    ti_lo -= gap;
    ti_hi -= gap;
  }
  const int t0 = WIN ? 0 : split * tps;                            // first key tile of this split (0 without split-KV)
  const int ntiles = WIN ? w_n : min(tps, tiles_all - t0);       // tiles are indexed locally below; global_tile(t) is the global tile
  auto global_tile = [&](int t) { return WIN ? (t < s_n ? t : t + gap) : t0 + t; };      // (WIN: one wave-uniform select)
  const unsigned k_step = (unsigned)(KVBLK * p.k_rs * 2), v_step = (unsigned)(KVBLK * p.v_rs * 2);
  unsigned k_go[2], v_go[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (tid + NT * i) >> 4;
    const int ch = (tid & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3));
    k_go[i] = (unsigned)(row * p.k_rs * 2 + ch * 16);
    v_go[i] = (unsigned)(row * p.v_rs * 2 + ch * 16);
  }
  const unsigned lds0 = (unsigned)(size_t)LDS_PTR(smem);
  auto issue_tile = [&](int t, int parts = 3, int tslot = -1) {      // parts: 1 = K, 2 = V; tslot: ring position (default t)
    const unsigned slot = lds0 + (unsigned)(((tslot < 0 ? t : tslot) & (NSLOT - 1)) * KV_TILE_BYTES + wave * 1024);   // wave-uniform; K ring, V ring = + V_RING
    const int tg = global_tile(t);
    const int skipped = HALO && tg >= s_n ? p.win_key_gap * KVBLK : 0;      // (HALO: key rows the buffer leaves out in front of this tile)
    if (FULL || (tg + 1) * KVBLK <= p.Lk) {
      // FULL: the last tile is the window [Lk - 64, Lk) (scalar select, no branch)
      const unsigned row0 = FULL && tg == tiles_all - 1 ? (unsigned)(p.Lk - KVBLK) : (unsigned)tg * KVBLK - (unsigned)skipped;
      const char* kt = kbase + (size_t)(row0 * (unsigned)(p.k_rs * 2));     // wave-uniform tile bases
      const char* vt = vbase + (size_t)(row0 * (unsigned)(p.v_rs * 2));
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (parts & 1) lds_dma16_sbase(kt, k_go[i], slot + i * 8192);
        if (parts & 2) lds_dma16_sbase(vt, v_go[i], slot + V_RING + i * 8192);
      }
    } else {                                 // last, partial tile: rows past Lk re-read the last key (masked later)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = (tid + NT * i) >> 4;
        const int col = ((tid & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3))) * 16;
        const int key = min(tg * KVBLK + row, p.Lk - 1) - skipped;
        if (parts & 1) lds_dma16(kbase + ((int64_t)key * p.k_rs * 2 + col), slot + i * 8192);
        if (parts & 2) lds_dma16(vbase + ((int64_t)key * p.v_rs * 2 + col), slot + V_RING + i * 8192);
      }
    }
  };
  // Half tile g lives in ring slot (g>>1)&3; the K slots fill the first 64 KiB of LDS and the V slots the second, so ONE set of
  // per-lane fragment addresses per ring reaches all four slots through the 16-bit ds_read immediate (slot, half and 16-key step
  // are compile-time constants once the tile loop is unrolled by 4).
  const char* kaddr[8];
  const char* vaddr[2][4];
#pragma unroll
  for (int ds = 0; ds < 8; ++ds) kaddr[ds] = smem + koff[ds];
#pragma unroll
  for (int half = 0; half < 2; ++half)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vaddr[half][dt] = smem + V_RING + voff[half][dt];
  // ---- the work units of this workgroup (one, unless SHORT)
  for (int u = unit; u < unit_end; ++u) {
  const int qbu = u % p.q_blocks, bh = u / p.q_blocks;
  const int qbi = WIN && p.win_left < 0 ? p.q_blocks - 1 - qbu : qbu;      // (WIN without a left bound: longest units first)
  head = bh % p.H; b = bh / p.H;
  qbase = p.q + (int64_t)b * p.q_bs + head * HD;
  kbase = (const char*)(p.k + (int64_t)b * p.k_bs + head * HD);
  vbase = (const char*)(p.v + (int64_t)b * p.v_bs + head * HD);
  // ---- Q fragment (B operand of S^T = K.Q^T): lane (r, h) holds Q[q0 + r][16*ds + 8h .. +7]
  const int q0 = qbi * QBLK + wave * 32;
  const int qrow = min(q0 + r, p.Lq - 1);
  if constexpr (AT) {
    if (ntiles == 0) {                       // no row of the unit sees a key: zeros, and no key tile read (uniform over the workgroup)
      f32x16 z[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) z[dt][e] = 0.f;
      store_output(p, z, 0.f, b, head, q0 + r, h);
      return;
    }
  }
  bf16x8 qf[8];
#pragma unroll
  for (int ds = 0; ds < 8; ++ds) qf[ds] = *(const bf16x8*)(qbase + (int64_t)qrow * p.q_rs + ds * 16 + h * 8);

  // PRE: row reference of the online softmax in exp2 units (a lane holds 32 scores of ONE query row, so it is one value per lane,
  // kept 16 times as the C operand that starts every S^T chain).  It is NOT the running maximum: it is only raised when a score
  // exceeds it by more than 2^THR (deferred rescale).
  f32x16 negref;
#pragma unroll
  for (int e = 0; e < 16; ++e) negref[e] = 0.f;
  float ref = 0.f;
  // ds0 == 0 starts a new accumulation: from a literal-zero C operand (no register zeroing), or from -ref (PRE)
  // `ghalf` (half-tile index modulo 8) must be a compile-time constant at every call site
  // K fragments ds0 .. ds0+3 of half `ghalf` (a compile-time constant at every call site) -> registers
  auto qk_read = [&](auto ghalf_c, auto ds0_c, bf16x8 (&kf)[4]) {
    constexpr int ghalf = decltype(ghalf_c)::value, ds0 = decltype(ds0_c)::value;
    constexpr int slot = (ghalf >> 1) & (NSLOT - 1);
    constexpr int imm = slot * KV_TILE_BYTES + (ghalf & 1) * 8192;
#pragma unroll
    for (int i = 0; i < 4; ++i) kf[i] = *(const bf16x8*)(kaddr[ds0 + i] + imm);
  };
  // ... and their 4 MFMAs of the S^T chain
  auto qk_mma = [&](auto ds0_c, const bf16x8 (&kf)[4], f32x16& sacc) {
    constexpr int ds0 = decltype(ds0_c)::value;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ds = ds0 + i;
      if (ds == 0) {
        const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if constexpr (PRE) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[i], qf[ds], negref, 0, 0, 0);   // S' = s - ref
        else sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[i], qf[ds], zero, 0, 0, 0);
      } else {
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[i], qf[ds], sacc, 0, 0, 0);
      }
    }
  };
  auto qk_part = [&](auto ghalf_c, auto ds0_c, f32x16& sacc) {      // fragments first, then the MFMAs
    bf16x8 kf[4];
    qk_read(ghalf_c, ds0_c, kf);
    qk_mma(ds0_c, kf, sacc);
  };
  bf16x8 kf_pre[4];      // the first four K fragments of the NEXT half tile, read one step ahead (block A starts on the matrix pipe)
  // weight of the LAST key as a score bias (multiplicity N of a key = + log2 N on its score): raw-score units in the non-PRE form
  const float last_bias = PRE ? p.last_key_bias : p.last_key_bias / p.scale_log2e;
  // FULL: keys of the shifted last tile that the tile before it already held -> -inf.  Branch-free; called in the tail tiles only.
  const int last_shift = tiles_all * KVBLK - p.Lk;      // 0..63: first valid in-tile position of the global last tile
  auto mask_shift = [&](int g, f32x16& sacc) {
    const int lim = (t0 + (g >> 1) == tiles_all - 1 ? last_shift : 0) - 32 * (g & 1) - 4 * h;      // element e is valid iff (e & 3) + 8 (e >> 2) >= lim
#pragma unroll
    for (int e = 0; e < 16; ++e) sacc[e] = (e & 3) + 8 * (e >> 2) >= lim ? sacc[e] : -INFINITY;
  };
  auto mask_half = [&](int g, f32x16& sacc) {      // g: local half index; keys are global
    if constexpr (FULL) return;
    const int gg = WIN ? 2 * global_tile(g >> 1) + (g & 1) : 2 * t0 + g;
    // past the end of the keys, or of this split's range -- or the half tile that holds a weighted last key
    if ((gg + 1) * 32 > p.Lk || g >= 2 * ntiles || (p.last_key_bias != 0.f && (gg + 1) * 32 == p.Lk)) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = gg * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (key >= p.Lk || g >= 2 * ntiles) sacc[e] = -INFINITY;
        else if (key == p.Lk - 1) sacc[e] += last_bias;
      }
    }
  };
  // WIN: keys outside the window of this lane's row -> -inf.  Element e is key 32 gg + 4 h + (e & 3) + 8 (e >> 2) of global half gg: seen iff
  // that lies in [row - left, row + right]: one per-lane value, the bounds' other terms are uniform.  Called in the tiles that are not interior only.
  // The sink: or that key lies below win_sink (`sk`: uniform but for the lane half; never true without a sink).
  // (the three bounds less `base` are kept per lane: as uniform values next to s_n, gap and s_full they cost the loop 40 SGPR lane reloads)
  // FRAMES: the range is that of the row's frame, [(f - left) T, (f + right + 1) T - 1] with f = row / T: one division
  // per row here, nothing in the tile loop.
  const int w_g = (AT ? p.win_q0 : 0) + q0 + r;      // the lane's row (AT: as a global token)
  const int w_row = w_g - 4 * h;
  int w_lo = w_row - (p.win_left < 0 ? (1 << 30) : p.win_left), w_hi = w_row + (p.win_right < 0 ? (1 << 30) : p.win_right);
  if constexpr (FRAMES) {
    const int w_f = (int)((unsigned)w_g / (unsigned)p.win_frame);
    if (p.win_left >= 0) w_lo = (w_f - p.win_left) * p.win_frame - 4 * h;
    if (p.win_right >= 0) w_hi = (w_f + p.win_right + 1) * p.win_frame - 1 - 4 * h;
  }
  const int w_sk = p.win_sink - 4 * h;
  auto mask_window = [&](int g, f32x16& sacc) {
    const int base = (2 * global_tile(g >> 1) + (g & 1)) * 32;
    const int lo = w_lo - base, hi = w_hi - base, sk = w_sk - base;
    // the lane's visible in-half positions as one bit mask (positions 0 .. 27 occur): [0, sk) or [lo, hi].  As three compares per element
    // hipcc turns the `or` into an exec-mask branch per element (+2700 instructions in the kernel)
    const unsigned below_sk = (1u << min(max(sk, 0), 28)) - 1u, below_lo = (1u << min(max(lo, 0), 28)) - 1u, to_hi = (1u << min(max(hi + 1, 0), 28)) - 1u;
    const unsigned seen = below_sk | (to_hi & ~below_lo);
#pragma unroll
    for (int e = 0; e < 16; ++e) sacc[e] = seen & (1u << ((e & 3) + 8 * (e >> 2))) ? sacc[e] : -INFINITY;
  };
  // WIN, PRE: what a lane's maximum must exceed for the reference to move: 2^THR once the row has met a finite score, anything before
  float gate = -INFINITY;
  f32x16 o_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o_acc[dt][e] = 0.f;
  bf16x8 pf_prev[2];       // packed P of the previous half, one fragment per 16-key step
  auto pv_half = [&](auto ghalf_c) {
    constexpr int ghalf = decltype(ghalf_c)::value;
    constexpr int slot = (ghalf >> 1) & (NSLOT - 1);
    constexpr int imm = slot * KV_TILE_BYTES + (ghalf & 1) * 8192;
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      bf16x8 vf[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {                                                   // 8 transposed reads first ...
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vaddr[0][dt] + imm + ss * 4096));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vaddr[1][dt] + imm + ss * 4096));
        const bf16x4 lo_b = __builtin_bit_cast(bf16x4, lo), hi_b = __builtin_bit_cast(bf16x4, hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          vf[dt][e] = lo_b[e];
          vf[dt][4 + e] = hi_b[e];
        }
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)                                                     // ... then 4 MFMAs
        o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[dt], pf_prev[ss], o_acc[dt], 0, 0, 0);
    }
  };

  float m_run = -INFINITY, l_run = 0.f;
  const float c = p.scale_log2e;

  // ---- prologue: tiles 0 and 1 on their way, S(half 0) computed; zero the V half that PV(-1) multiplies by P = 0
  if constexpr (SHORT) {
    if (bh != bh_loaded) {                 // first unit of a (batch, head): every tile of it into its slot, once
      if (bh_loaded >= 0) __builtin_amdgcn_s_barrier();      // every wave is done with the tiles of the head before
      bh_loaded = bh;
      if (ntiles < NSLOT) *(u32x4*)(smem + V_RING + (NSLOT - 1) * KV_TILE_BYTES + 8192 + tid * 16) = (u32x4){0u, 0u, 0u, 0u};   // (4 tiles: slot 3 holds finite data)
      for (int tt = 0; tt < ntiles; ++tt) issue_tile(tt);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  } else {
    *(u32x4*)(smem + V_RING + (NSLOT - 1) * KV_TILE_BYTES + 8192 + tid * 16) = (u32x4){0u, 0u, 0u, 0u};
    issue_tile(0);
    if (ntiles > 1) issue_tile(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  __builtin_amdgcn_sched_barrier(0);
  f32x16 s_a, s_b;         // scores of the current / next half, ping-ponged statically (no register copies)
  qk_part(IC<0>{}, IC<0>{}, s_a);
  qk_part(IC<0>{}, IC<4>{}, s_a);
  qk_read(IC<1>{}, IC<0>{}, kf_pre);
  constexpr bool FIRST_IN_PROLOGUE = PRE && FULL;
  if constexpr (FIRST_IN_PROLOGUE) {
    // the first reference = the row maximum of half tile 0, set HERE: as a `g == 0` case of the step's rescale test it costs a scalar
    // test and ~50 register copies (phi nodes of the loop-carried state) per loop iteration on the common path.  (FULL only: the
    // general instance has no register to spare for it.)
    float mx = s_a[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) mx = fmaxf(mx, s_a[e]);
    mx = pair_max(mx);
    ref = mx;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s_a[e] -= mx;
      negref[e] = -mx;
    }
  }
#pragma unroll
  for (int ss = 0; ss < 2; ++ss)
#pragma unroll
    for (int e = 0; e < 8; ++e) pf_prev[ss][e] = (bf16)0.f;

  // one half-tile step g, the same straight-line shape for every g:
  //  * S(g+1) is always computed; past the last half it reads stale LDS, mask_half turns it into -inf and the
  //    step that consumes it adds exactly 0 (exp2(-inf) = 0, no rescale);
  //  * PV(g-1) is always issued; for g = 0 P is zero and the V half it reads (slot 3, second half) was zeroed.
  // A half-tile step g in two parts.  Part A: first half of S(g+1) on the matrix pipe (fragments read during the previous step) |
  // row maximum of S(g) on the VALU, and the (rare) deferred rescale.  Part B: second half of S(g+1) and PV(g-1) on the matrix pipe |
  // exp2 / row sum / pack of S(g) on the VALU.
  // (Tried and not kept: 1..8 scores of every half exponentiated one part later, in part A of the next step.  It paid with a key-mask
  // branch in every step, profiles/r4g_*; with the one-block step none deferred is best, profiles/r4ab_*.)
  auto stepA = [&](int g, f32x16& s_cur, f32x16& s_nxt, auto mask_c) __attribute__((always_inline)) {
    if constexpr (WIN) {
      const int tl = g >> 1;               // (local: a tile below s_full is its own global index)
      // ONE uniform branch, as mask_half is in the general instances: interior tiles -- of the window, or wholly below the sink -- run unmasked
      if (tl >= s_full && (tl < ti_lo || tl > ti_hi)) {
        mask_half(g, s_cur);               // (the ragged last tile is not interior)
        mask_window(g, s_cur);
      }
    } else {
    if constexpr (FULL && decltype(mask_c)::value) mask_shift(g, s_cur);
    mask_half(g, s_cur);             // keys past Lk -> -inf (uniform branch, only taken in the last tile)
    }
    qk_mma(IC<0>{}, kf_pre, s_nxt);
    const float m0 = vmax8(s_cur[0], s_cur[1], s_cur[2], s_cur[3], s_cur[4], s_cur[5], s_cur[6], s_cur[7]);
    const float m1 = vmax8(s_cur[8], s_cur[9], s_cur[10], s_cur[11], s_cur[12], s_cur[13], s_cur[14], s_cur[15]);
    // the test needs no row maximum: any(lane maximum > THR) over the wave is any(row maximum > THR); the exchange between the
    // two lanes of a row happens in the rare branch only (-0.7 % of a step, profiles/r4e_*)
    const float mloc = vmax(m0, m1);
    if constexpr (PRE) {
      // ---- deferred rescale (always taken for half 0, which sets the reference to the first row maximum): O, l, the pending
      // P(g-1), the scores of this half and the already started chain of the next half all move to the new reference
      const bool first = !WIN && !FIRST_IN_PROLOGUE && g == 0;       // FULL: the first reference is set in the prologue
      if (WIN ? __any(mloc > gate) : first || __any(mloc > RESCALE_THR_LOG2)) {            // relative to ref
        const float mx = pair_max(mloc);
        float delta = first ? mx : fmaxf(mx, 0.f);
        float alpha = first ? 1.f : __builtin_amdgcn_exp2f(-delta);
        if constexpr (WIN) {
          // a row that has met no finite score yet (O = l = P = 0, reference 0) takes its first maximum as the reference, as `first` does
          // for every row of half 0; it stays unset while that maximum is -inf
          const bool started = gate > -INFINITY, live = mx > -INFINITY;
          delta = started ? delta : live ? mx : 0.f;
          alpha = started ? alpha : 1.f;
          gate = started || live ? RESCALE_THR_LOG2 : -INFINITY;
        }
        ref += delta;
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int e = 0; e < 16; ++e) o_acc[dt][e] *= alpha;
#pragma unroll
        for (int ss = 0; ss < 2; ++ss)
#pragma unroll
          for (int e = 0; e < 8; ++e) pf_prev[ss][e] = f2bf(bf2f(pf_prev[ss][e]) * alpha);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          s_cur[e] -= delta;
          s_nxt[e] -= delta;
          negref[e] = -ref;
        }
      }
    } else {
      // ---- deferred rescale (always taken for half 0): O, l AND the pending P(g-1) move to the new max
      if (__any((mloc - m_run) * c > RESCALE_THR_LOG2)) {
        const float mx = pair_max(mloc);
        const float m_new = fmaxf(m_run, mx);
        // (WIN: a row all of whose scores so far are masked keeps m = -inf; -inf - -inf is not a factor)
        const float alpha = WIN && m_new == -INFINITY ? 1.f : __builtin_amdgcn_exp2f((m_run - m_new) * c);
        l_run *= alpha;
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int e = 0; e < 16; ++e) o_acc[dt][e] *= alpha;
#pragma unroll
        for (int ss = 0; ss < 2; ++ss)
#pragma unroll
          for (int e = 0; e < 8; ++e) pf_prev[ss][e] = f2bf(bf2f(pf_prev[ss][e]) * alpha);
      }
    }
  };
  auto stepB = [&](auto g8_c, f32x16& s_cur, f32x16& s_nxt) __attribute__((always_inline)) {     // g8 = g mod 8 as a compile-time constant
    constexpr int g8 = decltype(g8_c)::value;
    float psum = 0.f;
    bf16x8 pn[2];
    qk_part(IC<((g8 + 1) & 7)>{}, IC<4>{}, s_nxt);      // (its four K fragments read at the end of part A instead: -0.2 %, profiles/r4g)
    pv_half(IC<((g8 + 7) & 7)>{});
    qk_read(IC<((g8 + 2) & 7)>{}, IC<0>{}, kf_pre);          // for the next step's part A
    const float mc = PRE ? 0.f : WIN && m_run == -INFINITY ? 0.f : m_run * c;      // (WIN: such a row holds -inf scores only: exp2(-inf) = 0)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float pv = PRE ? __builtin_amdgcn_exp2f(s_cur[e]) : __builtin_amdgcn_exp2f(__builtin_fmaf(s_cur[e], c, -mc));
      psum = e == 0 ? pv : psum + pv;                       // (0 + x is an instruction: x may be -0 as far as the compiler knows)
      pn[e >> 3][e & 7] = f2bf(pv);
    }
    l_run += psum;
    pf_prev[0] = pn[0];            // PV(g-1) above consumed the old value (program order)
    pf_prev[1] = pn[1];
    // pin the softmax results here: hipcc otherwise sinks the whole exp chain below the next step's branch
    asm volatile("" : "+v"(pf_prev[0]), "+v"(pf_prev[1]), "+v"(l_run));
    // Block B schedule: hipcc otherwise emits the 12 MFMAs first and the exp chain after them, leaving the matrix
    // pipe idle during the softmax.  Interleave: per MFMA two LDS reads (20 in the block) and ~5 VALU ops.
    // (2 / 4 / 6 more LDS reads in front of the block's first MFMA: +0.1 / -0.7 / -1.1 %, profiles/r4g)
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // DS read
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, PRE ? 4 : 5, 0);   // VALU (exp2 / fma / add / cvt)
    }
  };

  // Measured and not kept (profiles/r4e_attn_stagger_and_local_max.txt): waves 4-7 half a step behind their SIMD partners (their
  // barrier in front of part B instead of part A).  As two copies of the loop it does not fit the instruction cache (-10 %), as one
  // copy with two conditional barrier sites -1.4 % alone and +1.1 % on the step.
  auto tile = [&](int t, auto t4_c, auto mask_c) __attribute__((always_inline)) {       // t4 = t mod 4 as a compile-time constant
    constexpr int t4 = decltype(t4_c)::value;
    auto top = [&](int tt) __attribute__((always_inline)) {
      if constexpr (SHORT) return;         // every tile is resident
      if (FULL || tt > 0) {
        // top of 64-key tile tt: tile tt+1 (issued one tile ago) has landed and becomes visible; the slot of tile
        // tt-2 (last read by the PV of its second half) is free again
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      }
      // K pieces of tile tt+2 now, its V pieces half a tile later: two short bursts of LDS-DMA issue per tile instead
      // of one of four per wave right after the barrier (-1.2...-1.6 % time; placements inside the steps' MFMA blocks were slower)
      if constexpr (FULL) issue_tile(min(tt + 2, ntiles - 1), 1, tt + 2);
      else if (tt + 2 < ntiles) issue_tile(tt + 2, 1);
    };
    // (every wave with its barrier between parts A and B of the odd step instead: +1.1 % alone, -0.7 % on the step, not additive
    //  with the deferred scores: profiles/r4g_*)
    top(t);
    stepA(2 * t, s_a, s_b, mask_c);
    stepB(IC<2 * t4>{}, s_a, s_b);
    if constexpr (SHORT) {
    } else if constexpr (FULL) issue_tile(min(t + 2, ntiles - 1), 2, t + 2);
    else if (t + 2 < ntiles) issue_tile(t + 2, 2);
    stepA(2 * t + 1, s_b, s_a, mask_c);
    stepB(IC<2 * t4 + 1>{}, s_b, s_a);
  };
  using MaskOn = std::integral_constant<bool, true>;
  using MaskOff = std::integral_constant<bool, false>;
  int t = 0;
  // FULL: the main loop leaves 1..4 tail tiles (the only ones that may hold the shifted last tile); otherwise 0..3
  for (; t + 4 <= ntiles - (FULL ? 1 : 0); t += 4) {
    tile(t, IC<0>{}, MaskOff{});
    tile(t + 1, IC<1>{}, MaskOff{});
    tile(t + 2, IC<2>{}, MaskOff{});
    tile(t + 3, IC<3>{}, MaskOff{});
  }
  const int rem = ntiles - t;               // tail tiles, same code with static slots
  if (rem > 0) tile(t, IC<0>{}, MaskOn{});
  if (rem > 1) tile(t + 1, IC<1>{}, MaskOn{});
  if (rem > 2) tile(t + 2, IC<2>{}, MaskOn{});
  if (rem > 3) tile(t + 3, IC<3>{}, MaskOn{});
  // pending PV of the last half (2*ntiles - 1): its slot is (ntiles - 1) & 3
  switch ((ntiles - 1) & 3) {
    case 0: pv_half(IC<1>{}); break;
    case 1: pv_half(IC<3>{}); break;
    case 2: pv_half(IC<5>{}); break;
    default: pv_half(IC<7>{}); break;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  const float l_tot = pair_sum(l_run);
  if (partial) {
    store_partial<false>(p, o_acc, 1.0f, PRE ? ref : m_run, l_tot, split, ul, wave, r, h, q0 + r);      // PRE: reference in exp2 units
    return;
  }
  store_output(p, o_acc, AT && !(l_tot > 0.f) ? 0.f : 1.0f / l_tot, b, head, q0 + r, h);      // (AT: a row that saw no key is zeros)
  }   // q blocks of this workgroup
}
template <int KIND, bool PRE, bool FULL = false, bool SHORT = false>
__global__ __launch_bounds__(NT, 2) void attn_fwd_kernel(AttnParams p) { attn_fwd_body<KIND, PRE, FULL, SHORT, false>(p); }
// The windowed instances (a name of their own: the profiler and tools/kernel_resources.py tell them from the six above)
template <bool PRE>
__global__ __launch_bounds__(NT, 2) void attn_window_kernel(AttnParams p) { attn_fwd_body<0, PRE, false, false, true>(p); }
// ... and the same two with the window counted in frames (AttnParams::win_frame > 0).  Instances of their own, not a run-time branch on
// win_frame in the two above: the branch sits at kernel entry only, but with it hipcc schedules the whole kernel anew, and the token-window
// launches measured 0.2 - 1.8 % slower than the parent build's (tools/attn_window_bench.py --frames --base); so those two stay as they were
template <bool PRE>
__global__ __launch_bounds__(NT, 2) void attn_window_frames_kernel(AttnParams p) { attn_fwd_body<0, PRE, false, false, true, true>(p); }

#include "attn_fp8.inc"

// out[b][q][head][:] = sum_s w_s O_s / sum_s w_s l_s with w_s = exp2((m_s - max_s m_s) * scale_log2e) for the rows of the
// launch's units; one wave per row, two columns per lane.  OSHIFT: + p.o_shift[b][head * 128 + column] in fp32 in front of the rounding
// (once, here: the partials' weights w_s l_s / sum sum to 1)
template <bool OSHIFT>
__global__ __launch_bounds__(256) void attn_merge_kernel(AttnParams p) {
  const int64_t rows = (int64_t)p.n_units * QBLK;
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    const int ul = (int)(row / QBLK), rr = (int)(row % QBLK);
    const int unit = p.unit0 + ul;
    const int qb = unit % p.q_blocks, bh = unit / p.q_blocks;
    const int q = qb * QBLK + rr;
    if (q >= p.Lq) continue;
    float m = -INFINITY;
    for (int s = 0; s < p.n_slots; ++s) m = fmaxf(m, p.ws_ml[(s * rows + row) * 2]);
    float l = 0.f;
    f32x2 acc = {0.f, 0.f};
    for (int s = 0; s < p.n_slots; ++s) {
      const f32x2 ml = *(const f32x2*)(p.ws_ml + (s * rows + row) * 2);
      const float w = __builtin_amdgcn_exp2f((ml[0] - m) * (p.prescaled ? 1.0f : p.scale_log2e));
      l += w * ml[1];
      const f32x2 o = *(const f32x2*)(p.ws_o + (s * rows + row) * HD + 2 * lane);
      acc += o * w;
    }
    const int head = bh % p.H, b = bh / p.H;
    const float inv = 1.0f / l;
    bf16x2 ov;
    if constexpr (OSHIFT) {
      const f32x2 sh = *(const f32x2*)(p.o_shift + (int64_t)bh * HD + 2 * lane);
      ov[0] = f2bf(acc[0] * inv + sh[0]);
      ov[1] = f2bf(acc[1] * inv + sh[1]);
    } else {
      ov[0] = f2bf(acc[0] * inv);
      ov[1] = f2bf(acc[1] * inv);
    }
    *(bf16x2*)(p.o + (int64_t)b * p.o_bs + (int64_t)q * p.o_rs + head * HD + 2 * lane) = ov;
  }
}

// One attention call as its entry point states it: every extern "C" entry fills the fields it has.
struct AttnCall {
  const void *q = nullptr, *k = nullptr, *v = nullptr;
  void *o = nullptr, *stream = nullptr;
  int64_t q_bs = 0, q_rs = 0, k_bs = 0, k_rs = 0, v_bs = 0, v_rs = 0, o_bs = 0, o_rs = 0;
  int B = 0, H = 0, Lq = 0, Lk = 0, head_dim = 0;
  float softmax_scale = 0.f, last_key_bias = 0.f;
  // units from split_from_unit on run as kv_splits key ranges each; partial_slot0 >= 0: partials of every unit into the workspace slots from it on, no merge
  int kv_splits = 1, split_from_unit = 0, partial_slot0 = -1;
  float *ws_o = nullptr, *ws_ml = nullptr;
  const void *q8 = nullptr, *qs = nullptr, *kv8 = nullptr;   // MXFP8 operands (flexam_attn_fp8_pack) instead of q / k / v
  int kv8_chunk_tiles = 0;                     // 0 = one chunk holds all key tiles
  const float* o_shift = nullptr;              // MXFP8 only (flexam_attn_fwd_fp8_oshift): see AttnParams::o_shift
  int win_left = -1, win_right = -1;           // flexam_attn_fwd_window: see AttnParams::win_left; a negative side is unbounded
  int win_sink = 0;                            // flexam_attn_fwd_window_sink: see AttnParams::win_sink
  bool win_by_frames = false;                  // flexam_attn_fwd_window_frames: win_left / win_right count frames of win_frame tokens
  int win_frame = 0;                           // see AttnParams::win_frame; read under win_by_frames only
  // flexam_attn_fwd_window_at: row i is global token win_q0 + i, Lq and Lk two lengths.  Its entry point has normalised the window (the
  // sides and the sink as the kernel takes them, win_frame >= 1 with a token window as frames of one token): attn_run takes them as they are
  bool win_at = false;
  int win_q0 = 0;
  // flexam_attn_fwd_window_halo (with win_at): k and v are a compact buffer of win_k_rows rows, the sink tiles and then the key tiles from
  // global tile s_n + win_key_gap on.  attn_run walks the call's query blocks and refuses a buffer that a unit's tiles do not fit
  bool win_halo = false;
  int win_key_gap = 0, win_k_rows = 0;
};
// The twelve instances and the rule that picks one.  cross: separate symbols for the short-context (text) launches.  short_ctx: the text
// cross-attention (at most 4 key tiles, pre-scaled q, one launch without key splits): K/V resident, several q blocks per workgroup.
struct AttnInstance { void (*kern)(AttnParams); int smem, slot; };      // dynamic LDS: rings of 4 K and 4 V tiles, 128 KiB (fp8: 4 records, 68 KiB); slot in attr_set
constexpr int ATTN_INSTANCES = 16;
// the two windowed MXFP8 kernels take their mask as a second argument; defined at the end of this file, as the two below
struct Attn8WindowInstance { void (*kern)(AttnParams, Attn8Window); int slot; };      // slot in win_attr_set (attn_run)
Attn8WindowInstance attn8_window_instance(bool oshift);
// ... and the two at a query offset (slots 2 and 3), defined last of all in this file
struct Attn8WindowAtInstance { void (*kern)(AttnParams, Attn8WindowAt); int slot; };
Attn8WindowAtInstance attn8_window_at_instance(bool oshift);
// the two attn_window_frames_kernel instances (slots 10 and 11).  Defined at the end of this file, so that they are emitted behind every
// other kernel of it: a listing of this file then differs from one without them by the two kernels alone (tools/isa_diff.py)
AttnInstance attn_frames_instance(bool prescaled);
// ... and, behind those, the two attn_window_at_kernel instances (slots 12 and 13), for the same reason
AttnInstance attn_at_instance(bool prescaled);
// ... and, last, the two attn_window_halo_kernel instances (slots 14 and 15)
AttnInstance attn_halo_instance(bool prescaled);
AttnInstance attn_instance(bool fp8, bool oshift, bool cross, bool prescaled, bool full, bool short_ctx, bool window, bool frames) {
  constexpr int BF = NSLOT * 2 * KV_TILE_BYTES, F8 = NSLOT * REC_BYTES;
  static const AttnInstance table[10] = {{attn_fwd_kernel<0, false>, BF, 0}, {attn_fwd_kernel<1, false>, BF, 1}, {attn_fwd_kernel<0, true>, BF, 2},
                                        {attn_fwd_kernel<1, true>, BF, 3}, {attn_fwd_kernel<0, true, true>, BF, 4},
                                        {attn_fwd_kernel<1, true, false, true>, BF, 5}, {attn8_fwd_kernel<0>, F8, 6},
                                        {attn8_oshift_kernel, F8, 7},      // the MXFP8 kernel that adds AttnParams::o_shift (smooth-V)
                                        {attn_window_kernel<false>, BF, 8}, {attn_window_kernel<true>, BF, 9}};      // sliding window (bf16)
  if (window && frames) return attn_frames_instance(prescaled);
  if (window) return table[prescaled ? 9 : 8];
  return table[fp8 ? (oshift ? 7 : 6) : full ? 4 : short_ctx ? 5 : (cross ? 1 : 0) + (prescaled ? 2 : 0)];
}
// FLEXAM_ATTN_FULL / _SHORT / _FUSED_TAIL, read per call (A/B in one process): 0 = the general instance / one workgroup per q block / two launches
bool attn_switch(const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); }
void scale_and_blocks(AttnParams& p, float softmax_scale) {      // what the attention launches and the merge alone derive alike
  p.prescaled = softmax_scale < 0.f;                   // FLEXAM_ATTN_PRESCALED: q already carries softmax_scale * log2(e)
  p.scale_log2e = p.prescaled ? 1.0f : softmax_scale * 1.4426950408889634f;
  p.q_blocks = (p.Lq + QBLK - 1) / QBLK;
}
void split_part(AttnParams& p, int unit0, int n_units, int S, int tps) {      // n_units units from unit0 on as S key ranges of tps tiles each, written as partials
  p.unit0 = unit0; p.n_units = n_units; p.kv_splits = S; p.tiles_per_split = tps; p.partial = 1; p.n_slots = S;
}
void launch_merge(const AttnParams& p, void* stream) {      // one wave per row of the launch's units, grid-stride past 16384 workgroups
  const int64_t g = ((int64_t)p.n_units * QBLK + 3) / 4;
  const dim3 grid((unsigned)(g > 16384 ? 16384 : g));
  if (p.o_shift) hipLaunchKernelGGL(attn_merge_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(attn_merge_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
}

int attn_run(const AttnCall& c) {
  FX_REQUIRE(((c.q && c.k && c.v) || (c.q8 && c.qs && c.kv8)) && (c.o || c.partial_slot0 >= 0), FLEXAM_E_ARG, "attn_fwd: null pointer");
  FX_REQUIRE(c.head_dim == HD, FLEXAM_E_SHAPE, "attn_fwd: head_dim %d unsupported (128 only)", c.head_dim);
  FX_REQUIRE(c.B > 0 && c.H > 0 && c.Lq > 0 && c.Lk > 0, FLEXAM_E_SHAPE, "attn_fwd: empty problem B=%d H=%d Lq=%d Lk=%d", c.B, c.H, c.Lq, c.Lk);
  FX_REQUIRE(c.q_rs % 8 == 0 && c.k_rs % 8 == 0 && c.v_rs % 8 == 0 && c.o_rs % 8 == 0 && c.q_bs % 8 == 0 && c.k_bs % 8 == 0 && c.v_bs % 8 == 0 && c.o_bs % 8 == 0,
             FLEXAM_E_SHAPE, "attn_fwd: strides must keep 16-byte alignment of head rows");
  FX_REQUIRE(((uintptr_t)c.q | (uintptr_t)c.k | (uintptr_t)c.v | (uintptr_t)c.o | (uintptr_t)c.o_shift) % 16 == 0, FLEXAM_E_ARG, "attn_fwd: misaligned pointer");
  FX_REQUIRE(!c.o_shift || (c.q8 && c.partial_slot0 < 0), FLEXAM_E_ARG, "attn_fwd: an output shift goes with the MXFP8 operands and a final output");
  const int tiles_all = (c.Lk + KVBLK - 1) / KVBLK;
  FX_REQUIRE(c.kv_splits >= 1 && c.kv_splits <= tiles_all, FLEXAM_E_ARG, "attn_fwd: %d key splits for %d key tiles", c.kv_splits, tiles_all);
  FX_REQUIRE((c.kv_splits == 1 && c.partial_slot0 < 0) || (c.ws_o && c.ws_ml), FLEXAM_E_ARG, "attn_fwd: split-KV needs both workspaces");
  AttnParams p;
  p.q = (const bf16*)c.q; p.k = (const bf16*)c.k; p.v = (const bf16*)c.v; p.o = (bf16*)c.o; p.B = c.B; p.H = c.H; p.Lq = c.Lq; p.Lk = c.Lk;
  p.q_bs = c.q_bs; p.q_rs = c.q_rs; p.k_bs = c.k_bs; p.k_rs = c.k_rs; p.v_bs = c.v_bs; p.v_rs = c.v_rs; p.o_bs = c.o_bs; p.o_rs = c.o_rs;
  scale_and_blocks(p, c.softmax_scale);
  const int tps = (tiles_all + c.kv_splits - 1) / c.kv_splits;
  const int S = (tiles_all + tps - 1) / tps;           // drop empty trailing splits
  p.ws_o = c.ws_o; p.ws_ml = c.ws_ml; p.last_key_bias = c.last_key_bias;
  p.partial = 0; p.slot0 = 0; p.n_slots = S; p.whole_units = 0;
  p.q8 = (const unsigned char*)c.q8; p.qs = (const unsigned*)c.qs; p.kv8 = (const unsigned char*)c.kv8; p.lq_pad = p.q_blocks * QBLK;
  p.kv8_chunk_tiles = c.kv8_chunk_tiles > 0 ? c.kv8_chunk_tiles : tiles_all; p.o_shift = c.o_shift;
  // a side that reaches past the sequence from every row is no bound; no bound at all is the ordinary call, launch for launch
  // (in frames: the last frame is ceil(Lk / T) - 1, and frame_tokens >= Lk is one frame that holds every key)
  FX_REQUIRE(!c.win_by_frames || c.win_frame > 0, FLEXAM_E_ARG, "attn_fwd: frame_tokens %d (1 or more)", c.win_frame);
  const int win_reach = c.win_by_frames ? (int)(((int64_t)c.Lk + c.win_frame - 1) / c.win_frame) - 1 : c.Lk - 1;
  // (win_at: the sides as flexam_attn_fwd_window_at normalised them for the rows of ITS call, which are not rows 0 .. Lk - 1)
  const int win_left = c.win_left < 0 || (!c.win_at && c.win_left >= win_reach) ? -1 : c.win_left;
  const int win_right = c.win_right < 0 || (!c.win_at && c.win_right >= win_reach) ? -1 : c.win_right;
  FX_REQUIRE(c.win_sink >= 0, FLEXAM_E_ARG, "attn_fwd: negative sink %d", c.win_sink);
  // a sink that holds every key leaves no mask; one under a window without a left bound (nothing lies to the left of it) adds no key
  const bool window = (win_left >= 0 || win_right >= 0) && c.win_sink < c.Lk;
  const int win_sink = win_left < 0 ? 0 : c.win_sink;
  FX_REQUIRE(!c.win_at || (window && c.win_by_frames && c.win_q0 >= 0), FLEXAM_E_ARG, "attn_fwd: a window at an offset is a call under a mask");
  FX_REQUIRE(!window || ((c.Lq == c.Lk || c.win_at) && (c.kv8_chunk_tiles == 0 || (c.win_at && c.q8)) && c.kv_splits == 1 && c.partial_slot0 < 0 && c.last_key_bias == 0.f),
             FLEXAM_E_ARG, "attn_fwd: a window goes with operands of one length (MXFP8: one chunk) or a query offset, and whole work units");
  FX_REQUIRE(tiles_all < 65536, FLEXAM_E_SHAPE, "attn_fwd: %d key tiles (at most 65535)", tiles_all);
  p.kv8_chunk_magic = p.kv8_chunk_tiles > 1 ? (unsigned)(((1ull << 32) + (unsigned)p.kv8_chunk_tiles - 1) / (unsigned)p.kv8_chunk_tiles) : 0u;
  // (in the words of four MXFP8 fields above: see AttnParams.  A token window leaves win_frame 0, the low word of the null qs, and runs
  //  the instances that do not read it)
  const bool fp8 = c.q8 != nullptr, cross = c.Lk <= 1024;
  if (window && !fp8) { p.win_left = win_left; p.win_right = win_right; p.win_sink = win_sink; if (c.win_by_frames) p.win_frame = c.win_frame; }
  if (c.win_at) p.win_q0 = c.win_q0;       // (in the word of n_slots, which only a merge reads: see AttnParams)
  if (c.win_halo) {
    FX_REQUIRE(c.win_at && window, FLEXAM_E_ARG, "attn_fwd_window_halo: a call that sees every key reads all %d of them, not a compact buffer", c.Lk);
    FX_REQUIRE(c.win_key_gap >= 0 && c.win_k_rows >= 0 && c.win_k_rows <= c.Lk, FLEXAM_E_ARG, "attn_fwd_window_halo: key_gap_tiles %d, k_rows %d (of %d keys)",
               c.win_key_gap, c.win_k_rows, c.Lk);
    // The tiles every query block visits, by the arithmetic of attn_fwd_body (WIN, FRAMES, AT) on the words the kernel will read: the sink
    // tiles [0, s_n) and the window tiles [s_n + gap, w_n + gap).  A tile in the gap the buffer leaves out, or one whose last key row
    // (cut at Lk) lies behind the buffer's last row, is a wrong plan: refused here, never read
    const int T = p.win_frame, s_n = (std::min(p.win_sink, p.Lk) + KVBLK - 1) / KVBLK;
    for (int qb = 0; qb < p.q_blocks; ++qb) {
      const int qa = p.win_q0 + qb * QBLK, qz = p.win_q0 + std::min(qb * QBLK + QBLK, p.Lq) - 1;
      const int fa = (int)((unsigned)qa / (unsigned)T), fz = (int)((unsigned)qz / (unsigned)T);
      const int lo_a = (fa - p.win_left) * T, hi_z = (fz + p.win_right + 1) * T - 1;
      const int k_first = p.win_left < 0 ? 0 : std::max(0, lo_a), k_last = p.win_right < 0 ? p.Lk - 1 : std::min(p.Lk - 1, hi_z);
      int gap = std::max(0, k_first / KVBLK - s_n), w_n = std::max(k_last / KVBLK, s_n - 1) + 1 - gap;
      if (k_first > k_last) { gap = 0; w_n = s_n; }
      const int64_t sink_end = std::min<int64_t>((int64_t)s_n * KVBLK, p.Lk);                              // one behind the last key row read of each run
      const int64_t win_end = std::min<int64_t>((int64_t)(w_n + gap) * KVBLK, p.Lk) - (int64_t)c.win_key_gap * KVBLK;
      FX_REQUIRE(s_n == 0 || sink_end <= c.win_k_rows, FLEXAM_E_ARG, "attn_fwd_window_halo: query block %d reads the sink's %d key rows, the buffer holds %d",
                 qb, (int)sink_end, c.win_k_rows);
      FX_REQUIRE(w_n == s_n || (gap >= c.win_key_gap && win_end <= c.win_k_rows), FLEXAM_E_ARG,
                 "attn_fwd_window_halo: query block %d reads key tiles %d .. %d; the buffer (key_gap_tiles %d, k_rows %d) holds tiles %d .. %d behind %d sink tiles",
                 qb, s_n + gap, w_n + gap - 1, c.win_key_gap, c.win_k_rows, s_n + c.win_key_gap, (c.win_k_rows + KVBLK - 1) / KVBLK + c.win_key_gap - 1, s_n);
    }
    p.win_key_gap = c.win_key_gap;         // (in the low word of the null kv8: see AttnParams)
  }
  FX_REQUIRE(c.q8 || (int64_t)c.Lk * c.k_rs * 2 < (1ll << 31) && (int64_t)c.Lk * c.v_rs * 2 < (1ll << 31), FLEXAM_E_SHAPE,
             "attn_fwd: one (batch, head) K/V panel must span < 2 GiB (32-bit tile offsets)");
  if (window && fp8) {
    // the windowed MXFP8 kernels read the four MXFP8 words of AttnParams AND a window: theirs is an argument of its own (Attn8Window).
    // One workgroup per unit, every unit whole
    const Attn8Window w = {win_left, win_right, win_sink, c.win_by_frames ? c.win_frame : 0};
    const Attn8WindowInstance wi = attn8_window_instance(c.o_shift != nullptr);
    const Attn8WindowAtInstance ai = attn8_window_at_instance(c.o_shift != nullptr);      // (win_at: flexam_attn_fwd_fp8_window_at, the records in chunks)
    const void* kern = c.win_at ? (const void*)ai.kern : (const void*)wi.kern;
    constexpr int F8 = NSLOT * REC_BYTES;
    static bool win_attr_set[FLEXAM_MAX_DEVICES][4] = {};
    bool& raised = win_attr_set[flexam_current_device()][c.win_at ? ai.slot : wi.slot];
    if (!raised) {
      if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, F8) != hipSuccess)
        return flexam_fail(FLEXAM_E_LAUNCH, "attn_fwd: cannot raise dynamic LDS to %d bytes", F8);
      raised = true;
    }
    const int n = c.B * c.H * p.q_blocks;
    p.unit0 = 0; p.n_units = n; p.kv_splits = 1; p.tiles_per_split = tiles_all;
    if (c.win_at) {
      const Attn8WindowAt a = {w, c.win_q0};
      hipLaunchKernelGGL(ai.kern, dim3(n), dim3(NT), F8, (hipStream_t)c.stream, p, a);
      return flexam_check_launch("flexam_attn_fwd_fp8_window_at");
    }
    hipLaunchKernelGGL(wi.kern, dim3(n), dim3(NT), F8, (hipStream_t)c.stream, p, w);
    return flexam_check_launch("flexam_attn_fwd_fp8_window");
  }
  const bool short_ctx = !window && !fp8 && cross && p.prescaled && tiles_all <= NSLOT && c.kv_splits == 1 && c.partial_slot0 < 0 && attn_switch("FLEXAM_ATTN_SHORT");
  const bool full = !window && !fp8 && !cross && p.prescaled && c.Lk >= KVBLK && c.last_key_bias == 0.f && attn_switch("FLEXAM_ATTN_FULL");
  const AttnInstance inst = c.win_halo ? attn_halo_instance(p.prescaled) : c.win_at ? attn_at_instance(p.prescaled)
                                     : attn_instance(fp8, c.o_shift != nullptr, cross, p.prescaled, full, short_ctx, window, window && c.win_by_frames);
  static bool attr_set[FLEXAM_MAX_DEVICES][ATTN_INSTANCES] = {};      // per device and kernel instance
  bool& lds_raised = attr_set[flexam_current_device()][inst.slot];
  if (!lds_raised) {
    if (hipFuncSetAttribute((const void*)inst.kern, hipFuncAttributeMaxDynamicSharedMemorySize, inst.smem) != hipSuccess)
      return flexam_fail(FLEXAM_E_LAUNCH, "attn_fwd: cannot raise dynamic LDS to %d bytes", inst.smem);
    lds_raised = true;
  }
  const int units = c.B * c.H * p.q_blocks;
  FX_REQUIRE(c.split_from_unit >= 0 && c.split_from_unit <= units, FLEXAM_E_ARG, "attn_fwd: split_from_unit %d of %d units", c.split_from_unit, units);
  auto launch = [&](int grid) { hipLaunchKernelGGL(inst.kern, dim3(grid), dim3(NT), inst.smem, (hipStream_t)c.stream, p); };
  auto launch_whole = [&](int n_units, int grid) { p.unit0 = 0; p.n_units = n_units; p.kv_splits = 1; p.tiles_per_split = tiles_all; launch(grid); };
  if (c.partial_slot0 >= 0) {              // (a) every unit, this call's keys only: partials into slots slot0 .. slot0 + S - 1, no merge
    FX_REQUIRE(S == c.kv_splits, FLEXAM_E_ARG, "attn_fwd_partial: %d key ranges requested but %d key tiles give %d (use ceil(tiles / ceil(tiles / S)))",
               c.kv_splits, tiles_all, S);
    split_part(p, 0, units, S, tps);
    p.slot0 = c.partial_slot0;
    launch(units * S);
    return flexam_check_launch("flexam_attn_fwd_partial");
  }
  const int whole = S == 1 ? units : c.split_from_unit;      // units [0, whole): one pass over all keys; the rest: S key ranges each, then the merge
  if (short_ctx) {                         // (b) one persistent workgroup per CU, each with a contiguous share of the units
    const int cus = flexam_num_cus();
    launch_whole(units, units < cus ? units : cus);
  } else if (whole > 0 && whole < units && attn_switch("FLEXAM_ATTN_FUSED_TAIL")) {
    // (c) one launch: whole units and the split tail side by side on every XCD (see AttnParams::whole_units), then the merge
    p.whole_units = whole;
    split_part(p, whole, units - whole, S, tps);
    launch(8 * ((whole + 7) / 8 + (p.n_units * S + 7) / 8));
    launch_merge(p, c.stream);
  } else {                                 // (d) a launch for each kind
    if (whole > 0) launch_whole(whole, whole);
    if (whole < units) {
      split_part(p, whole, units - whole, S, tps);
      launch(p.n_units * S);
      launch_merge(p, c.stream);
    }
  }
  return flexam_check_launch("flexam_attn_fwd");
}

}  // namespace

extern "C" int flexam_attn_fwd(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs,
                               const void* v, int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H,
                               int Lq, int Lk, int head_dim, float softmax_scale, void* stream) {
  AttnCall c;
  c.q = q; c.q_bs = q_bs; c.q_rs = q_rs; c.k = k; c.k_bs = k_bs; c.k_rs = k_rs; c.v = v; c.v_bs = v_bs; c.v_rs = v_rs; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = Lq; c.Lk = Lk; c.head_dim = head_dim; c.softmax_scale = softmax_scale; c.stream = stream;
  return attn_run(c);
}

extern "C" int flexam_attn_fwd_window(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs,
                                      const void* v, int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H,
                                      int L, int head_dim, float softmax_scale, int window_left, int window_right, void* stream) {
  AttnCall c;
  c.q = q; c.q_bs = q_bs; c.q_rs = q_rs; c.k = k; c.k_bs = k_bs; c.k_rs = k_rs; c.v = v; c.v_bs = v_bs; c.v_rs = v_rs; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = L; c.Lk = L; c.head_dim = head_dim; c.softmax_scale = softmax_scale; c.stream = stream;
  c.win_left = window_left; c.win_right = window_right;
  return attn_run(c);
}

extern "C" int flexam_attn_fwd_window_sink(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs,
                                           const void* v, int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H,
                                           int L, int head_dim, float softmax_scale, int window_left, int window_right, int sink, void* stream) {
  AttnCall c;
  c.q = q; c.q_bs = q_bs; c.q_rs = q_rs; c.k = k; c.k_bs = k_bs; c.k_rs = k_rs; c.v = v; c.v_bs = v_bs; c.v_rs = v_rs; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = L; c.Lk = L; c.head_dim = head_dim; c.softmax_scale = softmax_scale; c.stream = stream;
  c.win_left = window_left; c.win_right = window_right; c.win_sink = sink;
  return attn_run(c);
}

extern "C" int flexam_attn_fwd_window_frames(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs,
                                             const void* v, int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H,
                                             int L, int head_dim, float softmax_scale, int frames_left, int frames_right, int frame_tokens,
                                             int sink, void* stream) {
  AttnCall c;
  c.q = q; c.q_bs = q_bs; c.q_rs = q_rs; c.k = k; c.k_bs = k_bs; c.k_rs = k_rs; c.v = v; c.v_bs = v_bs; c.v_rs = v_rs; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = L; c.Lk = L; c.head_dim = head_dim; c.softmax_scale = softmax_scale; c.stream = stream;
  c.win_left = frames_left; c.win_right = frames_right; c.win_sink = sink; c.win_by_frames = true; c.win_frame = frame_tokens;
  return attn_run(c);
}

// flexam_attn_fwd_window_at and, with c.win_halo set, flexam_attn_fwd_window_halo: c holds the operands, the sizes and the stream
static int attn_window_at(AttnCall c, int window_left, int window_right, int frame_tokens, int sink, int q_offset) {
  const int Lq = c.Lq, Lk = c.Lk;
  FX_REQUIRE(q_offset >= 0, FLEXAM_E_ARG, "attn_fwd_window_at: negative q_offset %d", q_offset);
  FX_REQUIRE(sink >= 0, FLEXAM_E_ARG, "attn_fwd: negative sink %d", sink);
  FX_REQUIRE(frame_tokens >= 0, FLEXAM_E_ARG, "attn_fwd_window_at: frame_tokens %d (0 = a token window)", frame_tokens);
  // (MXFP8, flexam_attn_fwd_fp8_window_at: its entry point leaves kv8_chunk_tiles 0 where one chunk holds exactly the call's tiles)
  if (q_offset == 0 && Lq == Lk && !c.win_halo && c.kv8_chunk_tiles == 0) {         // one length from token 0: the entry point of the form asked for, launch for launch
    c.win_left = window_left; c.win_right = window_right; c.win_sink = sink; c.win_by_frames = frame_tokens > 0; c.win_frame = frame_tokens;
    return attn_run(c);
  }
  if (Lq <= 0 || Lk <= 0) return attn_run(c);      // (attn_run says what is wrong with it)
  const int64_t rows = (int64_t)q_offset + Lq;     // the call's rows are the global tokens q_offset .. rows - 1
  // (the kernel's bounds are 32-bit: at most (2 (rows + Lk) / T + 3) T)
  FX_REQUIRE(rows + Lk < (1ll << 29), FLEXAM_E_SHAPE, "attn_fwd_window_at: q_offset %d + Lq %d + Lk %d tokens (below 2^29)", q_offset, Lq, Lk);
  // a token window is a window of one-token frames: lo(g) = (g / T - left) T, hi(g) = (g / T + right + 1) T - 1 are g - left and g + right
  // at T = 1.  A frame longer than every index of the call holds all of them; a side no shorter than the call's reach is that reach
  const int64_t T = frame_tokens == 0 ? 1 : frame_tokens < rows + Lk ? frame_tokens : rows + Lk;
  const int64_t reach = (rows + Lk) / T + 1;
  const int left = window_left < 0 ? -1 : (int)(window_left < reach ? window_left : reach);
  const int right = window_right < 0 ? -1 : (int)(window_right < reach ? window_right : reach);
  // does a side clip a row of THIS call?  lo and hi are non-decreasing in the row: the left side clips iff it clips the last row (pad rows,
  // whose window may lie behind every key, included), the right side iff it clips the first
  const bool clip_left = left >= 0 && ((rows - 1) / T - left) * T > 0;
  const bool clip_right = right >= 0 && (q_offset / T + right + 1) * T - 1 < Lk - 1;
  // every row sees every key: flexam_attn_fwd on (Lq, Lk).  (win_halo: a compact buffer cannot serve that call; attn_run refuses it)
  if ((!clip_left && !clip_right) || sink >= Lk) {
    // (MXFP8: flexam_attn_fwd_fp8_chunked at kv_splits = 1, which takes no output shift)
    FX_REQUIRE(!(c.q8 && c.o_shift), FLEXAM_E_ARG, "attn_fwd_fp8_window_at: no side of the window clips a row of this call, which is "
               "flexam_attn_fwd_fp8_chunked, and that call takes no o_shift");
    return attn_run(c);
  }
  c.win_at = true; c.win_q0 = q_offset; c.win_by_frames = true; c.win_frame = (int)T;
  c.win_left = left; c.win_right = right; c.win_sink = sink;      // (attn_run drops the sink under left < 0, as for the sibling entry points)
  return attn_run(c);
}

extern "C" int flexam_attn_fwd_window_at(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs,
                                         const void* v, int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H,
                                         int Lq, int Lk, int head_dim, float softmax_scale, int window_left, int window_right,
                                         int frame_tokens, int sink, int q_offset, void* stream) {
  AttnCall c;
  c.q = q; c.q_bs = q_bs; c.q_rs = q_rs; c.k = k; c.k_bs = k_bs; c.k_rs = k_rs; c.v = v; c.v_bs = v_bs; c.v_rs = v_rs; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = Lq; c.Lk = Lk; c.head_dim = head_dim; c.softmax_scale = softmax_scale; c.stream = stream;
  return attn_window_at(c, window_left, window_right, frame_tokens, sink, q_offset);
}

extern "C" int flexam_attn_fwd_window_halo(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs,
                                           const void* v, int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H,
                                           int Lq, int Lk, int head_dim, float softmax_scale, int window_left, int window_right,
                                           int frame_tokens, int sink, int q_offset, int key_gap_tiles, int k_rows, void* stream) {
  AttnCall c;
  c.q = q; c.q_bs = q_bs; c.q_rs = q_rs; c.k = k; c.k_bs = k_bs; c.k_rs = k_rs; c.v = v; c.v_bs = v_bs; c.v_rs = v_rs; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = Lq; c.Lk = Lk; c.head_dim = head_dim; c.softmax_scale = softmax_scale; c.stream = stream;
  // the whole sequence from row 0 on is flexam_attn_fwd_window_at, launch for launch
  c.win_halo = !(key_gap_tiles == 0 && k_rows == Lk); c.win_key_gap = key_gap_tiles; c.win_k_rows = k_rows;
  return attn_window_at(c, window_left, window_right, frame_tokens, sink, q_offset);
}

extern "C" int flexam_attn_fwd_lastkey(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs,
                                       const void* v, int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H,
                                       int Lq, int Lk, int head_dim, float softmax_scale, float last_key_multiplicity, void* stream) {
  FX_REQUIRE(last_key_multiplicity >= 1.0f, FLEXAM_E_ARG, "attn_fwd_lastkey: multiplicity %g < 1", (double)last_key_multiplicity);
  AttnCall c;
  c.q = q; c.q_bs = q_bs; c.q_rs = q_rs; c.k = k; c.k_bs = k_bs; c.k_rs = k_rs; c.v = v; c.v_bs = v_bs; c.v_rs = v_rs; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = Lq; c.Lk = Lk; c.head_dim = head_dim; c.softmax_scale = softmax_scale; c.stream = stream; c.last_key_bias = log2f(last_key_multiplicity);
  return attn_run(c);
}

extern "C" int flexam_attn_fwd_splitkv(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs,
                                       const void* v, int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H,
                                       int Lq, int Lk, int head_dim, float softmax_scale, int kv_splits, int split_from_unit,
                                       float* ws_o, float* ws_ml, void* stream) {
  AttnCall c;
  c.q = q; c.q_bs = q_bs; c.q_rs = q_rs; c.k = k; c.k_bs = k_bs; c.k_rs = k_rs; c.v = v; c.v_bs = v_bs; c.v_rs = v_rs; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = Lq; c.Lk = Lk; c.head_dim = head_dim; c.softmax_scale = softmax_scale; c.stream = stream;
  c.kv_splits = kv_splits; c.split_from_unit = split_from_unit; c.ws_o = ws_o; c.ws_ml = ws_ml;
  return attn_run(c);
}

extern "C" int flexam_attn_fwd_partial(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs,
                                       const void* v, int64_t v_bs, int64_t v_rs, int B, int H, int Lq, int Lk, int head_dim,
                                       float softmax_scale, int kv_splits, int slot0, float* ws_o, float* ws_ml, void* stream) {
  FX_REQUIRE(slot0 >= 0, FLEXAM_E_ARG, "attn_fwd_partial: negative slot");
  AttnCall c;
  c.q = q; c.q_bs = q_bs; c.q_rs = q_rs; c.k = k; c.k_bs = k_bs; c.k_rs = k_rs; c.v = v; c.v_bs = v_bs; c.v_rs = v_rs;
  c.B = B; c.H = H; c.Lq = Lq; c.Lk = Lk; c.head_dim = head_dim; c.softmax_scale = softmax_scale; c.stream = stream;
  c.kv_splits = kv_splits; c.partial_slot0 = slot0; c.ws_o = ws_o; c.ws_ml = ws_ml;
  return attn_run(c);
}

// the pack and the fused producer, without (k_shift = nullptr: the instances the plain entry points have always launched) and with smooth-K;
// the pack also with smooth-V (v_shift)
static int attn8_pack_run(const char* who, const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                          int64_t v_bs, int64_t v_rs, void* q8, void* qs, void* kv8, int B, int H, int L, int head_dim, const float* k_shift,
                          const float* v_shift, void* stream) {
  FX_REQUIRE(v && q8 && qs && kv8 && ((q == nullptr) == (k == nullptr)), FLEXAM_E_ARG, "attn_fp8_pack: null pointer (q and k: both or neither)");
  FX_REQUIRE(head_dim == HD && B > 0 && H > 0 && L > 0, FLEXAM_E_SHAPE, "attn_fp8_pack: bad sizes (head_dim 128 only)");
  FX_REQUIRE(q_rs % 8 == 0 && k_rs % 8 == 0 && v_rs % 8 == 0 && q_bs % 8 == 0 && k_bs % 8 == 0 && v_bs % 8 == 0, FLEXAM_E_SHAPE,
             "attn_fp8_pack: strides must keep 16-byte alignment of head rows");
  FX_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)q8 | (uintptr_t)qs | (uintptr_t)kv8 | (uintptr_t)k_shift | (uintptr_t)v_shift) % 16 == 0, FLEXAM_E_ARG,
             "attn_fp8_pack: misaligned pointer");
  Attn8Pack a;
  a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v;
  a.q_bs = q_bs; a.q_rs = q_rs; a.k_bs = k_bs; a.k_rs = k_rs; a.v_bs = v_bs; a.v_rs = v_rs;
  a.q8 = (unsigned char*)q8; a.qs = (unsigned char*)qs; a.kv8 = (unsigned char*)kv8;
  a.H = H; a.L = L; a.lq_pad = (L + QBLK - 1) / QBLK * QBLK; a.tiles = (L + KVBLK - 1) / KVBLK; a.k_shift = k_shift; a.v_shift = v_shift;
  const dim3 grid(a.lq_pad / KVBLK, H, B);
#define ATTN8_PACK_LAUNCH(K, V) hipLaunchKernelGGL((attn8_pack_kernel<K, V>), grid, dim3(256), 0, (hipStream_t)stream, a)
  if (v_shift) { if (k_shift) ATTN8_PACK_LAUNCH(true, true); else ATTN8_PACK_LAUNCH(false, true); }
  else if (k_shift) ATTN8_PACK_LAUNCH(true, false);
  else ATTN8_PACK_LAUNCH(false, false);
#undef ATTN8_PACK_LAUNCH
  return flexam_check_launch(who);
}

extern "C" int flexam_attn_fp8_pack(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                                    int64_t v_bs, int64_t v_rs, void* q8, void* qs, void* kv8, int B, int H, int L, int head_dim,
                                    void* stream) {
  return attn8_pack_run("flexam_attn_fp8_pack", q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, q8, qs, kv8, B, H, L, head_dim, nullptr, nullptr, stream);
}

extern "C" int flexam_attn_fp8_pack_shift(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                                          int64_t v_bs, int64_t v_rs, void* q8, void* qs, void* kv8, int B, int H, int L, int head_dim,
                                          const float* k_shift, void* stream) {
  FX_REQUIRE(k_shift && k, FLEXAM_E_ARG, "attn_fp8_pack_shift: null pointer (the shift needs its k)");
  return attn8_pack_run("flexam_attn_fp8_pack_shift", q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, q8, qs, kv8, B, H, L, head_dim, k_shift, nullptr, stream);
}

extern "C" int flexam_attn_fp8_pack_shift_kv(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                                             int64_t v_bs, int64_t v_rs, void* q8, void* qs, void* kv8, int B, int H, int L, int head_dim,
                                             const float* k_shift, const float* v_shift, void* stream) {
  FX_REQUIRE(!k_shift || k, FLEXAM_E_ARG, "attn_fp8_pack_shift_kv: null pointer (the K shift needs its k)");
  return attn8_pack_run("flexam_attn_fp8_pack_shift_kv", q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, q8, qs, kv8, B, H, L, head_dim, k_shift, v_shift,
                        stream);
}

static int rmsnorm_rope_mx_run(const char* who, const void* q, int64_t ldq, const float* wq, const void* k, int64_t ldk, const float* wk, void* q8,
                               void* qs, void* kv8, int64_t M, int C, float eps, const float* rope_cos, const float* rope_sin,
                               int64_t tokens_per_batch, int64_t token_offset, int H, int head_dim, const float* k_shift, void* stream) {
  FX_REQUIRE(q && k && wq && wk && q8 && qs && kv8 && rope_cos && rope_sin, FLEXAM_E_ARG, "rmsnorm_rope_mx: null pointer");
  FX_REQUIRE(head_dim == HD && H == 24 && C == H * HD, FLEXAM_E_SHAPE, "rmsnorm_rope_mx: 24 heads of 128 channels only (C = %d, H = %d)", C, H);
  FX_REQUIRE(M > 0 && tokens_per_batch > 0 && M % tokens_per_batch == 0 && ldq % 8 == 0 && ldk % 8 == 0, FLEXAM_E_SHAPE, "rmsnorm_rope_mx: bad sizes");
  FX_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)q8 | (uintptr_t)qs | (uintptr_t)kv8 | (uintptr_t)k_shift) % 16 == 0, FLEXAM_E_ARG, "rmsnorm_rope_mx: misaligned pointer");
  RmsRopeMx a;
  a.q = (const bf16*)q; a.k = (const bf16*)k; a.ldq = ldq; a.ldk = ldk; a.wq = wq; a.wk = wk; a.cs = rope_cos; a.sn = rope_sin;
  a.q8 = (unsigned char*)q8; a.qs = (unsigned char*)qs; a.kv8 = (unsigned char*)kv8;
  a.tokens_per_batch = tokens_per_batch; a.token_offset = token_offset; a.H = H; a.L = (int)tokens_per_batch;
  a.lq_pad = (a.L + QBLK - 1) / QBLK * QBLK; a.tiles = (a.L + KVBLK - 1) / KVBLK; a.eps = eps; a.k_shift = k_shift;
  // with a shift: the Q half by the plain instance (blockIdx.y = 0 only: its bytes are those of the plain call), the K half by the SHIFT one
  hipLaunchKernelGGL(rmsnorm_rope_mx_kernel<false>, dim3((unsigned)M, k_shift ? 1 : 2), dim3(128), 0, (hipStream_t)stream, a);
  if (k_shift) hipLaunchKernelGGL(rmsnorm_rope_mx_kernel<true>, dim3((unsigned)M, 1), dim3(128), 0, (hipStream_t)stream, a);
  return flexam_check_launch(who);
}

extern "C" int flexam_rmsnorm_rope_mx(const void* q, int64_t ldq, const float* wq, const void* k, int64_t ldk, const float* wk, void* q8,
                                      void* qs, void* kv8, int64_t M, int C, float eps, const float* rope_cos, const float* rope_sin,
                                      int64_t tokens_per_batch, int64_t token_offset, int H, int head_dim, void* stream) {
  return rmsnorm_rope_mx_run("flexam_rmsnorm_rope_mx", q, ldq, wq, k, ldk, wk, q8, qs, kv8, M, C, eps, rope_cos, rope_sin, tokens_per_batch,
                             token_offset, H, head_dim, nullptr, stream);
}

extern "C" int flexam_rmsnorm_rope_mx_shift(const void* q, int64_t ldq, const float* wq, const void* k, int64_t ldk, const float* wk, void* q8,
                                            void* qs, void* kv8, int64_t M, int C, float eps, const float* rope_cos, const float* rope_sin,
                                            int64_t tokens_per_batch, int64_t token_offset, int H, int head_dim, const float* k_shift,
                                            void* stream) {
  FX_REQUIRE(k_shift, FLEXAM_E_ARG, "rmsnorm_rope_mx_shift: null shift");
  return rmsnorm_rope_mx_run("flexam_rmsnorm_rope_mx_shift", q, ldq, wq, k, ldk, wk, q8, qs, kv8, M, C, eps, rope_cos, rope_sin,
                             tokens_per_batch, token_offset, H, head_dim, k_shift, stream);
}

extern "C" int flexam_k_mean(const void* k, int64_t ldk, const float* wk, int64_t M, int C, float eps, const float* rope_cos,
                             const float* rope_sin, int64_t tokens_per_batch, int64_t token_offset, int head_dim, int parts, float* partial,
                             float* mean, void* stream) {
  FX_REQUIRE(k && partial && mean, FLEXAM_E_ARG, "k_mean: null pointer");
  FX_REQUIRE(!wk || (rope_cos && rope_sin && head_dim == HD && C % HD == 0), FLEXAM_E_ARG,
             "k_mean: with a norm weight the RoPE tables are mandatory and heads are 128 channels (head_dim = %d, C = %d)", head_dim, C);
  FX_REQUIRE(M > 0 && tokens_per_batch > 0 && tokens_per_batch < (1 << 30) && M % tokens_per_batch == 0 && M / tokens_per_batch <= 65535 && C > 0 &&
                 C % 8 == 0 && ldk % 8 == 0 && ldk >= C && parts >= 1 && parts <= 65535 && parts <= tokens_per_batch,
             FLEXAM_E_SHAPE, "k_mean: bad sizes (M = %lld, tokens_per_batch = %lld, C = %d, ldk = %lld, parts = %d)", (long long)M,
             (long long)tokens_per_batch, C, (long long)ldk, parts);
  FX_REQUIRE(C <= (wk ? 3072 : 5120), FLEXAM_E_SHAPE, "k_mean: at most %d channels (C = %d)", wk ? 3072 : 5120, C);
  FX_REQUIRE(((uintptr_t)k | (uintptr_t)wk | (uintptr_t)partial | (uintptr_t)mean | (uintptr_t)rope_cos | (uintptr_t)rope_sin) % 16 == 0, FLEXAM_E_ARG,
             "k_mean: misaligned pointer");
  KMean a;
  a.k = (const bf16*)k; a.ldk = ldk; a.token_offset = token_offset; a.wk = wk; a.cs = rope_cos; a.sn = rope_sin; a.partial = partial; a.mean = mean;
  a.C = C; a.L = (int)tokens_per_batch; a.parts = parts; a.tpp = (a.L + parts - 1) / parts; a.eps = eps; a.inv_l = 1.0f / (float)a.L;
  const int B = (int)(M / tokens_per_batch), vpt = (C / 8 + 63) / 64;
  const dim3 grid(parts, B);
#define K_MEAN_LAUNCH(V, N) hipLaunchKernelGGL((k_mean_part_kernel<V, N>), grid, dim3(64), 0, (hipStream_t)stream, a)
  if (wk) {
    if (vpt <= 1) K_MEAN_LAUNCH(1, true); else if (vpt <= 2) K_MEAN_LAUNCH(2, true); else if (vpt <= 4) K_MEAN_LAUNCH(4, true); else K_MEAN_LAUNCH(6, true);
  } else {
    if (vpt <= 1) K_MEAN_LAUNCH(1, false); else if (vpt <= 2) K_MEAN_LAUNCH(2, false); else if (vpt <= 4) K_MEAN_LAUNCH(4, false);
    else if (vpt <= 6) K_MEAN_LAUNCH(6, false); else K_MEAN_LAUNCH(10, false);
  }
#undef K_MEAN_LAUNCH
  hipLaunchKernelGGL(k_mean_finish_kernel, dim3((B * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, B);
  return flexam_check_launch("flexam_k_mean");
}

extern "C" int flexam_attn_fwd_fp8(const void* q8, const void* qs, const void* kv8, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int L,
                                   int head_dim, int kv_splits, int split_from_unit, float* ws_o, float* ws_ml, void* stream) {
  FX_REQUIRE(q8 && qs && kv8, FLEXAM_E_ARG, "attn_fwd_fp8: null pointer");
  FX_REQUIRE(((uintptr_t)q8 | (uintptr_t)qs | (uintptr_t)kv8) % 16 == 0, FLEXAM_E_ARG, "attn_fwd_fp8: misaligned pointer");
  AttnCall c;
  c.q8 = q8; c.qs = qs; c.kv8 = kv8; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = L; c.Lk = L; c.head_dim = head_dim; c.softmax_scale = FLEXAM_ATTN_PRESCALED; c.stream = stream;
  c.kv_splits = kv_splits; c.split_from_unit = split_from_unit; c.ws_o = ws_o; c.ws_ml = ws_ml;
  return attn_run(c);
}

extern "C" int flexam_attn_fwd_fp8_oshift(const void* q8, const void* qs, const void* kv8, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int L,
                                          int head_dim, int kv_splits, int split_from_unit, float* ws_o, float* ws_ml, const float* o_shift,
                                          void* stream) {
  FX_REQUIRE(q8 && qs && kv8 && o_shift, FLEXAM_E_ARG, "attn_fwd_fp8_oshift: null pointer");
  FX_REQUIRE(((uintptr_t)q8 | (uintptr_t)qs | (uintptr_t)kv8) % 16 == 0, FLEXAM_E_ARG, "attn_fwd_fp8_oshift: misaligned pointer");
  AttnCall c;
  c.q8 = q8; c.qs = qs; c.kv8 = kv8; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = L; c.Lk = L; c.head_dim = head_dim; c.softmax_scale = FLEXAM_ATTN_PRESCALED; c.stream = stream;
  c.kv_splits = kv_splits; c.split_from_unit = split_from_unit; c.ws_o = ws_o; c.ws_ml = ws_ml; c.o_shift = o_shift;
  return attn_run(c);
}

extern "C" int flexam_attn_fwd_fp8_chunked(const void* q8, const void* qs, const void* kv8, void* o, int64_t o_bs, int64_t o_rs, int B, int H,
                                           int Lq, int Lk, int chunk_tiles, int head_dim, int kv_splits, int split_from_unit, float* ws_o,
                                           float* ws_ml, void* stream) {
  FX_REQUIRE(q8 && qs && kv8, FLEXAM_E_ARG, "attn_fwd_fp8_chunked: null pointer");
  FX_REQUIRE(((uintptr_t)q8 | (uintptr_t)qs | (uintptr_t)kv8) % 16 == 0, FLEXAM_E_ARG, "attn_fwd_fp8_chunked: misaligned pointer");
  FX_REQUIRE(chunk_tiles > 0, FLEXAM_E_SHAPE, "attn_fwd_fp8_chunked: chunk_tiles = %d", chunk_tiles);
  AttnCall c;
  c.q8 = q8; c.qs = qs; c.kv8 = kv8; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = Lq; c.Lk = Lk; c.head_dim = head_dim; c.softmax_scale = FLEXAM_ATTN_PRESCALED; c.stream = stream;
  c.kv_splits = kv_splits; c.split_from_unit = split_from_unit; c.ws_o = ws_o; c.ws_ml = ws_ml; c.kv8_chunk_tiles = chunk_tiles;
  return attn_run(c);
}

extern "C" int flexam_attn_fwd_fp8_window(const void* q8, const void* qs, const void* kv8, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int L,
                                          int head_dim, int window_left, int window_right, int sink, int frame_tokens, const float* o_shift,
                                          void* stream) {
  FX_REQUIRE(q8 && qs && kv8, FLEXAM_E_ARG, "attn_fwd_fp8_window: null pointer");
  FX_REQUIRE(((uintptr_t)q8 | (uintptr_t)qs | (uintptr_t)kv8) % 16 == 0, FLEXAM_E_ARG, "attn_fwd_fp8_window: misaligned pointer");
  FX_REQUIRE(frame_tokens >= 0, FLEXAM_E_ARG, "attn_fwd_fp8_window: frame_tokens %d (0 = a token window)", frame_tokens);
  AttnCall c;
  c.q8 = q8; c.qs = qs; c.kv8 = kv8; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = L; c.Lk = L; c.head_dim = head_dim; c.softmax_scale = FLEXAM_ATTN_PRESCALED; c.stream = stream; c.o_shift = o_shift;
  c.win_left = window_left; c.win_right = window_right; c.win_sink = sink; c.win_by_frames = frame_tokens > 0; c.win_frame = frame_tokens;
  return attn_run(c);
}

extern "C" int flexam_attn_fwd_fp8_window_at(const void* q8, const void* qs, const void* kv8, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int Lq,
                                             int Lk, int chunk_tiles, int head_dim, int window_left, int window_right, int sink, int frame_tokens,
                                             int q_offset, const float* o_shift, void* stream) {
  FX_REQUIRE(q8 && qs && kv8, FLEXAM_E_ARG, "attn_fwd_fp8_window_at: null pointer");
  FX_REQUIRE(((uintptr_t)q8 | (uintptr_t)qs | (uintptr_t)kv8) % 16 == 0, FLEXAM_E_ARG, "attn_fwd_fp8_window_at: misaligned pointer");
  FX_REQUIRE(chunk_tiles > 0, FLEXAM_E_ARG, "attn_fwd_fp8_window_at: chunk_tiles = %d", chunk_tiles);
  AttnCall c;
  c.q8 = q8; c.qs = qs; c.kv8 = kv8; c.o = o; c.o_bs = o_bs; c.o_rs = o_rs;
  c.B = B; c.H = H; c.Lq = Lq; c.Lk = Lk; c.head_dim = head_dim; c.softmax_scale = FLEXAM_ATTN_PRESCALED; c.stream = stream; c.o_shift = o_shift;
  // one chunk that holds exactly the call's tiles is the record layout of the plain call: with q_offset = 0 and Lq == Lk, flexam_attn_fwd_fp8_window
  c.kv8_chunk_tiles = q_offset == 0 && Lq == Lk && Lk > 0 && chunk_tiles == (Lk + KVBLK - 1) / KVBLK ? 0 : chunk_tiles;
  return attn_window_at(c, window_left, window_right, frame_tokens, sink, q_offset);
}

extern "C" int flexam_attn_merge(void* o, int64_t o_bs, int64_t o_rs, int B, int H, int Lq, int head_dim, float softmax_scale,
                                 int n_slots, const float* ws_o, const float* ws_ml, void* stream) {
  FX_REQUIRE(o && ws_o && ws_ml, FLEXAM_E_ARG, "attn_merge: null pointer");
  FX_REQUIRE(head_dim == HD && B > 0 && H > 0 && Lq > 0 && n_slots >= 1, FLEXAM_E_SHAPE, "attn_merge: bad sizes");
  FX_REQUIRE(o_rs % 4 == 0 && o_bs % 4 == 0 && (uintptr_t)o % 8 == 0, FLEXAM_E_SHAPE, "attn_merge: output rows must keep 8-byte alignment");
  AttnParams p{};
  p.o = (bf16*)o; p.o_bs = o_bs; p.o_rs = o_rs; p.B = B; p.H = H; p.Lq = Lq;
  scale_and_blocks(p, softmax_scale);
  p.unit0 = 0; p.n_units = B * H * p.q_blocks; p.n_slots = n_slots; p.ws_o = const_cast<float*>(ws_o); p.ws_ml = const_cast<float*>(ws_ml);
  launch_merge(p, stream);
  return flexam_check_launch("flexam_attn_merge");
}

namespace {
AttnInstance attn_frames_instance(bool prescaled) {      // (declared next to attn_instance: why it stands here)
  constexpr int BF = NSLOT * 2 * KV_TILE_BYTES;
  if (prescaled) return {attn_window_frames_kernel<true>, BF, 11};
  return {attn_window_frames_kernel<false>, BF, 10};
}
Attn8WindowInstance attn8_window_instance(bool oshift) {      // (the windowed MXFP8 kernels, see attn_fp8.inc: why it stands here)
  if (oshift) return {attn8_window_oshift_kernel<0>, 1};
  return {attn8_window_kernel<0>, 0};
}
// The windowed kernel at a query offset (flexam_attn_fwd_window_at; AT in attn_fwd_body).  Two instances, not four: the frame form
// serves a token window as frames of one token, so the bounds are derived one way and nothing branches on the form.  Defined here, behind
// every other kernel of the file: the instances above are emitted as they were.
template <bool PRE>
__global__ __launch_bounds__(NT, 2) void attn_window_at_kernel(AttnParams p) { attn_fwd_body<0, PRE, false, false, true, true, true>(p); }
AttnInstance attn_at_instance(bool prescaled) {
  constexpr int BF = NSLOT * 2 * KV_TILE_BYTES;
  if (prescaled) return {attn_window_at_kernel<true>, BF, 13};
  return {attn_window_at_kernel<false>, BF, 12};
}
// ... and the same kernel on a compact key buffer (flexam_attn_fwd_window_halo; HALO in attn_fwd_body), behind those
template <bool PRE>
__global__ __launch_bounds__(NT, 2) void attn_window_halo_kernel(AttnParams p) { attn_fwd_body<0, PRE, false, false, true, true, true, true>(p); }
AttnInstance attn_halo_instance(bool prescaled) {
  constexpr int BF = NSLOT * 2 * KV_TILE_BYTES;
  if (prescaled) return {attn_window_halo_kernel<true>, BF, 15};
  return {attn_window_halo_kernel<false>, BF, 14};
}
// ... and, last, the windowed MXFP8 kernels at a query offset (flexam_attn_fwd_fp8_window_at; AT in attn8_fwd_body)
Attn8WindowAtInstance attn8_window_at_instance(bool oshift) {
  if (oshift) return {attn8_window_at_oshift_kernel<0>, 3};
  return {attn8_window_at_kernel<0>, 2};
}
}  // namespace
