/* include/flexam_hip.h -- C ABI of libflexam_hip.so: the MI355X (gfx950) kernels behind the
 * FlexAM denoising hot path (Wan2.2-Fun-5B-FLEXAM DiT forward, sampler step, Wan2.2 3D-VAE
 * decode).  This is the drop-in boundary: plain pointers and sizes, no torch types.
 *
 * Conventions
 *   - every function returns 0 (FLEXAM_OK) or a negative FLEXAM_E_* code; flexam_last_error()
 *     returns the message of the last failure on the calling thread;
 *   - all pointers are DEVICE pointers unless a comment says host; the caller (PyTorch-ROCm in
 *     flexam_amd/hip.py) owns every buffer, the library never allocates, frees or retains one:
 *     scratch (GEMM split-K slabs, split-KV attention partials) is an argument of the call that uses it;
 *   - `stream` is a hipStream_t; calls are asynchronous and ordered on it, no hidden syncs,
 *     safe to capture into a hipGraph; calls on different streams / devices are independent as long
 *     as they are given different scratch buffers (the only process-global state is a per-device
 *     "kernel attribute set" flag table and the per-device CU count);
 *   - bf16 = IEEE bfloat16 (torch.bfloat16); "f32 table row" arguments are row pointers of
 *     small fp32 tables selected per token through an int32 row index ("two-row
 *     modulation").
 * Each entry point cites the reference code it replaces (paths relative to the FlexAM repo).
 */
#ifndef FLEXAM_HIP_H
#define FLEXAM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLEXAM_HIP_VERSION 2
#define FLEXAM_OK 0
#define FLEXAM_E_ARG (-1)
#define FLEXAM_E_SHAPE (-2)
#define FLEXAM_E_ARCH (-3)
#define FLEXAM_E_LAUNCH (-4)

#define FLEXAM_EPI_NONE 0
#define FLEXAM_EPI_GELU_TANH 1

int flexam_version(void);
const char* flexam_arch(void);          /* "gfx950" */
const char* flexam_last_error(void);
int flexam_device_check(void);        /* FLEXAM_E_ARCH unless the current device is gfx950 */

/* Compute units of the current device that the library plans its grids for (the device's CU count rounded down to a multiple
 * of 8: one persistent workgroup per CU, blockIdx & 7 = XCD; 256 on MI355X).  Callers that plan work units themselves -- the
 * key split of flexam_attn_fwd_splitkv -- use the same figure. */
int flexam_device_cus(void);
/* Plan the persistent grids of the current device for `cus` compute units (a multiple of 8: blockIdx & 7 stays the XCD; 0 = all of them,
 * the default) -- flexam_device_cus() answers with the budget from then on.  For callers that run collectives BESIDE these kernels: a
 * one-workgroup-per-CU kernel on every CU leaves a collective's own kernels nowhere to run until it ends (flexam_amd/dit_engine.py sets 8
 * CUs aside under the overlapped sequence-parallel exchanges).  Process-global per device, not stream-ordered: set it between launches. */
int flexam_set_cu_budget(int cus);

/* C[M,N] = epi(A[M,K] . W[N,K]^T + bias[N]); A, W bf16 row-major with K contiguous (nn.Linear
 * weight layout), fp32 accumulate on MFMA; C bf16 (out_f32 = 0) or fp32 (out_f32 = 1).
 * K % 64 == 0, N % 4 == 0, lda/ldw % 8 == 0 (pad on the host).  a_koff (optional, [K/64] int64,
 * device): element offset added to every A row base for K block kb instead of kb*64 -- the
 * implicit-GEMM form of the VAE's causal convolutions (one entry per (tap, 64-channel slice)).
 * ws / ws_bytes (optional): scratch for the tail split-K -- the tiles of the last, partial round of the CUs are cut along K so
 * that all CUs work; the slices' partial sums are parked in `ws` and a second launch on the same stream adds them up in slice
 * order (deterministic) and runs the epilogue.  Device memory, 16-byte aligned, slabs of 256 KiB, no initialisation needed;
 * FLEXAM_GEMM_WS_BYTES covers every shape.  NULL / too small: the GEMM never splits.  The buffer is used only by this call
 * (stream-ordered): calls that may run concurrently (other streams, other devices) need their own.  (The Python binding keeps
 * one 64 MiB buffer per (device, stream) in an LRU of 8 slots, flexam_amd/hip.py:_gemm_workspace: that is the per-stream cost of
 * using the library from several streams.)
 * Replaces nn.Linear -> cuBLAS (+ its workspace): FlexAM/models/wan_transformer3d_FlexAM.py:242-244,261,363-365,
 * 370,415-416,487,626-636 and Conv3d/Conv2d -> cuDNN: FlexAM/models/wan_vae3_8.py:39-47,94,99. */
#define FLEXAM_GEMM_WS_BYTES (256 * 262144)
int flexam_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* C, int64_t ldc,
                     int64_t M, int64_t N, int64_t K, int epilogue, int out_f32, const int64_t* a_koff, void* ws,
                     int64_t ws_bytes, void* stream);

/* X[m,n] += bf16(A.W^T + bias)[m,n] * gate[row(m), n]   (fp32 residual stream updated in place)
 * row(m) = gate_row[m] if gate_row else m / rows_per_batch; gate == NULL means gate = 1.
 * Replaces Linear + `x = x + y * e[2]` / `x + cross_attn(...)` / `x + y * e[5]`:
 * FlexAM/models/wan_transformer3d_FlexAM.py:261+456, 370+461, 416+468; with a_koff (see flexam_gemm_bf16)
 * also the second conv + skip of the VAE ResidualBlock, FlexAM/models/wan_vae3_8.py:213,240. */
int flexam_gemm_bf16_gate_residual(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, float* X,
                                   int64_t ldx, const float* gate, int64_t gate_ld, const int32_t* gate_row,
                                   int64_t rows_per_batch, int64_t M, int64_t N, int64_t K, const int64_t* a_koff,
                                   void* ws, int64_t ws_bytes, void* stream);

/* The two GEMMs above with W held as OCP e4m3 bytes (float8_e4m3fn; ldw in BYTES, % 16 == 0; 16-byte aligned pointers): the
 * weight-only fp8 storage of the reference's qfloat8 GPU_memory_modes (FlexAM/utils/fp8_optimization.py:20-57,
 * comfyui/wan2_2_fun_flexam/nodes.py:327-343), read as e4m3 from HBM and LDS and widened to bf16 in registers -- exact, so the
 * result is bit-identical to flexam_gemm_bf16 / _gate_residual on W upcast to bf16 (same tile plan, same FLEXAM_GEMM_* switches,
 * same MFMA order).  Output widths that take the bf16 GEMM's 160-wide tile (N <= 160; N = 320, 480) are refused. */
int flexam_gemm_w8(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* C, int64_t ldc,
                   int64_t M, int64_t N, int64_t K, int epilogue, int out_f32, const int64_t* a_koff, void* ws,
                   int64_t ws_bytes, void* stream);
int flexam_gemm_w8_gate_residual(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, float* X,
                                 int64_t ldx, const float* gate, int64_t gate_ld, const int32_t* gate_row,
                                 int64_t rows_per_batch, int64_t M, int64_t N, int64_t K, const int64_t* a_koff,
                                 void* ws, int64_t ws_bytes, void* stream);

/* fp8 variant of the two GEMMs above for the DiT's QKV / FFN projections (BASELINE.json configs[4]; selected explicitly, never
 * the default).  A8 [M,K], W8 [N,K]: OCP e4m3 bytes, K contiguous, K % 128 == 0, lda / ldw % 16 == 0; a_scale [M], w_scale [N]
 * fp32 row scales (value = byte * scale); fp32 accumulation on the block-scaled MFMA with unit block scales:
 *   C = epi((A8 . W8^T) * a_scale[m] * w_scale[n] + bias[n])   (bf16 out; epilogue NONE | GELU_TANH)
 *   X[m,n] += bf16(...)[m,n] * gate[row(m), n]                  (gate-residual form, as flexam_gemm_bf16_gate_residual)
 * flexam_quantize_rows_fp8: q[m,:] = e4m3(x[m,:] / scale[m]), scale[m] = absmax(x[m,:]) / 448 (bf16 in); used for activations per
 * call and for weights once.  The reference only STORES weights as float8_e4m3fn and upcasts them per call
 * (FlexAM/utils/fp8_optimization.py:1-57); fp8 arithmetic is this build's addition. */
int flexam_quantize_rows_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int64_t M, int K, void* stream);
int flexam_gemm_fp8(const void* A, int64_t lda, const float* a_scale, const void* W, int64_t ldw, const float* w_scale,
                    const float* bias, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue, void* stream);
int flexam_gemm_fp8_gate_residual(const void* A, int64_t lda, const float* a_scale, const void* W, int64_t ldw, const float* w_scale,
                                  const float* bias, float* X, int64_t ldx, const float* gate, int64_t gate_ld,
                                  const int32_t* gate_row, int64_t rows_per_batch, int64_t M, int64_t N, int64_t K, void* stream);
/* The fp8 FFN without a quantise pass between its two GEMMs: Q[m,n] = e4m3(gelu_tanh((A8 . W8^T) * a_scale[m] * w_scale[n] + bias[n])
 * / out_scale[m]) -- the A operand of the next flexam_gemm_fp8* call with a_scale = out_scale.  out_scale [M] comes from
 * flexam_ln_modulate_fp8 (next_scale: a bound on the row's outputs, so nothing saturates).  Q: e4m3 bytes, ldq % 16 == 0. */
int flexam_gemm_fp8_gelu_q(const void* A, int64_t lda, const float* a_scale, const void* W, int64_t ldw, const float* w_scale,
                           const float* bias, const float* out_scale, void* Q, int64_t ldq, int64_t M, int64_t N, int64_t K,
                           void* stream);

/* Flash attention forward, head_dim 128, non-causal, keys [0, Lk): o = softmax(q k^T * scale) v.
 * q/k/v/o are [B, L, H, 128] views given by batch stride `*_bs` and row stride `*_rs` (elements);
 * head h starts at column h*128 of a row.  bf16 in/out, fp32 softmax/accumulate.
 * Replaces attention() -> flash_attn / sageattn / SDPA: FlexAM/models/attention_utils.py:43-233
 * (call sites wan_transformer3d_FlexAM.py:251-256 self, :367 cross).
 * softmax_scale > 0: the scale of the formula.  softmax_scale = FLEXAM_ATTN_PRESCALED: the producer of q already multiplied it
 * by scale * log2(e) before its one rounding to bf16 (the DiT engine folds that factor into the RMSNorm weight of q), so the
 * scores are in exp2 units and the kernel saves one FMA per score: o = softmax2(q k^T) v with softmax2 built on 2^x. */
#define FLEXAM_ATTN_PRESCALED (-1.0f)
/* The kernels' geometry, for whoever sizes their buffers: a work unit is FLEXAM_ATTN_Q_BLOCK query rows of one (batch, head), keys
 * are taken in tiles of FLEXAM_ATTN_KV_TILE, and one MXFP8 key / value record (below) holds one such tile of one head. */
#define FLEXAM_ATTN_Q_BLOCK 256
#define FLEXAM_ATTN_KV_TILE 64
#define FLEXAM_ATTN_HEAD_DIM 128
#define FLEXAM_ATTN8_REC_BYTES 18432
int flexam_attn_fwd(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                    int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int Lq, int Lk,
                    int head_dim, float softmax_scale, void* stream);
/* flexam_attn_fwd with the LAST key counted `last_key_multiplicity` (>= 1) times: softmax over {k_0 .. k_{Lk-2}, N copies of
 * k_{Lk-1}} -- exactly what attention over a context whose trailing rows are identical computes, at the cost of one copy
 * (the copy's score gets + log2 N before the exponential).  The reference pads every prompt to text_len = 512 rows with
 * zeros BEFORE the text-embedding MLP and attends to all of them (wan_transformer3d_FlexAM.py:958-964, context_lens = None at
 * :367): the 386+ padded rows of a 126-token prompt are one and the same K/V row. */
int flexam_attn_fwd_lastkey(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                            int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int Lq, int Lk,
                            int head_dim, float softmax_scale, float last_key_multiplicity, void* stream);
/* flexam_attn_fwd over ONE length L (Lq = Lk) under flash-attn's sliding-window mask, which the reference hands to its kernel
 * (attention_utils.py:43-171: flash_attn_varlen_func(..., causal=, window_size=)): query i sees key j iff
 * (window_left < 0 or j >= i - window_left) and (window_right < 0 or j <= i + window_right); a negative side is unbounded, causal is
 * window_right = 0, and (-1, -1) -- or a window no shorter than the sequence on both sides -- is flexam_attn_fwd itself.  Every row sees
 * at least itself.  A work unit visits only the key tiles that hold a key one of its 256 rows sees, and masks only those of them that
 * hold a key one of its rows does not see; whole units only (no split-KV).  softmax_scale as flexam_attn_fwd takes it,
 * FLEXAM_ATTN_PRESCALED included. */
int flexam_attn_fwd_window(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                           int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int L, int head_dim,
                           float softmax_scale, int window_left, int window_right, void* stream);
/* flexam_attn_fwd_window with the first `sink` keys visible to every query (the "attention sink" of StreamingLLM; here the
 * reference-image tokens that lead the frame-major sequence): query i sees key j iff
 *   j < sink  or  ((window_left < 0 or j >= i - window_left) and (window_right < 0 or j <= i + window_right)).
 * The sink is visible to every row whatever window_right says: the model is not causal.  A work unit visits the sink tiles
 * [0, (sink - 1) / 64] and its window tiles, as one run where they touch and as two runs otherwise; a tile wholly below the sink is
 * not masked.  Normalisations, each the very launch named: sink = 0, or window_left < 0 (nothing lies to the left of the window), is
 * flexam_attn_fwd_window(window_left, window_right); sink >= L, or a window that is no bound on either side, is flexam_attn_fwd itself.
 * sink < 0 is FLEXAM_E_ARG. */
int flexam_attn_fwd_window_sink(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                                int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int L, int head_dim,
                                float softmax_scale, int window_left, int window_right, int sink, void* stream);
/* flexam_attn_fwd_window_sink with the window counted in frames of `frame_tokens` = T tokens instead of tokens (the masks video
 * transformers are trained with: the sequence is frame-major, the reference image's tokens are frame 0 and the latent frames follow,
 * the grid [F + 1, h, w] RoPE uses, T = h * w).  Frames are counted from token 0, frame(t) = t / T; query i sees key j iff
 *   j < sink  or  ((frames_left < 0 or j / T >= i / T - frames_left) and (frames_right < 0 or j / T <= i / T + frames_right)),
 * i.e. the keys [(i / T - frames_left) T, (i / T + frames_right + 1) T - 1] clipped to [0, L): whole frames, its own among them, so no
 * row is empty.  (-1, 0) is frame-block-causal, (0, 0) per-frame attention.  L need not be a multiple of T (a ragged last frame).  A
 * work unit visits the tiles that hold a key one of its rows sees, and the sink tiles, as flexam_attn_fwd_window_sink does; where T is
 * a multiple of 64 every frame boundary is a tile boundary and no window tile is masked.  Normalisations, each the very launch named:
 * both sides negative (or reaching the first and the last frame from every row), frame_tokens >= L, or sink >= L, is flexam_attn_fwd
 * itself; frames_left < 0 drops the sink (nothing lies to the left of such a window).  frame_tokens <= 0 and sink < 0 are FLEXAM_E_ARG. */
int flexam_attn_fwd_window_frames(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                                  int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int L, int head_dim,
                                  float softmax_scale, int frames_left, int frames_right, int frame_tokens, int sink, void* stream);
/* The three masks above for a call whose Lq queries are the global tokens q_offset .. q_offset + Lq - 1 of a sequence whose first Lk
 * tokens are the keys: what a rank runs under sequence parallelism (its chunk of queries against the gathered keys, q_offset = the
 * chunk's first token; or every padded row of its heads at q_offset = 0 with Lq >= Lk).  Row i is global token g = q_offset + i and sees
 * key j (0 <= j < Lk) iff j < sink or lo(g) <= j <= hi(g): frame_tokens = 0, a token window, lo = g - window_left and hi = g +
 * window_right; frame_tokens = T > 0, the two words count frames, lo = (g / T - window_left) T and hi = (g / T + window_right + 1) T - 1.
 * A negative side is unbounded.  q_offset + Lq may exceed Lk: those rows are the zero pad rows of a sequence that does not divide over
 * the ranks; they are never keys, as queries they follow the same rule, and a row that sees no key is written as zeros.  A work unit
 * visits the sink tiles and the tiles that hold a key one of its 256 rows sees, as one run or two, interior tiles unmasked, as the
 * sibling kernels do; a unit none of whose rows sees a key reads no key tile and writes zeros.  Whole units only (no split-KV).  The
 * kernels are instances of their own (attn_window_at_kernel).  Normalisations, each the very launch named: q_offset = 0 and Lq = Lk is
 * flexam_attn_fwd_window, _window_sink or _window_frames; a window that clips no row of this call on either side, or sink >= Lk, is
 * flexam_attn_fwd on (Lq, Lk); window_left < 0 drops the sink.  q_offset < 0, sink < 0 and frame_tokens < 0 are FLEXAM_E_ARG. */
int flexam_attn_fwd_window_at(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                              int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int Lq, int Lk, int head_dim,
                              float softmax_scale, int window_left, int window_right, int frame_tokens, int sink, int q_offset,
                              void* stream);
/* flexam_attn_fwd_window_at on a COMPACT key buffer: what a rank runs when it has fetched only the halo of keys its window reaches.  Lk
 * stays the global key count and every mask and bound is the one above; k and v point at k_rows rows that hold, with s_n =
 * ceil(min(sink, Lk) / 64) (0 under window_left < 0, which drops the sink): the key rows of the sink tiles [0, s_n) at buffer rows
 * 0 .. 64 s_n - 1, and behind them the key rows from global tile s_n + key_gap_tiles on -- global key j >= 64 s_n lies at buffer row
 * j - 64 key_gap_tiles.  A last tile is cut at Lk as ever: no row past key Lk - 1 is read.  Before the launch the call walks its
 * ceil(Lq / 256) query blocks on the host, by the kernel's own arithmetic; a block that visits a tile of the gap left out, or a tile whose
 * key rows end behind buffer row k_rows - 1, makes the call FLEXAM_E_ARG and nothing is launched: a wrong plan is never an out-of-range
 * read.  (The rows of a visited tile that no query sees are multiplied by a probability of exactly 0: they must be written, by anyone.)
 * key_gap_tiles = 0 with k_rows = Lk is flexam_attn_fwd_window_at, launch for launch.  Otherwise the kernels are instances of their own
 * (attn_window_halo_kernel), q_offset = 0 with Lq = Lk included; a call that no side clips, or sink >= Lk, reads every key and is
 * FLEXAM_E_ARG on a compact buffer, as are key_gap_tiles < 0 and k_rows outside 0 .. Lk. */
int flexam_attn_fwd_window_halo(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                                int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int Lq, int Lk, int head_dim,
                                float softmax_scale, int window_left, int window_right, int frame_tokens, int sink, int q_offset,
                                int key_gap_tiles, int k_rows, void* stream);
/* flexam_attn_fwd with the work units u =(batch*H + head)*ceil(Lq/256) + q_block at and after `split_from_unit` cut into kv_splits key
 * ranges each (flash-decoding style partial softmaxes + a merge launch), the units before it in one pass: with
 * split_from_unit = floor(units/256)*256 only the last, partial round of the 256 CUs is split; 0 splits everything (ranks of a
 * sequence-parallel run hold few query rows).  ws_o: fp32 [kv_splits, n, 256, 128], ws_ml: fp32 [kv_splits, n, 256, 2] scratch
 * with n = units - split_from_unit.  kv_splits = 1 == flexam_attn_fwd.  Whole and split units go out as ONE kernel launch (each XCD
 * gets an eighth of both kinds, its whole units first: the short workgroups start as its CUs finish their last whole unit),
 * followed by the merge launch. */
int flexam_attn_fwd_splitkv(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                            int64_t v_bs, int64_t v_rs, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int Lq, int Lk,
                            int head_dim, float softmax_scale, int kv_splits, int split_from_unit, float* ws_o, float* ws_ml,
                            void* stream);

/* Attention over a PART of the keys, finished later: flexam_attn_fwd_partial leaves, for every query row, the un-normalised
 * output and (reference, row sum) of the softmax over the keys it was given -- cut into kv_splits ranges, workspace slots slot0 ..
 * slot0 + kv_splits - 1 (kv_splits must equal ceil(tiles / ceil(tiles / kv_splits)), tiles = ceil(Lk / 64)); any number of such
 * calls on disjoint key sets may fill the slots, in any order; flexam_attn_merge combines n_slots of them into o.  Lets a
 * sequence-parallel rank attend to its LOCAL K/V chunk while the all-gather of the other ranks' chunks is still in flight
 * (the exchange the reference delegates to the missing FlexAM/dist, wan_transformer3d_FlexAM.py:801-815).
 * ws_o: fp32 [n_slots, units, 256, 128], ws_ml: fp32 [n_slots, units, 256, 2], units = B * H * ceil(Lq / 256). */
int flexam_attn_fwd_partial(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                            int64_t v_bs, int64_t v_rs, int B, int H, int Lq, int Lk, int head_dim, float softmax_scale,
                            int kv_splits, int slot0, float* ws_o, float* ws_ml, void* stream);
int flexam_attn_merge(void* o, int64_t o_bs, int64_t o_rs, int B, int H, int Lq, int head_dim, float softmax_scale, int n_slots,
                      const float* ws_o, const float* ws_ml, void* stream);

/* Self-attention with MXFP8 operands (OCP e4m3 + one E8M0 scale per 32 elements; both products on
 * v_mfma_scale_f32_32x32x64_f8f6f4 at twice the bf16 MFMA rate, fp32 softmax and accumulation) -- the quantised variant behind
 * VIDEOX_ATTENTION_TYPE=SAGE_ATTENTION, FlexAM/models/attention_utils.py:195-203 (the reference calls the third-party
 * `sageattn`, which quantises Q, K and the P.V product; kept here: its contract, softmax attention within a stated tolerance).
 * flexam_attn_fp8_pack: q, k, v bf16 [B, L, H, 128] as flexam_attn_fwd takes them (q carrying softmax_scale * log2 e, i.e. the
 * FLEXAM_ATTN_PRESCALED form) -> q8 [B][H][Lp][128] e4m3, qs [B][H][Lp] four E8M0 bytes per row, kv8 [B][H][T] records of
 * FLEXAM_ATTN8_REC_BYTES bytes (K tile image, V^T tile image with the key order the P.V operand needs, their scales), Lp = ceil(L / 256) * 256,
 * T = ceil(L / 64); rows past L are written as zeros; q = k = NULL: only the V half of the records is written.  flexam_attn_fwd_fp8: o [B, L, H, 128] bf16 from those buffers; kv_splits /
 * split_from_unit / ws_o / ws_ml as flexam_attn_fwd_splitkv (kv_splits = 1: no workspace). */
int flexam_attn_fp8_pack(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                         int64_t v_bs, int64_t v_rs, void* q8, void* qs, void* kv8, int B, int H, int L, int head_dim, void* stream);
/* The producer of those operands inside the DiT: RMSNorm over the full width + RoPE of q and k (flexam_rmsnorm_rope's arithmetic,
 * q's weight carrying softmax_scale * log2 e) written as q8 / qs and the K image + K scales of the kv8 records directly, quantised
 * from fp32; 24 heads of 128 channels; M = B * tokens_per_batch rows.  The buffers' padding rows (past L) must have been zeroed once
 * (they are never written here); the V half of the records then comes from flexam_attn_fp8_pack with q = k = NULL. */
int flexam_rmsnorm_rope_mx(const void* q, int64_t ldq, const float* wq, const void* k, int64_t ldk, const float* wk, void* q8, void* qs,
                           void* kv8, int64_t M, int C, float eps, const float* rope_cos, const float* rope_sin,
                           int64_t tokens_per_batch, int64_t token_offset, int H, int head_dim, void* stream);
/* Smooth-K, SageAttention's preprocessing of K: the producers above with k_shift[b][c] (fp32 [B][H * 128], taken as given) subtracted
 * from K before it is quantised.  softmax(q.(k_j - c)) = softmax(q.k_j - q.c) = softmax(q.k_j) for ANY vector c, q.c being one number
 * per query row: the attention's result is that of the unshifted K, while e4m3 -- whose error is relative to the element -- no longer
 * pays for a channel offset all keys share in every score.  With k_shift = the token mean (flexam_k_mean) the operands are those of
 * K - mean_tokens(K); flexam_attn_fwd_fp8 is unchanged and cannot tell.
 * flexam_attn_fp8_pack_shift: K rows below L are quantised from float(k) - k_shift[b][h * 128 + c], one fp32 subtraction; rows past L
 * stay zero rows (codes 0, scale byte 1), not -shift; Q and V as flexam_attn_fp8_pack writes them (q and k must be given).
 * flexam_rmsnorm_rope_mx_shift: the K half writes the operands of y - k_shift[b][c], subtracted in fp32 after the rotation and before
 * the block amax (one more rounding than flexam_rmsnorm_rope_mx); the Q half is flexam_rmsnorm_rope_mx's, byte for byte (its own launch). */
int flexam_attn_fp8_pack_shift(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                               int64_t v_bs, int64_t v_rs, void* q8, void* qs, void* kv8, int B, int H, int L, int head_dim,
                               const float* k_shift, void* stream);
int flexam_rmsnorm_rope_mx_shift(const void* q, int64_t ldq, const float* wq, const void* k, int64_t ldk, const float* wk, void* q8,
                                 void* qs, void* kv8, int64_t M, int C, float eps, const float* rope_cos, const float* rope_sin,
                                 int64_t tokens_per_batch, int64_t token_offset, int H, int head_dim, const float* k_shift, void* stream);
/* mean[b][c] (fp32 [B][C]) = the mean over the tokens_per_batch tokens of batch b of K as the attention will see it; k: M = B *
 * tokens_per_batch bf16 rows of C channels, row pitch ldk.  wk != NULL: RMSNorm over the full row + RoPE are applied first --
 * flexam_rmsnorm_rope's arithmetic in fp32, unrounded, with this eps, these tables and token(m) = token_offset + m % tokens_per_batch
 * (head_dim 128, C <= 3072): the K flexam_rmsnorm_rope_mx quantises and never writes.  wk == NULL: k is taken as given, already
 * normed and rotated (C <= 5120; rope_cos / rope_sin / eps unused).
 * Deterministic and independent of the device: no atomics, no CU count.  Part p < parts of batch b adds the rows of tokens
 * p * T .. min((p + 1) * T, L) - 1, T = ceil(L / parts), in token order in fp32 into partial[b][p][:] (caller's scratch, fp32
 * [B][parts][C]; 1 <= parts <= tokens_per_batch; a part past the end holds zeros); a second launch adds the parts in index order and
 * multiplies by the fp32 1 / L.  Equal arguments give equal bits. */
int flexam_k_mean(const void* k, int64_t ldk, const float* wk, int64_t M, int C, float eps, const float* rope_cos, const float* rope_sin,
                  int64_t tokens_per_batch, int64_t token_offset, int head_dim, int parts, float* partial, float* mean, void* stream);
int flexam_attn_fwd_fp8(const void* q8, const void* qs, const void* kv8, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int L,
                        int head_dim, int kv_splits, int split_from_unit, float* ws_o, float* ws_ml, void* stream);
/* Smooth-V, SageAttention's `smooth_v`: the rows of softmax sum to 1, so softmax(S).(V - 1 c^T) + c^T = softmax(S).V for ANY vector c per
 * (batch, head).  V is quantised with one E8M0 scale per channel and 32-key half tile and e4m3's error is relative to the element, so a
 * channel offset all keys share is paid for in every product -- and multiplied by the e4m3 rounding of P as well (the plain output is
 * sum p~ (v - c) / l + c sum p~ / l with sum p~ / l != 1).  With c = the token mean of V (flexam_k_mean in its as-given form, wk = NULL,
 * on the V columns) both are gone.  Independent of smooth-K; the two compose.
 * flexam_attn_fp8_pack_shift_kv: flexam_attn_fp8_pack with K quantised from float(k) - k_shift[b][h * 128 + c] (as flexam_attn_fp8_pack_shift)
 * and V from float(v) - v_shift[b][h * 128 + c], one fp32 subtraction each in front of the block amax (fp32 [B][H * 128], taken as given).
 * Either shift may be NULL (that operand is packed as it is); k_shift needs q and k, v_shift also serves the V-only call (q = k = NULL).
 * Keys past L stay zero (codes 0, scale byte 1), not -shift; Q is flexam_attn_fp8_pack's, byte for byte.
 * flexam_attn_fwd_fp8_oshift: flexam_attn_fwd_fp8 (kv_splits, split_from_unit, ws_o and ws_ml as there) with o_shift[b][h * 128 + c]
 * (fp32 [B][H * 128], not NULL) added to O / l in fp32 BEFORE the one rounding to bf16, in both final writers: the attention kernel's own
 * epilogue (an instance under its own symbol; the shift is loaded behind the key loop) and, for the units split over key ranges, the
 * merge.  The partial results never carry it: their weights sum to 1, the merge adds it once. */
int flexam_attn_fp8_pack_shift_kv(const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v,
                                  int64_t v_bs, int64_t v_rs, void* q8, void* qs, void* kv8, int B, int H, int L, int head_dim,
                                  const float* k_shift, const float* v_shift, void* stream);
int flexam_attn_fwd_fp8_oshift(const void* q8, const void* qs, const void* kv8, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int L,
                               int head_dim, int kv_splits, int split_from_unit, float* ws_o, float* ws_ml, const float* o_shift,
                               void* stream);
/* The same kernel with Lq != Lk and the key records in CHUNKS of `chunk_tiles` 64-key tiles: kv8 = [n_chunks][B][H][chunk_tiles] records,
 * n_chunks = ceil(ceil(Lk / 64) / chunk_tiles) -- the rank-major result of all-gathering every rank's own records under sequence
 * parallelism (each rank's token chunk a multiple of 64 tokens: MXFP8 K|V travel instead of bf16 rows, 288 instead of 512 bytes per key
 * and head; the missing exchange of FlexAM/dist, wan_transformer3d_FlexAM.py:801-815, for VIDEOX_ATTENTION_TYPE=SAGE_ATTENTION).
 * q8 / qs: [B][H][ceil(Lq / 256) * 256] rows as flexam_attn_fp8_pack writes them for L = Lq.  Keys >= Lk are masked. */
int flexam_attn_fwd_fp8_chunked(const void* q8, const void* qs, const void* kv8, void* o, int64_t o_bs, int64_t o_rs, int B, int H,
                                int Lq, int Lk, int chunk_tiles, int head_dim, int kv_splits, int split_from_unit, float* ws_o,
                                float* ws_ml, void* stream);
/* flexam_attn_fwd_fp8 under the masks of flexam_attn_fwd_window / _window_sink / _window_frames, Lq == Lk = L, whole work units (no
 * split-KV): query i sees key j iff j < sink or lo(i) <= j <= hi(i), both clipped to [0, L) and a negative side unbounded.
 * frame_tokens = 0: a token window, lo = i - window_left, hi = i + window_right.  frame_tokens = T > 0: the two words count frames of T
 * tokens from token 0, lo = (i / T - window_left) T, hi = (i / T + window_right + 1) T - 1.  The operands are what flexam_attn_fp8_pack*
 * and flexam_rmsnorm_rope_mx* write (one chunk).  A work unit visits the sink tiles and the tiles that hold a key one of its 256 rows
 * sees, as the bf16 windowed kernel does; the kernels are instances of the MXFP8 kernel under their own symbols (attn8_window_kernel,
 * attn8_window_oshift_kernel) that take the four window words as a kernel argument of their own.  A row's first reference comes from
 * the first half tile in which it sees a key (floor(max of the scores it sees there) - 6), and the cap of 96 counts from there; keys it
 * does not see weigh exactly 0 and are in no row sum.  Smooth-K's operands need nothing new (q.c is one number per row whatever the
 * mask); o_shift != NULL adds smooth-V's shift as flexam_attn_fwd_fp8_oshift does (the rows of a masked softmax sum to 1 as well), NULL
 * is the plain instance.  Normalisations, each the very launch named: no bound on either side (or both reaching past the sequence from
 * every row), sink >= L, or frame_tokens >= L is flexam_attn_fwd_fp8 (with o_shift: _oshift) at kv_splits = 1; window_left < 0 drops
 * the sink.  sink < 0 and frame_tokens < 0 are FLEXAM_E_ARG. */
int flexam_attn_fwd_fp8_window(const void* q8, const void* qs, const void* kv8, void* o, int64_t o_bs, int64_t o_rs, int B, int H, int L,
                               int head_dim, int window_left, int window_right, int sink, int frame_tokens, const float* o_shift,
                               void* stream);
/* flexam_attn_fwd_fp8_window at a query offset, on the chunked records of flexam_attn_fwd_fp8_chunked: a rank's call under sequence
 * parallelism and the MXFP8 record gather.  The semantics are flexam_attn_fwd_window_at's: row i of the call is global token
 * g = q_offset + i and sees key j (0 <= j < Lk) iff j < sink or lo(g) <= j <= hi(g), lo / hi of flexam_attn_fwd_fp8_window taken at g; a
 * negative side is unbounded and window_left < 0 drops the sink.  q_offset + Lq may exceed Lk: the rows from global token Lk on are pad
 * rows, queries and never keys.  A row that sees no key is written as zeros (with o_shift as well: not as the shift), and a work unit
 * none of whose rows sees a key reads no record.  q8 / qs as for flexam_attn_fwd_fp8_chunked (L = Lq); kv8 = [n_chunks][B][H][chunk_tiles]
 * records.  The kernels are two further instances of the MXFP8 kernel under their own symbols (attn8_window_at_kernel,
 * attn8_window_at_oshift_kernel), whose argument is the four window words and q_offset; the first-reference rule, the cap and the whole
 * units are those of flexam_attn_fwd_fp8_window.  Normalisations, each the very launch named: q_offset = 0, Lq == Lk and chunk_tiles =
 * ceil(Lk / 64) (one chunk that holds exactly the call's tiles) is flexam_attn_fwd_fp8_window; a window that clips no row of THIS call
 * on either side, or sink >= Lk, is flexam_attn_fwd_fp8_chunked at kv_splits = 1 -- which takes no output shift, so that case with
 * o_shift != NULL is FLEXAM_E_ARG.  q_offset < 0, sink < 0, frame_tokens < 0 and chunk_tiles <= 0 are FLEXAM_E_ARG.  The number of
 * chunks is not an argument: that Lk fits the chunks the buffer holds is the caller's to check (hip.attn_fwd_fp8_chunked does, against
 * the tensor's shape). */
int flexam_attn_fwd_fp8_window_at(const void* q8, const void* qs, const void* kv8, void* o, int64_t o_bs, int64_t o_rs,
                                  int B, int H, int Lq, int Lk, int chunk_tiles, int head_dim,
                                  int window_left, int window_right, int sink, int frame_tokens, int q_offset,
                                  const float* o_shift, void* stream);

/* out_bf16[m,:] = LN(x_f32[m,:]; eps) [* ln_w + ln_b] [* scale[row(m),:] + shift[row(m),:]]
 * row(m) = row_index[m] if row_index else m / rows_per_batch; scale rows already hold (1+scale),
 * shift rows already hold shift + density shift (flexam_mod_table).  Replaces WanLayerNorm +
 * modulate: FlexAM/models/wan_transformer3d_FlexAM.py:192-202,452-453,461(norm3),464-465,506. */
int flexam_ln_modulate(const float* x, int64_t ldx, int64_t M, int C, float eps, const float* shift, const float* scale,
                       int64_t tab_ld, const int32_t* row_index, int64_t rows_per_batch, const float* ln_w,
                       const float* ln_b, void* out, int64_t ldo, void* stream);

/* The same row operation with the output quantised for flexam_gemm_fp8: q_out[m,:] = e4m3(y / row_scale[m]), row_scale[m] =
 * absmax(y[m,:]) / 448 (C a multiple of 512, at most 4096): the fp8 variant's QKV / FFN1 inputs without a second pass. */
/* next_scale (optional, [M]): a scale for the e4m3 OUTPUT of the GEMM + GELU this row feeds (flexam_gemm_fp8_gelu_q), known before
 * that GEMM runs: next_scale[m] = (1.07 |y[m,:]|_2 * next_wnorm + next_bias) / 448 with next_wnorm >= max_j |w_j|_2 of the
 * (dequantised) weight rows and next_bias >= max_j |b_j| -- by Cauchy-Schwarz no output element exceeds 448 next_scale[m]. */
int flexam_ln_modulate_fp8(const float* x, int64_t ldx, int64_t M, int C, float eps, const float* shift, const float* scale,
                           int64_t tab_ld, const int32_t* row_index, int64_t rows_per_batch, const float* ln_w, const float* ln_b,
                           void* q_out, int64_t ldq, float* row_scale, float* next_scale, float next_wnorm, float next_bias,
                           void* stream);

/* x_f32[m,:] += y_bf16[m,:] * gate[row(m),:] (gate NULL = 1).  wan_transformer3d_FlexAM.py:456,461,468. */
int flexam_gate_residual(float* x, int64_t ldx, const void* y, int64_t ldy, const float* gate, int64_t gate_ld,
                         const int32_t* row_index, int64_t rows_per_batch, int64_t M, int C, void* stream);

/* WanRMSNorm over the full row (all heads) followed by the 3-axis interleaved-pair RoPE, for q and
 * (optionally) k in one launch; bf16 in/out (in place allowed), fp32 math, one rounding.
 * rope_cos/rope_sin: [tokens, head_dim/2] fp32 per-token tables (identity rows = pass-through);
 * NULL = no rotation (cross-attention q).  token(m) = token_offset + m % tokens_per_batch.
 * Replaces WanRMSNorm.forward + rope_apply_qk: wan_transformer3d_FlexAM.py:137-170,173-189,242-249. */
int flexam_rmsnorm_rope(const void* q_in, int64_t ldq_in, void* q_out, int64_t ldq_out, const float* wq, const void* k_in,
                        int64_t ldk_in, void* k_out, int64_t ldk_out, const float* wk, int64_t M, int C, float eps,
                        const float* rope_cos, const float* rope_sin, int64_t tokens_per_batch, int64_t token_offset,
                        int head_dim, void* stream);

/* Same arithmetic, written straight into a sequence-parallel SEND layout (no pack copy): q and k are normed + rotated, v is
 * copied through; element (m, col) of each goes to
 *   *_out + (m / tokens_per_batch) * out_bs + (m % tokens_per_batch) * ld_out + (col / col_block) * block_stride + col % col_block
 * so a row is cut into column blocks (one per destination rank's group of heads) that land block_stride elements apart, and the
 * three tensors interleave through their base pointers (q_out, k_out = q_out + col_block, ...).  q / v may be NULL (the K|V
 * all-gather layout norms only k).  Replaces the missing FlexAM/dist exchange plumbing behind wan_transformer3d_FlexAM.py:801-815. */
int flexam_rmsnorm_rope_scatter(const void* q_in, int64_t ldq_in, const float* wq, const void* k_in, int64_t ldk_in, const float* wk,
                                const void* v_in, int64_t ldv_in, void* q_out, void* k_out, void* v_out, int64_t ld_out,
                                int64_t out_bs, int col_block, int64_t block_stride, int64_t M, int C, float eps,
                                const float* rope_cos, const float* rope_sin, int64_t tokens_per_batch, int64_t token_offset,
                                int head_dim, void* stream);

/* out[blk][r][j][:] = mod[blk][j][:] + e[r][j][:] + ((scale_mask>>j)&1) + density terms, where slot
 * s = (dens_slots >> 4j) & 0xF (0xF = none) adds mdens[blk][s][:] + dens[r / rows_per_batch][s][:].
 * One launch per denoise step builds the AdaLN tables of all blocks (wan_transformer3d_FlexAM.py:
 * 444-449,452,464; head :500-506). */
int flexam_mod_table(const float* mod, const float* e, const float* mdens, const float* dens, float* out, int nblk, int R,
                     int nj, int nslot, int C, int rows_per_batch, int scale_mask, int dens_slots, void* stream);

/* y[M,N] = silu_in?(x[M,K]) . W[N,K]^T + b, fp32 math, 1 <= M <= 32, W bf16 or fp32.  The time /
 * density embedding MLPs (forced fp32 in the reference: wan_transformer3d_FlexAM.py:928-955).  Every output is summed in the
 * same order whatever M is (M <= 8: one output per wave; above: four per wave and 32 rows per pass over W, for foreground
 * masks with many distinct per-token timesteps). */
int flexam_small_linear_f32(const float* x, int64_t ldx, const void* W, int w_is_bf16, int64_t ldw, const float* b, float* y,
                            int64_t ldy, int M, int N, int K, int silu_in, void* stream);

/* out[r][:dim/2] = cos(t[r] f_i), out[r][dim/2:] = sin(t[r] f_i), f_i = 10000^(-i/(dim/2)), fp64 math
 * (sinusoidal_embedding_1d, wan_transformer3d_FlexAM.py:31-41). */
int flexam_sinusoid_embed(const float* t, float* out, int R, int dim, void* stream);

/* im2col of a kernel = stride = (1,2,2) conv: src [C,F,H,W] (fp32 or bf16) ->
 * dst[row0 + (f,h/2,w/2)][col0 + c*4 + ph*2 + pw] bf16 (weight.flatten(1) column order).
 * patch_embedding / ref_conv inputs: wan_transformer3d_FlexAM.py:624-625,676,885,896. */
int flexam_patchify(const void* src, int src_is_bf16, int C, int F, int H, int W, void* dst, int64_t ldd, int col0,
                    int64_t row0, void* stream);

/* Head output tokens [L, 4C] fp32 (col = (ph*2+pw)*C + c), starting at token tok0 -> [C,F,H,W].
 * unpatchify, wan_transformer3d_FlexAM.py:1126-1149 (tok0 skips the reference-image tokens, :1106-1109). */
int flexam_unpatchify(const float* tok, int64_t ldt, int64_t tok0, int C, int F, int H, int W, void* dst, int dst_is_bf16,
                      void* stream);

/* One fused sampler step on fp32 latents [C,F,H,W]: v = u + guidance (c - u) (tok_cond NULL: v = u),
 * x += dt v, x = (1 - mask) known + mask x (mask [F,H,W], NULL: no blend).
 * FlexAM/pipeline/pipeline_wan2_2_fun_control_FlexAM.py:926-934 (+ unpatchify of both CFG rows). */
int flexam_cfg_euler_blend(const float* tok_uncond, const float* tok_cond, int64_t ldt, int64_t tok0, float guidance, float dt,
                           float* latents, const float* known, const float* mask, int C, int F, int H, int W, void* stream);

/* Multistep samplers (FlexAM/utils/fm_solvers_unipc.py:640-724, fm_solvers.py:706-798; PIPE.py:926-934 around them):
 * cfg_velocity: v[C,F,H,W] = unpatchify(u + g (c - u)) -- the noise_pred handed to scheduler.step;
 * lincomb_f32:  out = sum_i coefs[i] * terms[i] (n_terms <= 8; `terms` / `coefs` are HOST arrays, terms[i] device
 *               pointers; out may alias a term) -- every UniPC / DPM-Solver++ update is one such combination;
 * mask_blend_f32: x = (1 - mask) known + mask x, mask [fhw] broadcast over C channels. */
int flexam_cfg_velocity(const float* tok_uncond, const float* tok_cond, int64_t ldt, int64_t tok0, float guidance, float* v, int C,
                        int F, int H, int W, void* stream);
int flexam_lincomb_f32(float* out, int64_t n, int n_terms, const float* const* terms, const float* coefs, void* stream);
int flexam_mask_blend_f32(float* x, const float* known, const float* mask, int C, int64_t fhw, void* stream);

/* y[i] = a*x[i] + b*y[i], fp32, n % 4 == 0.  TeaCache bookkeeping: residual = x_after_blocks - x_before and
 * x += cached residual on skipped steps (wan_transformer3d_FlexAM.py:1003-1051). */
int flexam_axpby_f32(float* y, float a, const float* x, float b, int64_t n, void* stream);

/* out2[0] += sum of the buffer's 32-bit words, out2[1] += sum of word * (index + 1), mod 2^64 (out2: two uint64 the caller
 * zeroed).  A content key for the step-invariant conditioning tensors that the reference sampler re-creates with torch.cat on
 * every step (pipeline_wan2_2_fun_control_FlexAM.py:850-886): the DiT's per-clip work is redone only when it changes. */
int flexam_checksum(const void* data, int64_t nbytes, uint64_t* out2, void* stream);

/* Channels-last helpers around the implicit-GEMM convolutions (cnn-block: wan_transformer3d_FlexAM.py:
 * 680-705,869-881; VAE decoder: wan_vae3_8.py).  A conv input is a spatially zero-padded bf16 image
 * img[f][H+2][W+2][Cp]; tap (dh,dw) of a 3x3 kernel is then the constant A offset
 * ((dh-1)*(W+2)+(dw-1))*Cp handed to flexam_gemm_bf16 through a_koff.
 * pack_cl:   src [C,F,H,W] (fp32|bf16) -> interior of img at channel offset c0.
 * unpack_cl: rows [(f,hp,wp)][ld] (fp32|bf16), interior positions -> dst [C,F,H,W] fp32.
 * groupnorm_silu_cl: GroupNorm(groups, eps) over all interior positions of x [(f,hp,wp)][ld] fp32
 *   (stats: scratch [2*groups] fp32), * gamma + beta, SiLU, optional + residual (bf16 padded image,
 *   channel stride res_cp) -> interior of the bf16 padded image dst (channel stride Cp). */
int flexam_pack_cl(const void* src, int src_is_bf16, int C, int F, int H, int W, void* dst, int Cp, int c0, void* stream);
int flexam_unpack_cl(const void* src, int src_is_bf16, int64_t ld, int C, int F, int H, int W, float* dst, void* stream);
int flexam_groupnorm_silu_cl(const float* x, int64_t ld, int C, int F, int H, int W, int groups, float eps, const float* gamma,
                             const float* beta, float* stats, const void* residual, int res_cp, void* dst, int Cp, void* stream);

/* Wan2.2 3D-VAE decoder helpers (FlexAM/models/wan_vae3_8.py).  "rows" = [(t,hp,wp), ld] matrices
 * indexed by PADDED position (GEMM outputs), "image" = zero-bordered bf16 [frames,H+2,W+2,Cp].
 * vae_prep_cl: interior rows -> image (frame offset t0) or compact matrix; mode 0 cast, 1 RMS_norm
 *   (F.normalize over channels * sqrt(C) * gamma, :50-64), 2 RMS_norm + SiLU (:206-212, :671-673).
 * upsample2x_cl: nearest-exact 2x (+ frame de-interleave of the time_conv output, :153-156) -> image.
 * dupup_add_cl: x_main += DupUp3D(x_in) (:375-417), drop = leading frames cropped on the first chunk.
 * softmax_rows: bf16 softmax(scale * s) rows, zero padded to Npad columns (AttentionBlock :272).
 * scatter_add_cl: x[padded rows] += y[compact rows] (AttentionBlock residual :282).
 * vae_unpatchify_clamp: 12-channel rows -> video[3][Ftot][2H][2W] at frame f0, clamped (:304-318, :1043).
 * pack_affine_cl: z [C,T,H,W] * mul[c] + add[c] -> image (latent de-normalisation, :823-828). */
int flexam_vae_prep_cl(const void* src, int src_is_bf16, int64_t ld_src, int C, int T, int H, int W, const float* gamma, int mode,
                       void* dst, int Cp, int t0, int dst_compact, void* stream);
int flexam_upsample2x_cl(const void* src, int src_is_bf16, int64_t ld_src, int C, int T, int H, int W, int interleave, void* dst,
                         int Cp, void* stream);
int flexam_dupup_add_cl(float* x_main, int64_t ld_main, int Co, int To, int Ho, int Wo, const float* x_in, int64_t ld_in, int Ci,
                        int ft, int drop, void* stream);
/* Phase-decomposed "nearest 2x upsample + Conv2d 3x3" (Resample upsample2d / upsample3d, wan_vae3_8.py:76-99,153-160): output pixels of
 * parity (a, b) are a 2x2 convolution of the LOW-resolution image with pre-summed taps -- four flexam_gemm_bf16 launches over the low-
 * resolution image (16 instead of 36 tap products per low-resolution pixel; the upsampled image is never built).
 * deinterleave_cl: rows [T, 2C] -> padded image of 2T frames at the same resolution, frame 2t + s = channels [sC, (s+1)C) of frame t
 *   (the temporal half of upsample3d, :153-156).
 * phase_dupup_cl: x_main[(t', h', w')] = phases[(h'&1)*2 + (w'&1)][(t', h'>>1, w'>>1)] + DupUp3D(x_in) (the shortcut of dupup_add_cl,
 *   :375-417); phases = four [rows of the padded low-resolution image, Co] fp32 matrices `phase_stride` elements apart. */
int flexam_deinterleave_cl(const void* src, int src_is_bf16, int64_t ld_src, int C, int T, int H, int W, void* dst, int Cp, void* stream);
int flexam_phase_dupup_cl(const float* phases, int64_t ld_ph, int64_t phase_stride, float* x_main, int64_t ld_main, int Co, int To, int Ho,
                          int Wo, const float* x_in, int64_t ld_in, int Ci, int ft, int drop, void* stream);
/* tapsum_cl: a causal kt x 3 x 3 convolution with FEW output channels (decoder head 256 -> 12, wan_vae3_8.py:668-672) as one plain GEMM
 * over the input pixels (Y[pixel, tap * Co + o] = W[o, :, tap] . x[pixel, :], K = Cin: every activation read once) and this gather:
 * out[(t,h,w), o] = bias[o] + sum_taps Y[(t + dt, h + dh - 1, w + dw - 1), tap * Co + o].  Y rows = padded positions of the kt - 1 history
 * frames followed by the T current frames; out rows = padded positions of the T current frames (interior written). */
int flexam_tapsum_cl(const float* y, int64_t ld_y, int T, int H, int W, int kt, int Co, const float* bias, float* out, int64_t ld_out,
                     void* stream);
int flexam_softmax_rows(const float* s, int64_t ld_s, int64_t M, int N, float scale, void* out, int64_t ld_out, int Npad, void* stream);
int flexam_scatter_add_cl(float* x, int64_t ldx, const void* y, int64_t ldy, int C, int T, int H, int W, void* stream);
int flexam_vae_unpatchify_clamp(const float* src, int64_t ld_src, int T, int H, int W, float* video, int Ftot, int f0, float lo,
                                float hi, void* stream);
int flexam_pack_affine_cl(const float* src, int C, int T, int H, int W, const float* mul, const float* add, void* dst, int Cp,
                          void* stream);


/* Wan2.2 3D-VAE encoder helpers (FlexAM/models/wan_vae3_8.py:505-618 Encoder3d, :420-457 Down_ResidualBlock).
 * vae_patchify_cl: video[3][Ftot][2H][2W] frames f0..f0+T -> 12-channel image (patchify :285-301,
 *   channel c*4 + r*2 + q), frame offset t0 (history frames of the causal conv1).
 * space_to_depth_cl: rows at HxW -> image at H/2 x W/2 with 4 sub-pixel channel groups of Cs channels, so
 *   that ZeroPad2d((0,1,0,1)) + Conv2d(3, stride 2) (:104-113) is a unit-stride implicit GEMM.
 * avgdown_add_cl: x_main += AvgDown3D(x_in) (:321-372; front zero pad in time when Ti % ft != 0). */
int flexam_vae_patchify_cl(const float* video, int Ftot, int f0, int T, int H, int W, void* dst, int Cp, int t0, void* stream);
int flexam_space_to_depth_cl(const void* src, int src_is_bf16, int64_t ld_src, int C, int T, int H, int W, void* dst, int Cs, int t0,
                             void* stream);
int flexam_avgdown_add_cl(float* x_main, int64_t ld_main, int Co, int To, int Ho, int Wo, const float* x_in, int64_t ld_in, int Ci,
                          int Ti, int ft, int fs, void* stream);


/* umT5 text encoder helpers (FlexAM/models/wan_text_encoder.py; projections are flexam_gemm_bf16).
 * t5_norm: out = w * x * rsqrt(mean(x^2) + eps) per row (T5LayerNorm :44-56), bf16 or fp32 out.
 * softmax_bias_rows: P = softmax(scale * s + bias) over the keys with key_mask != 0 (T5Attention :91-103:
 *   relative-position bias [M, N], padding mask [N]; bias / key_mask may be NULL), bf16, zero padded to Npad; a row whose keys
 *   are all masked is uniform over the N keys, as the reference's finfo.min fill makes it.
 * mul_bf16: out = a * b elementwise (fc1(x) * gate(x), :125-126). */
int flexam_t5_norm(const float* x, int64_t ldx, int64_t M, int C, float eps, const float* w, void* out, int64_t ld_out, int out_f32,
                   void* stream);
int flexam_softmax_bias_rows(const float* s, int64_t ld_s, int64_t M, int N, float scale, const float* bias, int64_t ld_bias,
                             const float* key_mask, void* out, int64_t ld_out, int Npad, void* stream);
int flexam_mul_bf16(const void* a, const void* b, void* out, int64_t n, void* stream);



/* Conditioning rasteriser: tracked points [T, N, 3] (u, v, depth; fp32) -> conditioning video frames.  Replaces the per-point PIL
 * drawing loops of the reference's pipelines.py -- fun_visualize_tracking_with_depth :1501-1575 (valid_mask :1200-1212,
 * sort_points_by_depth :1214-1232, draw_rectangle :1234-1253), _render_cosine_encoded_frame :1694-1728, _visualize_depth_tracking
 * :1763-1820, _should_draw_point :1842-1850, _convert_frames_to_tensor :1658-1660 -- whose result per pixel is the colour of the
 * NEAREST point among the squares covering it (far-to-near painting).
 * raster_keys: keys[T][H][W] (uint64) = min over the drawn points whose square [x - half, x + half] x [y - half, y + half] (clipped to
 *   the frame) covers the pixel of (order-preserving code of the depth << 32 | point index); all ones = no point.  A point is drawn when
 *   visible[t][n] != 0 (NULL: all), its (u, v) are finite, (x, y) = (u, v) truncated towards zero lie in [0, W) x [y_min, H) (y_min = 1
 *   for the tracking video, whose frame test is y > 0, else 0) and, with a mask video [T][H][W], mask[t][y][x] > 0.5.  Equal depths: the
 *   lower index wins; NaN depths lose against everything.  The call clears `keys` itself.
 * raster_resolve: out_u8[T][H][W][3] and / or out_f32[3][T][H][W] (= byte / 255, correctly rounded) from the winners' colours;
 *   colors[N][3] bytes shared by all frames (color_frame_stride = 0) or [T][N][3] (stride N * 3: the depth video's per-frame colours).
 *   N = rows of a colour table = the point count the keys were made with: a key whose index is >= N (keys of another point set) resolves
 *   to black instead of reading past the table; a per-frame stride other than 0 or N * 3 is refused. */
int flexam_raster_keys(const float* points, const unsigned char* visible, int T, int N, int H, int W, int half, int y_min,
                       const float* mask, unsigned long long* keys, void* stream);
int flexam_raster_resolve(const unsigned long long* keys, const unsigned char* colors, int64_t color_frame_stride, int N, int T, int H, int W,
                          unsigned char* out_u8, float* out_f32, void* stream);

/* Command lists: a recorded sequence of this library's stream-ordered calls re-issued from ONE call (csrc/replay.hip).  The reference
 * has no counterpart -- its step loop is Python over PyTorch ops (pipeline_wan2_2_fun_control_FlexAM.py:844-949, one Python frame per
 * nn.Module call of wan_transformer3d_FlexAM.py:1053-1089); this is what replaces that per-op host cost when one rank of eight has
 * ~40 ms per step for ~450 launches.  A command = the id of an entry point of THIS header whose last parameter is `void* stream`
 * (flexam_fn_id(name); ids are positions in the header, never hard-coded) + its arguments without the stream as 8-byte words in
 * declaration order: pointers -> p, float -> f (as double), integers -> i.  flexam_replay calls them in order on `stream`; every call
 * checks its own arguments as usual; it stops at the first failure (its code returned, its message in flexam_last_error(),
 * *failed_at = index; -1 = none).  The list is HOST memory of the caller, read during the call only. */
/* Emulation aid (not on the product path): one wave that waits `us` microseconds of the constant 100 MHz counter on `stream`.  The
 * one-GPU emulation of a multi-GPU rank (bench.py --emulate-rank, flexam_amd.dist.LoopbackGroup) puts it where a collective's transfer
 * time would sit -- bytes per xGMI link / an ASSUMED link rate -- on the side stream RCCL's kernels would occupy. */
int flexam_delay_us(float us, void* stream);

#define FLEXAM_REPLAY_MAX_ARGS 26
typedef union { int64_t i; double f; void* p; } flexam_arg;
typedef struct { int32_t fn; int32_t nargs; flexam_arg a[FLEXAM_REPLAY_MAX_ARGS]; } flexam_cmd;
int flexam_fn_id(const char* name);            /* -1: not a replayable entry point */
int flexam_fn_count(void);
const char* flexam_fn_name(int id);
int flexam_replay(const flexam_cmd* cmds, int64_t n, int64_t* failed_at, void* stream);

/* Foreground-edit mask refinement (flexam_amd/edit_masks.py; csrc/edit_mask.hip).  Replaces the per-frame host loop of
 * demo.py:33-96, generate_mask_fg_tracking_for_validation: scipy gaussian_filter, cv2 findContours / convexHull / fillPoly, cv2.dilate.
 * Frames are n x H x W bytes, H <= 4096, W <= 16384; S = (W + 1) / 2 is the most runs a row can hold.
 * edit_mask_blur: dst = (gaussian(src) > 0.5) for src in {0, 1}: scipy.ndimage.gaussian_filter's arithmetic (fp64 sums in its order,
 *   mode 'reflect', float32 after each axis, axis 0 first).  weights[radius + 1]: the normalised kernel from its centre outwards (fp64);
 *   tmp: n x H x W float32 scratch.
 * edit_mask_hull: for every 8-connected component of bin (non-zero = set) the pixels in the closed convex hull of its pixel centres or
 *   on the hull's edges drawn as 8-connected lines; components with collinear centres give nothing.  Out: nruns[n][H] and, per run slot
 *   runs[n][H][S], the interval (lo | hi << 16) of its component in its row (lo > hi: none).  ws: slots x 5 x H x S ints of scratch;
 *   frames are processed `slots` at a time.
 * edit_mask_dilate: out[n][H][W] = 1 where some interval of a row y' with |y - y'| <= radius, widened by half_widths[|y - y'|] on both
 *   sides, covers the pixel (the element's rows); 0 elsewhere.  radius 0, half_widths {0}: the intervals themselves. */
int flexam_edit_mask_blur(const unsigned char* src, int n, int H, int W, const double* weights, int radius, float* tmp, unsigned char* dst,
                          void* stream);
int flexam_edit_mask_hull(const unsigned char* bin, int n, int H, int W, unsigned* runs, int* nruns, int* ws, int slots, void* stream);
int flexam_edit_mask_dilate(const unsigned* runs, const int* nruns, int n, int H, int W, const int* half_widths, int radius, unsigned char* out,
                            void* stream);

/* Edit tracks: camera and object motion on the 3-D tracks (flexam_amd/motion.py; csrc/motion.hip).  Replaces the per-point half of
 * pipelines.py:195-850 CameraMotionGenerator (w2s_moge :512-530, s2w_vggt :356-417, w2s_vggt :419-510), :852-1038 ObjectMotionGenerator
 * (_get_points_in_mask :857-876, apply_motion :937-945, 1010-1038) and :1255-1291 convert_moge_to_delta_format, i.e. demo.py:216-358;
 * the [T, 4, 4] matrices are made on the host and arrive as device arrays of their first three rows.  Points are (x, y, z) triples.
 * motion_select_map:    flags[n] = mask[n] != 0 and no coordinate of points[n] is NaN (:939).
 * motion_select_pixels: flags[n] = mask[clamp(round(y_n), 0, mask_h - 1)][clamp(round(x_n), 0, mask_w - 1)] != 0, halves rounded to even,
 *   NaN -> 0 (:867-874); points = the first frame [N, 3].
 *   Both also leave sums[0..2] = the sums of the selected points' x, y, z and sums[3] = their number, accumulated in double in a fixed
 *   order (one partial per FLEXAM_MOTION_CHUNK points, combined by index): the same bits on every run.  ws: 32 bytes per started chunk.
 * motion_compact: index[0 .. *count) = the positions n with mask[n] != 0, ascending (the order of a boolean-mask gather, :1282); the
 *   rest of index [N] is left alone.  ws: 4 bytes per started chunk.  N < 2^31.
 * motion_transform_f32: out[t][m] for t < T, m < M from source point n = index[m] (index NULL: n = m, M == N) of frame t (src +
 *   t * src_frame_stride floats; stride 0 = one [N, 3] map for all frames), in this order, each step rounded to float32 (k = 0..3 fmaf chain):
 *     motion != NULL and (flags == NULL or flags[n]):  p = motion[t] (p, 1)                     (motion [T][3][4])
 *     pose != NULL (then intr != NULL):                 c = pose[t] (p, 1); h = intr c; p = (h_x / h_z, h_y / h_z, c_z)   (pose [T][3][4], intr [3][3])
 *     p = (p_x * scale_u, p_y * scale_v, p_z)
 *   A fused call gives the bits of the same steps run as separate calls.
 * motion_unproject_f64 (s2w_vggt): out[t][n] = rinv[t] (kinv[t] (u, v, 1) * z - tvec[t]) where z > 0, else (0, 0, 0); points and out
 *   [T, N, 3] are both float32 (points_f32 != 0: computed in double, rounded once) or both double; kinv, rinv [T][3][3], tvec [T][3] double.
 * motion_project_f64 (w2s_vggt): c = pose[t] (p, 1); out[t][n] = (intr[t] (c / (c_z + 1e-10)))_xy, c_z where c_z > 0, else (0, 0, 0);
 *   points float32 or double, out double; pose [T][3][4], intr [T][3][3] double.
 * double pointers must be 8-byte, float / int pointers 4-byte aligned. */
#define FLEXAM_MOTION_CHUNK 1024
int flexam_motion_select_map(const float* points, int64_t N, const unsigned char* mask, unsigned char* flags, double* ws, int64_t ws_bytes,
                             double* sums, void* stream);
int flexam_motion_select_pixels(const float* points, int64_t N, const unsigned char* mask, int mask_h, int mask_w, unsigned char* flags,
                                double* ws, int64_t ws_bytes, double* sums, void* stream);
int flexam_motion_compact(const unsigned char* mask, int64_t N, int* index, int* count, int* ws, int64_t ws_bytes, void* stream);
int flexam_motion_transform_f32(const float* src, int64_t src_frame_stride, int T, int64_t N, const unsigned char* flags, const float* motion,
                                const float* pose, const float* intr, float scale_u, float scale_v, const int* index, int64_t M, float* out,
                                void* stream);
int flexam_motion_unproject_f64(const void* points, int points_f32, int T, int64_t N, const double* kinv, const double* rinv,
                                const double* tvec, void* out, void* stream);
int flexam_motion_project_f64(const void* points, int points_f32, int T, int64_t N, const double* pose, const double* intr, double* out,
                              void* stream);

/* Colour tables of the conditioning videos on the device (flexam_amd/conditioning_raster.py; csrc/raster_colors.hip): what
 * pipelines.py:1523-1545 (tracking), :1775-1792 (depth) and :1675-1692 (cosine codes -> bytes) compute with np.percentile on the host.
 * select_f32: exact order statistics.  Value (s, i), s < S, i < seg_len, is src[((s * seg_len + i) * stride + comp)], through
 *   transform (0: as it is; 1: 1 / (x + 1e-10f), both steps rounded to float32); it is VALID when mask == NULL or
 *   mask[s * seg_len + i] != 0.  Per segment: info[s][0] = number of valid values n, info[s][1] = 1 if a valid (transformed) value is
 *   NaN, info[s][2] = 1 if a valid value is != 0 BEFORE the transform (NaN counts), info[s][3] = 0; and, for K > 0,
 *   values[s][k] = the element of rank min(max(ranks[s][k], 0), n - 1) of the valid values in ascending order (NaN last, -0 before
 *   +0; n = 0: NaN).  K = 0 (ranks, values NULL) counts only.  Radix select on an order-preserving 32-bit code, 8 bits a pass:
 *   workgroups histogram the values under each rank's prefix in LDS and flush with integer atomics, a one-workgroup-per-segment
 *   kernel picks the bins between passes: the same bits on every run.  stride 1 .. 64, comp < stride, K <= FLEXAM_SELECT_MAX_RANKS,
 *   S <= 65535, seg_len < 2^31; ws: FLEXAM_SELECT_WS_SEGMENT_BYTES per segment (the call clears it); ranks [S][K] int64 on the device.
 * select_lerp: numpy's `_lerp` between neighbouring order statistics.  values [S][Q][2] = (lower, upper) as select_f32 leaves them for
 *   ranks (lo_0, hi_0, lo_1, hi_1, ..), gamma [S][Q] double = the weights; d = upper - lower in float32; out[s][q] =
 *   gamma >= 0.5 ? upper - d (1 - gamma) : lower + d gamma, evaluated in double into double out (f32_form = 0: np.percentile(a, [..])
 *   of float32 data) or in float32 into float out (f32_form != 0: np.percentile(a, scalar)); NaN where info[s][1] or info[s][0] == 0.
 * raster_colors_tracking: colors[N][3] from the first frame's points [N][3]: (clip(u / W), clip(v / H), clip((1 / (z + 1e-10) - p2) /
 *   (p98 - p2 + 1e-10))) * 255 truncated, all float32 and correctly rounded, NaN -> 0; pct = (p2, p98) float on the device.  With
 *   blue [N] != NULL that is the third byte instead (the all-zero-depth route, whose bytes the caller's generator draws).
 * raster_colors_depth: colors[T][N][3]: 0 where visible[t][n] == 0 (NULL: all visible), else lut[index of
 *   (clip(z, p2_t, p98_t) - p2_t) / (p98_t - p2_t)] in double where p98_t > p2_t, lut[0] otherwise; pct [T][2] double; lut [258][3] =
 *   256 colormap entries + under + over (matplotlib's Colormap.__call__ indexing: int(x * 256), 256 -> 255, NaN -> black).
 * raster_colors_cosine: colors[N][3] = clip((code + 1) / 2, 0, 1) * 255 truncated, float32, NaN -> 0; code [N][3].
 * colors must be 4-byte aligned. */
#define FLEXAM_SELECT_MAX_RANKS 8
#define FLEXAM_SELECT_WS_SEGMENT_BYTES 8320
int flexam_select_f32(const float* src, int stride, int comp, int transform, const unsigned char* mask, int S, int64_t seg_len,
                      const int64_t* ranks, int K, float* values, int64_t* info, void* ws, int64_t ws_bytes, void* stream);
int flexam_select_lerp(const float* values, const double* gamma, const int64_t* info, int S, int Q, int f32_form, void* out, void* stream);
int flexam_raster_colors_tracking(const float* points, int64_t N, int H, int W, const float* pct, const unsigned char* blue,
                                  unsigned char* colors, void* stream);
int flexam_raster_colors_depth(const float* points, const unsigned char* visible, int T, int64_t N, const double* pct,
                               const unsigned char* lut, unsigned char* colors, void* stream);
int flexam_raster_colors_cosine(const float* code, int64_t N, unsigned char* colors, void* stream);

/* Frames across the boundary (flexam_amd/frames.py; csrc/frames.hip).  Replaces the host resizes of FlexAM/utils/utils.py:473-517
 * get_maskvideo_to_video_latent (torchvision resize of float frames: bilinear, antialiased) and :424-438 get_video_to_video_latent's
 * tensor branch (F.interpolate bilinear, align_corners=False, then * 255, / 255 in numpy / torch), and the byte conversion of
 * utils.py:59-88 save_videos_grid behind the pipeline's decode_latents.
 * frames_resize: dst[t][c][oy][ox] = (sum_j wy[oy][j] * sum_i wx[ox][i] * src[t][c][y0 + j][x0 + i]) * mul / div + add, fp32, taps in
 *   ascending order, the three closing steps rounded one at a time (each skipped at its neutral value 1, 1, 0; div != 0).  src: uint8
 *   (src_is_u8 != 0; widened exactly) or float32, element strides s_t, s_c, s_y, s_x (>= 0), so [T, H, W, C] and [T, C, H, W] are both
 *   views of it; dst float32, element strides d_t, d_c, d_y, columns contiguous.  Per axis a table made on the host: index [n_out][2] =
 *   (first source index, tap count), weights [n_out][k] fp32 padded with zeros to the axis's largest tap count k (1 <= k <=
 *   FLEXAM_FRAMES_MAX_TAPS, k <= the axis's source size).  The kernel clamps what it reads from a table into the source.
 * frames_to_bytes: src [C][T][H][W] float32 or bf16 (C <= 4) -> dst [T][H][W][C] bytes.  is_signed != 0: x / 2, + 0.5 first; then clamp
 *   to [0, 1], * 255, truncation toward zero; every step one float32 rounding.  NaN -> 0. */
#define FLEXAM_FRAMES_MAX_TAPS 256
int flexam_frames_resize(const void* src, int src_is_u8, int64_t s_t, int64_t s_c, int64_t s_y, int64_t s_x, int T, int C, int H, int W,
                         float* dst, int64_t d_t, int64_t d_c, int64_t d_y, int oh, int ow, const int* y_index, const float* y_weights,
                         int ky, const int* x_index, const float* x_weights, int kx, float mul, float div, float add, void* stream);
int flexam_frames_to_bytes(const void* src, int src_is_bf16, int C, int T, int H, int W, int is_signed, unsigned char* dst, void* stream);

/* LoRA merge into stored weights (flexam_amd/lora_utils.py; csrc/lora.hip).  Replaces `weight.data += multiplier * alpha *
 * torch.mm(up, down)` of FlexAM/utils/lora_utils.py:480-485 (and `-=` of :594-599: unmerge is the same call with -s).
 * lora_merge: W[n][k] <- round_to_W_dtype(float(W[n][k]) + s * sum_{j < r} U[n][j] * D[j][k]).  W [N][K], row stride ldw elements
 *   (>= K: the rows of a fused q|k|v buffer are views), stored as bf16, fp32 or OCP e4m3 (w_dtype = FLEXAM_LORA_*); U [N][r], row
 *   stride ldu; D [r][K], row stride ldd; both fp32 or both bf16 (u_dtype == d_dtype; e4m3 factors are refused).  Every product and
 *   sum is fp32: acc = fma(U[n][j], D[j][k], acc) from 0 with j ascending, then fma(s, acc, W[n][k]); the result is rounded to the
 *   storage type once, to nearest even.  e4m3: a result whose magnitude exceeds 448 saturates to +-448 (NaN stays NaN).  Any N, K,
 *   r >= 1; in place, no allocation, no workspace.  FLEXAM_E_ARG: null pointer, unknown or mismatched dtype code; FLEXAM_E_SHAPE: a
 *   size < 1 or a row stride shorter than its row. */
#define FLEXAM_LORA_BF16 0
#define FLEXAM_LORA_F32 1
#define FLEXAM_LORA_E4M3 2
int flexam_lora_merge(void* W, int w_dtype, int64_t ldw, int64_t N, int64_t K, const void* U, int u_dtype, int64_t ldu, const void* D,
                      int d_dtype, int64_t ldd, int r, float s, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLEXAM_HIP_H */
