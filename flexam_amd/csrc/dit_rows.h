// flexam_amd/csrc/dit_rows.h -- the two numerical contracts that the DiT row kernels (dit_elementwise.hip) and the GEMM epilogues
// around them (gemm.hip, gemm_fp8.hip) share: which row of a modulation table a token reads, and how a row becomes e4m3 bytes plus
// a scale.  (Not in common.h: the attention kernel's counter record is keyed on that file's text, benchlib/kernels.py:ATTN_SOURCES.)
#pragma once
#include "common.h"

__device__ __forceinline__ float wave_max(float v) {   // wave_sum's (common.h) counterpart
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// AdaLN: the row of a modulation / gate table that token m reads -- its entry of the per-token index where there is one, else
// one row per rows_per_batch consecutive tokens
__device__ __forceinline__ int64_t batch_row(int64_t rows_per_batch, int64_t m) { return m / rows_per_batch; }
__device__ __forceinline__ int64_t mod_row(const int32_t* row_index, int64_t rows_per_batch, int64_t m) {
  return row_index ? (int64_t)row_index[m] : batch_row(rows_per_batch, m);
}

// The e4m3 row quantiser, on which the producer of a row scale and the consumer of the bytes agree bit for bit: a row with
// absolute maximum amax is stored as e4m3(x * inv) next to scale = amax / 448 (the largest e4m3 value; 1 for an all-zero row)
struct RowScale8 { float scale, inv; };
__device__ __forceinline__ RowScale8 e4m3_row_scale(float amax) {
  const float scale = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;
  return {scale, 1.0f / scale};
}
// four values times the inverse scale -> four e4m3 bytes, v[0] in the lowest
__device__ __forceinline__ unsigned e4m3_pack4(f32x4 v, float inv) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, w, true);
  return (unsigned)w;
}
