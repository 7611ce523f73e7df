// flexam_amd/csrc/gemm_tile.h -- the skeleton of the persistent MFMA GEMM kernels (gemm.hip: bf16 and e4m3-W; gemm_fp8.hip: fp8
// operands), described once, and the pieces of it the two files share as code.  (attn.hip keeps its own copies of the LDS-DMA issue
// and of the LDS attribute call: profiles/head_attn_traffic.json is pinned to the text of the attention sources.)  K is counted in BYTES: a tile row of one K block is 128 bytes -- 64 bf16 or 128 fp8 values -- so the
// skeleton is the same for both element sizes:
//  * LDS image of a K block: [A tile | W tile], rows of 128 bytes, brought in by 16-byte LDS-DMA (lds_dma_b128) in pieces of 64
//    rows per workgroup instruction.  The LDS image must stay lane-linear for LDS-DMA, so the 16-byte chunk index is XOR-swizzled
//    with (row >> 1) & 7 on the SOURCE address (stage_setup in the kernels) and again on the fragment reads (frag_setup):
//    conflict-free per tools/lds_sim.py.
//  * persistent workgroups over an XCD-aware (XcdWalk), grouped (tile_origin in the kernels) tile order.
//  * two K-block buffers; the next unit's first two K blocks are issued in front of this unit's epilogue, and the hand-over between
//    units is counted (wait_barrier, wait_vm; the ordering argument is at the top-of-unit wait in gemm.hip).
//  * epilogues that turn a row tile of bf16 outputs round through a per-wave LDS slice, and a bounds-checked edge-tile form.
//  * host side: dynamic LDS raised once per device and kernel, the persistent grid, the tile-height chooser.
// Shared as code is what compiles to the same gfx950 instructions in every instance as the hand-written copies did
// (tools/isa_diff.py).  Still written out in both kernels, because a shared form changed instructions of some instance: the grouped
// tile origin and the staging offsets (operand order of scalar adds / one v_bitop3), the top-of-unit three-way wait (operand order of
// two s_and / s_or), the fragment offsets (the e4m3-W instances share subexpressions with their 64-byte-row form), stg_write and
// the bf16 / edge-tile epilogues (different address arithmetic and scheduling of the edge path).  By design not shared: the K
// block's inner order (bf16: cut by K halves; fp8: cut by m-tiles), the e4m3-W forms and the gate-residual read-modify-write bodies.
// Everything is in namespace gemm_tile; the kernels' own constants (BN, TILE_BYTES, ...) stay in their files.
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "flexam_hip.h"

namespace gemm_tile {

enum { EPI_NONE = 0, EPI_GELU = 1, EPI_GATE_RESIDUAL = 2, EPI_GELU_Q = 3 };      // GELU_Q (fp8 kernel only): GELU, then e4m3 / out_scale[m] (the next GEMM's A operand)
static_assert(EPI_NONE == FLEXAM_EPI_NONE && EPI_GELU == FLEXAM_EPI_GELU_TANH, "the `epilogue` argument of the C ABI is passed through as is");

template <int V>
using IC = std::integral_constant<int, V>;
using T_ = std::integral_constant<bool, true>;
using F_ = std::integral_constant<bool, false>;

// ---- LDS-DMA: global memory -> LDS without a VGPR round trip, 16 or 4 bytes per lane to lds_dst + 16 (4) * lane.  Inline asm, not
// the builtin: hipcc then does not know an LDS write is in flight and puts no s_waitcnt vmcnt(0) of its own in front of the LDS reads;
// completion is tracked by hand (wait_barrier / wait_vm).  Scalar-base form: uniform 64-bit base in SGPRs + one 32-bit per-lane
// offset, so a tile's pieces cost no 64-bit vector address arithmetic.
// M0 (the LDS base of the DMA) is written and NOT restored: nothing else in these kernels uses it (gfx9+ LDS instructions do not;
// tools/isa_loopwaits.py lists any other M0 reader of a listing), and the save / restore pair was 2 of the 6 scalar instructions
// of every piece.
__device__ __forceinline__ void lds_dma_b128(uint32_t voff, const void* sbase, uint32_t lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void lds_dma_b32(uint32_t voff, const void* sbase, uint32_t lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// ---- persistent workgroups over an XCD-aware tile order: workgroup w lives on XCD w & 7 (round-robin dispatch); that XCD owns a
// contiguous chunk of the `units` whole tiles and its gridDim/8 workgroups walk the chunk with stride gridDim/8, so the tiles
// resident on an XCD at any time are neighbours in the list (shared A / W panels in its private 4 MiB L2) and a workgroup pays its
// launch latency once, not once per tile.  Unit j (< n_units) of this workgroup is chunk0 + local + j * per_xcd.
struct XcdWalk {
  int chunk0, local, per_xcd, n_units;
  __device__ __forceinline__ explicit XcdWalk(int units) {
    const int q8 = units >> 3, r8 = units & 7, xcd = blockIdx.x & 7;
    per_xcd = gridDim.x >> 3;
    chunk0 = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
    const int chunk_n = q8 + (xcd < r8 ? 1 : 0);
    local = blockIdx.x >> 3;
    n_units = local < chunk_n ? (chunk_n - local + per_xcd - 1) / per_xcd : 0;
  }
};

// ---- waits.  s_waitcnt immediate of gfx9: vmcnt in bits 3:0 and 15:14, expcnt 6:4, lgkmcnt 11:8; the other two counters left alone
constexpr int waitcnt_vm(int n) { return (15 << 8) | (7 << 4) | (n & 15) | ((n >> 4) << 14); }
// at most N of this wave's vector-memory operations still in flight.  As a builtin the compiler's own wait bookkeeping sees it: at
// the end of an epilogue it says that every load has been consumed and keeps hipcc from putting a vmcnt(0) in front of the next
// unit's first register reuse, behind the stores.
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
  __builtin_amdgcn_s_waitcnt(waitcnt_vm(N));
}
// ... then barrier (asm: invisible to that bookkeeping, like the LDS-DMA issues it waits for)
template <int N>
__device__ __forceinline__ void wait_barrier(IC<N>) {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
  __syncthreads();
}
// ---- host
// Dynamic LDS above 64 KiB is raised once per kernel and device (the attribute belongs to the device's copy of the code object);
// `done` is the caller's flag row for this kernel.
inline int set_dynamic_lds_once(const void* kernel, int bytes, const char* who, bool (&done)[FLEXAM_MAX_DEVICES]) {
  const int dev = flexam_current_device();
  if (!done[dev]) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
      return flexam_fail(FLEXAM_E_LAUNCH, "%s: cannot raise dynamic LDS to %d bytes", who, bytes);
    done[dev] = true;
  }
  return FLEXAM_OK;
}
inline int persistent_grid(int units) {
  int grid = (units + 7) / 8 * 8;                                  // a multiple of 8 so that blockIdx & 7 is the XCD
  if (grid > flexam_num_cus()) grid = flexam_num_cus();            // one persistent workgroup per CU (156 of its 160 KiB of LDS)
  return grid;
}

// scratch for the tail split-K, handed in by the caller with every launch (nothing is retained between calls):
// slabs of 256 x 256 fp32, no initialisation needed.  Empty = no split-K.
struct GemmWorkspace {
  float* slabs = nullptr;
  int64_t n_slabs = 0;
};

// Tail split-K plan: `rem` = tiles of the last, partial round of the CUs.  Cutting each of them into S K slices turns that
// round into ceil(rem*S/G) passes of 1/S of a tile; every pass parks 256 KiB of partial sums per workgroup (~4 K blocks of main
// loop), and the finish launch costs a kernel boundary plus rem * S slabs read chip-wide (~4 + 0.03 * rem * S K blocks).  S (<= 8,
// slabs must fit the workspace) minimises the sum; with K = 3072 (48 K blocks) the hand-off eats most of the gain, with
// K = 14336 the tail shrinks to ~0.4 tile times.  `cost` = resulting length of the tail in tile times (1.0 without a split).
inline void plan_split(const GemmWorkspace& g_ws, int tiles, int nk, int& S, int& rem, double* cost = nullptr) {
  const int G = flexam_num_cus();
  static const int enabled = [] { const char* e = getenv("FLEXAM_GEMM_SPLITK"); return e ? atoi(e) : 1; }();
  rem = tiles % G;
  S = 1;
  double best = rem ? 1.0 : 0.0;
  if (enabled && g_ws.slabs && rem) {
    for (int s = 2; s <= 8 && s <= nk / 8 && (int64_t)rem * s <= g_ws.n_slabs; ++s) {
      const int passes = (rem * s + G - 1) / G;
      const double c = passes * (1.0 / s + 4.0 / nk) + (4.0 + 0.03 * rem * s) / nk;
      if (c < best - 0.05) { best = c; S = s; }
    }
  }
  if (cost) *cost = best;
}

// Length of a launch on the tile-height chooser's scale: rounds of the concurrently resident workgroups (whole ones + the tail
// plan_split leaves; without a workspace that is ceil(tiles / CUs)) x relative cost of one tile.
inline double launch_cost(const GemmWorkspace& g_ws, int tiles, int nk, double tile_cost) {
  int S, rem;
  double tail;
  plan_split(g_ws, tiles, nk, S, rem, &tail);
  return (tiles / flexam_num_cus() + tail) * tile_cost;
}

// The best 256-wide plan: tile heights MT = mt_hi..mt_lo, a tile costing its MT m-tiles of MFMA work plus a fixed part for the W
// side, barriers and the epilogue.  A smaller tile replaces a larger one only below `keep` x its cost; returns the cost of the plan kept.
inline double best_256wide(const GemmWorkspace& g_ws, int M, int tiles_n, int nk, double keep, int mt_hi, int mt_lo, int* best_mt = nullptr) {
  int best = mt_hi;
  double best_cost = 1e30;
  for (int mt = mt_hi; mt >= mt_lo; --mt) {
    const int tiles = (int)((long)((M + 32 * mt - 1) / (32 * mt)) * tiles_n);
    const double cost = launch_cost(g_ws, tiles, nk, mt + 1.25);
    if (cost < best_cost * keep) { best_cost = cost; best = mt; }
  }
  if (best_mt) *best_mt = best;
  return best_cost;
}

// Tile height of the 256-wide shapes, MT = mt_hi..mt_lo; FLEXAM_GEMM_MT in that range forces one (tuning only).
inline int pick_mt(const GemmWorkspace& g_ws, int M, int tiles_n, int nk, int mt_hi, int mt_lo) {
  const char* e = getenv("FLEXAM_GEMM_MT");
  const int forced = e ? atoi(e) : 0;
  if (forced >= mt_lo && forced <= mt_hi) return forced;
  int mt;
  best_256wide(g_ws, M, tiles_n, nk, 0.97, mt_hi, mt_lo, &mt);         // a smaller tile must win by > 3 %
  return mt;
}

}  // namespace gemm_tile
