// Device helpers shared by the fused attention kernels (kernels/attention.hip: head_dim 64,
// kernels/attention_hd128.hip: head_dim 128): the swizzled 64x64 bf16 LDS tile with its row and
// transposed reads, the LDS-DMA staging primitives with their counted waits, the XCD-aware block
// order, the key-length mask decode and the cross-half softmax reductions.  Everything lives in an
// anonymous namespace: each translation unit gets its own copy and nothing is exported.
#pragma once

#include "dl_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s4_t __attribute__((ext_vector_type(4)));
typedef short s8_t __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s4_t lds_s4;

constexpr int TILE_BYTES = 64 * 128;  // one 64-row x 64-column bf16 tile
constexpr float NEG_BIG = -1.0e30f;

// One LDS image per 64x64 bf16 tile serves both the row reads and the transposed reads: 16-byte
// chunk c of row r lives at chunk c ^ f((r>>1)&7), f(x) = x ^ ((x&1)<<2) — conflict-free for the
// ds_read_b128 lane groups and for the 4-row tr-read blocks (derivation in docs/KERNELS.md).
__device__ __forceinline__ int swzf(int x) { return x ^ ((x & 1) << 2); }
__device__ __forceinline__ int chunk_off(int row, int c) { return row * 128 + ((c ^ swzf((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int crow(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

__device__ __forceinline__ floatx16 mfma32(bf16x8 a, bf16x8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// 16-byte row fragment: row `row`, chunk `c` of a swizzled tile
__device__ __forceinline__ bf16x8 lds_row_frag(const uint8_t* tile, int row, int c) {
  return *reinterpret_cast<const bf16x8*>(tile + chunk_off(row, c));
}

// ds_read_b64_tr_b16 on a swizzled tile: the calling lane (index i within its 16-lane group)
// supplies row row0 + (i>>2), columns col0 + 4*(i&3) .. +3; it receives column col0 + i of the
// four rows row0..row0+3.
__device__ __forceinline__ s4_t lds_tr(const uint8_t* tile, int row0, int col0, int i) {
  const int row = row0 + (i >> 2);
  const int col = col0 + 4 * (i & 3);
  const int off = chunk_off(row, col >> 3) + ((col & 7) << 1);
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(tile + off));
}

// A-operand fragment whose element e is taken from k-row 16*s + 8*(e>>2) + 4*hh + (e&3) of the
// tile (matching the permuted k order of an accumulator used as B operand), column = 32*t + r.
__device__ __forceinline__ bf16x8 tr_operand(const uint8_t* tile, int kbase, int hh, int t, int lane) {
  const int col0 = 32 * t + 16 * ((lane >> 4) & 1);
  const s4_t lo = lds_tr(tile, kbase + 4 * hh, col0, lane & 15);
  const s4_t hi = lds_tr(tile, kbase + 8 + 4 * hh, col0, lane & 15);
  // whole-vector shuffle + bit_cast: per-element __bf16 bit_casts of an s4 vector miscompile
  // (hipcc 7.2 broadcast element 0) — see tests/hip/primitives_test.hip
  const s8_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// accumulator registers 8s..8s+7 -> bf16 B-operand fragment
__device__ __forceinline__ bf16x8 pack_acc(const floatx16& x, int s) {
  bf16x8 b;
#pragma unroll
  for (int e = 0; e < 8; ++e) b[e] = (__bf16)x[8 * s + e];
  return b;
}

__device__ __forceinline__ bf16x8 gload8(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }

// ---- LDS-DMA staging primitives -------------------------------------------------------------------
// LDS-DMA writes lane-linearly (lane i -> base + 16 i), so the XOR swizzle of chunk_off is applied
// to the SOURCE: lane i of 1-KiB piece p loads row 8p + i/8, chunk (i & 7) ^ swz(row).
typedef __attribute__((address_space(3))) void lds_void;

// The DMA instructions are issued from inline asm.  With __builtin_amdgcn_global_load_lds the
// compiler's wait-count pass, which cannot tell ring slots apart, puts s_waitcnt vmcnt(0) in front
// of the first LDS read after any in-flight DMA (seen in the ISA: before the V tr-reads), which
// drains the whole prefetch every tile.  Hidden in asm, the DMAs are covered by the ring's own
// counted waits; the compiler's waits for its own loads stay correct (they only get stricter).
// M0 (the LDS base of the DMA) is written here and used by nothing else in these kernels.
__device__ __forceinline__ uint32_t lds_u32(const void* p) {
  return __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(const lds_void*)p);
}
__device__ __forceinline__ void dma16(const void* g, uint32_t lds) {
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds), "v"(g) : "memory", "m0");
}
__device__ __forceinline__ void dma4(const void* g, uint32_t lds) {
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dword %1, off" ::"s"(lds), "v"(g) : "memory", "m0");
}

// Prologue order in the ring kernels: issue the first NBUF-1 stages, THEN the block's compiler-visible
// register loads (Q / dO / K / V rows, lse ...), then this real s_waitcnt vmcnt(0) (the builtin, so
// the compiler's wait-count pass sees it): the asm DMAs are invisible to that pass, and a
// compiler-placed partial vmcnt for those register loads inside the tile loop would drain the ring.
// (the empty asm keeps the scheduler from sinking those loads below the wait; loads from const
// __restrict__ arguments may still move, so values the tile loop reads are also passed through
// `settle`, which makes the compiler complete the load before the asm and treat the register as
// the asm's output)
__device__ __forceinline__ void wait_vm_all() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
}
template <typename T>
__device__ __forceinline__ void settle(T& v) { asm volatile("" : "+v"(v)); }

// this wave's 1-KiB pieces (p = w, w + NW, ...) of a 64-row tile starting at global row row0
template <int NW = 4>
__device__ __forceinline__ void dma_tile(const bf16_t* g, long ld, int row0, uint8_t* tile, int w, int lane) {
#pragma unroll
  for (int j = 0; j < 8 / NW; ++j) {
    const int p = w + NW * j;
    const int row = 8 * p + (lane >> 3);
    const int c = (lane & 7) ^ swzf((row >> 1) & 7);
    dma16(g + (long)(row0 + row) * ld + c * 8, lds_u32(tile + p * 1024));
  }
}

// 64 consecutive floats -> 256 B of LDS (one dword per lane)
__device__ __forceinline__ void dma_f32x64(const float* g, uint8_t* dst, int lane) {
  dma4(g + lane, lds_u32(dst));
}

// Wait until this wave's pieces of the oldest in-flight stage have landed, leaving `ahead` later
// stages (0..NBUF-2) in flight; N = vector-memory ops this wave issues per stage.
template <int N>
__device__ __forceinline__ void wait_cnt(int ahead) {
  if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * N) : "memory");
  else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// PIECES = K + V tile pieces per wave per stage; the optional mask-bias piece adds one
template <int PIECES = 4>
__device__ __forceinline__ void wait_stages(int ahead, bool bias) {
  if (bias) wait_cnt<PIECES + 1>(ahead);
  else wait_cnt<PIECES>(ahead);
}

// 4 floats -> 4 consecutive bf16 (8 bytes)
__device__ __forceinline__ uint2 pack4(float a, float b, float c, float d) {
  uint2 v;
  v.x = (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16);
  v.y = (uint32_t)f2bf(c) | ((uint32_t)f2bf(d) << 16);
  return v;
}
__device__ __forceinline__ void store4(bf16_t* p, float a, float b, float c, float d) {
  *reinterpret_cast<uint2*>(p) = pack4(a, b, c, d);
}

// Wide store of one 64-column bf16 row held as two 32x32 accumulator tiles (cdna_hip_programming.md
// T21).  Lane L (hh = 0) holds columns 8k .. 8k+3 of 8-column group k = 4t + v, lane L + 32 columns
// 8k+4 .. 8k+7 of the same row.  For each pair of groups (k, k+1) a half exchange (vdst = group k,
// src = group k+1) leaves the lower lane with all 8 columns of group k and the upper lane with all 8
// of group k+1: one 16-byte store per pair, the upper half 8 elements further on.  Same bytes at
// the same addresses as 16 store4 calls, in 8 store instructions.  Every lane of the wave must call
// this (the exchange reads both halves); `live` guards the stores only, and is the same for the two
// lanes of a row.  `row` = the row's first column, 16-byte aligned.
__device__ __forceinline__ void store_row64(bf16_t* row, const floatx16 (&x)[2], float scale, int hh, bool live) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int vp = 0; vp < 2; ++vp) {
      const int i0 = 8 * vp;
      uint2 a = pack4(x[t][i0] * scale, x[t][i0 + 1] * scale, x[t][i0 + 2] * scale, x[t][i0 + 3] * scale);
      uint2 b = pack4(x[t][i0 + 4] * scale, x[t][i0 + 5] * scale, x[t][i0 + 6] * scale, x[t][i0 + 7] * scale);
      const auto rx = __builtin_amdgcn_permlane32_swap(a.x, b.x, false, false);
      const auto ry = __builtin_amdgcn_permlane32_swap(a.y, b.y, false, false);
      if (live) *reinterpret_cast<uint4*>(row + 32 * t + 16 * vp + 8 * hh) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
    }
}

// Sum over the 32 lanes of each half-wave (the two halves stay apart): DPP inside each row of 16
// lanes, then the gfx950 row-pair swap — wave_sum_dpp (dl_common.h) without its last step.  Every
// lane of a half gets that half's total.
__device__ __forceinline__ float half_wave_sum(float v) {
  v += dpp_f32<0xB1>(v);   // lane ^ 1
  v += dpp_f32<0x4E>(v);   // lane ^ 2
  v += dpp_f32<0x141>(v);  // row_half_mirror
  v += dpp_f32<0x140>(v);  // row_mirror
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);  // rows 0+1, 2+3
}

// The online-softmax rescale of O is deferred until a row's max grows by more than 2^RESCALE_THR
// (cdna_hip_programming.md T13: P <= 2^8 is exact enough in bf16 for P.V)
constexpr float RESCALE_THR = 8.f;

// XCD-aware block order (T1): the hardware deals consecutive workgroups round-robin to the 8 XCDs,
// which would put the query (or key) blocks of one head on different XCDs, each re-reading
// that head's K/V (Q/dO) into its own L2.  Renumber so each XCD gets a contiguous run of logical
// blocks: all blocks of a head then share one L2.
struct BlockId {
  int x, h, b;
};
__device__ __forceinline__ BlockId block_id(int xcd) {
  const int gx = gridDim.x, gy = gridDim.y;
  const int n = gx * gy * gridDim.z;
  int p = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
  if (xcd && (n & 7) == 0) p = (p & 7) * (n >> 3) + (p >> 3);
  return BlockId{p % gx, (p / gx) % gy, p / (gx * gy)};
}

// kvinfo = int32[B + 1]: lengths of right-padded key masks plus an "every mask is a prefix" flag
// in kvinfo[B].  Returns the key count to visit; use_len says whether the length mask applies.
__device__ __forceinline__ int kv_end_of(const int* kvinfo, int B, int b, int S, bool& use_len) {
  use_len = false;
  if (kvinfo == nullptr || kvinfo[B] == 0) return S;
  const int len = kvinfo[b];
  if (len <= 0 || len > S) return S;  // empty / malformed rows take the generic path
  use_len = true;
  return len;
}

// Where the rows of one (sequence, head) work item live.  Fixed-S form: sequence b owns rows
// b*S .. b*S + S of the token buffer, its lse / delta rows start at (b*H + h)*S and the key length
// comes from kvinfo (above).  Packed form (VARLEN): info = seqinfo = int32[2B + 1], B + 1 row
// offsets (multiples of 64) followed by B key lengths; sequence b owns the slot
// rows[b] .. rows[b+1], lse / delta are [H, T] (T arrives in the kernels' S argument) and the
// length mask always applies, so the generic additive bias is compiled out of the packed kernels.
// Slots are whole 64-row tiles: no tile load of a work item leaves its slot.
// (One helper per expression, each used where the fixed-S kernels compute it: their instruction
// streams are the same with and without the packed instantiations in the file.)
template <bool VARLEN>
__device__ __forceinline__ int seq_rows(const int* info, int b, int S) {  // rows of sequence b (its slot)
  if constexpr (VARLEN) return info[b + 1] - info[b];
  else return S;
}
template <bool VARLEN>
__device__ __forceinline__ long seq_base(const int* info, int b, int S) {  // its first row in the token buffer
  if constexpr (VARLEN) return info[b];
  else return (long)b * S;
}
template <bool VARLEN>
__device__ __forceinline__ int seq_kv_end(const int* info, int B, int b, int S, bool& use_len) {
  if constexpr (VARLEN) {
    use_len = true;
    return info[B + 1 + b];
  } else {
    return kv_end_of(info, B, b, S, use_len);
  }
}
// first lse / delta element of (sequence b, head h); T = rows of the packed token buffer
template <bool VARLEN>
__device__ __forceinline__ long seq_stat(int b, int h, int H, int S, int T, long rb) {
  if constexpr (VARLEN) return (long)h * T + rb;
  else return ((long)b * H + h) * S;
}

// v_max3_f32 without the canonicalising v_max the compiler inserts in front of fmaxf on MFMA results
// (MI355X_MICROARCH.md pitfalls): one instruction per two new scores
__device__ __forceinline__ float vmax3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// Cross-half (lane L <-> L ^ 32) max / sum through v_permlane32_swap (a VALU op; __shfl_xor(x, 32)
// is an LDS round trip on the softmax's critical path, T12).  After the swap r[0] holds, in lanes
// 32..63, the value of lane L - 32 and r[1], in lanes 0..31, the value of lane L + 32, so one op
// over r[0], r[1] combines the pair in every lane.
__device__ __forceinline__ float half_max(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  float m;
  asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(__uint_as_float(r[0])), "v"(__uint_as_float(r[1])));
  return m;
}
__device__ __forceinline__ float half_sum(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

}  // namespace
