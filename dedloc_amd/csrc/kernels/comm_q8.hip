// BLOCKWISE_8BIT wire codec of the averaging data plane (the 8-bit companion of comm.hip).
//
// One encoded segment of n fp32 values (nb = ceil(n / 256) blocks of 256 values, the last one may be
// short) is a byte buffer of round_up(4 nb, 16) + round_up(n, 16) bytes, 16-byte aligned:
//   bytes [0, 4 nb)                     nb fp32 block scales, scale = max|x| / 127
//   bytes [round_up(4 nb, 16), +n)      n int8 codes, code = clamp(rint(x / scale), -127, 127)
// and every padding byte is written as 0.  decode(code) = code * scale.  A block that holds a
// non-finite value gets scale = NaN (and codes 0), so it decodes to NaN as a whole.
//
// pack_q8         : dst = encode(src)
// reduce_delta_q8 : the contract of reduce_delta on decoded rows: avg = v_0 + sum_k w_k (v_k - v_0) /
//                   sum_k w_k in fp32, delta_k = encode(avg - v_k) with its own block scales
// unpack_q8       : dst (+)= decode(src)
//
// Work split: a lane owns 16 consecutive values (four 16-byte fp32 accesses, one 16-byte access of
// codes), the 16 lanes of a DPP row own one block, a wave four blocks.  The block maximum is a
// butterfly over the row (DPP, no LDS); one lane per block writes the scale.
#include "dl_common.h"
#include "dl_kernels.h"

namespace {

constexpr int QB = 256;  // values per block
constexpr int QL = 16;   // values per lane

__host__ __device__ inline size_t q8_code_offset(size_t n) { return (4 * ((n + QB - 1) / QB) + 15) & ~(size_t)15; }

// max over the 16 lanes of a row, left in every lane: xor 1, xor 2 inside the quad, then the other
// quad of the half (row_half_mirror), then the other half (row_mirror)
__device__ __forceinline__ uint32_t row_max(uint32_t m) {
  int x = (int)m;
  x = max(x, __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));   // quad_perm:[1,0,3,2]
  x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));   // quad_perm:[2,3,0,1]
  x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true));  // row_half_mirror
  x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true));  // row_mirror
  return (uint32_t)x;
}

// Encode the lane's 16 values (entries past the segment's end are 0) into 16 codes; returns the
// block scale, the same in the row's 16 lanes.
__device__ __forceinline__ float encode16(const float* v, uint4& q) {
  // the order of (bits & 0x7fffffff) as integers is the order of |x|, and infinity and every NaN
  // lie above all finite values: one integer maximum gives the block amax and the non-finite test
  // (fmaxf would drop a NaN)
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < QL; ++j) m = max(m, __float_as_uint(v[j]) & 0x7fffffffu);
  m = row_max(m);
  q = uint4{0u, 0u, 0u, 0u};
  if (m >= 0x7f800000u) return __uint_as_float(0x7fc00000u);
  const float amax = __uint_as_float(m);
  const float scale = amax * (1.0f / 127.0f);
  if (scale == 0.f) return scale;  // a zero block (or one whose scale underflows): zero codes
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  // x / scale as a product with the reciprocal; blocks of tiny values, whose reciprocal would
  // overflow, are first scaled up by 2^64 (exact)
  const float up = amax < 1e-30f ? 0x1p64f : 1.f;
  const float inv = 1.0f / (scale * up);
#pragma unroll
  for (int j = 0; j < QL; ++j) {
    const float r = fminf(fmaxf(rintf(v[j] * up * inv), -127.f), 127.f);
    w[j >> 2] |= ((uint32_t)(int)r & 0xffu) << (8 * (j & 3));
  }
  q = uint4{w[0], w[1], w[2], w[3]};
  return scale;
}

// The decoded value is the ROUNDED product code * scale.  This file is built with -ffp-contract=on
// (_build.py FILE_FLAGS): the multiply below is never fused into a later addition, so a value decoded
// twice is the same number both times and identical rows reduce to exactly zero deltas.
__device__ __forceinline__ void decode16(const uint4& q, float scale, float* v) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int j = 0; j < QL; ++j) v[j] = (float)(int8_t)(w[j >> 2] >> (8 * (j & 3))) * scale;
}

__device__ __forceinline__ int lane_valid(size_t i0, size_t n) {
  return i0 >= n ? 0 : (n - i0 >= (size_t)QL ? QL : (int)(n - i0));
}

// The block's scale, written by the row's first lane; the lane of the last block also zeroes the
// padding between the scales and the codes.
__device__ __forceinline__ void store_scale(uint8_t* row, size_t b, size_t nb, size_t coff, float scale) {
  float* scales = reinterpret_cast<float*>(row);
  scales[b] = scale;
  if (b == nb - 1)
    for (size_t p = nb; p < coff / 4; ++p) scales[p] = 0.f;
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void pack_q8_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst,
                                                      size_t n) {
  const size_t nb = (n + QB - 1) / QB, coff = q8_code_offset(n);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // the loop condition is the same in the 16 lanes of a row (they share the block c / 16)
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; (c >> 4) < nb; c += stride) {
    const size_t i0 = c * QL;
    const int valid = lane_valid(i0, n);
    float v[QL];
    if (ALIGNED && valid == QL) {
      const float4* p = reinterpret_cast<const float4*>(src + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 f = p[j];
        v[4 * j] = f.x, v[4 * j + 1] = f.y, v[4 * j + 2] = f.z, v[4 * j + 3] = f.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < QL; ++j) v[j] = j < valid ? src[i0 + j] : 0.f;
    }
    uint4 q;
    const float scale = encode16(v, q);
    if (valid) *reinterpret_cast<uint4*>(dst + coff + i0) = q;  // the codes region ends at round_up(n, 16)
    if ((threadIdx.x & 15) == 0) store_scale(dst, c >> 4, nb, coff, scale);
  }
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void unpack_q8_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                        int add, size_t n) {
  const size_t coff = q8_code_offset(n);
  const float* scales = reinterpret_cast<const float*>(src);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c * QL < n; c += stride) {
    const size_t i0 = c * QL;
    const int valid = lane_valid(i0, n);
    const uint4 q = *reinterpret_cast<const uint4*>(src + coff + i0);
    float v[QL];
    decode16(q, scales[c >> 4], v);
    if (ALIGNED && valid == QL) {
      float4* p = reinterpret_cast<float4*>(dst + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float4 f = add ? p[j] : float4{0.f, 0.f, 0.f, 0.f};
        f.x += v[4 * j], f.y += v[4 * j + 1], f.z += v[4 * j + 2], f.w += v[4 * j + 3];
        p[j] = f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < QL; ++j)
        if (j < valid) dst[i0 + j] = add ? dst[i0 + j] + v[j] : v[j];
    }
  }
}

// KEEP: how many senders' codes and scales stay in registers (decoding again is three VALU
// operations a value); senders beyond that are read twice.  Small groups get a small KEEP and with
// it enough waves per SIMD to cover the memory latency.
template <int KEEP>
__global__ __launch_bounds__(256) void reduce_delta_q8_kernel(const uint8_t* __restrict__ parts, size_t row_bytes,
                                                              int nparts, const float* __restrict__ weights,
                                                              uint8_t* __restrict__ deltas, size_t n) {
  float wsum = 0.f;
  for (int k = 0; k < nparts; ++k) wsum += weights[k];
  // no weight at all: a no-op round (zero deltas), as in reduce_delta_kernel
  const bool none = !(wsum > 0.f);
  const float inv = none ? 0.f : 1.f / wsum;
  const size_t nb = (n + QB - 1) / QB, coff = q8_code_offset(n);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const bool lead = (threadIdx.x & 15) == 0;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; (c >> 4) < nb; c += stride) {
    const size_t b = c >> 4, i0 = c * QL;
    const int valid = lane_valid(i0, n);
    const size_t at = coff + i0;  // this lane's 16 codes in a row (inside the row only when valid > 0)
    const uint4 zero = uint4{0u, 0u, 0u, 0u};
    if (none) {
      for (int k = 0; k < nparts; ++k) {
        if (valid) *reinterpret_cast<uint4*>(deltas + k * row_bytes + at) = zero;
        if (lead) store_scale(deltas + k * row_bytes, b, nb, coff, 0.f);
      }
      continue;
    }
    uint4 q[KEEP];
    float sc[KEEP];
    q[0] = valid ? *reinterpret_cast<const uint4*>(parts + at) : zero;
    sc[0] = reinterpret_cast<const float*>(parts)[b];
    float v0[QL], s[QL], t[QL];
    decode16(q[0], sc[0], v0);
#pragma unroll
    for (int j = 0; j < QL; ++j) s[j] = 0.f;
    // avg = v_0 + sum_k w_k (v_k - v_0) / sum_k w_k: identical rows give exactly v_0 and zero deltas
#pragma unroll
    for (int k = 1; k < KEEP; ++k) {
      if (k < nparts) {
        const uint8_t* row = parts + k * row_bytes;
        q[k] = valid ? *reinterpret_cast<const uint4*>(row + at) : zero;
        sc[k] = reinterpret_cast<const float*>(row)[b];
        decode16(q[k], sc[k], t);
        const float w = weights[k];
#pragma unroll
        for (int j = 0; j < QL; ++j) s[j] += w * (t[j] - v0[j]);
      }
    }
    for (int k = KEEP; k < nparts; ++k) {
      const uint8_t* row = parts + k * row_bytes;
      const uint4 qk = valid ? *reinterpret_cast<const uint4*>(row + at) : zero;
      decode16(qk, reinterpret_cast<const float*>(row)[b], t);
      const float w = weights[k];
#pragma unroll
      for (int j = 0; j < QL; ++j) s[j] += w * (t[j] - v0[j]);
    }
#pragma unroll
    for (int j = 0; j < QL; ++j) s[j] = v0[j] + s[j] * inv;  // the average
    float d[QL];
    uint4 qo;
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
      if (k < nparts) {
        decode16(q[k], sc[k], t);
#pragma unroll
        for (int j = 0; j < QL; ++j) d[j] = j < valid ? s[j] - t[j] : 0.f;
        const float scale = encode16(d, qo);
        uint8_t* row = deltas + k * row_bytes;
        if (valid) *reinterpret_cast<uint4*>(row + at) = qo;
        if (lead) store_scale(row, b, nb, coff, scale);
      }
    }
    for (int k = KEEP; k < nparts; ++k) {
      const uint8_t* row = parts + k * row_bytes;
      const uint4 qk = valid ? *reinterpret_cast<const uint4*>(row + at) : zero;
      decode16(qk, reinterpret_cast<const float*>(row)[b], t);
#pragma unroll
      for (int j = 0; j < QL; ++j) d[j] = j < valid ? s[j] - t[j] : 0.f;
      const float scale = encode16(d, qo);
      uint8_t* out = deltas + k * row_bytes;
      if (valid) *reinterpret_cast<uint4*>(out + at) = qo;
      if (lead) store_scale(out, b, nb, coff, scale);
    }
  }
}

// one lane per 16 values, whole blocks: 16 lanes per block of 256 values
inline int grid_q8(size_t n) {
  const size_t lanes = (n + QB - 1) / QB * (QB / QL);
  const size_t g = (lanes + 255) / 256;
  return (int)(g < 4096 ? (g == 0 ? 1 : g) : 4096);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

size_t dl_q8_bytes(size_t n) { return q8_code_offset(n) + ((n + 15) & ~(size_t)15); }

int dl_pack_q8(const float* src, void* dst, size_t n, hipStream_t st) {
  if (n == 0 || !aligned16(dst)) return -1;
  if (aligned16(src)) pack_q8_kernel<true><<<grid_q8(n), 256, 0, st>>>(src, (uint8_t*)dst, n);
  else pack_q8_kernel<false><<<grid_q8(n), 256, 0, st>>>(src, (uint8_t*)dst, n);
  return 0;
}

int dl_unpack_q8(const void* src, float* dst, int add, size_t n, hipStream_t st) {
  if (n == 0 || !aligned16(src)) return -1;
  if (aligned16(dst)) unpack_q8_kernel<true><<<grid_q8(n), 256, 0, st>>>((const uint8_t*)src, dst, add, n);
  else unpack_q8_kernel<false><<<grid_q8(n), 256, 0, st>>>((const uint8_t*)src, dst, add, n);
  return 0;
}

int dl_reduce_delta_q8(const void* parts, void* deltas, int nparts, const float* weights, size_t n, hipStream_t st) {
  if (n == 0 || nparts < 1 || nparts > 64 || !aligned16(parts) || !aligned16(deltas)) return -1;
  const uint8_t* p = (const uint8_t*)parts;
  uint8_t* d = (uint8_t*)deltas;
  const size_t row = dl_q8_bytes(n);
  if (nparts <= 4) reduce_delta_q8_kernel<4><<<grid_q8(n), 256, 0, st>>>(p, row, nparts, weights, d, n);
  else if (nparts <= 8) reduce_delta_q8_kernel<8><<<grid_q8(n), 256, 0, st>>>(p, row, nparts, weights, d, n);
  else reduce_delta_q8_kernel<16><<<grid_q8(n), 256, 0, st>>>(p, row, nparts, weights, d, n);
  return 0;
}
