// Flash-style self-attention for head_dim 128 (albert-xlarge-v2: 16 heads of 128): the same
// contract, layouts, masking and MFMA operand arrangement as the head_dim-64 kernels in
// attention.hip (see its header), reached through dl_attn_hd128_fwd / _bwd at the end of this file.
//
// A 64-row x 128-dim block of K, V, Q or dO is held in LDS as TWO of the swizzled 64x64 tiles of
// dl_attn_tile.h (dims 0-63, dims 64-127), so the row reads, the transposed reads and the LDS-DMA
// fill are the head_dim-64 ones; only the global column offset (+64) and the tile count per stage
// change.  Every kernel stages through an LDS-DMA ring (one slot = four tiles + 512 B of per-row
// floats = 33,280 B): two slots in the forward and dQ, three in dK/dV.
//
// Register budget (per lane, fp32 accumulators of 16 registers per 32x32 block):
//   fwd   : Q 32 + O 64 + S 32                  -> one 32-query sub-block per wave, 2 waves / SIMD
//   bwd dq: Q 32 + dO 32 + dQ 64 + S,dP 32      -> one 32-query sub-block per wave, 2 waves / SIMD
//   dkdv  : K 32 + V 32 + dK 64 + dV 64 + S,dP 32 -> one 32-key sub-block per wave, 1 wave / SIMD
//           (the whole 512-entry file, as the head_dim-64 KS = 2 form)
// A workgroup is 4 waves = 128 queries (keys) of one (batch, head).
#include <cstdlib>
#include <type_traits>

#include "dl_attn_tile.h"
#include "dl_common.h"
#include "dl_kernels.h"

namespace {

constexpr int HD = 128;                        // head dim
constexpr int NBUF = 2;                        // ring slots (forward, dQ)
constexpr int STAGE = 4 * TILE_BYTES + 512;    // [X dims 0-63 | X dims 64-127 | Y 0-63 | Y 64-127 | 128 floats]
constexpr int PIECES = 8;                      // 1-KiB DMA pieces per wave per stage (4 tiles x 2)
// dK/dV runs one workgroup per CU (registers), so its ring can be a slot deeper: three slots
// measured 1.2-1.7% faster on the whole backward than two on one box and within noise on another
// (profiles/README.md, "attention head_dim 128")
constexpr int KV_NBUF = 3;
constexpr int QB = 128;                        // queries (keys) per workgroup

// the two 64x64 tiles of a 64-row x 128-dim block starting at row row0
__device__ __forceinline__ void dma_block(const bf16_t* g, long ld, int row0, uint8_t* tiles, int w, int lane) {
  dma_tile(g, ld, row0, tiles, w, lane);
  dma_tile(g + 64, ld, row0, tiles + TILE_BYTES, w, lane);
}

// row fragment ks (0..7) of a block: dims 16 ks + 8 hh .. +7 of row `row`
__device__ __forceinline__ bf16x8 block_row_frag(const uint8_t* tiles, int row, int ks, int hh) {
  return lds_row_frag(tiles + (ks >> 2) * TILE_BYTES, row, 2 * (ks & 3) + hh);
}
// transposed operand for dim block t (0..3: dims 32 t .. 32 t + 31)
__device__ __forceinline__ bf16x8 block_tr(const uint8_t* tiles, int kbase, int hh, int t, int lane) {
  return tr_operand(tiles + (t >> 1) * TILE_BYTES, kbase, hh, t & 1, lane);
}

// ------------------------------------------------------------------------------------------ fwd
struct FwdCtx {
  const bf16_t* Kg;
  const bf16_t* Vg;
  long ld;
  int kv_end;
  const float* mb_g;
  float sl2;
  uint8_t* smem;
  int w, lane;
  __device__ __forceinline__ void issue(int s) const {  // key tile s -> ring slot s % NBUF
    uint8_t* slot = smem + (s % NBUF) * STAGE;
    dma_block(Kg, ld, s * 64, slot, w, lane);
    dma_block(Vg, ld, s * 64, slot + 2 * TILE_BYTES, w, lane);
    if (mb_g) dma_f32x64(mb_g + s * 64, slot + 4 * TILE_BYTES, lane);
  }
};

// Key tiles [kt0, kt1) of nt.  LEAN: unmasked tiles (raw scores, the scale rides in the exp FMA);
// !LEAN: the generic additive bias from the stage, or the length mask of the boundary tile.
template <bool LEAN>
__device__ __forceinline__ void fwd_tiles(const FwdCtx& c, int kt0, int kt1, int nt, const bf16x8 (&qf)[8],
                                          floatx16 (&o)[4], float& m, float& l, int r, int hh, int lane) {
  for (int kt = kt0; kt < kt1; ++kt) {
    // stage kt landed (this wave) -> barrier: every wave's pieces landed and every wave is done
    // with slot (kt - 1) % NBUF, which the stage issued next overwrites
    wait_stages<PIECES>(min(nt - 1 - kt, NBUF - 2), c.mb_g != nullptr);
    __syncthreads();
    if (kt + NBUF - 1 < nt) c.issue(kt + NBUF - 1);
    const uint8_t* Ks = c.smem + (kt % NBUF) * STAGE;
    const uint8_t* Vs = Ks + 2 * TILE_BYTES;
    const float* mb = reinterpret_cast<const float*>(Ks + 4 * TILE_BYTES);
    floatx16 s[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) s[j][i] = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) s[j] = mfma32(block_row_frag(Ks, 32 * j + r, ks, hh), qf[ks], s[j]);
    if (!LEAN) {
      if (c.mb_g) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 16; ++i) s[j][i] = fmaf(s[j][i], c.sl2, mb[32 * j + crow(i, hh)]);
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            s[j][i] = fmaf(s[j][i], c.sl2, kt * 64 + 32 * j + crow(i, hh) < c.kv_end ? 0.f : NEG_BIG);
      }
    }
    // row max as four independent max3 chains of 8 scores, then the halves
    float mc[4];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const floatx16& sv = s[q4 >> 1];
      const int o8 = (q4 & 1) * 8;
      float v = vmax3(sv[o8], sv[o8 + 1], sv[o8 + 2]);
      v = vmax3(v, sv[o8 + 3], sv[o8 + 4]);
      v = vmax3(v, sv[o8 + 5], sv[o8 + 6]);
      mc[q4] = v;
    }
    float mx = vmax3(vmax3(mc[0], mc[1], s[0][7]), vmax3(mc[2], mc[3], s[0][15]), vmax3(s[1][7], s[1][15], mc[0]));
    mx = half_max(mx);
    if (LEAN) mx *= c.sl2;
    const bool grow = mx > m + RESCALE_THR;
    if (__ballot(grow) != 0) {  // rare after the first tile: rescale O and l to the new max
      const float mn = grow ? mx : m;
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      l *= alpha;
      m = mn;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[t][i] *= alpha;
    }
    const float nm = -m;
    float rsa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float pv = __builtin_amdgcn_exp2f(LEAN ? fmaf(s[j][i], c.sl2, nm) : s[j][i] + nm);
        s[j][i] = pv;
        rsa[i & 7] += pv;
      }
    const float rs = ((rsa[0] + rsa[1]) + (rsa[2] + rsa[3])) + ((rsa[4] + rsa[5]) + (rsa[6] + rsa[7]));
    l += half_sum(rs);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        const bf16x8 pb = pack_acc(s[j], ss);
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = mfma32(block_tr(Vs, 32 * j + 16 * ss, hh, t, lane), pb, o[t]);
      }
  }
}

// VARLEN: the packed layout (seq_rows .. seq_stat in dl_attn_tile.h): kvinfo is seqinfo, S_ is T, the grid's x
// extent covers the largest slot and a block past its own slot leaves before any DMA or barrier.
template <bool VARLEN = false>
__global__ __launch_bounds__(256, 2) void attn128_fwd_kernel(const bf16_t* __restrict__ qkv, long ld,
                                                             const float* __restrict__ mbias,
                                                             const int* __restrict__ kvinfo, bf16_t* __restrict__ out,
                                                             long ldo, float* __restrict__ lse, int B, int H, int S_,
                                                             float sl2, int xcd) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * STAGE];
  const BlockId bid = block_id(xcd);
  const int b = bid.b, h = bid.h;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int S = seq_rows<VARLEN>(kvinfo, b, S_);
  if constexpr (VARLEN) {
    if (bid.x * QB >= S) return;  // uniform over the block
  }
  const long rb = seq_base<VARLEN>(kvinfo, b, S);
  const bf16_t* Qg = qkv + rb * ld + h * HD;
  bool use_len;
  FwdCtx c;
  c.Kg = qkv + rb * ld + (long)H * HD + h * HD;
  c.Vg = qkv + rb * ld + 2L * H * HD + h * HD;
  c.ld = ld;
  c.kv_end = seq_kv_end<VARLEN>(kvinfo, B, b, S, use_len);
  c.mb_g = (!use_len && mbias) ? mbias + rb : nullptr;
  c.sl2 = sl2;
  c.smem = smem;
  c.w = w;
  c.lane = lane;

  const int nt = (c.kv_end + 63) / 64;
  for (int s0 = 0; s0 < NBUF - 1 && s0 < nt; ++s0) c.issue(s0);
  const int q = bid.x * QB + w * 32 + r;
  const int qc = min(q, S - 1);
  bf16x8 qf[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) qf[ks] = gload8(Qg + (long)qc * ld + ks * 16 + 8 * hh);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) settle(qf[ks]);

  floatx16 o[4];
  float m = NEG_BIG, l = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[t][i] = 0.f;

  wait_vm_all();
  // lean tiles first (every tile when there is no mask), then the masked remainder: the boundary
  // tile of a length mask, or all tiles of a generic additive mask
  const int nlean = c.mb_g ? 0 : c.kv_end / 64;
  fwd_tiles<true>(c, 0, nlean, nt, qf, o, m, l, r, hh, lane);
  fwd_tiles<false>(c, nlean, nt, nt, qf, o, m, l, r, hh, lane);

  if (q < S) {
    const float inv = 1.f / l;
    bf16_t* op = out + (rb + q) * ldo + h * HD;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        store4(op + 32 * t + 8 * v + 4 * hh, o[t][4 * v] * inv, o[t][4 * v + 1] * inv, o[t][4 * v + 2] * inv,
               o[t][4 * v + 3] * inv);
    if (hh == 0) lse[seq_stat<VARLEN>(b, h, H, S, S_, rb) + q] = m + log2f(l);
  }
}

// ------------------------------------------------------------------------------------------ bwd dq
// Also computes delta = rowsum(dO * O) for its queries and publishes it for the dkdv kernel.
template <bool VARLEN = false>
__global__ __launch_bounds__(256, 2) void attn128_bwd_dq_kernel(
    const bf16_t* __restrict__ qkv, long ld, const float* __restrict__ mbias, const int* __restrict__ kvinfo,
    const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout, long ldo, const float* __restrict__ lse,
    float* __restrict__ delta, bf16_t* __restrict__ dqkv, float* __restrict__ dbias, int B, int H, int S_, float sl2,
    float scale, int xcd) {
  // the epilogue reuses the first 33 KiB for its column sums
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * STAGE];
  const BlockId bid = block_id(xcd);
  const int b = bid.b, h = bid.h;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int S = seq_rows<VARLEN>(kvinfo, b, S_);
  if constexpr (VARLEN) {
    if (bid.x * QB >= S) return;  // uniform over the block
  }
  const long rb = seq_base<VARLEN>(kvinfo, b, S);
  const bf16_t* Qg = qkv + rb * ld + h * HD;
  const bf16_t* Kg = qkv + rb * ld + (long)H * HD + h * HD;
  const bf16_t* Vg = qkv + rb * ld + 2L * H * HD + h * HD;
  bool use_len;
  const int kv_end = seq_kv_end<VARLEN>(kvinfo, B, b, S, use_len);
  const float* mb_g = (!use_len && mbias) ? mbias + rb : nullptr;
  const int nt = (kv_end + 63) / 64;
  auto issue = [&](int st) {  // key tile st -> slot st % NBUF
    uint8_t* slot = smem + (st % NBUF) * STAGE;
    dma_block(Kg, ld, st * 64, slot, w, lane);
    dma_block(Vg, ld, st * 64, slot + 2 * TILE_BYTES, w, lane);
    if (mb_g) dma_f32x64(mb_g + st * 64, slot + 4 * TILE_BYTES, lane);
  };
  for (int s0 = 0; s0 < NBUF - 1 && s0 < nt; ++s0) issue(s0);

  const int q = bid.x * QB + w * 32 + r;
  const int qc = min(q, S - 1);
  bf16x8 qf[8], df[8];
  float dl = 0.f;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    qf[ks] = gload8(Qg + (long)qc * ld + ks * 16 + 8 * hh);
    const long oo = (rb + qc) * ldo + h * HD + ks * 16 + 8 * hh;
    df[ks] = gload8(dout + oo);
    const bf16x8 of = gload8(out + oo);
#pragma unroll
    for (int e = 0; e < 8; ++e) dl += (float)df[ks][e] * (float)of[e];
  }
  dl += __shfl_xor(dl, 32, 64);
  float l2 = lse[seq_stat<VARLEN>(b, h, H, S, S_, rb) + qc];
  settle(l2);
  settle(dl);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    settle(qf[ks]);
    settle(df[ks]);
  }
  // (delta is stored after the tile loop: a store issued here would sit in the vmcnt queue ahead of
  // the ring's loads, and CDNA4 counts stores in vmcnt too)

  floatx16 dq[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[t][i] = 0.f;

  wait_vm_all();
  for (int kt = 0; kt < nt; ++kt) {
    wait_stages<PIECES>(min(nt - 1 - kt, NBUF - 2), mb_g != nullptr);
    __syncthreads();
    if (kt + NBUF - 1 < nt) issue(kt + NBUF - 1);
    const uint8_t* Ks = smem + (kt % NBUF) * STAGE;
    const uint8_t* Vs = Ks + 2 * TILE_BYTES;
    const float* mb = reinterpret_cast<const float*>(Ks + 4 * TILE_BYTES);
    const bool interior = mb_g == nullptr && (kt + 1) * 64 <= kv_end;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      floatx16 st, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) { st[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        st = mfma32(block_row_frag(Ks, 32 * j + r, ks, hh), qf[ks], st);
        dp = mfma32(block_row_frag(Vs, 32 * j + r, ks, hh), df[ks], dp);
      }
      if (interior) {  // interior tile: no mask
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = __builtin_amdgcn_exp2f(fmaf(st[i], sl2, -l2));
          st[i] = p * (dp[i] - dl);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = kt * 64 + 32 * j + crow(i, hh);
          const float bias = mb_g ? mb[32 * j + crow(i, hh)] : (key < kv_end ? 0.f : NEG_BIG);
          const float p = __builtin_amdgcn_exp2f(st[i] * sl2 + bias - l2);
          st[i] = p * (dp[i] - dl);
        }
      }
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        const bf16x8 pb = pack_acc(st, ss);
#pragma unroll
        for (int t = 0; t < 4; ++t) dq[t] = mfma32(block_tr(Ks, 32 * j + 16 * ss, hh, t, lane), pb, dq[t]);
      }
    }
  }
  __syncthreads();  // every wave is done with the ring before the epilogue reuses it
  if (q < S && hh == 0) delta[seq_stat<VARLEN>(b, h, H, S, S_, rb) + q] = dl;
  if (q < S) {
    bf16_t* dp_ = dqkv + (rb + q) * ld + h * HD;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        store4(dp_ + 32 * t + 8 * v + 4 * hh, dq[t][4 * v] * scale, dq[t][4 * v + 1] * scale, dq[t][4 * v + 2] * scale,
               dq[t][4 * v + 3] * scale);
  }
  if (dbias) {
    // Fused bias gradient of the QKV projection, as in the head_dim-64 kernel (query bias: column
    // sums of the bf16-rounded dQ just stored; value bias: column sums of the dO this block loaded;
    // key bias: exactly zero, nothing is added), through the same [4 waves][32 rows][64 columns]
    // fp32 LDS block (16-B chunk c of row r at c ^ (r & 15)), one 64-column half of the head at a
    // time so the scratch stays at 33 KiB.
    float* red = reinterpret_cast<float*>(smem);  // [4 waves][32 rows][64 columns]
    float* part = red + 4 * 32 * 64;              // [4 waves][64 columns]
    auto chunk_addr = [&](int row, int ch) { return red + (w * 32 + row) * 64 + ((ch ^ (row & 15)) << 2); };
    const bool live = q < S;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        if (which == 0) {
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4) {  // dQ columns 64 hf + 32 t + 8 v4 + 4 hh + (0..3), as stored above
              const floatx16& a = dq[2 * hf + t];
              float4 v = float4{0.f, 0.f, 0.f, 0.f};
              if (live)
                v = float4{round_bf16(a[4 * v4] * scale), round_bf16(a[4 * v4 + 1] * scale),
                           round_bf16(a[4 * v4 + 2] * scale), round_bf16(a[4 * v4 + 3] * scale)};
              *reinterpret_cast<float4*>(chunk_addr(r, 8 * t + 2 * v4 + hh)) = v;
            }
        } else {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int g = 0; g < 2; ++g) {  // dO columns 64 hf + 16 ks + 8 hh + 4 g + (0..3), as loaded above
              const bf16x8& d = df[4 * hf + ks];
              float4 v = float4{0.f, 0.f, 0.f, 0.f};
              if (live) v = float4{(float)d[4 * g], (float)d[4 * g + 1], (float)d[4 * g + 2], (float)d[4 * g + 3]};
              *reinterpret_cast<float4*>(chunk_addr(r, 4 * ks + 2 * hh + g)) = v;
            }
        }
        __syncthreads();
        {
          const int c = lane;  // this thread: column c of wave w's 32 rows
          float sum = 0.f;
#pragma unroll 8
          for (int row = 0; row < 32; ++row)
            sum += red[(w * 32 + row) * 64 + (((c >> 2) ^ (row & 15)) << 2) + (c & 3)];
          part[w * 64 + c] = sum;
        }
        __syncthreads();
        if (threadIdx.x < 64) {
          const int c = threadIdx.x;
          atomicAdd(&dbias[(which ? 2L * H * HD : 0L) + h * HD + 64 * hf + c],
                    part[c] + part[64 + c] + part[128 + c] + part[192 + c]);
        }
        __syncthreads();
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ bwd dkdv
// One 32-key sub-block per wave; Q / dO blocks (and lse / delta) of 64 queries stream through the ring.
// NB = ring slots: with one workgroup per CU the LDS has room for a deeper ring than the forward's.
template <int NB, bool VARLEN = false>
__global__ __launch_bounds__(256, 1) void attn128_bwd_dkdv_kernel(
    const bf16_t* __restrict__ qkv, long ld, const float* __restrict__ mbias, const int* __restrict__ kvinfo,
    const bf16_t* __restrict__ dout, long ldo, const float* __restrict__ lse, const float* __restrict__ delta,
    bf16_t* __restrict__ dqkv, int B, int H, int S_, float sl2, float scale, int xcd) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[NB * STAGE];
  const BlockId bid = block_id(xcd);
  const int b = bid.b, h = bid.h;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int S = seq_rows<VARLEN>(kvinfo, b, S_);
  if constexpr (VARLEN) {
    if (bid.x * QB >= S) return;  // uniform over the block
  }
  const long rb = seq_base<VARLEN>(kvinfo, b, S);
  const bf16_t* Qg = qkv + rb * ld + h * HD;
  const bf16_t* Kg = qkv + rb * ld + (long)H * HD + h * HD;
  const bf16_t* Vg = qkv + rb * ld + 2L * H * HD + h * HD;
  const bf16_t* dOg = dout + rb * ldo + h * HD;
  const float* lse_g = lse + seq_stat<VARLEN>(b, h, H, S, S_, rb);
  const float* del_g = delta + seq_stat<VARLEN>(b, h, H, S, S_, rb);

  const int k = bid.x * QB + w * 32 + r;
  bool use_len;
  const int kv_end = seq_kv_end<VARLEN>(kvinfo, B, b, S, use_len);
  if (use_len && bid.x * QB >= kv_end) {  // every key of this block is padding: dK = dV = 0
    if (k < S) {
      bf16_t* dkp = dqkv + (rb + k) * ld + (long)H * HD + h * HD;
      bf16_t* dvp = dqkv + (rb + k) * ld + 2L * H * HD + h * HD;
#pragma unroll
      for (int v = 0; v < 16; ++v) {  // the same 128 columns the regular epilogue covers (32t + 8v' + 4hh)
        store4(dkp + 8 * v + 4 * hh, 0.f, 0.f, 0.f, 0.f);
        store4(dvp + 8 * v + 4 * hh, 0.f, 0.f, 0.f, 0.f);
      }
    }
    return;
  }
  const int nt = S / 64;
  auto issue = [&](int st) {  // query tile st -> slot st % NB; waves 0-1 fetch lse, 2-3 delta
    uint8_t* slot = smem + (st % NB) * STAGE;
    dma_block(Qg, ld, st * 64, slot, w, lane);
    dma_block(dOg, ldo, st * 64, slot + 2 * TILE_BYTES, w, lane);
    dma_f32x64((w < 2 ? lse_g : del_g) + st * 64, slot + 4 * TILE_BYTES + (w < 2 ? 0 : 256), lane);
  };
  for (int s0 = 0; s0 < NB - 1 && s0 < nt; ++s0) issue(s0);

  const int kc = min(k, S - 1);
  bf16x8 kf[8], vf[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    kf[ks] = gload8(Kg + (long)kc * ld + ks * 16 + 8 * hh);
    vf[ks] = gload8(Vg + (long)kc * ld + ks * 16 + 8 * hh);
  }
  float mbk = use_len ? (k < kv_end ? 0.f : NEG_BIG) : (mbias ? mbias[rb + kc] : 0.f);
  settle(mbk);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    settle(kf[ks]);
    settle(vf[ks]);
  }

  floatx16 dk[4], dv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk[t][i] = 0.f; dv[t][i] = 0.f; }

  wait_vm_all();

  // LEAN (a key-length mask, the model's case): the mask term leaves the loop — a masked key's P
  // is computed as if it were live and its dK / dV rows are zeroed once at the end (dK / dV of a
  // key depend on that key's P and dS only); the generic additive mask keeps the bias in the
  // exponent.
  auto qloop = [&](auto lean_tag) {
    constexpr bool LEAN = decltype(lean_tag)::value;
    for (int qt = 0; qt < nt; ++qt) {
      wait_stages<PIECES>(min(nt - 1 - qt, NB - 2), true);
      __syncthreads();
      if (qt + NB - 1 < nt) issue(qt + NB - 1);
      const uint8_t* Qs = smem + (qt % NB) * STAGE;
      const uint8_t* Ds = Qs + 2 * TILE_BYTES;
      const float* lse_s = reinterpret_cast<const float*>(Qs + 4 * TILE_BYTES);
      const float* del_s = lse_s + 64;
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2) {
        floatx16 sc, dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) { sc[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          sc = mfma32(block_row_frag(Qs, 32 * i2 + r, ks, hh), kf[ks], sc);
          dp = mfma32(block_row_frag(Ds, 32 * i2 + r, ks, hh), vf[ks], dp);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int qq = 32 * i2 + crow(i, hh);
          // LEAN: one FMA per score (-lse is a free operand modifier)
          const float p = __builtin_amdgcn_exp2f(LEAN ? fmaf(sc[i], sl2, -lse_s[qq]) : sc[i] * sl2 + mbk - lse_s[qq]);
          sc[i] = p;
          dp[i] = p * (dp[i] - del_s[qq]);
        }
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
          const bf16x8 pb = pack_acc(sc, ss);
          const bf16x8 db = pack_acc(dp, ss);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            dv[t] = mfma32(block_tr(Ds, 32 * i2 + 16 * ss, hh, t, lane), pb, dv[t]);
            dk[t] = mfma32(block_tr(Qs, 32 * i2 + 16 * ss, hh, t, lane), db, dk[t]);
          }
        }
      }
    }
  };
  if (use_len) {
    qloop(std::true_type{});
    if (k >= kv_end)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) dk[t][i] = dv[t][i] = 0.f;
  } else {
    qloop(std::false_type{});
  }
  if (k < S) {
    bf16_t* dkp = dqkv + (rb + k) * ld + (long)H * HD + h * HD;
    bf16_t* dvp = dqkv + (rb + k) * ld + 2L * H * HD + h * HD;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        store4(dkp + 32 * t + 8 * v + 4 * hh, dk[t][4 * v] * scale, dk[t][4 * v + 1] * scale, dk[t][4 * v + 2] * scale,
               dk[t][4 * v + 3] * scale);
        store4(dvp + 32 * t + 8 * v + 4 * hh, dv[t][4 * v], dv[t][4 * v + 1], dv[t][4 * v + 2], dv[t][4 * v + 3]);
      }
  }
}

// Block order remapped so that the query (key) blocks of one (batch, head) share an XCD's L2.
constexpr int kAttnXcd = 1;

}  // namespace

// This unit's kernels take the fused QKV buffer (no compact queries) at head_dim 128 with 16-byte
// aligned rows, and S % 64 == 0 or the packed layout (the callers validate what seqinfo holds:
// csrc/bindings.cpp)
static bool hd128_ok(const DlAttn& a) {
  if (a.q || a.D != HD || a.ld % 8 != 0 || a.ldo % 8 != 0) return false;
  if (!a.seqinfo) return a.S % 64 == 0;
  return a.B >= 1 && a.T % 64 == 0 && a.max_slot >= 64 && a.max_slot % 64 == 0 && a.max_slot <= a.T;
}

// All launch sites of one layout (as hd64_launch in attention.hip, and with its reason for the
// order: the fixed-S three, then the packed three).  One grid serves all three kernels: query blocks
// for the forward and dQ, key blocks for dK/dV, all of QB rows.
template <bool PACKED>
static int hd128_launch(const DlAttn& a, bool bwd, hipStream_t st) {
  if (!hd128_ok(a)) return -1;
  const float* mbias = PACKED ? nullptr : a.mbias;
  const int* info = PACKED ? a.seqinfo : a.kvinfo;
  const int S = PACKED ? a.T : a.S, rows = PACKED ? a.max_slot : a.S;
  const float sl2 = a.scale_log2();
  dim3 grid((rows + QB - 1) / QB, a.H, a.B);
  if (!bwd) {
    attn128_fwd_kernel<PACKED><<<grid, 256, 0, st>>>(a.kv, a.ld, mbias, info, a.out, a.ldo, a.lse, a.B, a.H, S, sl2,
                                                     kAttnXcd);
    return 0;
  }
  attn128_bwd_dq_kernel<PACKED><<<grid, 256, 0, st>>>(a.kv, a.ld, mbias, info, a.out, a.dout, a.ldo, a.lse, a.delta,
                                                      a.dqkv, a.dbias, a.B, a.H, S, sl2, a.scale, kAttnXcd);
  attn128_bwd_dkdv_kernel<KV_NBUF, PACKED><<<grid, 256, 0, st>>>(a.kv, a.ld, mbias, info, a.dout, a.ldo, a.lse,
                                                                 a.delta, a.dqkv, a.B, a.H, S, sl2, a.scale, kAttnXcd);
  return 0;
}

int dl_attn_hd128_fwd(const DlAttn& a, hipStream_t st) {
  return !a.seqinfo ? hd128_launch<false>(a, false, st) : hd128_launch<true>(a, false, st);
}

int dl_attn_hd128_bwd(const DlAttn& a, hipStream_t st) {
  return !a.seqinfo ? hd128_launch<false>(a, true, st) : hd128_launch<true>(a, true, st);
}
