// Flash-style multi-head self-attention for ALBERT: head_dim 64 (head_dim 128:
// attention_hd128.hip; csrc/bindings.cpp picks the file by head size), S % 64 == 0,
// additive key-padding bias, bf16 in/out, fp32 softmax state, never materialises [B,H,S,S].
//
// Inputs come straight from the fused QKV projection: qkv is [B*S, 3*H*64] (Q | K | V, head h at
// columns h*64 of each third) and the context is written as [B*S, H*64] — exactly the layout the
// output projection consumes, so no transposes exist anywhere in the attention path.
//
// MFMA: v_mfma_f32_32x32x16_bf16 (cdna_hip_programming.md §3).  Every product is arranged so that
// the "reduction-side" operand comes out of the previous MFMA's accumulator with no lane movement
// (§3 "An accumulator tile as the next MFMA's operand"), and the other operand is read from LDS
// either by rows (ds_read_b128) or transposed (ds_read_b64_tr_b16, T10):
//   fwd   : S^T = K Q^T (query on the lane -> softmax row state is per-lane)
//           O^T += V^T P^T (P^T accumulator is the B operand; V^T via tr-reads)
//   bwd dq: S^T, dP^T = V dO^T, dQ^T += K^T dS^T        (query on the lane)
//   bwd dkdv: S = Q K^T, dP = dO V^T (key on the lane), dV^T += dO^T P, dK^T += Q^T dS
// One LDS image per 64x64 bf16 tile serves both the row reads and the transposed reads: 16-byte
// chunk c of row r lives at chunk c ^ f((r>>1)&7), f(x) = x ^ ((x&1)<<2) — conflict-free for the
// ds_read_b128 lane groups and for the 4-row tr-read blocks (derivation in docs/KERNELS.md).
#include <cstdlib>
#include <type_traits>

#include "dl_attn_tile.h"  // tile image, tr-reads, LDS-DMA primitives, block order: shared with head_dim 128
#include "dl_common.h"
#include "dl_kernels.h"

namespace {

constexpr int HD = 64;          // head dim

// The one launched configuration.  Blocks are 4 waves (256 threads, two blocks per CU); a wave of
// the forward and dQ kernels carries QS = 2 query sub-blocks of 32 rows, a wave of the dK/dV kernel
// one 32-key sub-block; every kernel stages its tiles through the LDS-DMA ring below.  With QS = 2
// every K fragment (row reads) and V fragment (tr-reads) read from LDS feeds two MFMAs, and each
// wave carries two independent softmax chains the scheduler can interleave (the loops are
// latency-bound: PMC, profiles/README.md "Round 2: attention latency work").  The forms measured
// against it and no longer in the file:
//   - one sub-block per wave (forward, dQ): forward 555 us against 507 us, dQ backward 5.5% slower
//     (same section; profiles/attn_bwd_dq_qs_ab_b256.jsonl);
//   - 8-wave forward blocks (one 512-query block per head at S = 512, K / V staged once per head):
//     5% slower (profiles/attn_fwd_nw8_ab_b256.jsonl);
//   - two key sub-blocks per wave in dK/dV: its 128 accumulator registers need the whole register
//     file, so it ran one wave per SIMD (launch bound 256 x 1) and measured 8% slower
//     (profiles/attn_dkdv_ks_ab_b256.jsonl);
//   - register staging (global -> VGPR -> ds_write, two-deep) instead of the ring: 26-43% of wave
//     cycles parked in s_waitcnt / barrier (profiles/attn_pmc_regstaged_b256.txt), the forward's
//     second sub-block spilled (the ring frees 16 staging VGPRs), and dK/dV was 3.5% slower at
//     B = 512 (profiles/README.md, "dK/dV through the LDS-DMA ring").
constexpr int QS = 2;

// ---- LDS-DMA staging ring ------------------------------------------------------------------------
// Each pipeline stage holds the two 64x64 tiles of one key (or query) block plus 64-128 floats of
// per-row data, written by global_load_lds (no VGPR round trip, no ds_write).  NBUF stages: the
// loads of stage s + NBUF - 1 are issued while stage s computes, and a counted vmcnt waits for
// stage s only.  LDS-DMA writes lane-linearly (lane i -> base + 16 i), so the XOR swizzle of
// chunk_off is applied to the SOURCE: lane i of 1-KiB piece p loads row 8p + i/8, chunk
// (i & 7) ^ swz(row).  The DMA primitives and the counted waits are in dl_attn_tile.h.
// Two stages: the next tile's DMA is issued at the top of the current tile and has a whole tile of
// MFMA / softmax work to land (4 stages measured 1.3% slower forward, 0.5% slower dQ at B=512:
// profiles/r5_attn_ring_depth_occupancy.jsonl).
constexpr int NBUF = 2;
constexpr int STAGE = 2 * TILE_BYTES + 512;

// ------------------------------------------------------------------------------------------ fwd
// Key masking comes in two forms.  kvinfo = int32[B + 1] (lengths of right-padded key masks plus a
// device-side "every mask is a prefix" flag in kvinfo[B], computed by the model without a host
// sync): then tiles past the batch's length are skipped and only the boundary tile is masked.
// Otherwise (or when kvinfo[B] == 0) the generic additive bias mbias[B, S] (log2 units) is used.
// Interior tiles run the lean softmax: one FMA (scale, -max) + exp2 + add per score, row max via
// max3, and the online-softmax rescale of O is deferred until a row's max grows by more than
// 2^RESCALE_THR (cdna_hip_programming.md T13: P <= 2^8 is exact enough in bf16 for P.V; the
// rescale decision precedes the tile's exponentiation, so nothing is ever scaled twice).
// RESCALE_THR, the XCD-aware block order (block_id), kv_end_of and the cross-half reductions are in
// dl_attn_tile.h.

// The K / V ring of the forward and dQ kernels: stage s is key tile s (K, V and, under a generic
// additive mask, its 64 bias floats mb_g[64 s ..]) in slot s % NBUF of smem.
struct KvRing {
  const bf16_t* Kg;
  const bf16_t* Vg;
  long ld;
  const float* mb_g;
  uint8_t* smem;
  int w, lane;
  __device__ __forceinline__ void issue(int s) const {
    uint8_t* slot = smem + (s % NBUF) * STAGE;
    dma_tile(Kg, ld, s * 64, slot, w, lane);
    dma_tile(Vg, ld, s * 64, slot + TILE_BYTES, w, lane);
    if (mb_g) dma_f32x64(mb_g + s * 64, slot + 2 * TILE_BYTES, lane);
  }
};

// Forward tile loop over key tiles [kt0, kt1) of nt; the ring's prologue has issued tile 0 (the
// first NBUF - 1 stages).
// LEAN: unmasked tiles — raw scores, the softmax scale rides in the exp FMA, no bias reads.
// !LEAN: s = s*sl2 + bias[key] with the bias staged in LDS (additive mask or 0/-1e30 from the
// key length).  The two instantiations run as consecutive loops (lean body, then the boundary
// tile), never in one loop body, so they do not add register pressure to each other.
template <bool LEAN>
__device__ __forceinline__ void fwd_tiles(const KvRing& c, int kv_end, float sl2, int kt0, int kt1, int nt,
                                          const bf16x8 (&qf)[QS][4], floatx16 (&o)[QS][2], float (&m)[QS],
                                          float (&l)[QS], int r, int hh, int lane) {
  for (int kt = kt0; kt < kt1; ++kt) {
    // stage kt landed (this wave) -> barrier: every wave's pieces landed and every wave is done
    // with slot (kt - 1) % NBUF, which the stage issued next overwrites
    wait_stages(min(nt - 1 - kt, NBUF - 2), c.mb_g != nullptr);
    __syncthreads();
    if (kt + NBUF - 1 < nt) c.issue(kt + NBUF - 1);
    const uint8_t* Ks = c.smem + (kt % NBUF) * STAGE;
    const float* mb = reinterpret_cast<const float*>(Ks + 2 * TILE_BYTES);
    const uint8_t* Vs = Ks + TILE_BYTES;
    floatx16 s[QS][2];
#pragma unroll
    for (int u = 0; u < QS; ++u)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[u][j][i] = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 kfr = lds_row_frag(Ks, 32 * j + r, 2 * ks + hh);
#pragma unroll
        for (int u = 0; u < QS; ++u) s[u][j] = mfma32(kfr, qf[u][ks], s[u][j]);
      }
#pragma unroll
    for (int u = 0; u < QS; ++u) {
      if (!LEAN) {
        if (c.mb_g) {
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) s[u][j][i] = fmaf(s[u][j][i], sl2, mb[32 * j + crow(i, hh)]);
        } else {  // stages carry the generic additive bias only; the length mask is computed here
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i)
              s[u][j][i] = fmaf(s[u][j][i], sl2, kt * 64 + 32 * j + crow(i, hh) < kv_end ? 0.f : NEG_BIG);
        }
      }
      // row max as four independent max3 chains of 8 scores (depth 6 instead of 16), then the halves
      float mc[4];
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const floatx16& sv = s[u][q4 >> 1];
        const int o8 = (q4 & 1) * 8;
        float v = vmax3(sv[o8], sv[o8 + 1], sv[o8 + 2]);
        v = vmax3(v, sv[o8 + 3], sv[o8 + 4]);
        v = vmax3(v, sv[o8 + 5], sv[o8 + 6]);
        mc[q4] = v;
      }
      float mx = vmax3(vmax3(mc[0], mc[1], s[u][0][7]), vmax3(mc[2], mc[3], s[u][0][15]),
                       vmax3(s[u][1][7], s[u][1][15], mc[0]));
      mx = half_max(mx);
      if (LEAN) mx *= sl2;
      const bool grow = mx > m[u] + RESCALE_THR;
      if (__ballot(grow) != 0) {  // rare after the first tile: rescale O and l to the new max
        const float mn = grow ? mx : m[u];
        const float alpha = __builtin_amdgcn_exp2f(m[u] - mn);
        l[u] *= alpha;
        m[u] = mn;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) o[u][t][i] *= alpha;
      }
      const float nm = -m[u];
      float rsa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // 8 independent add chains (latency bound)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float pv = __builtin_amdgcn_exp2f(LEAN ? fmaf(s[u][j][i], sl2, nm) : s[u][j][i] + nm);
          s[u][j][i] = pv;
          rsa[i & 7] += pv;
        }
      float rs = ((rsa[0] + rsa[1]) + (rsa[2] + rsa[3])) + ((rsa[4] + rsa[5]) + (rsa[6] + rsa[7]));
      l[u] += half_sum(rs);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        bf16x8 pb[QS];
#pragma unroll
        for (int u = 0; u < QS; ++u) pb[u] = pack_acc(s[u][j], ss);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 vfr = tr_operand(Vs, 32 * j + 16 * ss, hh, t, lane);
#pragma unroll
          for (int u = 0; u < QS; ++u) o[u][t] = mfma32(vfr, pb[u], o[u][t]);
        }
      }
  }
}

// Compact queries (CQ instantiations): the queries of sequence b are the first cnt[b] rows of its
// slot of Sq rows (Sq % 64 == 0, Sq <= S) in q [B*Sq, H*64]; out / dout / dq share that layout and
// row stride (ldo), lse / delta are [B, H, Sq].  Keys and values stay in the token buffer: the
// kernels' qkv argument then points at K's first column (V is H*64 columns further on), and dK / dV
// go to dkv [B*S, 2*H*64] (dK | dV, row stride lddkv).  Slot rows past cnt[b] are dead, as rows
// past S are to the other forms: clamped loads, nothing written to lse / delta, no part in dK / dV
// or the bias gradients.  Their out / dq rows are stored as zeros, not skipped: the compact buffers
// go on into GEMMs (weight gradients sum over their rows), where unwritten memory must not appear.
// The CQ instantiations take it as one more kernel argument (a parameter pack that is empty in the
// other instantiations, so those keep their argument layout and their code).
struct CompactQ {
  const bf16_t* q;
  bf16_t* dq;
  bf16_t* dkv;
  long lddkv;
  const int* cnt;
  int Sq;
};
struct NoCompactQ {};
template <bool CQ>
using CompactArg = std::conditional_t<CQ, CompactQ, NoCompactQ>;
__device__ __forceinline__ NoCompactQ compact_arg() { return {}; }
__device__ __forceinline__ const CompactQ& compact_arg(const CompactQ& cq) { return cq; }
// first lse / delta element of (sequence b, head h) for the query rows
template <bool VARLEN, bool CQ>
__device__ __forceinline__ long q_stat(const CompactArg<CQ>& cq, int b, int h, int H, int S, int T, long rb) {
  if constexpr (CQ) return ((long)b * H + h) * cq.Sq;
  else return seq_stat<VARLEN>(b, h, H, S, T, rb);
}
// first row of sequence b's queries / outputs, and head h's first query element
template <bool CQ>
__device__ __forceinline__ long q_first(const CompactArg<CQ>& cq, int b, long rb) {
  if constexpr (CQ) return (long)b * cq.Sq;
  else return rb;
}
template <bool CQ>
__device__ __forceinline__ const bf16_t* q_head(const CompactArg<CQ>& cq, const bf16_t* qkv, long ld, long ldo, long rb,
                                                 long qb, int h) {
  if constexpr (CQ) return cq.q + qb * ldo + h * 64;
  else return qkv + rb * ld + h * 64;
}
// 64 columns of up to blockDim.x rows of a [., ld] bf16 buffer <- 0, one row per thread
__device__ __forceinline__ void zero_rows64(bf16_t* g, long ld, int rows) {
  if ((int)threadIdx.x < rows) {
    uint4* p = reinterpret_cast<uint4*>(g + (long)threadIdx.x * ld);
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = make_uint4(0u, 0u, 0u, 0u);
  }
}
// live query rows of sequence b: the slot's count (CQ), else the sequence's rows
template <bool CQ>
__device__ __forceinline__ int q_rows(const CompactArg<CQ>& cq, int b, int S) {
  if constexpr (CQ) return max(1, min(cq.cnt[b], cq.Sq));
  else return S;
}

// Block = 4 waves x QS x 32 query rows of one (batch, head).
// VARLEN: the packed layout (seq_rows .. seq_stat in dl_attn_tile.h): kvinfo is seqinfo, S_ is T, the grid's x
// extent covers the largest slot and a block past its own slot leaves before any DMA or barrier.
template <bool VARLEN, typename... CQA>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(const bf16_t* __restrict__ qkv, long ld,
                                                          const float* __restrict__ mbias,
                                                          const int* __restrict__ kvinfo, bf16_t* __restrict__ out,
                                                          long ldo, float* __restrict__ lse, int B, int H, int S_,
                                                          float sl2, int xcd, CQA... cqa) {
  constexpr bool CQ = sizeof...(CQA) == 1;
  const CompactArg<CQ> cq = compact_arg(cqa...);
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * STAGE];
  const BlockId bid = block_id(xcd);
  const int b = bid.b, h = bid.h;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int S = seq_rows<VARLEN>(kvinfo, b, S_);
  const int nq = q_rows<CQ>(cq, b, S);
  if constexpr (VARLEN || CQ) {
    if (bid.x * (128 * QS) >= nq) {  // uniform over the block
      if constexpr (CQ) {  // a block of dead rows: zeros
        const int q0 = bid.x * (128 * QS);
        zero_rows64(out + ((long)b * cq.Sq + q0) * ldo + h * HD, ldo, cq.Sq - q0);
      }
      return;
    }
  }
  const long rb = seq_base<VARLEN>(kvinfo, b, S);
  const long qb = q_first<CQ>(cq, b, rb);
  const long ldq = CQ ? ldo : ld;
  const bf16_t* Qg = q_head<CQ>(cq, qkv, ld, ldo, rb, qb, h);
  const bf16_t* Kg = qkv + rb * ld + (CQ ? 0L : (long)H * HD) + h * HD;
  const bf16_t* Vg = qkv + rb * ld + (CQ ? (long)H * HD : 2L * H * HD) + h * HD;
  bool use_len;
  const int kv_end = seq_kv_end<VARLEN>(kvinfo, B, b, S, use_len);
  const int nt = (kv_end + 63) / 64;
  const KvRing ring{Kg, Vg, ld, (!use_len && mbias) ? mbias + rb : nullptr, smem, w, lane};
  for (int s0 = 0; s0 < NBUF - 1 && s0 < nt; ++s0) ring.issue(s0);
  int q[QS];
  bf16x8 qf[QS][4];
#pragma unroll
  for (int u = 0; u < QS; ++u) {
    q[u] = bid.x * (128 * QS) + w * (32 * QS) + 32 * u + r;
    const int qc = min(q[u], nq - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[u][ks] = gload8(Qg + (long)qc * ldq + ks * 16 + 8 * hh);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) settle(qf[u][ks]);
  }

  floatx16 o[QS][2];
  float m[QS], l[QS];
#pragma unroll
  for (int u = 0; u < QS; ++u) {
    m[u] = NEG_BIG;
    l[u] = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[u][t][i] = 0.f;
  }

  wait_vm_all();
  // lean tiles first (every tile when there is no mask), then the masked remainder: the boundary
  // tile of a length mask, or all tiles of a generic additive mask
  const int nlean = ring.mb_g ? 0 : kv_end / 64;
  fwd_tiles<true>(ring, kv_end, sl2, 0, nlean, nt, qf, o, m, l, r, hh, lane);
  fwd_tiles<false>(ring, kv_end, sl2, nlean, nt, nt, qf, o, m, l, r, hh, lane);

#pragma unroll
  for (int u = 0; u < QS; ++u) {
    const bool live = q[u] < nq;
    if constexpr (CQ)  // dead rows of the slot: zeros (o is finite there, it comes from a clamped live row)
      store_row64(out + (qb + q[u]) * ldo + h * HD, o[u], live ? 1.f / l[u] : 0.f, hh, q[u] < cq.Sq);
    else
      store_row64(out + (qb + q[u]) * ldo + h * HD, o[u], 1.f / l[u], hh, live);
    if (live && hh == 0) lse[q_stat<VARLEN, CQ>(cq, b, h, H, S, S_, rb) + q[u]] = m[u] + log2f(l[u]);
  }
}

// ------------------------------------------------------------------------------------------ bwd dq
// Also computes delta = rowsum(dO * O) for its queries and publishes it for the dkdv kernel.
template <bool VARLEN, typename... CQA>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(const bf16_t* __restrict__ qkv, long ld,
                                                             const float* __restrict__ mbias,
                                                             const int* __restrict__ kvinfo,
                                                             const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                                             long ldo, const float* __restrict__ lse,
                                                             float* __restrict__ delta, bf16_t* __restrict__ dqkv,
                                                             float* __restrict__ dbias, int B, int H, int S_, float sl2,
                                                             float scale, int xcd, CQA... cqa) {
  constexpr bool CQ = sizeof...(CQA) == 1;
  const CompactArg<CQ> cq = compact_arg(cqa...);
  // (the epilogue reuses the first 2 KiB for the waves' bias-gradient partials)
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * STAGE];
  const BlockId bid = block_id(xcd);
  const int b = bid.b, h = bid.h;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int S = seq_rows<VARLEN>(kvinfo, b, S_);
  const int nq = q_rows<CQ>(cq, b, S);
  if constexpr (VARLEN || CQ) {
    if (bid.x * (128 * QS) >= nq) {  // uniform over the block
      if constexpr (CQ) {  // a block of dead rows: zeros
        const int q0 = bid.x * (128 * QS);
        zero_rows64(cq.dq + ((long)b * cq.Sq + q0) * ldo + h * HD, ldo, cq.Sq - q0);
      }
      return;
    }
  }
  const long rb = seq_base<VARLEN>(kvinfo, b, S);
  const long qb = q_first<CQ>(cq, b, rb);
  const long ldq = CQ ? ldo : ld;
  const bf16_t* Qg = q_head<CQ>(cq, qkv, ld, ldo, rb, qb, h);
  const bf16_t* Kg = qkv + rb * ld + (CQ ? 0L : (long)H * HD) + h * HD;
  const bf16_t* Vg = qkv + rb * ld + (CQ ? (long)H * HD : 2L * H * HD) + h * HD;
  bool use_len;
  const int kv_end = seq_kv_end<VARLEN>(kvinfo, B, b, S, use_len);
  const float* mb_g = (!use_len && mbias) ? mbias + rb : nullptr;
  const int nt = (kv_end + 63) / 64;
  const KvRing ring{Kg, Vg, ld, mb_g, smem, w, lane};
  for (int s0 = 0; s0 < NBUF - 1 && s0 < nt; ++s0) ring.issue(s0);

  int q[QS];
  bf16x8 qf[QS][4], df[QS][4];
  float dl[QS], l2[QS];
#pragma unroll
  for (int u = 0; u < QS; ++u) {
    q[u] = bid.x * (128 * QS) + w * (32 * QS) + 32 * u + r;
    const int qc = min(q[u], nq - 1);
    dl[u] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[u][ks] = gload8(Qg + (long)qc * ldq + ks * 16 + 8 * hh);
      const long oo = (qb + qc) * ldo + h * HD + ks * 16 + 8 * hh;
      df[u][ks] = gload8(dout + oo);
      const bf16x8 of = gload8(out + oo);
#pragma unroll
      for (int e = 0; e < 8; ++e) dl[u] += (float)df[u][ks][e] * (float)of[e];
    }
    dl[u] += __shfl_xor(dl[u], 32, 64);
    l2[u] = lse[q_stat<VARLEN, CQ>(cq, b, h, H, S, S_, rb) + qc];
    settle(l2[u]);
    settle(dl[u]);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      settle(qf[u][ks]);
      settle(df[u][ks]);
    }
  }
  // (delta is stored after the tile loop: a store issued here would sit in the vmcnt queue ahead of
  // the ring's loads, and CDNA4 counts stores in vmcnt too)

  floatx16 dq[QS][2];
#pragma unroll
  for (int u = 0; u < QS; ++u)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) dq[u][t][i] = 0.f;

  wait_vm_all();

  // One tile body, two instantiations run as consecutive loops (as in the forward), so the masked
  // form adds no register pressure or branches to the lean one: LEAN for the unmasked tiles
  // [0, nlean), then the boundary tile of a length mask or every tile of a generic additive mask.
  // kt keeps counting across the hand-over, so the ring's slot parity (kt % NBUF) and the counted
  // waits (stages left = nt - 1 - kt) carry over for any nlean in [0, nt].
  auto tiles = [&](auto lean_tag, int kt0, int kt1) {
  constexpr bool LEAN = decltype(lean_tag)::value;
  // the masked form takes its lane coordinates from an opaque copy of the thread index, so its
  // per-lane LDS addresses and mask operands are formed after the lean loop, not carried through it
  int tm = threadIdx.x;
  if constexpr (!LEAN) settle(tm);
  const int lm = tm & 63, rm = tm & 31, hm = (tm >> 5) & 1;
  for (int kt = kt0; kt < kt1; ++kt) {
    wait_stages(min(nt - 1 - kt, NBUF - 2), mb_g != nullptr);
    __syncthreads();
    if (kt + NBUF - 1 < nt) ring.issue(kt + NBUF - 1);
    const uint8_t* Ks = smem + (kt % NBUF) * STAGE;
    const float* mb = reinterpret_cast<const float*>(Ks + 2 * TILE_BYTES);
    const uint8_t* Vs = Ks + TILE_BYTES;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      floatx16 st[QS], dp[QS];
#pragma unroll
      for (int u = 0; u < QS; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) { st[u][i] = 0.f; dp[u][i] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 kfr = lds_row_frag(Ks, 32 * j + rm, 2 * ks + hm);
        const bf16x8 vfr = lds_row_frag(Vs, 32 * j + rm, 2 * ks + hm);
#pragma unroll
        for (int u = 0; u < QS; ++u) {
          st[u] = mfma32(kfr, qf[u][ks], st[u]);
          dp[u] = mfma32(vfr, df[u][ks], dp[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < QS; ++u) {
        if constexpr (LEAN) {  // interior tile: no mask
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float p = __builtin_amdgcn_exp2f(fmaf(st[u][i], sl2, -l2[u]));
            st[u][i] = p * (dp[u][i] - dl[u]);
          }
        } else if (mb_g) {  // generic additive bias, staged with the tile
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float p = __builtin_amdgcn_exp2f(st[u][i] * sl2 + mb[32 * j + crow(i, hm)] - l2[u]);
            st[u][i] = p * (dp[u][i] - dl[u]);
          }
        } else {  // boundary tile of a length mask
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int key = kt * 64 + 32 * j + crow(i, hm);
            const float p = __builtin_amdgcn_exp2f(st[u][i] * sl2 + (key < kv_end ? 0.f : NEG_BIG) - l2[u]);
            st[u][i] = p * (dp[u][i] - dl[u]);
          }
        }
      }
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        bf16x8 pb[QS];
#pragma unroll
        for (int u = 0; u < QS; ++u) pb[u] = pack_acc(st[u], ss);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 ktr = tr_operand(Ks, 32 * j + 16 * ss, hm, t, lm);
#pragma unroll
          for (int u = 0; u < QS; ++u) dq[u][t] = mfma32(ktr, pb[u], dq[u][t]);
        }
      }
    }
  }
  };
  const int nlean = mb_g ? 0 : kv_end / 64;
  tiles(std::true_type{}, 0, nlean);
  tiles(std::false_type{}, nlean, nt);
  __syncthreads();  // every wave is done with the ring before the epilogue reuses it
  // The epilogue forms its lane coordinates again from the thread index, behind an opaque copy, so
  // that none of them stays live across the tile loops (the loops run at the 256-register limit).
  int tid = threadIdx.x;
  settle(tid);
  const int w_ = tid >> 6, r_ = tid & 31, hh_ = (tid >> 5) & 1;
  int qe[QS];
#pragma unroll
  for (int u = 0; u < QS; ++u) qe[u] = bid.x * (128 * QS) + w_ * (32 * QS) + 32 * u + r_;
#pragma unroll
  for (int u = 0; u < QS; ++u) {
    const bool live = qe[u] < nq;
    if (live && hh_ == 0) delta[q_stat<VARLEN, CQ>(cq, b, h, H, S, S_, rb) + qe[u]] = dl[u];
    if constexpr (CQ)  // dead rows of the slot: zeros
      store_row64(cq.dq + (qb + qe[u]) * ldo + h * HD, dq[u], live ? scale : 0.f, hh_, qe[u] < cq.Sq);
    else
      store_row64(dqkv + (rb + qe[u]) * ld + h * HD, dq[u], scale, hh_, live);
  }
  if (dbias) {
    // Fused bias gradient of the QKV projection (replaces a [T, 3H*64] column-sum pass):
    //   query bias: column sums of the dQ just stored (bf16-rounded, as stored);
    //   value bias: sum_k dV[k] = sum_q dO[q] (softmax rows sum to one), from the dO this block loaded;
    //   key bias:   sum_k dK[k] = 0 exactly (sum_k dS[q,k] = delta - delta), so nothing is added.
    // A lane holds 32 dQ and 32 dO columns of its query row(s), and the two half-waves hold
    // different columns.  So the sums over queries stay in registers: the QS sub-blocks are added
    // first (rows past S count as zero), then each value is summed over the 32 lanes of its
    // half-wave (half_wave_sum: DPP + row-pair swap, no LDS).  Lanes 0 and 32 of every wave put the
    // wave's 2 x 64 column sums in LDS, and after one barrier 128 threads add the four waves'
    // partials and issue one atomic per column.
    float* part = reinterpret_cast<float*>(smem);  // [4 waves][dQ 64 | dO 64]
    float cq[2][16], cd[4][8];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {  // dQ column 32 t + 8 (i >> 2) + 4 hh_ + (i & 3), as stored above
        float v = 0.f;
#pragma unroll
        for (int u = 0; u < QS; ++u) v += qe[u] < nq ? round_bf16(dq[u][t][i] * scale) : 0.f;
        cq[t][i] = half_wave_sum(v);
      }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) {  // dO column 16 ks + 8 hh_ + e, as loaded above
        float v = 0.f;
#pragma unroll
        for (int u = 0; u < QS; ++u) v += qe[u] < nq ? (float)df[u][ks][e] : 0.f;
        cd[ks][e] = half_wave_sum(v);
      }
    if (r_ == 0) {
      float* pw = part + w_ * 128;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v4 = 0; v4 < 4; ++v4)
          *reinterpret_cast<float4*>(pw + 32 * t + 8 * v4 + 4 * hh_) =
              float4{cq[t][4 * v4], cq[t][4 * v4 + 1], cq[t][4 * v4 + 2], cq[t][4 * v4 + 3]};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int g = 0; g < 2; ++g)
          *reinterpret_cast<float4*>(pw + 64 + 16 * ks + 8 * hh_ + 4 * g) =
              float4{cd[ks][4 * g], cd[ks][4 * g + 1], cd[ks][4 * g + 2], cd[ks][4 * g + 3]};
    }
    __syncthreads();
    if (threadIdx.x < 128) {
      const int c = threadIdx.x & 63, which = threadIdx.x >> 6;  // which: 0 query bias, 1 value bias
      const float* pc = part + which * 64 + c;
      atomicAdd(&dbias[(which ? 2L * H * HD : 0L) + h * HD + c], pc[0] + pc[128] + pc[256] + pc[384]);
    }
  }
}

// ------------------------------------------------------------------------------------------ bwd dkdv
// Block = 4 waves x 32 keys of one (batch, head); the ring stages the query tiles (Q, dO, lse, delta).
template <bool VARLEN, typename... CQA>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkdv_kernel(
    const bf16_t* __restrict__ qkv, long ld, const float* __restrict__ mbias, const int* __restrict__ kvinfo,
    const bf16_t* __restrict__ dout, long ldo, const float* __restrict__ lse, const float* __restrict__ delta,
    bf16_t* __restrict__ dqkv, int B, int H, int S_, float sl2, float scale, int xcd, CQA... cqa) {
  constexpr bool CQ = sizeof...(CQA) == 1;
  const CompactArg<CQ> cq = compact_arg(cqa...);
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * STAGE];
  const BlockId bid = block_id(xcd);
  const int b = bid.b, h = bid.h;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int S = seq_rows<VARLEN>(kvinfo, b, S_);
  if constexpr (VARLEN) {
    if (bid.x * 128 >= S) return;  // uniform over the block
  }
  const long rb = seq_base<VARLEN>(kvinfo, b, S);
  const int nq = q_rows<CQ>(cq, b, S);
  const long qb = q_first<CQ>(cq, b, rb);
  const long ldq = CQ ? ldo : ld;
  const bf16_t* Qg = q_head<CQ>(cq, qkv, ld, ldo, rb, qb, h);
  const bf16_t* Kg = qkv + rb * ld + (CQ ? 0L : (long)H * HD) + h * HD;
  const bf16_t* Vg = qkv + rb * ld + (CQ ? (long)H * HD : 2L * H * HD) + h * HD;
  const bf16_t* dOg = dout + qb * ldo + h * HD;
  const float* lse_g = lse + q_stat<VARLEN, CQ>(cq, b, h, H, S, S_, rb);
  const float* del_g = delta + q_stat<VARLEN, CQ>(cq, b, h, H, S, S_, rb);
  // dK / dV of this head go to thirds 2 and 3 of dqkv, or (CQ) to the two halves of cq.dkv
  bf16_t* dkv_g;
  long ldd;
  if constexpr (CQ) {
    dkv_g = cq.dkv - (long)H * HD;  // so that dK sits H*HD columns in, as in dqkv
    ldd = cq.lddkv;
  } else {
    dkv_g = dqkv;
    ldd = ld;
  }

  // This lane's key row.  It stays a one-element array, filled and read in one-trip `u` loops
  // where it forms addresses (here, the all-padding exit, the K / V row loads), and the score
  // MFMA pair of the tile loop keeps such a loop too: those are the places where the plain scalar
  // form compiles to other code (another association of the row's address sums, swapped operands
  // of one v_pk_mul_f32), and this kernel's code is held byte-identical across source clean-ups.
  int k[1];
#pragma unroll
  for (int u = 0; u < 1; ++u) k[u] = bid.x * 128 + w * 32 + 32 * u + r;
  bool use_len;
  const int kv_end = seq_kv_end<VARLEN>(kvinfo, B, b, S, use_len);
  if (use_len && bid.x * 128 >= kv_end) {  // every key of this block is padding: dK = dV = 0
#pragma unroll
    for (int u = 0; u < 1; ++u) {
      if (k[u] < S) {
        bf16_t* dkp = dkv_g + (rb + k[u]) * ldd + (long)H * HD + h * HD;
        bf16_t* dvp = dkv_g + (rb + k[u]) * ldd + 2L * H * HD + h * HD;
#pragma unroll
        for (int v = 0; v < 8; ++v) {  // the same 64 columns the regular epilogue covers (32t + 8v' + 4hh)
          store4(dkp + 8 * v + 4 * hh, 0.f, 0.f, 0.f, 0.f);
          store4(dvp + 8 * v + 4 * hh, 0.f, 0.f, 0.f, 0.f);
        }
      }
    }
    return;
  }
  // query tiles: all of the sequence's, or (CQ) the slot's tiles that hold a live row
  const int nt = CQ ? (nq + 63) / 64 : S / 64;
  auto issue = [&](int st) {  // query tile st -> slot st % NBUF; waves 0-1 fetch lse, 2-3 delta
    uint8_t* slot = smem + (st % NBUF) * STAGE;
    dma_tile(Qg, ldq, st * 64, slot, w, lane);
    dma_tile(dOg, ldo, st * 64, slot + TILE_BYTES, w, lane);
    dma_f32x64((w < 2 ? lse_g : del_g) + st * 64, slot + 2 * TILE_BYTES + (w < 2 ? 0 : 256), lane);
  };
  for (int s0 = 0; s0 < NBUF - 1 && s0 < nt; ++s0) issue(s0);
  bf16x8 kf[4], vf[4];
  float mbk;
#pragma unroll
  for (int u = 0; u < 1; ++u) {
    const int kc = min(k[u], S - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      kf[ks] = gload8(Kg + (long)kc * ld + ks * 16 + 8 * hh);
      vf[ks] = gload8(Vg + (long)kc * ld + ks * 16 + 8 * hh);
    }
    mbk = use_len ? (k[u] < kv_end ? 0.f : NEG_BIG) : (mbias ? mbias[rb + kc] : 0.f);
    settle(mbk);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      settle(kf[ks]);
      settle(vf[ks]);
    }
  }

  floatx16 dk[2], dv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
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
    wait_stages(min(nt - 1 - qt, NBUF - 2), true);
    __syncthreads();
    if (qt + NBUF - 1 < nt) issue(qt + NBUF - 1);
    const uint8_t* Qs = smem + (qt % NBUF) * STAGE;
    const float* lse_s = reinterpret_cast<const float*>(Qs + 2 * TILE_BYTES);
    const uint8_t* Ds = Qs + TILE_BYTES;
    const float* del_s = lse_s + 64;
    if constexpr (CQ) {
      // The slot's last live tile may end in dead rows, whose lse / delta were never written: give
      // them lse = +1e30 (P = exp2(s - 1e30) = 0, so dV and dS get nothing from them) and delta = 0.
      // The tile has landed and no later stage overwrites it (it is the loop's last).
      if (qt == nt - 1 && (nq & 63) != 0) {  // uniform over the block
        if (threadIdx.x < 64 && qt * 64 + (int)threadIdx.x >= nq) {
          const_cast<float*>(lse_s)[threadIdx.x] = -NEG_BIG;
          const_cast<float*>(del_s)[threadIdx.x] = 0.f;
        }
        __syncthreads();
      }
    }
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2) {
      floatx16 sc, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) { sc[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 qfr = lds_row_frag(Qs, 32 * i2 + r, 2 * ks + hh);
        const bf16x8 dfr = lds_row_frag(Ds, 32 * i2 + r, 2 * ks + hh);
#pragma unroll
        for (int u = 0; u < 1; ++u) {  // (one trip: see k above)
          sc = mfma32(qfr, kf[ks], sc);
          dp = mfma32(dfr, vf[ks], dp);
        }
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
        const bf16x8 pb = pack_acc(sc, ss), db = pack_acc(dp, ss);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 dtr = tr_operand(Ds, 32 * i2 + 16 * ss, hh, t, lane);
          const bf16x8 qtr = tr_operand(Qs, 32 * i2 + 16 * ss, hh, t, lane);
          dv[t] = mfma32(dtr, pb, dv[t]);
          dk[t] = mfma32(qtr, db, dk[t]);
        }
      }
    }
  }
  };
  if (use_len) {
    qloop(std::true_type{});
    if (k[0] >= kv_end)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) dk[t][i] = dv[t][i] = 0.f;
  } else {
    qloop(std::false_type{});
  }
  const bool live = k[0] < S;
  store_row64(dkv_g + (rb + k[0]) * ldd + (long)H * HD + h * HD, dk, scale, hh, live);
  store_row64(dkv_g + (rb + k[0]) * ldd + 2L * H * HD + h * HD, dv, 1.f, hh, live);
}

// Block order remapped so that the query blocks of one (batch, head) share an XCD's L2 (their K/V
// tiles are read by every one of them).
constexpr int kAttnXcd = 1;

}  // namespace

// The compact-query instantiations and their entry points are compiled in a translation unit of
// their own (attention_compact_q.hip, which includes this file for the kernel templates), so that
// this unit's code object holds exactly the kernels it held before, at the same addresses: moving a
// kernel inside its code object was measured to change output bits with unchanged assembly
// (tests/test_attention_varlen_gpu.py, packed against fixed-S).
// Read from the disassembly: in the lean forward loop the row maximum's first v_max3_f32 (vmax3,
// inline asm in dl_attn_tile.h) follows the last MFMA of the score chain it reads with no wait
// state between them, where an 8-pass MFMA's result needs 12 before a VALU reads it; the compiler
// pads no hazard for an instruction inside an asm statement (cdna_hip_programming.md 5.7 item 2).
// The maximum can so be taken from accumulator registers the MFMA has not written yet.  The result
// stays a valid softmax (the maximum is only the deferred-rescale reference point).  Supposed, not
// measured: that this is why bits move with a kernel's address and with a row's 32-row sub-block.
// docs/KERNELS.md ("Compact queries") has the listing; the pad is a change of its own, since it
// changes output bits.
#ifndef DL_ATTN_COMPACT_Q_UNIT

// This unit's kernels take the fused QKV buffer (no compact queries) at head_dim 64 with 16-byte
// aligned rows, and S % 64 == 0 or the packed layout (the callers validate what seqinfo holds:
// csrc/bindings.cpp)
static bool hd64_ok(const DlAttn& a) {
  if (a.q || a.D != HD || a.ld % 8 != 0 || a.ldo % 8 != 0) return false;
  if (!a.seqinfo) return a.S % 64 == 0;
  return a.B >= 1 && a.T % 64 == 0 && a.max_slot >= 64 && a.max_slot % 64 == 0 && a.max_slot <= a.T;
}

// All launch sites of one layout.  The kernels are emitted in the order of their first launch
// site, which is part of what the comment above protects: the fixed-S three (forward, dQ, dK/dV),
// then the packed three, as the entry points below instantiate this.  The packed kernels read no
// mbias, take seqinfo in kvinfo's place and T in S's, and the largest slot sizes their grids.
template <bool PACKED>
static int hd64_launch(const DlAttn& a, bool bwd, hipStream_t st) {
  if (!hd64_ok(a)) return -1;
  const float* mbias = PACKED ? nullptr : a.mbias;
  const int* info = PACKED ? a.seqinfo : a.kvinfo;
  const int S = PACKED ? a.T : a.S, rows = PACKED ? a.max_slot : a.S;
  const float sl2 = a.scale_log2();
  dim3 grid((rows + 255) / 256, a.H, a.B), grid_kv((rows + 127) / 128, a.H, a.B);
  if (!bwd) {
    attn_fwd_kernel<PACKED><<<grid, 256, 0, st>>>(a.kv, a.ld, mbias, info, a.out, a.ldo, a.lse, a.B, a.H, S, sl2,
                                                  kAttnXcd);
    return 0;
  }
  attn_bwd_dq_kernel<PACKED><<<grid, 256, 0, st>>>(a.kv, a.ld, mbias, info, a.out, a.dout, a.ldo, a.lse, a.delta,
                                                   a.dqkv, a.dbias, a.B, a.H, S, sl2, a.scale, kAttnXcd);
  attn_bwd_dkdv_kernel<PACKED><<<grid_kv, 256, 0, st>>>(a.kv, a.ld, mbias, info, a.dout, a.ldo, a.lse, a.delta, a.dqkv,
                                                        a.B, a.H, S, sl2, a.scale, kAttnXcd);
  return 0;
}

int dl_attn_hd64_fwd(const DlAttn& a, hipStream_t st) {
  return !a.seqinfo ? hd64_launch<false>(a, false, st) : hd64_launch<true>(a, false, st);
}

int dl_attn_hd64_bwd(const DlAttn& a, hipStream_t st) {
  return !a.seqinfo ? hd64_launch<false>(a, true, st) : hd64_launch<true>(a, true, st);
}

#else  // DL_ATTN_COMPACT_Q_UNIT

// Compact queries (struct CompactQ above, DlAttn's compact block): head_dim 64 and the fixed-S
// layout only; q / out rows of H*64 columns and key / value rows of 2*H*64, all 16-byte aligned
static bool hd64q_ok(const DlAttn& a) {
  return a.q && a.kv && a.qcnt && !a.seqinfo && a.B >= 1 && a.H >= 1 && a.D == HD && a.S % 64 == 0 &&
         a.Sq % 64 == 0 && a.Sq >= 64 && a.Sq <= a.S && a.ld % 8 == 0 && a.ld >= 2L * a.H * HD && a.ldo % 8 == 0 &&
         a.ldo >= (long)a.H * HD;
}

int dl_attn_hd64q_fwd(const DlAttn& a, hipStream_t st) {
  if (!hd64q_ok(a)) return -1;
  const CompactQ cq{a.q, nullptr, nullptr, 0, a.qcnt, a.Sq};
  dim3 grid((a.Sq + 255) / 256, a.H, a.B);
  attn_fwd_kernel<false, CompactQ><<<grid, 256, 0, st>>>(a.kv, a.ld, a.mbias, a.kvinfo, a.out, a.ldo, a.lse, a.B, a.H,
                                                         a.S, a.scale_log2(), kAttnXcd, cq);
  return 0;
}

int dl_attn_hd64q_bwd(const DlAttn& a, hipStream_t st) {
  if (!hd64q_ok(a) || !a.dq || !a.dkv) return -1;
  const float sl2 = a.scale_log2();
  const CompactQ cq{a.q, a.dq, a.dkv, 2L * a.H * HD, a.qcnt, a.Sq};
  dim3 grid_dq((a.Sq + 255) / 256, a.H, a.B), grid_kv((a.S + 127) / 128, a.H, a.B);
  attn_bwd_dq_kernel<false, CompactQ><<<grid_dq, 256, 0, st>>>(a.kv, a.ld, a.mbias, a.kvinfo, a.out, a.dout, a.ldo,
                                                               a.lse, a.delta, nullptr, a.dbias, a.B, a.H, a.S, sl2,
                                                               a.scale, kAttnXcd, cq);
  attn_bwd_dkdv_kernel<false, CompactQ><<<grid_kv, 256, 0, st>>>(a.kv, a.ld, a.mbias, a.kvinfo, a.dout, a.ldo, a.lse,
                                                                 a.delta, nullptr, a.B, a.H, a.S, sl2, a.scale,
                                                                 kAttnXcd, cq);
  return 0;
}

#endif  // DL_ATTN_COMPACT_Q_UNIT
