// Fused MLM head: the tied decoder GEMM logits = t W^T + bias and the token cross-entropy over
// them, forward and backward, without the [M, V] logits (or their gradient) ever reaching memory.
//
//   t [M, 128] bf16   the head's LayerNorm output          labels int64 [M] (ignore_index: dead row)
//   w [V, 128] bf16   the word embeddings (tied decoder)   bias [V] bf16 or fp32
//
// It is the head_dim-128 flash attention (attention_hd128.hip) with "keys = vocabulary rows": one
// operand's fragments stay in registers, 64-row blocks of the other stream through a two-slot
// LDS-DMA ring as the two swizzled 64x64 tiles of dl_attn_tile.h, scores come out of
// v_mfma_f32_32x32x16_bf16 with one row of the register operand per lane, and the softmax runs in
// log2 units.  Three kernels, split as the attention forward, dQ and dK/dV are:
//
//   fwd    token on the lane.  A wave holds TWO 32-token sub-blocks of t (64 VGPRs): there is no
//          output accumulator, and every w fragment read from LDS then feeds two MFMAs.  Running
//          max / sum per lane, halves combined by v_permlane32_swap, the target logit picked up in
//          the tile that holds the label.  Writes lse (log2 units) and the per-row loss.
//   eval   the forward's split swept twice in one launch, forward only: per-row loss and the
//          label's rank among the fp32 scores (see the kernel).  One or two sub-blocks per wave.
//   bwd dt token on the lane, one sub-block per wave: t 32 + dt 64 + scores 32 registers.
//          P = exp2(s + bias - lse) is recomputed, dS = (P - onehot) g / count is packed to bf16
//          and dt += dS W accumulates from transposed reads of the same w tiles.
//   bwd dw vocabulary on the lane.  A workgroup owns 64 vocabulary rows: waves 0/1 and 2/3 hold the
//          two 32-row sub-blocks of w, and of every streamed 64-token block waves 0-1 take the
//          first 32 tokens, waves 2-3 the other 32.  dW^T += t^T dS (64 registers) and dbias from
//          the same dS; the two token halves meet in LDS in a fixed order, then the owning wave
//          ADDS into the fp32 gradient rows with plain loads and stores (no atomics).
//
// Tails.  The bias goes through a small preparation kernel into fp32 log2 units, padded to whole
// tiles with -1e30: a vocabulary row past V - 1 is loaded as row V - 1 and its score is masked by
// its bias.  Token rows past M - 1 are loaded as row M - 1, stored nowhere and counted nowhere
// (scale 0, lse +1e30 in the backward's per-row table).
// The mean is taken by one block in a fixed order: no float atomics anywhere in this file.
//
// fwd, eval and bwd dt also exist in a form that splits the vocabulary across workgroups, for calls
// whose row blocks alone leave compute units idle ("vocabulary split" below; dl_mlm_xent_splits
// chooses).  One slice runs exactly the kernels described above.
#include "dl_attn_tile.h"
#include "dl_common.h"
#include "dl_kernels.h"

namespace {

constexpr int E = 128;  // embedding size: a 64-row block is two 64x64 tiles
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
constexpr int NBUF = 2;                           // ring slots
constexpr int W_STAGE = 2 * TILE_BYTES + 256;     // fwd, dt: [w dims 0-63 | w dims 64-127 | 64 bias]
constexpr int T_STAGE = 2 * TILE_BYTES + 768;     // dw: [t dims 0-63 | t dims 64-127 | lse | scale | label]
constexpr int FWD_ROWS = 256, DT_ROWS = 128, DW_ROWS = 64;  // rows a workgroup owns
constexpr int EVAL_SMALL_M = 256 * 256;  // eval: up to here 256-row blocks are fewer than the 256 compute units

// dma_tile with the source row clamped to n - 1 (the last tile of a tail re-reads the last row)
__device__ __forceinline__ void dma_tile_clamp(const bf16_t* g, long ld, int row0, int n, uint8_t* tile, int w,
                                               int lane) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = w + 4 * j;
    const int row = 8 * p + (lane >> 3);
    const int c = (lane & 7) ^ swzf((row >> 1) & 7);
    dma16(g + (long)min(row0 + row, n - 1) * ld + c * 8, lds_u32(tile + p * 1024));
  }
}
// the two 64x64 tiles of the 64-row x 128-column block starting at row row0 of an n-row matrix
__device__ __forceinline__ void dma_block(const bf16_t* g, long ld, int row0, int n, uint8_t* tiles, int w, int lane) {
  if (row0 + 64 <= n) {
    dma_tile(g, ld, row0, tiles, w, lane);
    dma_tile(g + 64, ld, row0, tiles + TILE_BYTES, w, lane);
  } else {
    dma_tile_clamp(g, ld, row0, n, tiles, w, lane);
    dma_tile_clamp(g + 64, ld, row0, n, tiles + TILE_BYTES, w, lane);
  }
}
// row fragment ks (0..7) of a block: columns 16 ks + 8 hh .. +7 of row `row`
__device__ __forceinline__ bf16x8 block_row_frag(const uint8_t* tiles, int row, int ks, int hh) {
  return lds_row_frag(tiles + (ks >> 2) * TILE_BYTES, row, 2 * (ks & 3) + hh);
}
// transposed operand for column block t (0..3: columns 32 t .. 32 t + 31)
__device__ __forceinline__ bf16x8 block_tr(const uint8_t* tiles, int kbase, int hh, int t, int lane) {
  return tr_operand(tiles + (t >> 1) * TILE_BYTES, kbase, hh, t & 1, lane);
}
// this lane's fragments of row `row`: columns 16 ks + 8 hh .. +7
__device__ __forceinline__ void load_row_frags(const bf16_t* g, long ld, int row, int hh, bf16x8 (&f)[8]) {
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) f[ks] = gload8(g + (long)row * ld + ks * 16 + 8 * hh);
}
__device__ __forceinline__ float max16(const floatx16& x) {
  float v = vmax3(x[0], x[1], x[2]);
  v = vmax3(v, x[3], x[4]);
  v = vmax3(v, x[5], x[6]);
  v = vmax3(v, x[7], x[8]);
  v = vmax3(v, x[9], x[10]);
  v = vmax3(v, x[11], x[12]);
  v = vmax3(v, x[13], x[14]);
  return vmax3(v, x[15], x[15]);
}
__device__ __forceinline__ void zero(floatx16& x) {
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = 0.f;
}
__device__ __forceinline__ void ring_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---------------------------------------------------------------------------------- preparation
// out[i] = bias[i] * log2(e) for i < V, -1e30 up to the next multiple of 64; NATURAL: a second
// array out[Vp + i] = bias[i] with the same padding (the evaluation's rank sweep compares in the
// logits' own units)
template <bool NATURAL = false>
__global__ void mlm_bias_kernel(const void* __restrict__ bias, int bias_bf16, float* __restrict__ out, int V, int Vp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Vp) return;
  if constexpr (NATURAL) {
    const float b = i < V ? (bias_bf16 ? bf2f(static_cast<const bf16_t*>(bias)[i]) : static_cast<const float*>(bias)[i])
                          : NEG_BIG;
    out[i] = i < V ? b * LOG2E : NEG_BIG;
    out[Vp + i] = b;
  } else {
    float b = NEG_BIG;
    if (i < V) b = (bias_bf16 ? bf2f(static_cast<const bf16_t*>(bias)[i]) : static_cast<const float*>(bias)[i]) * LOG2E;
    out[i] = b;
  }
}

__device__ __forceinline__ float live_rows(const long* __restrict__ labels, int M, int ignore_index, float* scratch) {
  float c = 0.f;
  for (int i = threadIdx.x; i < M; i += blockDim.x) c += labels[i] != ignore_index ? 1.f : 0.f;
  return block_sum(c, scratch);
}

// loss = sum of the per-row losses / live rows (0 without a live row), one block, fixed order
__global__ __launch_bounds__(1024) void mlm_loss_kernel(const float* __restrict__ row_loss,
                                                         const long* __restrict__ labels, int M, int ignore_index,
                                                         float* __restrict__ loss) {
  __shared__ float scratch[16];
  const float c = live_rows(labels, M, ignore_index, scratch);
  float s = 0.f;
  for (int i = threadIdx.x; i < M; i += blockDim.x) s += row_loss[i];
  s = block_sum(s, scratch);
  if (threadIdx.x == 0) loss[0] = c > 0.f ? s / c : 0.f;
}

// The backward's per-row table, three arrays of Mp = M rounded up to 64: lse (+1e30 past M - 1),
// scale = gloss / live rows on live rows and 0 elsewhere, label as int32 (-1 on dead rows).
__global__ __launch_bounds__(1024) void mlm_rows_kernel(const float* __restrict__ lse, const long* __restrict__ labels,
                                                         const float* __restrict__ gloss, int M, int Mp,
                                                         int ignore_index, float* __restrict__ info) {
  __shared__ float scratch[16];
  const float c = live_rows(labels, M, ignore_index, scratch);
  const float scale = c > 0.f ? gloss[0] / c : 0.f;
  int* lab = reinterpret_cast<int*>(info + 2 * (long)Mp);
  for (int i = threadIdx.x; i < Mp; i += blockDim.x) {
    const bool live = i < M && labels[i] != ignore_index;
    info[i] = i < M ? lse[i] : -NEG_BIG;
    info[Mp + i] = live ? scale : 0.f;
    lab[i] = live ? (int)labels[i] : -1;
  }
}

// ------------------------------------------------------------------------------------------ fwd
__global__ __launch_bounds__(256, 2) void mlm_xent_fwd_kernel(const bf16_t* __restrict__ t, long ldt,
                                                               const bf16_t* __restrict__ w, long ldw,
                                                               const float* __restrict__ biasl2,
                                                               const long* __restrict__ labels, float* __restrict__ lse,
                                                               float* __restrict__ row_loss, int M, int V,
                                                               int ignore_index) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * W_STAGE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int nt = (V + 63) / 64;
  auto issue = [&](int vt) {  // vocabulary tile vt -> slot vt % NBUF
    uint8_t* slot = smem + (vt % NBUF) * W_STAGE;
    dma_block(w, ldw, vt * 64, V, slot, wv, lane);
    dma_f32x64(biasl2 + vt * 64, slot + 2 * TILE_BYTES, lane);
  };
  issue(0);

  const int row0 = blockIdx.x * FWD_ROWS + wv * 64 + r;
  bf16x8 tf[2][8];
  int lab[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = row0 + 32 * u;
    const int rc = min(row, M - 1);
    load_row_frags(t, ldt, rc, hh, tf[u]);
    const long l = labels[rc];
    lab[u] = (row < M && l != ignore_index) ? (int)l : -1;
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    settle(lab[u]);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) settle(tf[u][ks]);
  }
  float m[2] = {NEG_BIG, NEG_BIG}, l[2] = {0.f, 0.f}, xl[2] = {0.f, 0.f};

  wait_vm_all();
  for (int vt = 0; vt < nt; ++vt) {
    // stage vt landed (this wave) -> barrier: every wave's pieces landed and every wave is done
    // with the other slot, which the stage issued next overwrites
    ring_wait();
    __syncthreads();
    if (vt + 1 < nt) issue(vt + 1);
    const uint8_t* Ws = smem + (vt % NBUF) * W_STAGE;
    const float* bs = reinterpret_cast<const float*>(Ws + 2 * TILE_BYTES);
    floatx16 s[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 2; ++j) zero(s[u][j]);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const bf16x8 a = block_row_frag(Ws, 32 * j + r, ks, hh);
        s[0][j] = mfma32(a, tf[0][ks], s[0][j]);
        s[1][j] = mfma32(a, tf[1][ks], s[1][j]);
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[u][j][i] = fmaf(s[u][j][i], LOG2E, bs[32 * j + crow(i, hh)]);
      const int d = lab[u] - vt * 64;  // the label's row in this tile
      if (__ballot((unsigned)d < 64u) != 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (32 * j + crow(i, hh) == d) xl[u] = s[u][j][i];
      }
      const float mx = half_max(vmax3(max16(s[u][0]), max16(s[u][1]), m[u]));
      const float nm = -mx;
      float rsa[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) rsa[i & 3] += __builtin_amdgcn_exp2f(s[u][j][i] + nm);
      l[u] = fmaf(l[u], __builtin_amdgcn_exp2f(m[u] + nm), half_sum((rsa[0] + rsa[1]) + (rsa[2] + rsa[3])));
      m[u] = mx;
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = row0 + 32 * u;
    const float target = half_sum(xl[u]);  // one half found it, the other holds 0
    const float l2 = m[u] + log2f(l[u]);
    if (row < M && hh == 0) {
      lse[row] = l2;
      row_loss[row] = lab[u] >= 0 ? (l2 - target) * LN2 : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------ eval
// The forward's split (token on the lane, U sub-blocks per wave, 128 U rows per workgroup) swept
// twice over the vocabulary in one launch.  Sweep 1 is the forward with one difference: the label's
// RAW accumulator is picked up, so that afterwards both its log2 score (for the loss, the forward's
// arithmetic) and its natural score sy = acc + bias (for the rank) follow from it.  Sweep 2 restarts
// the ring at vocabulary row 0, now staging the natural bias, with the t fragments still in
// registers, and counts per lane the columns that beat the label: s_j > sy, or s_j == sy and j < y.
// The recomputed accumulators carry the bits sweep 1 saw, so ties are exact.
//
// Per score the count is one add, one compare and one add-with-carry-in: the tie rule is folded
// into the threshold.  In a tile that lies wholly below the label's column every tie counts, and
// s >= sy is s > lo with lo the next float below sy (fp32 denormals are not flushed in this file's
// kernels: .amdhsa_float_denorm_mode_32 3); in a tile wholly above it the threshold is sy.  Each lane
// selects its own once per tile; only the tile that holds a label of the wave selects per column.
// The vocabulary tail's -1e30 bias keeps its columns below every threshold.

// the largest float below x (x finite)
__device__ __forceinline__ float next_below(float x) {
  const uint32_t b = __float_as_uint(x);
  return __uint_as_float(x > 0.f ? b - 1u : (x < 0.f ? b + 1u : 0x80000001u));
}
__device__ __forceinline__ int half_sum_int(int x) {
  const auto r = __builtin_amdgcn_permlane32_swap((uint32_t)x, (uint32_t)x, false, false);
  return (int)(r[0] + r[1]);
}
// raw scores of the staged 64 vocabulary rows against this wave's U t sub-blocks
template <int U>
__device__ __forceinline__ void tile_scores(const uint8_t* Ws, const bf16x8 (&tf)[U][8], int r, int hh,
                                            floatx16 (&s)[U][2]) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int j = 0; j < 2; ++j) zero(s[u][j]);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const bf16x8 a = block_row_frag(Ws, 32 * j + r, ks, hh);
#pragma unroll
      for (int u = 0; u < U; ++u) s[u][j] = mfma32(a, tf[u][ks], s[u][j]);
    }
}

// bias2 = [log2-unit bias | natural bias], Vp floats each.  row_loss 0 / row_rank -1 on an ignored
// row; a label outside [0, V) that is not ignore_index is never used as an index: (NaN, -1).
template <int U>
__global__ __launch_bounds__(256, 2) void mlm_xent_eval_kernel(const bf16_t* __restrict__ t, long ldt,
                                                                const bf16_t* __restrict__ w, long ldw,
                                                                const float* __restrict__ bias2, int Vp,
                                                                const long* __restrict__ labels,
                                                                float* __restrict__ row_loss, int* __restrict__ row_rank,
                                                                int M, int V, int ignore_index) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * W_STAGE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int nt = (V + 63) / 64;
  auto issue = [&](int vt, const float* bias) {  // vocabulary tile vt -> slot vt % NBUF
    uint8_t* slot = smem + (vt % NBUF) * W_STAGE;
    dma_block(w, ldw, vt * 64, V, slot, wv, lane);
    dma_f32x64(bias + vt * 64, slot + 2 * TILE_BYTES, lane);
  };
  issue(0, bias2);

  const int row0 = blockIdx.x * (128 * U) + wv * (32 * U) + r;
  bf16x8 tf[U][8];
  int lab[U];
  bool bad[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int row = row0 + 32 * u;
    const int rc = min(row, M - 1);
    load_row_frags(t, ldt, rc, hh, tf[u]);
    const long l = labels[rc];
    const bool in = l >= 0 && l < V;
    lab[u] = (row < M && l != ignore_index && in) ? (int)l : -1;
    bad[u] = l != ignore_index && !in;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    settle(lab[u]);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) settle(tf[u][ks]);
  }
  float m[U], l[U], xa[U];
#pragma unroll
  for (int u = 0; u < U; ++u) m[u] = NEG_BIG, l[u] = 0.f, xa[u] = 0.f;

  // ---- sweep 1: running max / sum and the label's raw accumulator
  wait_vm_all();
  for (int vt = 0; vt < nt; ++vt) {
    ring_wait();
    __syncthreads();
    if (vt + 1 < nt) issue(vt + 1, bias2);
    const uint8_t* Ws = smem + (vt % NBUF) * W_STAGE;
    const float* bs = reinterpret_cast<const float*>(Ws + 2 * TILE_BYTES);
    floatx16 s[U][2];
    tile_scores<U>(Ws, tf, r, hh, s);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int d = lab[u] - vt * 64;  // the label's row in this tile
      if (__ballot((unsigned)d < 64u) != 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (32 * j + crow(i, hh) == d) xa[u] = s[u][j][i];
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[u][j][i] = fmaf(s[u][j][i], LOG2E, bs[32 * j + crow(i, hh)]);
      const float mx = half_max(vmax3(max16(s[u][0]), max16(s[u][1]), m[u]));
      const float nm = -mx;
      float rsa[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) rsa[i & 3] += __builtin_amdgcn_exp2f(s[u][j][i] + nm);
      l[u] = fmaf(l[u], __builtin_amdgcn_exp2f(m[u] + nm), half_sum((rsa[0] + rsa[1]) + (rsa[2] + rsa[3])));
      m[u] = mx;
    }
  }

  // ---- between the sweeps: both halves of a row learn the label's scores
  float loss[U], sy[U], lo[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float acc = half_sum(xa[u]);  // one half found it, the other holds 0
    const int li = max(lab[u], 0);
    const float l2 = m[u] + log2f(l[u]);
    loss[u] = lab[u] >= 0 ? (l2 - fmaf(acc, LOG2E, bias2[li])) * LN2 : (bad[u] ? __builtin_nanf("") : 0.f);
    sy[u] = acc + bias2[Vp + li];
    lo[u] = next_below(sy[u]);
    settle(loss[u]);
    settle(sy[u]);
    settle(lo[u]);
  }
  wait_vm_all();
  __syncthreads();  // every wave is done with sweep 1's last slot before tile 0 lands on slot 0 again
  const float* biasn = bias2 + Vp;
  issue(0, biasn);

  // ---- sweep 2: count the columns that beat the label
  int cnt[U];
#pragma unroll
  for (int u = 0; u < U; ++u) cnt[u] = 0;
  for (int vt = 0; vt < nt; ++vt) {
    ring_wait();
    __syncthreads();
    if (vt + 1 < nt) issue(vt + 1, biasn);
    const uint8_t* Ws = smem + (vt % NBUF) * W_STAGE;
    const float* bs = reinterpret_cast<const float*>(Ws + 2 * TILE_BYTES);
    floatx16 s[U][2];
    tile_scores<U>(Ws, tf, r, hh, s);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int d = lab[u] - vt * 64;
      int c4[4] = {0, 0, 0, 0};
      if (__ballot((unsigned)d < 64u) == 0) {  // no label of this wave's rows in the tile
        const float thr = d >= 64 ? lo[u] : sy[u];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 16; ++i) c4[i & 3] += s[u][j][i] + bs[32 * j + crow(i, hh)] > thr ? 1 : 0;
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int col = 32 * j + crow(i, hh);
            c4[i & 3] += s[u][j][i] + bs[col] > (col < d ? lo[u] : sy[u]) ? 1 : 0;
          }
      }
      cnt[u] += (c4[0] + c4[1]) + (c4[2] + c4[3]);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int row = row0 + 32 * u;
    const int rank = half_sum_int(cnt[u]);
    if (row < M && hh == 0) {
      row_loss[row] = loss[u];
      row_rank[row] = lab[u] >= 0 ? rank : -1;
    }
  }
}

// ------------------------------------------------------------------------------------------ bwd dt
__global__ __launch_bounds__(256, 2) void mlm_xent_bwd_dt_kernel(const bf16_t* __restrict__ t, long ldt,
                                                                  const bf16_t* __restrict__ w, long ldw,
                                                                  const float* __restrict__ biasl2,
                                                                  const float* __restrict__ info, int Mp,
                                                                  bf16_t* __restrict__ dt, long lddt, int M, int V) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * W_STAGE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int nt = (V + 63) / 64;
  auto issue = [&](int vt) {
    uint8_t* slot = smem + (vt % NBUF) * W_STAGE;
    dma_block(w, ldw, vt * 64, V, slot, wv, lane);
    dma_f32x64(biasl2 + vt * 64, slot + 2 * TILE_BYTES, lane);
  };
  issue(0);

  const int row = blockIdx.x * DT_ROWS + wv * 32 + r;
  const int rc = min(row, M - 1);
  bf16x8 tf[8];
  load_row_frags(t, ldt, rc, hh, tf);
  float l2 = info[rc];
  float gs = row < M ? info[Mp + rc] : 0.f;
  int lab = row < M ? reinterpret_cast<const int*>(info)[2 * (long)Mp + rc] : -1;
  settle(l2);
  settle(gs);
  settle(lab);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) settle(tf[ks]);
  floatx16 o[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) zero(o[c]);

  wait_vm_all();
  for (int vt = 0; vt < nt; ++vt) {
    ring_wait();
    __syncthreads();
    if (vt + 1 < nt) issue(vt + 1);
    const uint8_t* Ws = smem + (vt % NBUF) * W_STAGE;
    const float* bs = reinterpret_cast<const float*>(Ws + 2 * TILE_BYTES);
    floatx16 s[2];
    zero(s[0]);
    zero(s[1]);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) s[j] = mfma32(block_row_frag(Ws, 32 * j + r, ks, hh), tf[ks], s[j]);
    const int d = lab - vt * 64;
    if (__ballot((unsigned)d < 64u) == 0) {  // no label of this wave's rows in the tile: dS = P g / count
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          s[j][i] = __builtin_amdgcn_exp2f(fmaf(s[j][i], LOG2E, bs[32 * j + crow(i, hh)] - l2)) * gs;
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[j][i], LOG2E, bs[32 * j + crow(i, hh)] - l2));
          s[j][i] = (p - (32 * j + crow(i, hh) == d ? 1.f : 0.f)) * gs;
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        const bf16x8 pb = pack_acc(s[j], ss);
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = mfma32(block_tr(Ws, 32 * j + 16 * ss, hh, c, lane), pb, o[c]);
      }
  }
  if (row < M) {
    bf16_t* op = dt + (long)row * lddt;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        store4(op + 32 * c + 8 * v + 4 * hh, o[c][4 * v], o[c][4 * v + 1], o[c][4 * v + 2], o[c][4 * v + 3]);
  }
}

// ------------------------------------------------------------------------------- vocabulary split
// The kernels above give a workgroup a block of token rows and the whole vocabulary, so a call with
// few rows runs on a handful of compute units for as long as one workgroup needs for all of V.  The
// split forms below partition the vocabulary instead (the flash-decoding split): the grid is
// (128-row blocks, slices), slice s of n owns the whole 64-row tiles [s nt / n, (s + 1) nt / n) of
// the nt = ceil(V / 64), and every workgroup is the one-sub-block-per-wave form (token on the lane,
// t fragments in registers, the same two-slot ring) swept over its slice alone.  What a row needs
// from all of V goes through a workspace and a small streaming kernel, slice by slice in a fixed
// order: no atomics, and a call repeated gives the same bits.
//
//   part    a slice's running max m and sum l (log2 units) and the label's RAW accumulator, 0 in
//           every slice but the one that holds the label, so the sum over slices is exact.
//           Workspace part[3][n][Mp]: the merge's lanes read consecutive rows of one slice.
//   merge   mx = max_s m_s, lse = mx + log2(sum_s l_s 2^(m_s - mx)); the label's log2 score is the
//           forward's fmaf(acc, log2 e, bias) and the row loss follows as in the forward.  For the
//           evaluation it also writes the label's natural score sy = acc + bias.
//   rank    the evaluation's second sweep over a slice, against sy: the tile-below / tile-above /
//           own-tile thresholds of mlm_xent_eval_kernel work on the global tile index, so they hold
//           across slices as they are.  Integer counts cnt[n][Mp], summed by mlm_xent_count_kernel.
//   dt      mlm_xent_bwd_dt_kernel over a slice; the fp32 partial goes to slab[n][Mp][128] and
//           mlm_xent_dt_reduce_kernel adds the slabs in slice order and rounds to bf16 once.
constexpr int SPLIT_ROWS = 128;  // rows a workgroup of the split forms owns

__device__ __forceinline__ int slice_tile(int s, int n, int nt) { return (int)((long)s * nt / n); }

__global__ __launch_bounds__(256, 2) void mlm_xent_part_kernel(const bf16_t* __restrict__ t, long ldt,
                                                                const bf16_t* __restrict__ w, long ldw,
                                                                const float* __restrict__ biasl2,
                                                                const long* __restrict__ labels, float* __restrict__ part,
                                                                int Mp, int M, int V, int ignore_index) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * W_STAGE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int nt = (V + 63) / 64, ns = gridDim.y, sl = blockIdx.y;
  const int vt0 = slice_tile(sl, ns, nt), vt1 = slice_tile(sl + 1, ns, nt);
  auto issue = [&](int vt) {  // vocabulary tile vt -> slot vt % NBUF
    uint8_t* slot = smem + (vt % NBUF) * W_STAGE;
    dma_block(w, ldw, vt * 64, V, slot, wv, lane);
    dma_f32x64(biasl2 + vt * 64, slot + 2 * TILE_BYTES, lane);
  };
  issue(vt0);

  const int row = blockIdx.x * SPLIT_ROWS + wv * 32 + r;
  const int rc = min(row, M - 1);
  bf16x8 tf[1][8];
  load_row_frags(t, ldt, rc, hh, tf[0]);
  const long lb = labels[rc];
  int lab = (row < M && lb != ignore_index && lb >= 0 && lb < V) ? (int)lb : -1;
  settle(lab);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) settle(tf[0][ks]);
  float m = NEG_BIG, l = 0.f, xa = 0.f;

  wait_vm_all();
  for (int vt = vt0; vt < vt1; ++vt) {
    ring_wait();
    __syncthreads();
    if (vt + 1 < vt1) issue(vt + 1);
    const uint8_t* Ws = smem + (vt % NBUF) * W_STAGE;
    const float* bs = reinterpret_cast<const float*>(Ws + 2 * TILE_BYTES);
    floatx16 s[1][2];
    tile_scores<1>(Ws, tf, r, hh, s);
    const int d = lab - vt * 64;  // the label's row in this tile
    if (__ballot((unsigned)d < 64u) != 0) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (32 * j + crow(i, hh) == d) xa = s[0][j][i];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) s[0][j][i] = fmaf(s[0][j][i], LOG2E, bs[32 * j + crow(i, hh)]);
    const float mx = half_max(vmax3(max16(s[0][0]), max16(s[0][1]), m));
    const float nm = -mx;
    float rsa[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) rsa[i & 3] += __builtin_amdgcn_exp2f(s[0][j][i] + nm);
    l = fmaf(l, __builtin_amdgcn_exp2f(m + nm), half_sum((rsa[0] + rsa[1]) + (rsa[2] + rsa[3])));
    m = mx;
  }
  const float acc = half_sum(xa);  // one half found it (in one slice), the other holds 0
  if (row < M && hh == 0) {
    float* p = part + (long)sl * Mp + row;
    p[0] = m;
    p[(long)ns * Mp] = l;
    p[2L * ns * Mp] = acc;
  }
}

// bias2 = [log2-unit bias | natural bias (sy != nullptr only)], Vp floats each.  lse and sy may be
// nullptr.  As in the evaluation kernel, a label outside [0, V) that is not ignore_index is never
// used as an index: its row's loss is NaN.
__global__ __launch_bounds__(256) void mlm_xent_merge_kernel(const float* __restrict__ part, int ns, int Mp,
                                                              const float* __restrict__ bias2, int Vp,
                                                              const long* __restrict__ labels, float* __restrict__ lse,
                                                              float* __restrict__ row_loss, float* __restrict__ sy, int M,
                                                              int V, int ignore_index) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= M) return;
  const float* pm = part + row;
  const float* pl = pm + (long)ns * Mp;
  const float* pa = pl + (long)ns * Mp;
  float mx = NEG_BIG;
  for (int s = 0; s < ns; ++s) mx = fmaxf(mx, pm[(long)s * Mp]);
  float l = 0.f, acc = 0.f;
  for (int s = 0; s < ns; ++s) {
    l = fmaf(pl[(long)s * Mp], __builtin_amdgcn_exp2f(pm[(long)s * Mp] - mx), l);
    acc += pa[(long)s * Mp];
  }
  const float l2 = mx + log2f(l);
  const long lb = labels[row];
  const bool in = lb >= 0 && lb < V;
  const long li = in ? lb : 0;
  if (lse) lse[row] = l2;
  row_loss[row] = lb == ignore_index ? 0.f : (in ? (l2 - fmaf(acc, LOG2E, bias2[li])) * LN2 : __builtin_nanf(""));
  if (sy) sy[row] = acc + bias2[Vp + li];
}

__global__ __launch_bounds__(256, 2) void mlm_xent_rank_kernel(const bf16_t* __restrict__ t, long ldt,
                                                                const bf16_t* __restrict__ w, long ldw,
                                                                const float* __restrict__ biasn,
                                                                const long* __restrict__ labels,
                                                                const float* __restrict__ sy_ws, int* __restrict__ cnt_ws,
                                                                int Mp, int M, int V, int ignore_index) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * W_STAGE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int nt = (V + 63) / 64, ns = gridDim.y, sl = blockIdx.y;
  const int vt0 = slice_tile(sl, ns, nt), vt1 = slice_tile(sl + 1, ns, nt);
  auto issue = [&](int vt) {
    uint8_t* slot = smem + (vt % NBUF) * W_STAGE;
    dma_block(w, ldw, vt * 64, V, slot, wv, lane);
    dma_f32x64(biasn + vt * 64, slot + 2 * TILE_BYTES, lane);
  };
  issue(vt0);

  const int row = blockIdx.x * SPLIT_ROWS + wv * 32 + r;
  const int rc = min(row, M - 1);
  bf16x8 tf[1][8];
  load_row_frags(t, ldt, rc, hh, tf[0]);
  const long lb = labels[rc];
  int lab = (row < M && lb != ignore_index && lb >= 0 && lb < V) ? (int)lb : -1;
  float sy = sy_ws[rc];
  float lo = next_below(sy);
  settle(lab);
  settle(sy);
  settle(lo);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) settle(tf[0][ks]);
  int cnt = 0;

  wait_vm_all();
  for (int vt = vt0; vt < vt1; ++vt) {
    ring_wait();
    __syncthreads();
    if (vt + 1 < vt1) issue(vt + 1);
    const uint8_t* Ws = smem + (vt % NBUF) * W_STAGE;
    const float* bs = reinterpret_cast<const float*>(Ws + 2 * TILE_BYTES);
    floatx16 s[1][2];
    tile_scores<1>(Ws, tf, r, hh, s);
    const int d = lab - vt * 64;
    int c4[4] = {0, 0, 0, 0};
    if (__ballot((unsigned)d < 64u) == 0) {  // no label of this wave's rows in the tile
      const float thr = d >= 64 ? lo : sy;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) c4[i & 3] += s[0][j][i] + bs[32 * j + crow(i, hh)] > thr ? 1 : 0;
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int col = 32 * j + crow(i, hh);
          c4[i & 3] += s[0][j][i] + bs[col] > (col < d ? lo : sy) ? 1 : 0;
        }
    }
    cnt += (c4[0] + c4[1]) + (c4[2] + c4[3]);
  }
  const int total = half_sum_int(cnt);
  if (row < M && hh == 0) cnt_ws[(long)sl * Mp + row] = total;
}

__global__ __launch_bounds__(256) void mlm_xent_count_kernel(const int* __restrict__ cnt_ws, int ns, int Mp,
                                                              const long* __restrict__ labels,
                                                              int* __restrict__ row_rank, int M, int V,
                                                              int ignore_index) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= M) return;
  int c = 0;
  for (int s = 0; s < ns; ++s) c += cnt_ws[(long)s * Mp + row];
  const long lb = labels[row];
  row_rank[row] = (lb != ignore_index && lb >= 0 && lb < V) ? c : -1;
}

__global__ __launch_bounds__(256, 2) void mlm_xent_bwd_dt_part_kernel(const bf16_t* __restrict__ t, long ldt,
                                                                       const bf16_t* __restrict__ w, long ldw,
                                                                       const float* __restrict__ biasl2,
                                                                       const float* __restrict__ info, int Mp,
                                                                       float* __restrict__ slab, int M, int V) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * W_STAGE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int nt = (V + 63) / 64, ns = gridDim.y, sl = blockIdx.y;
  const int vt0 = slice_tile(sl, ns, nt), vt1 = slice_tile(sl + 1, ns, nt);
  auto issue = [&](int vt) {
    uint8_t* slot = smem + (vt % NBUF) * W_STAGE;
    dma_block(w, ldw, vt * 64, V, slot, wv, lane);
    dma_f32x64(biasl2 + vt * 64, slot + 2 * TILE_BYTES, lane);
  };
  issue(vt0);

  const int row = blockIdx.x * SPLIT_ROWS + wv * 32 + r;
  const int rc = min(row, M - 1);
  bf16x8 tf[8];
  load_row_frags(t, ldt, rc, hh, tf);
  float l2 = info[rc];
  float gs = row < M ? info[Mp + rc] : 0.f;
  int lab = row < M ? reinterpret_cast<const int*>(info)[2 * (long)Mp + rc] : -1;
  settle(l2);
  settle(gs);
  settle(lab);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) settle(tf[ks]);
  floatx16 o[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) zero(o[c]);

  wait_vm_all();
  for (int vt = vt0; vt < vt1; ++vt) {
    ring_wait();
    __syncthreads();
    if (vt + 1 < vt1) issue(vt + 1);
    const uint8_t* Ws = smem + (vt % NBUF) * W_STAGE;
    const float* bs = reinterpret_cast<const float*>(Ws + 2 * TILE_BYTES);
    floatx16 s[2];
    zero(s[0]);
    zero(s[1]);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) s[j] = mfma32(block_row_frag(Ws, 32 * j + r, ks, hh), tf[ks], s[j]);
    const int d = lab - vt * 64;
    if (__ballot((unsigned)d < 64u) == 0) {  // no label of this wave's rows in the tile: dS = P g / count
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          s[j][i] = __builtin_amdgcn_exp2f(fmaf(s[j][i], LOG2E, bs[32 * j + crow(i, hh)] - l2)) * gs;
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[j][i], LOG2E, bs[32 * j + crow(i, hh)] - l2));
          s[j][i] = (p - (32 * j + crow(i, hh) == d ? 1.f : 0.f)) * gs;
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        const bf16x8 pb = pack_acc(s[j], ss);
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = mfma32(block_tr(Ws, 32 * j + 16 * ss, hh, c, lane), pb, o[c]);
      }
  }
  if (row < M) {
    float* op = slab + ((long)sl * Mp + row) * E;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        *reinterpret_cast<float4*>(op + 32 * c + 8 * v + 4 * hh) =
            make_float4(o[c][4 * v], o[c][4 * v + 1], o[c][4 * v + 2], o[c][4 * v + 3]);
  }
}

// dt[row] = bf16(sum over slices, in slice order, of slab[s][row]): a thread takes 8 columns of a
// row (two 16-byte loads per slice, one 16-byte store), so a wave reads 2 KiB in a row per slice
__global__ __launch_bounds__(256) void mlm_xent_dt_reduce_kernel(const float* __restrict__ slab, int ns, int Mp,
                                                                  bf16_t* __restrict__ dt, long lddt, int M) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long row = i >> 4;
  const int c8 = (int)(i & 15) * 8;
  if (row >= M) return;
  const float4* p = reinterpret_cast<const float4*>(slab + row * E + c8);
  float4 a = p[0], b = p[1];
  for (int s = 1; s < ns; ++s) {
    const float4* q = p + (long)s * Mp * (E / 4);
    const float4 x = q[0], y = q[1];
    a.x += x.x, a.y += x.y, a.z += x.z, a.w += x.w;
    b.x += y.x, b.y += y.y, b.z += y.z, b.w += y.w;
  }
  const uint2 lo = pack4(a.x, a.y, a.z, a.w), hi = pack4(b.x, b.y, b.z, b.w);
  *reinterpret_cast<uint4*>(dt + row * lddt + c8) = make_uint4(lo.x, lo.y, hi.x, hi.y);
}

// ------------------------------------------------------------------------------------------ bwd dw
__global__ __launch_bounds__(256, 2) void mlm_xent_bwd_dw_kernel(const bf16_t* __restrict__ t, long ldt,
                                                                  const bf16_t* __restrict__ w, long ldw,
                                                                  const float* __restrict__ biasl2,
                                                                  const float* __restrict__ info, int Mp,
                                                                  float* __restrict__ gw, float* __restrict__ gb, int M,
                                                                  int V) {
  // the epilogue reuses the ring for the second token half's partial sums (2 x 65 x 64 floats)
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * T_STAGE];
  static_assert(2 * 65 * 64 * 4 <= NBUF * T_STAGE, "partial sums must fit in the ring");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int vs = wv & 1, i2 = wv >> 1;  // vocabulary sub-block, token half of every tile
  const int nt = Mp / 64;
  auto issue = [&](int qt) {  // token tile qt -> slot qt % NBUF; waves 0..2 fetch lse, scale, label
    uint8_t* slot = smem + (qt % NBUF) * T_STAGE;
    dma_block(t, ldt, qt * 64, M, slot, wv, lane);
    if (wv < 3) dma_f32x64(info + (long)wv * Mp + qt * 64, slot + 2 * TILE_BYTES + wv * 256, lane);
  };
  issue(0);

  const int vbase = blockIdx.x * DW_ROWS + 32 * vs;
  const int v = vbase + r;
  bf16x8 wf[8];
  load_row_frags(w, ldw, min(v, V - 1), hh, wf);
  float bl = biasl2[v];  // padded to whole tiles: -1e30 past V - 1
  settle(bl);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) settle(wf[ks]);
  floatx16 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) zero(acc[c]);
  float db = 0.f;

  wait_vm_all();
  for (int qt = 0; qt < nt; ++qt) {
    ring_wait();
    __syncthreads();
    if (qt + 1 < nt) issue(qt + 1);
    const uint8_t* Ts = smem + (qt % NBUF) * T_STAGE;
    const float* lse_s = reinterpret_cast<const float*>(Ts + 2 * TILE_BYTES) + 32 * i2;
    const float* gs_s = lse_s + 64;
    const int* lab_s = reinterpret_cast<const int*>(lse_s + 128);
    floatx16 sc;
    zero(sc);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) sc = mfma32(block_row_frag(Ts, 32 * i2 + r, ks, hh), wf[ks], sc);
    if (__ballot((unsigned)(lab_s[r] - vbase) < 32u) == 0) {  // no label among this wave's vocabulary rows
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int tok = crow(i, hh);
        sc[i] = __builtin_amdgcn_exp2f(fmaf(sc[i], LOG2E, bl - lse_s[tok])) * gs_s[tok];
        db += sc[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int tok = crow(i, hh);
        const float p = __builtin_amdgcn_exp2f(fmaf(sc[i], LOG2E, bl - lse_s[tok]));
        sc[i] = (p - (lab_s[tok] == v ? 1.f : 0.f)) * gs_s[tok];
        db += sc[i];
      }
    }
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      const bf16x8 pb = pack_acc(sc, ss);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = mfma32(block_tr(Ts, 32 * i2 + 16 * ss, hh, c, lane), pb, acc[c]);
    }
  }
  db = half_sum(db);
  __syncthreads();  // every wave is done with the ring before the epilogue reuses it
  float* red = reinterpret_cast<float*>(smem) + vs * 65 * 64 + lane;  // [vs][65 values][64 lanes]
  if (i2 == 1) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) red[(16 * c + i) * 64] = acc[c][i];
    red[64 * 64] = db;
  }
  __syncthreads();
  if (i2 == 0 && v < V) {
    float* gp = gw + (long)v * E;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int q = 0; q < 4; ++q) {  // columns 32 c + 8 q + 4 hh + (0..3) of vocabulary row v
        float4* p = reinterpret_cast<float4*>(gp + 32 * c + 8 * q + 4 * hh);
        float4 g = *p;
        g.x += acc[c][4 * q] + red[(16 * c + 4 * q) * 64];
        g.y += acc[c][4 * q + 1] + red[(16 * c + 4 * q + 1) * 64];
        g.z += acc[c][4 * q + 2] + red[(16 * c + 4 * q + 2) * 64];
        g.w += acc[c][4 * q + 3] + red[(16 * c + 4 * q + 3) * 64];
        *p = g;
      }
    if (hh == 0) gb[v] += db + red[64 * 64];
  }
}

}  // namespace

// What the kernels need: the embedding size they are written for and 16-byte aligned rows.
static bool mlm_xent_ok(const DlMlmXent& a) {
  return a.E == E && a.M >= 0 && a.V >= 1 && a.ldt % 8 == 0 && a.ldw % 8 == 0 && a.lddt % 8 == 0 &&
         (uintptr_t)a.t % 16 == 0 && (uintptr_t)a.w % 16 == 0 && (uintptr_t)a.dt % 16 == 0 && (uintptr_t)a.gw % 16 == 0;
}

static void mlm_bias(const DlMlmXent& a, hipStream_t st) {
  const int Vp = (a.V + 63) / 64 * 64;
  mlm_bias_kernel<><<<(Vp + 255) / 256, 256, 0, st>>>(a.bias, a.bias_bf16, a.bias_ws, a.V, Vp);
}

// The number of vocabulary slices a call runs with: `splits` > 0 forces it (clamped to the tiles of
// V and the grid's y limit), 0 chooses, from the sweeps of forced counts in
// profiles/mlm_head_split.jsonl (V = 30000, M = 308 .. 157696, 256 compute units):
//   - the split forms make ceil(M / 128) row blocks, and slices are added while the grid still fits
//     SPLIT_FILL workgroups per compute unit, one resident wave of workgroups: at 39 row blocks 13
//     slices (507 workgroups) take 291 us forward + backward, 16 slices 319 us, 8 slices 351 us;
//   - a slice keeps at least SPLIT_MIN_TILES tiles, a workgroup's fixed cost (its t fragments, the
//     ring's first stage, its workspace rows): at 10 row blocks 29 slices take 167 us, 58 take 189 us.
//     A vocabulary of fewer than 128 SPLIT_MIN_TILES rows is therefore never split;
//   - with more row blocks than that fill leaves SPLIT_MANY slices for, SPLIT_MANY slices still even
//     out the last wave of workgroups (M = 39424: 1.91 ms against 2.50 ms unsplit; 8 slices 1.86 ms).
//     That held up to the largest M measured, 157696 (7.7 ms against 8.1 ms); past
//     SPLIT_MANY_BLOCKS row blocks per compute unit nothing was measured, the dt slabs pass half a
//     gigabyte, and the call stays unsplit.
// -1: a negative `splits`.
constexpr int SPLIT_FILL = 2, SPLIT_MIN_TILES = 16, SPLIT_MANY = 4, SPLIT_MANY_BLOCKS = 8;
int dl_mlm_xent_splits(int M, int V, int splits, int compute_units) {
  const int nt = (V + 63) / 64;
  if (splits < 0) return -1;
  if (splits > 0) return std::min(splits, std::min(nt, 65535));
  const int rb = std::max((M + SPLIT_ROWS - 1) / SPLIT_ROWS, 1);
  int n = SPLIT_FILL * compute_units / rb;
  if (n < SPLIT_MANY) n = rb <= SPLIT_MANY_BLOCKS * compute_units ? SPLIT_MANY : 1;
  return std::max(1, std::min(n, nt / SPLIT_MIN_TILES));
}

// slices of this call (1: the unsplit kernels), 0 when the workspace a split needs is missing
static int mlm_slices(const DlMlmXent& a, const void* ws) {
  const int n = a.M > 0 ? dl_mlm_xent_splits(a.M, a.V, std::max(a.splits, 1), 0) : 1;
  return n > 1 && ws == nullptr ? 0 : n;
}

int dl_mlm_xent_fwd(const DlMlmXent& a, hipStream_t st) {
  const int n = mlm_slices(a, a.part_ws);
  if (!mlm_xent_ok(a) || n == 0) return -1;
  if (a.M > 0) {
    mlm_bias(a, st);
    if (n == 1) {
      mlm_xent_fwd_kernel<<<(a.M + FWD_ROWS - 1) / FWD_ROWS, 256, 0, st>>>(a.t, a.ldt, a.w, a.ldw, a.bias_ws, a.labels,
                                                                           a.lse, a.row_loss, a.M, a.V, a.ignore_index);
    } else {
      const int Mp = (a.M + 63) / 64 * 64;
      mlm_xent_part_kernel<<<dim3((a.M + SPLIT_ROWS - 1) / SPLIT_ROWS, n), 256, 0, st>>>(
          a.t, a.ldt, a.w, a.ldw, a.bias_ws, a.labels, a.part_ws, Mp, a.M, a.V, a.ignore_index);
      mlm_xent_merge_kernel<<<(a.M + 255) / 256, 256, 0, st>>>(a.part_ws, n, Mp, a.bias_ws, 0, a.labels, a.lse,
                                                               a.row_loss, nullptr, a.M, a.V, a.ignore_index);
    }
  }
  mlm_loss_kernel<<<1, 1024, 0, st>>>(a.row_loss, a.labels, a.M, a.ignore_index, a.loss);
  return 0;
}

int dl_mlm_xent_eval(const DlMlmXent& a, hipStream_t st) {
  const int n = mlm_slices(a, a.part_ws);
  if (!mlm_xent_ok(a) || n == 0) return -1;
  if (a.M == 0) return 0;
  const int Vp = (a.V + 63) / 64 * 64;
  mlm_bias_kernel<true><<<(Vp + 255) / 256, 256, 0, st>>>(a.bias, a.bias_bf16, a.bias_ws, a.V, Vp);
  if (n > 1) {  // two launches: the rank sweep needs the label's score, which another slice may hold
    const int Mp = (a.M + 63) / 64 * 64;
    const dim3 grid((a.M + SPLIT_ROWS - 1) / SPLIT_ROWS, n);
    float* sy = a.part_ws + 3L * n * Mp;
    int* cnt = reinterpret_cast<int*>(sy + Mp);
    mlm_xent_part_kernel<<<grid, 256, 0, st>>>(a.t, a.ldt, a.w, a.ldw, a.bias_ws, a.labels, a.part_ws, Mp, a.M, a.V,
                                               a.ignore_index);
    mlm_xent_merge_kernel<<<(a.M + 255) / 256, 256, 0, st>>>(a.part_ws, n, Mp, a.bias_ws, Vp, a.labels, nullptr,
                                                             a.row_loss, sy, a.M, a.V, a.ignore_index);
    mlm_xent_rank_kernel<<<grid, 256, 0, st>>>(a.t, a.ldt, a.w, a.ldw, a.bias_ws + Vp, a.labels, sy, cnt, Mp, a.M, a.V,
                                               a.ignore_index);
    mlm_xent_count_kernel<<<(a.M + 255) / 256, 256, 0, st>>>(cnt, n, Mp, a.labels, a.row_rank, a.M, a.V, a.ignore_index);
    return 0;
  }
  // A workgroup walks the whole vocabulary twice, so the call takes as long as one workgroup does:
  // while 256-row blocks would leave compute units idle, 128-row blocks (one sub-block per wave)
  // halve the work per tile and double the workgroups
  if (a.M <= EVAL_SMALL_M)
    mlm_xent_eval_kernel<1><<<(a.M + 127) / 128, 256, 0, st>>>(a.t, a.ldt, a.w, a.ldw, a.bias_ws, Vp, a.labels, a.row_loss,
                                                              a.row_rank, a.M, a.V, a.ignore_index);
  else
    mlm_xent_eval_kernel<2><<<(a.M + 255) / 256, 256, 0, st>>>(a.t, a.ldt, a.w, a.ldw, a.bias_ws, Vp, a.labels, a.row_loss,
                                                              a.row_rank, a.M, a.V, a.ignore_index);
  return 0;
}

int dl_mlm_xent_bwd(const DlMlmXent& a, hipStream_t st) {
  const int n = mlm_slices(a, a.dt_ws);
  if (!mlm_xent_ok(a) || n == 0 || (a.gw == nullptr) != (a.gb == nullptr)) return -1;
  if (a.M == 0) return 0;
  const int Mp = (a.M + 63) / 64 * 64;
  mlm_bias(a, st);
  mlm_rows_kernel<<<1, 1024, 0, st>>>(a.lse, a.labels, a.gloss, a.M, Mp, a.ignore_index, a.row_ws);
  if (n == 1) {
    mlm_xent_bwd_dt_kernel<<<(a.M + DT_ROWS - 1) / DT_ROWS, 256, 0, st>>>(a.t, a.ldt, a.w, a.ldw, a.bias_ws, a.row_ws,
                                                                          Mp, a.dt, a.lddt, a.M, a.V);
  } else {
    mlm_xent_bwd_dt_part_kernel<<<dim3((a.M + SPLIT_ROWS - 1) / SPLIT_ROWS, n), 256, 0, st>>>(
        a.t, a.ldt, a.w, a.ldw, a.bias_ws, a.row_ws, Mp, a.dt_ws, a.M, a.V);
    mlm_xent_dt_reduce_kernel<<<(a.M + 15) / 16, 256, 0, st>>>(a.dt_ws, n, Mp, a.dt, a.lddt, a.M);
  }
  if (a.gw)
    mlm_xent_bwd_dw_kernel<<<(a.V + DW_ROWS - 1) / DW_ROWS, 256, 0, st>>>(a.t, a.ldt, a.w, a.ldw, a.bias_ws, a.row_ws,
                                                                          Mp, a.gw, a.gb, a.M, a.V);
  return 0;
}
