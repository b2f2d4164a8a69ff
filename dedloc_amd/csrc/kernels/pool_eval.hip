// Evaluation pools: the strided, padded, overlapping average pool of the five-head linear evaluation
// (reference vissl/models/heads/linear_eval_mlp.py: AvgPool2d(k, stride, pad) -> BatchNorm2d ->
// flatten -> Linear on conv1 / res2 .. res5) over channels-last bf16 activations, with the train-mode
// BatchNorm's statistics taken in the same pass.
//
//   avgpool_stats : y[n,oh,ow,c] = (1 / k^2) sum_{i,j < k} x[n, oh*s - p + i, ow*s - p + j, c]
//                   (torch AvgPool2d defaults: padded taps are zero and count in the divisor, floor
//                   output size), y stored fp32; part[g, 0, c] = sum y, part[g, 1, c] = sum y^2 over
//                   the workgroup's outputs
//   stats_reduce  : sums[0, c] / sums[1, c] = the partials added up in one fixed order (the [2C]
//                   statistics layout of batchnorm.hip)
//   bn_f32        : f = (y - mean) gamma rstd + beta, bf16, from fp32 y and those sums; mean / rstd
//                   saved, running statistics updated as batchnorm.hip's forward does (evaluation
//                   form: the running statistics as they are); bn_f32_bwd: dgamma / dbeta from dy and
//                   the fp32 y, added up in a fixed order.  y stays fp32
//                   up to here because a pooled channel's batch spread can be a small fraction of
//                   its mean (late, post-ReLU stages; small batches): a bf16 y would lose 2^-9 |y|
//                   before the mean is taken off, which is then divided by that small spread.
//
// Work split.  A workgroup owns one image x one slab of 64 channels x one strip of output rows; a
// thread owns 8 consecutive channels (one 16-byte vector): cv = tid & 7, and the 32 pixel lanes
// pl = tid >> 3 walk the pixels.  The pool is separable and every input element is loaded once:
//   phase 1  a batch of RB input rows goes HBM -> LDS as raw bf16 vectors, all loads of a thread's
//            share issued before the first LDS store (up to 8 in flight per thread);
//   phase 2  thread (ow, cv) forms the row sum over its window's columns from LDS, once per input
//            row, and adds it to the fp32 column accumulators acc[oh, ow, :] (LDS) of the output
//            rows whose window holds that input row (ceil(k / s) of them at most).  An accumulator
//            is only ever touched by its one owner thread, rows in ascending order: no atomics, and
//            the same bits on every launch.  OW is 2 to 12 at the default taps, so only 16 to 96 of
//            the 256 threads work here; sharing a window's columns among the idle pixel lanes
//            (strided columns, per-lane accumulators added up in the epilogue) was built and
//            measured slower on four of the five taps (docs/KERNELS.md), so it is not kept.
// One image is one strip whenever images x slabs already fill the machine (every default tap at an
// evaluation batch except conv1, whose windows do not overlap, k = s); else the output rows are cut
// into strips, and two neighbouring strips both load the k - s input rows their windows share.
// The epilogue scales by 1 / k^2, stores y, and reduces the statistics over the 32 pixel lanes in
// lane order through LDS.  No MFMA: the kernel moves bytes.
#include <algorithm>

#include "dl_common.h"
#include "dl_kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSlab = 64;             // channels per workgroup: 8 lanes x 8 channels = 128-byte rows
constexpr int kRowBytes = 32 * 1024;  // LDS for the staged input rows
constexpr int kAccBytes = 24 * 1024;  // LDS for the column accumulators
constexpr int kMaxRows = 8;           // input rows per batch at most
constexpr int kFill = 512;            // workgroups wanted before an image is kept as one strip

struct PoolArgs {
  int H, W, C, OH, OW, k, s, p;
  int Wuse;   // input columns some window covers
  int OHs;    // output rows per strip
  int RB;     // input rows per batch
  float inv;  // 1 / k^2
};

__device__ __forceinline__ void unpack_add(const uint4& u, float* a) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[2 * j] += __uint_as_float(w[j] << 16);
    a[2 * j + 1] += __uint_as_float(w[j] & 0xffff0000u);
  }
}

__global__ __launch_bounds__(kThreads) void avgpool_stats_kernel(const bf16_t* __restrict__ x, float* __restrict__ y,
                                                                 float* __restrict__ part, const PoolArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* rows = reinterpret_cast<uint4*>(smem);                             // [RB][Wuse][8] bf16x8
  float* acc = reinterpret_cast<float*>(smem + (size_t)a.RB * a.Wuse * 128);  // [OHs][OW][64]
  const int tid = threadIdx.x, cv = tid & 7, pl = tid >> 3;
  const int c0 = blockIdx.x * kSlab + cv * 8;
  const bool live = c0 < a.C;  // the last slab's tail lanes (C % 64 != 0) hold zeros throughout
  const int strip = blockIdx.y, n = blockIdx.z;
  const int oh0 = strip * a.OHs, oh1 = min(a.OH, oh0 + a.OHs);
  const int h_lo = max(0, oh0 * a.s - a.p), h_hi = min(a.H, (oh1 - 1) * a.s - a.p + a.k);

  for (int i = tid; i < (oh1 - oh0) * a.OW * (kSlab / 4); i += kThreads)
    reinterpret_cast<float4*>(acc)[i] = float4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  const bf16_t* xn = x + (long)n * a.H * a.W * a.C + c0;
  for (int hb = h_lo; hb < h_hi; hb += a.RB) {
    const int nr = min(a.RB, h_hi - hb);
    const int npix = nr * a.Wuse;
    __syncthreads();  // the previous batch's readers are done (first pass: the accumulators are zeroed)
    for (int base = pl; base < npix; base += 32 * 8) {
      uint4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int pi = base + 32 * u;
        v[u] = uint4{0u, 0u, 0u, 0u};
        if (live && pi < npix) {
          const int r = pi / a.Wuse, w = pi - r * a.Wuse;
          v[u] = *reinterpret_cast<const uint4*>(xn + ((long)(hb + r) * a.W + w) * a.C);
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int pi = base + 32 * u;
        if (pi < npix) rows[pi * 8 + cv] = v[u];
      }
    }
    __syncthreads();
    for (int ow = pl; ow < a.OW; ow += 32) {
      const int w0 = max(0, ow * a.s - a.p), w1 = min(a.W, ow * a.s - a.p + a.k);
      for (int r = 0; r < nr; ++r) {
        const int hp = hb + r + a.p;  // the row's index in the padded image
        // output rows oh with oh*s <= hp < oh*s + k, inside this strip
        const int ohA = max(oh0, hp - a.k + 1 <= 0 ? 0 : (hp - a.k + a.s) / a.s), ohB = min(oh1 - 1, hp / a.s);
        if (ohA > ohB) continue;  // a row no window of this strip covers (k < s)
        float rs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int w = w0; w < w1; ++w) unpack_add(rows[(r * a.Wuse + w) * 8 + cv], rs);
        for (int oh = ohA; oh <= ohB; ++oh) {
          float4* t = reinterpret_cast<float4*>(acc + ((long)(oh - oh0) * a.OW + ow) * kSlab + cv * 8);
          float4 t0 = t[0], t1 = t[1];
          t0.x += rs[0]; t0.y += rs[1]; t0.z += rs[2]; t0.w += rs[3];
          t1.x += rs[4]; t1.y += rs[5]; t1.z += rs[6]; t1.w += rs[7];
          t[0] = t0;
          t[1] = t1;
        }
      }
    }
  }

  // epilogue: every thread reads only accumulators it wrote itself
  float s1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, s2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int oh = oh0; oh < oh1; ++oh)
    for (int ow = pl; ow < a.OW; ow += 32) {
      const float* t = acc + ((long)(oh - oh0) * a.OW + ow) * kSlab + cv * 8;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[j] = t[j] * a.inv;
        s1[j] += v[j];
        s2[j] = fmaf(v[j], v[j], s2[j]);
      }
      if (live) {
        float4* o = reinterpret_cast<float4*>(y + (((long)n * a.OH + oh) * a.OW + ow) * a.C + c0);
        o[0] = float4{v[0], v[1], v[2], v[3]};
        o[1] = float4{v[4], v[5], v[6], v[7]};
      }
    }
  __syncthreads();  // the staged rows are dead: their LDS carries the statistics, [32 lanes][2][64]
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[(pl * 2 + 0) * kSlab + cv * 8 + j] = s1[j];
    red[(pl * 2 + 1) * kSlab + cv * 8 + j] = s2[j];
  }
  __syncthreads();
  if (tid < 2 * kSlab) {
    const int which = tid >> 6, c = tid & 63;
    float t = 0.f;
    for (int l = 0; l < 32; ++l) t += red[(l * 2 + which) * kSlab + c];
    const int ch = blockIdx.x * kSlab + c;
    const long g = (long)n * gridDim.y + strip;
    if (ch < a.C) part[(g * 2 + which) * a.C + ch] = t;
  }
}

// one block per 64-channel slab: 4 quarters of the groups are summed side by side (each in ascending
// group order), then the 4 quarter sums in quarter order
// (out0 / out1: the two rows' targets; accumulate: += into them, the backward's gradient buffers)
__global__ __launch_bounds__(kThreads) void stats_reduce_kernel(const float* __restrict__ part,
                                                                float* __restrict__ out0, float* __restrict__ out1,
                                                                int groups, int C, int accumulate) {
  __shared__ float q[4][2][kSlab];
  const int c = threadIdx.x & 63, qi = threadIdx.x >> 6;
  const int ch = blockIdx.x * kSlab + c;
  float t0 = 0.f, t1 = 0.f;
  if (ch < C)
    for (int g = qi; g < groups; g += 4) {
      t0 += part[((long)g * 2 + 0) * C + ch];
      t1 += part[((long)g * 2 + 1) * C + ch];
    }
  q[qi][0][c] = t0;
  q[qi][1][c] = t1;
  __syncthreads();
  if (threadIdx.x < 2 * kSlab && ch < C) {
    const int which = threadIdx.x >> 6;  // the first two waves: sum, then sum of squares
    const float t = ((q[0][which][c] + q[1][which][c]) + q[2][which][c]) + q[3][which][c];
    float* o = which ? out1 : out0;
    o[ch] = accumulate ? o[ch] + t : t;
  }
}

// one thread per 8 channels of one row; the channel's scale / shift are rebuilt from the sums by
// every thread (a pooled tensor is a few MB: the sums stay in cache), with batchnorm.hip's expressions
// EV: evaluation mode, the statistics are run_mean / run_var themselves and nothing is written but f
template <bool EV>
__global__ __launch_bounds__(kThreads) void bn_f32_kernel(const float* __restrict__ y, bf16_t* __restrict__ f,
                                                          const float* __restrict__ sum,
                                                          const float* __restrict__ sumsq,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ mean_out,
                                                          float* __restrict__ rstd_out, float* __restrict__ run_mean,
                                                          float* __restrict__ run_var, long R, int C, float eps,
                                                          float momentum) {
  const int CV = C >> 3;
  const long nvec = R * CV;
  const float invR = 1.f / (float)R;
  for (long i = blockIdx.x * (long)kThreads + threadIdx.x; i < nvec; i += (long)gridDim.x * kThreads) {
    const int c0 = (int)(i % CV) * 8;
    const float4 a0 = *reinterpret_cast<const float4*>(y + i * 8), a1 = *reinterpret_cast<const float4*>(y + i * 8 + 4);
    float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      const float mean = EV ? run_mean[c] : sum[c] * invR;
      const float var = EV ? run_var[c] : fmaxf(sumsq[c] * invR - mean * mean, 0.f);
      const float rstd = rsqrtf(var + eps);
      const float g = gamma[c] * rstd;
      v[j] = fmaf(v[j], g, beta[c] - mean * g);
      if (!EV && i < CV) {  // the first row's threads also publish the statistics
        mean_out[c] = mean;
        rstd_out[c] = rstd;
        if (run_mean != nullptr) {
          run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mean;
          run_var[c] = (1.f - momentum) * run_var[c] + momentum * var * ((float)R / (float)max(R - 1, 1L));
        }
      }
    }
    *reinterpret_cast<uint4*>(f + i * 8) = pack8_bf16(v);
  }
}

// The heads' BatchNorm backward for the parameters alone (the pooled input takes no gradient):
// part[g, 0, c] = sum dy, part[g, 1, c] = sum dy * (y - mean) * rstd over the block's rows, xhat rebuilt
// from the fp32 y.  Block (slab, g): thread cv = tid & 7 owns 8 channels, the 32 row lanes take rows
// g * rpb + lane, + 32, ...; the lanes are added in lane order through LDS, the blocks by stats_reduce.
__global__ __launch_bounds__(kThreads) void bn_f32_bwd_kernel(const bf16_t* __restrict__ dy,
                                                              const float* __restrict__ y,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, float* __restrict__ part,
                                                              long R, int C, long rpb) {
  __shared__ float red[32 * 2 * kSlab];
  const int tid = threadIdx.x, cv = tid & 7, pl = tid >> 3;
  const int c0 = blockIdx.x * kSlab + cv * 8;
  const bool live = c0 < C;
  float m[8], rs[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    m[j] = live ? mean[c0 + j] : 0.f;
    rs[j] = live ? rstd[c0 + j] : 0.f;
    s1[j] = s2[j] = 0.f;
  }
  const long r1 = min(R, (blockIdx.y + 1) * rpb);
  if (live)
    for (long r = blockIdx.y * rpb + pl; r < r1; r += 32) {
      float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      unpack_add(*reinterpret_cast<const uint4*>(dy + r * C + c0), g);
      const float4 a0 = *reinterpret_cast<const float4*>(y + r * C + c0);
      const float4 a1 = *reinterpret_cast<const float4*>(y + r * C + c0 + 4);
      const float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s1[j] += g[j];
        s2[j] = fmaf(g[j], (v[j] - m[j]) * rs[j], s2[j]);
      }
    }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[(pl * 2 + 0) * kSlab + cv * 8 + j] = s1[j];
    red[(pl * 2 + 1) * kSlab + cv * 8 + j] = s2[j];
  }
  __syncthreads();
  if (tid < 2 * kSlab) {
    const int which = tid >> 6, c = tid & 63;
    float t = 0.f;
    for (int l = 0; l < 32; ++l) t += red[(l * 2 + which) * kSlab + c];
    const int ch = blockIdx.x * kSlab + c;
    if (ch < C) part[((long)blockIdx.y * 2 + which) * C + ch] = t;
  }
}

bool plan(int N, int H, int W, int C, int k, int s, int p, PoolArgs& a, int& strips) {
  if (N < 1 || C < 8 || C % 8 || k < 1 || s < 1 || p < 0 || 2 * p > k || H + 2 * p < k || W + 2 * p < k) return false;
  a.H = H, a.W = W, a.C = C, a.k = k, a.s = s, a.p = p;
  a.OH = (H + 2 * p - k) / s + 1;
  a.OW = (W + 2 * p - k) / s + 1;
  a.Wuse = std::min(W, (a.OW - 1) * s - p + k);
  a.inv = 1.f / (float)(k * k);
  if (a.Wuse * 128 > kRowBytes || a.OW * kSlab * 4 > kAccBytes || N > 65535) return false;
  const int slabs = (C + kSlab - 1) / kSlab;
  const long wgs = (long)N * slabs;
  int want = (int)std::min<long>(a.OH, std::max<long>(1, (kFill + wgs - 1) / wgs));
  a.OHs = std::min((a.OH + want - 1) / want, kAccBytes / (a.OW * kSlab * 4));
  strips = (a.OH + a.OHs - 1) / a.OHs;
  a.RB = std::max(1, std::min(kMaxRows, kRowBytes / (a.Wuse * 128)));
  return strips <= 65535;
}

}  // namespace

int dl_avgpool_stats_groups(int N, int H, int W, int C, int k, int s, int p) {
  PoolArgs a;
  int strips;
  return plan(N, H, W, C, k, s, p, a, strips) ? N * strips : -1;
}

// part: fp32 [dl_avgpool_stats_groups(...), 2, C] scratch, every element written before it is read;
// sums: fp32 [2, C]; y: fp32 [N, OH, OW, C]
int dl_avgpool_stats_fwd(const bf16_t* x, float* y, float* part, float* sums, int N, int H, int W, int C, int k, int s,
                         int p, hipStream_t st) {
  PoolArgs a;
  int strips;
  if (!plan(N, H, W, C, k, s, p, a, strips)) return -1;
  const int slabs = (C + kSlab - 1) / kSlab;
  // staged rows | accumulators; the statistics reduction reuses both once they are dead: at least
  // 32 x 2 x 64 floats
  const size_t lds = std::max<size_t>((size_t)a.RB * a.Wuse * 128 + (size_t)a.OHs * a.OW * kSlab * sizeof(float),
                                      32 * 2 * kSlab * sizeof(float));
  avgpool_stats_kernel<<<dim3(slabs, strips, N), kThreads, lds, st>>>(x, y, part, a);
  stats_reduce_kernel<<<slabs, kThreads, 0, st>>>(part, sums, sums + C, N * strips, C, 0);
  return 0;
}

// f [R, C] bf16 = BatchNorm(y [R, C] fp32) over the statistics sum / sumsq [C] of dl_avgpool_stats_fwd;
// mean / rstd [C] out; run_mean / run_var (may be null) take one momentum update
int dl_bn_f32_fwd(const float* y, bf16_t* f, const float* sum, const float* sumsq, const float* gamma,
                  const float* beta, float* mean, float* rstd, float* run_mean, float* run_var, long R, int C, float eps,
                  float momentum, hipStream_t st) {
  if (C < 8 || C % 8 || R < 1) return -1;
  const long blocks = (R * (C / 8) + kThreads - 1) / kThreads;
  bn_f32_kernel<false><<<(int)std::min<long>(blocks, 2048), kThreads, 0, st>>>(y, f, sum, sumsq, gamma, beta, mean, rstd,
                                                                               run_mean, run_var, R, C, eps, momentum);
  return 0;
}

// evaluation mode: f = (y - run_mean) gamma / sqrt(run_var + eps) + beta; nothing else is written
int dl_bn_f32_eval(const float* y, bf16_t* f, const float* gamma, const float* beta, const float* run_mean,
                   const float* run_var, long R, int C, float eps, hipStream_t st) {
  if (C < 8 || C % 8 || R < 1) return -1;
  const long blocks = (R * (C / 8) + kThreads - 1) / kThreads;
  bn_f32_kernel<true><<<(int)std::min<long>(blocks, 2048), kThreads, 0, st>>>(
      y, f, nullptr, nullptr, gamma, beta, nullptr, nullptr, const_cast<float*>(run_mean), const_cast<float*>(run_var),
      R, C, eps, 0.f);
  return 0;
}

int dl_bn_f32_bwd_groups(long R) { return (int)std::min<long>(64, (R + 255) / 256); }

// dgamma / dbeta [C] += the BatchNorm parameter gradients for dy [R, C] bf16 over y [R, C] fp32 and the
// forward's mean / rstd; part: scratch of dl_bn_f32_bwd_groups(R) * 2 * C floats
int dl_bn_f32_bwd(const bf16_t* dy, const float* y, const float* mean, const float* rstd, float* part, float* dgamma,
                  float* dbeta, long R, int C, hipStream_t st) {
  if (C < 8 || C % 8 || R < 1) return -1;
  const int groups = dl_bn_f32_bwd_groups(R), slabs = (C + kSlab - 1) / kSlab;
  const long rpb = (R + groups - 1) / groups;
  bn_f32_bwd_kernel<<<dim3(slabs, groups), kThreads, 0, st>>>(dy, y, mean, rstd, part, R, C, rpb);
  stats_reduce_kernel<<<slabs, kThreads, 0, st>>>(part, dbeta, dgamma, groups, C, 1);
  return 0;
}
