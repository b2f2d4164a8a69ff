// Forward-only softmax cross-entropy with the label's rank, for evaluation (docs/KERNELS.md).
// One 256-thread block per row reads the [V] bf16 logits ONCE: the online (max, sum-exp) state and
// the count of logits that beat the label ride in the same loop, so a row costs V * 2 bytes of HBM
// traffic against the training kernel's two reads and one write.  Per row:
//   row_loss = logsumexp(x) - x[label]                                             (fp32)
//   row_rank = #{ j : x[j] > x[label]  or  (x[j] == x[label] and j < label) }      (int32)
// compared on the bf16 values as stored, so top-k is rank < k and ties resolve to the lower index.
// Rows with label == ignore_index get (0, -1) and never form an address into the logits.
// Outputs are per row (no atomics: bitwise reproducible); nothing synchronises with the host.
#include "dl_common.h"
#include "dl_kernels.h"

namespace {

// (m, s) <- (m, s) (+) (mo, so) for the online softmax; an empty state is (-inf, 0) and two empty
// states combine to an empty one (never exp(-inf - -inf))
__device__ __forceinline__ void lse_combine(float& m, float& s, float mo, float so) {
  const float mn = fmaxf(m, mo);
  s = (mn == -INFINITY) ? 0.f : s * __expf(m - mn) + so * __expf(mo - mn);
  m = mn;
}

// one online step over 8 values in registers: v[j] is column i0 + j of the row
__device__ __forceinline__ void lse_rank_step8(const uint4& raw, int i0, float xl, int label, float& m, float& s,
                                               int& cnt) {
  float v[8];
  unpack8_bf16(raw, v);
  float mx = v[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) mx = fmaxf(mx, v[j]);
  const float mn = fmaxf(m, mx);
  // mn == -inf (every value so far is -inf): the sum stays 0 instead of exp(-inf - -inf)
  float acc = (mn == -INFINITY) ? 0.f : s * __expf(m - mn);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    acc += (mn == -INFINITY) ? 0.f : __expf(v[j] - mn);
    cnt += (v[j] > xl || (v[j] == xl && i0 + j < label)) ? 1 : 0;
  }
  m = mn;
  s = acc;
}

__global__ __launch_bounds__(256) void xent_eval_kernel(const bf16_t* __restrict__ logits,
                                                        const long* __restrict__ labels,
                                                        float* __restrict__ row_loss, int* __restrict__ row_rank,
                                                        int V, long ld, int ignore_index) {
  __shared__ float red_m[4], red_s[4];
  __shared__ int red_c[4];
  const int row = blockIdx.x;
  const long lab = labels[row];
  // ignored rows, and labels outside the row (which must not become an index), return here
  if (lab == ignore_index || lab < 0 || lab >= V) {
    if (threadIdx.x == 0) {
      row_loss[row] = lab == ignore_index ? 0.f : __builtin_nanf("");
      row_rank[row] = -1;
    }
    return;
  }
  const bf16_t* x = logits + (long)row * ld;
  const int label = (int)lab;
  const float xl = bf2f(x[label]);  // the label logit first: every thread compares against it
  float m = -INFINITY, s = 0.f;
  int cnt = 0;
  // The row splits at its 16-byte boundaries: `head` (< 8) columns before the first one, nvec whole
  // 8-column vectors, and the (< 8) columns after the last whole vector.  With V % 8 == 0,
  // ld % 8 == 0 and an aligned base every row is vectors only; an odd V or ld (sahajBERT: 31995)
  // moves the boundary from row to row, and only the two edges are read one column at a time.
  const int mis = (int)((reinterpret_cast<uintptr_t>(x) >> 1) & 7);
  const int head = min(V, (8 - mis) & 7);
  const int nvec = (V - head) >> 3;
  const int tail0 = head + (nvec << 3);
  if ((int)threadIdx.x < head + (V - tail0)) {  // the edges: at most 14 columns, one per thread
    const int i = (int)threadIdx.x < head ? (int)threadIdx.x : tail0 + ((int)threadIdx.x - head);
    const float v = bf2f(x[i]);
    m = v;
    s = (v == -INFINITY) ? 0.f : 1.f;
    cnt = (v > xl || (v == xl && i < label)) ? 1 : 0;
  }
  const uint4* xv = reinterpret_cast<const uint4*>(x + head);
  int k = threadIdx.x;
  for (; k + 256 < nvec; k += 512) {  // two 16-byte loads in flight per thread
    const uint4 a = xv[k], b = xv[k + 256];
    lse_rank_step8(a, head + 8 * k, xl, label, m, s, cnt);
    lse_rank_step8(b, head + 8 * (k + 256), xl, label, m, s, cnt);
  }
  if (k < nvec) lse_rank_step8(xv[k], head + 8 * k, xl, label, m, s, cnt);
  // wave-64 shuffles, then one LDS combine over the four waves in a fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lse_combine(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { red_m[wid] = m; red_s[wid] = s; red_c[wid] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = red_m[0], S = red_s[0];
    int C = red_c[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      lse_combine(M, S, red_m[w], red_s[w]);
      C += red_c[w];
    }
    row_loss[row] = M + __logf(S) - xl;
    row_rank[row] = C;
  }
}

}  // namespace

int dl_xent_eval(const bf16_t* logits, const long* labels, float* row_loss, int* row_rank, int M, int V, long ld,
                 int ignore_index, hipStream_t st) {
  if (M < 0 || V < 1 || ld < V) return 1;
  if (M == 0) return 0;
  xent_eval_kernel<<<M, 256, 0, st>>>(logits, labels, row_loss, row_rank, V, ld, ignore_index);
  return 0;
}
