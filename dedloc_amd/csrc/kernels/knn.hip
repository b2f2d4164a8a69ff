// k-nearest-neighbour evaluation (docs/KERNELS.md "kNN evaluation"): a fused similarity + top-k
// kernel, the merge of its bank slices, and the weighted vote with the target's rank.
//
//   knn_topk   s[i, j] = sum_d q[i, d] bank[j, d]  (bf16 products, fp32 MFMA accumulation); per query
//              row the k largest under the total order (score descending, bank index ascending),
//              sorted in that order.  The score matrix never reaches memory.
//
// One 256-thread workgroup owns a (128-query tile, bank slice) pair and walks the slice in tiles of
// 128 bank rows: the GEMM main loop of gemm_small.hip (global -> registers -> LDS rows of 32 k, next
// K-step prefetched under the MFMAs, 4 waves as 2 x 2 of 64 x 64 = 4 x 4 v_mfma_f32_16x16x32_bf16).
// The epilogue compares every accumulator with its row's threshold in LDS (the row's current k-th
// score, -inf until the row has k candidates) and appends the survivors to that row's candidate list
// as one 64-bit key
//     key = orderable(score) << 32 | ~index         (larger key = better under the total order)
// through an LDS counter (an integer atomic: the list's order varies, its sorted content does not).
// The lists live in a global workspace that only the owning workgroup touches (cap = round_up(k, 64)
// + 256 entries per row: a row holding at most cap - 128 entries can take a whole tile).
// A row whose list grew past that is pruned by one wave in registers (prune_row: the k-th largest key
// by a bitwise search with ballot counts, the best k packed to the list's front) and the threshold
// rises to the k-th score.  A later score equal to the threshold has a higher index than every kept
// entry, so the strict compare is the tie rule.  Only the slice's final result is sorted (bitonic,
// in LDS, one wave per row).
// Rows past Q and bank rows past the slice never survive; k <= N keeps the empty key (0) out of
// the result.  LDS: 2 x 10 KiB operand tiles + 1 KiB thresholds / counters + 4 x 4 KiB sort buffers.
//
// With more than one slice each workgroup leaves its sorted best k keys in part[row][slice][k] and a
// second launch (knn_merge_kernel, one workgroup per row) sorts the row's slices * k keys: no
// workgroup ever reads what another wrote inside a launch.  Every score is the same MFMA sequence
// whatever the slicing, so the outputs do not depend on `splits`, and nothing is accumulated with
// float atomics: two runs agree bitwise.
//
//   knn_vote   neighbour j votes for class bank_labels[idx[., j]] with weight
//              exp((vals[., j] - vals[., 0]) / sigma); class sums in fp32 in neighbour order; the
//              winning class (lower id on ties) and the target's rank among the classes.
#include <algorithm>

#include "dl_common.h"
#include "dl_kernels.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned long long u64;

constexpr int TQ = 128, TN = 128, TK = 32, ROW = TK + 8, NTH = 256;
constexpr int SORT_MAX = 512;    // a row's list: at most round_up(256, 64) + 256 keys
constexpr int MERGE_MAX = 4096;  // slices * k keys of one row in the merge

__device__ __forceinline__ u64 knn_key(float v, int idx) {
  uint32_t b = __float_as_uint(v + 0.f);  // -0 -> +0: equal scores have equal bits
  b ^= (b >> 31) ? 0xffffffffu : 0x80000000u;
  return ((u64)b << 32) | (uint32_t)~(uint32_t)idx;
}
__device__ __forceinline__ float key_score(u64 key) {
  uint32_t b = (uint32_t)(key >> 32);
  b ^= (b >> 31) ? 0x80000000u : 0xffffffffu;
  return __uint_as_float(b);
}
__device__ __forceinline__ int key_index(u64 key) { return (int)~(uint32_t)key; }

// LDS written by some lanes of this wave is read by others: order the accesses (one wave, so no
// workgroup barrier; the rows a wave prunes are its own)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// this wave's stores of list keys have reached L2 (ahead of the barrier behind which other waves of
// the workgroup load them from there)
__device__ __forceinline__ void list_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// one compare-exchange step of a descending bitonic sort over P keys, pair t
__device__ __forceinline__ void bitonic_step(u64* s, int t, int size, int stride) {
  const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
  const int j = i + stride;
  const u64 a = s[i], b = s[j];
  if ((a < b) == ((i & size) == 0)) {
    s[i] = b;
    s[j] = a;
  }
}

__device__ __forceinline__ void wave_sort_desc(u64* s, int P, int lane) {
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < (P >> 1); t += 64) bitonic_step(s, t, size, stride);
      wave_lds_sync();
    }
}

struct KnnArgs {
  const bf16_t* q;
  const bf16_t* bank;
  int Q, N, D, k, splits, cap;
  u64* lists;  // [slices][query tiles][TQ][cap]
  u64* part;   // [Q][splits][k]  (splits > 1)
  float* vals;
  int* idx;
};

// two 8-element chunks of a 128 x 32 operand tile per thread (rows of D bf16, 16-byte aligned)
__device__ __forceinline__ void gload(const bf16_t* __restrict__ p, int D, int r0, int rows, int k0, uint4 (&v)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int idx = threadIdx.x + NTH * u;
    const int gr = r0 + (idx >> 2), gk = k0 + (idx & 3) * 8;
    v[u] = (gr < rows && gk + 8 <= D) ? *reinterpret_cast<const uint4*>(p + (long)gr * D + gk) : uint4{0, 0, 0, 0};
  }
}
__device__ __forceinline__ void lds_put(bf16_t* img, const uint4 (&v)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int idx = threadIdx.x + NTH * u;
    *reinterpret_cast<uint4*>(img + (idx >> 2) * ROW + (idx & 3) * 8) = v[u];
  }
}

// the row's list (c keys in global memory) into buf, padded with empty keys to a power of two, sorted
__device__ __forceinline__ int load_sort_row(const u64* list, int c, u64* buf, int lane) {
  int P = 2;
  while (P < c) P <<= 1;
  // agent-scope loads: served by L2, where this workgroup's stores of the keys have landed
  for (int t = lane; t < P; t += 64)
    buf[t] = t < c ? __hip_atomic_load(list + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
  wave_lds_sync();
  wave_sort_desc(buf, P, lane);
  return P;
}

// Prune a row's list of c keys (k <= c <= 64 NK) to its best k, by one wave and in registers: the
// k-th largest key is found bit by bit from the top (the largest T with at least k keys >= T; counts
// by ballot), then the keys >= T, exactly k of them since keys are distinct, are packed to the
// front of the list in any order.  Every load has returned before the first store: the stores
// depend on T.  Returns T.
constexpr int NK = 8;
__device__ __forceinline__ u64 prune_row(u64* list, int c, int k, int lane) {
  u64 keys[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    const int t = lane + 64 * j;
    keys[j] = t < c ? __hip_atomic_load(list + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
  }
  u64 kth = 0;
  for (int bit = 63; bit >= 0; --bit) {
    const u64 cand = kth | (1ull << bit);
    int n = 0;
#pragma unroll
    for (int j = 0; j < NK; ++j) n += __popcll(__ballot(keys[j] >= cand));
    if (n >= k) kth = cand;
  }
  int base = 0;
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    const bool keep = keys[j] >= kth;
    const u64 b = __ballot(keep);
    if (keep) list[base + __popcll(b & ((1ull << lane) - 1ull))] = keys[j];
    base += __popcll(b);
  }
  return kth;
}

__global__ __launch_bounds__(NTH) void knn_topk_kernel(KnnArgs p) {
  __shared__ __attribute__((aligned(16))) bf16_t sa[TQ * ROW];
  __shared__ __attribute__((aligned(16))) bf16_t sb[TN * ROW];
  __shared__ float thr_s[TQ];
  __shared__ int cnt_s[TQ];
  __shared__ u64 sort_s[NTH / 64][SORT_MAX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int m0 = blockIdx.x * TQ, slice = blockIdx.y;
  const int nbeg = (int)((long)slice * p.N / p.splits), nend = (int)((long)(slice + 1) * p.N / p.splits);
  const int cap = p.cap, kcap = cap - TN;
  u64* list = p.lists + ((long)slice * gridDim.x + blockIdx.x) * (long)TQ * cap;
  if (threadIdx.x < TQ) {
    thr_s[threadIdx.x] = -INFINITY;
    cnt_s[threadIdx.x] = 0;
  }
  __syncthreads();

  for (int n0 = nbeg; n0 < nend; n0 += TN) {
    floatx4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
    uint4 ra[2], rb[2];
    gload(p.q, p.D, m0, p.Q, 0, ra);
    gload(p.bank, p.D, n0, nend, 0, rb);
    for (int k0 = 0; k0 < p.D; k0 += TK) {
      lds_put(sa, ra);
      lds_put(sb, rb);
      __syncthreads();
      if (k0 + TK < p.D) {  // next K-step's loads are in flight during this one's MFMAs
        gload(p.q, p.D, m0, p.Q, k0 + TK, ra);
        gload(p.bank, p.D, n0, nend, k0 + TK, rb);
      }
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(sa + (wm * 64 + i * 16 + (lane & 15)) * ROW + 8 * (lane >> 4));
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bfr[j] = *reinterpret_cast<const bf16x8*>(sb + (wn * 64 + j * 16 + (lane & 15)) * ROW + 8 * (lane >> 4));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      __syncthreads();
    }
    // survivors of this score tile: accumulator e of tile (i, j) is query row
    // wm*64 + i*16 + 4*(lane >> 4) + e, bank row n0 + wn*64 + j*16 + (lane & 15)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = wm * 64 + i * 16 + 4 * (lane >> 4) + e;
        if (m0 + r >= p.Q) continue;
        const float t = thr_s[r];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = n0 + wn * 64 + j * 16 + (lane & 15);
          const float v = acc[i][j][e];
          if (n < nend && v > t) {
            // at most TN appends per row and tile onto at most kcap entries: slot < cap
            const int slot = atomicAdd(&cnt_s[r], 1);
            list[(long)r * cap + slot] = knn_key(v, n);
          }
        }
      }
    list_stores_done();
    __syncthreads();
    for (int r = w; r < TQ; r += NTH / 64) {
      const int c = __builtin_amdgcn_readfirstlane(cnt_s[r]);  // wave-uniform: prune_row counts by ballot
      if (c <= kcap) continue;  // c > kcap >= k: the row has a k-th key
      const u64 kth = prune_row(list + (long)r * cap, c, p.k, lane);
      if (lane == 0) {
        cnt_s[r] = p.k;
        thr_s[r] = key_score(kth);
      }
    }
    list_stores_done();
    __syncthreads();
  }

  // the slice's result per row: the sorted best k (fewer in a slice shorter than k: empty keys follow)
  for (int r = w; r < TQ; r += NTH / 64) {
    const int m = m0 + r;
    if (m >= p.Q) break;
    const int c = cnt_s[r];
    u64* buf = sort_s[w];
    const int P = c > 0 ? load_sort_row(list + (long)r * cap, c, buf, lane) : 0;
    for (int t = lane; t < p.k; t += 64) {
      const u64 key = t < P ? buf[t] : 0ull;
      if (p.splits == 1) {
        p.vals[(long)m * p.k + t] = key_score(key);
        p.idx[(long)m * p.k + t] = key_index(key);
      } else {
        p.part[((long)m * p.splits + slice) * p.k + t] = key;
      }
    }
    wave_lds_sync();
  }
}

// one workgroup per query row: the row's splits * k keys (n of them, padded to the power of two P)
// sorted; the first k are the result
__global__ __launch_bounds__(NTH) void knn_merge_kernel(const u64* __restrict__ part, float* __restrict__ vals,
                                                        int* __restrict__ idx, int n, int P, int k) {
  __shared__ u64 s[MERGE_MAX];
  const long row = blockIdx.x;
  for (int t = threadIdx.x; t < P; t += NTH) s[t] = t < n ? part[row * n + t] : 0ull;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += NTH) bitonic_step(s, t, size, stride);
      __syncthreads();
    }
  for (int t = threadIdx.x; t < k; t += NTH) {
    vals[row * k + t] = key_score(s[t]);
    idx[row * k + t] = key_index(s[t]);
  }
}

// one workgroup per query row, thread j = neighbour j (k <= 256).  The first neighbour of each class
// owns that class and sums its votes in neighbour order.
__global__ __launch_bounds__(NTH) void knn_vote_kernel(const float* __restrict__ vals, const int* __restrict__ idx,
                                                       const int* __restrict__ labels,
                                                       const long* __restrict__ targets, int* __restrict__ pred,
                                                       int* __restrict__ rank, int k, int N, int C, float sigma) {
  __shared__ int cls_s[NTH];
  __shared__ float w_s[NTH];
  __shared__ u64 best_s[NTH / 64];
  __shared__ float pt_s;
  __shared__ int voted_s, beats_s, below_s;
  const long row = blockIdx.x;
  const int t = threadIdx.x;
  if (t == 0) {
    pt_s = 0.f;
    voted_s = beats_s = below_s = 0;
  }
  int c = -1;
  float wgt = 0.f;
  if (t < k) {
    const int i = idx[row * k + t];
    if (i >= 0 && i < N) {  // a bank label outside [0, C) casts no vote and forms no address
      const int l = labels[i];
      if (l >= 0 && l < C) c = l;
    }
    wgt = expf((vals[row * k + t] - vals[row * k]) / sigma);
  }
  cls_s[t] = c;
  w_s[t] = wgt;
  __syncthreads();
  bool owner = c >= 0;
  for (int j = 0; j < t && owner; ++j) owner = cls_s[j] != c;
  float sum = 0.f;
  if (owner)
    for (int j = t; j < k; ++j)
      if (cls_s[j] == c) sum += w_s[j];
  const long tl = targets[row];
  const bool valid = tl >= 0 && tl < C;
  const int tgt = valid ? (int)tl : -1;
  if (owner && c == tgt) {
    pt_s = sum;
    voted_s = 1;
  }
  // sums are >= 0: their bits order like the values; lower class id wins a tie
  u64 key = owner ? ((u64)__float_as_uint(sum) << 32) | (0xffffffffu - (uint32_t)c) : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((t & 63) == 0) best_s[t >> 6] = key;
  __syncthreads();
  const float pt = pt_s;
  const bool beats = owner && (sum > pt || (sum == pt && c < tgt));
  const bool below = owner && c < tgt;
  const int nb = __popcll(__ballot(beats)), nl = __popcll(__ballot(below));
  if ((t & 63) == 0) {
    atomicAdd(&beats_s, nb);
    atomicAdd(&below_s, nl);
  }
  __syncthreads();
  if (t == 0) {
    u64 best = best_s[0];
    for (int i = 1; i < NTH / 64; ++i) best = best_s[i] > best ? best_s[i] : best;
    pred[row] = best ? (int)(0xffffffffu - (uint32_t)best) : 0;  // no vote at all: every sum is 0, class 0
    // a voted target whose sum underflowed to 0 ties with the classes that got no vote
    rank[row] = (valid && voted_s) ? beats_s + (pt == 0.f ? tgt - below_s : 0) : -1;
  }
}

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

}  // namespace

// two tiles of room above round_up(k, 64): a prune at most every other tile (<= 512 = 64 NK keys)
int dl_knn_cap(int k) { return round_up(k, 64) + 2 * TN; }

long dl_knn_list_entries(int Q, int k, int splits) {
  return (long)splits * ((Q + TQ - 1) / TQ) * TQ * dl_knn_cap(k);
}

int dl_knn_max_splits(int N, int k) { return std::max(1, std::min(std::min(32, MERGE_MAX / k), N)); }

// slices for about two workgroups per CU, each slice at least 4 tiles and 2 k bank rows long
int dl_knn_splits(int Q, int N, int k, int cus) {
  if (Q < 1 || N < 1 || k < 1) return 1;
  const int tiles = (Q + TQ - 1) / TQ;
  const int want = (2 * std::max(cus, 1) + tiles - 1) / tiles;
  const int fit = N / std::max(4 * TN, 2 * k);
  return std::max(1, std::min(std::min(want, fit), dl_knn_max_splits(N, k)));
}

int dl_knn_topk(const bf16_t* q, const bf16_t* bank, int Q, int N, int D, int k, int splits, unsigned long long* lists,
                unsigned long long* part, float* vals, int* idx, hipStream_t st) {
  if (Q < 0 || N < 1 || k < 1 || k > 256 || k > N || D < 16 || D > 4096 || D % 16) return -1;
  if (splits < 1 || splits > dl_knn_max_splits(N, k) || !lists || (splits > 1 && !part)) return -1;
  if (((uintptr_t)q | (uintptr_t)bank) & 15) return -1;
  if (Q == 0) return 0;
  const int tiles = (Q + TQ - 1) / TQ;
  KnnArgs a{q, bank, Q, N, D, k, splits, dl_knn_cap(k), lists, part, vals, idx};
  knn_topk_kernel<<<dim3(tiles, splits), NTH, 0, st>>>(a);
  if (splits > 1) {
    const int n = splits * k;
    int P = 2;
    while (P < n) P <<= 1;
    knn_merge_kernel<<<Q, NTH, 0, st>>>(part, vals, idx, n, P, k);
  }
  return 0;
}

int dl_knn_vote(const float* vals, const int* idx, const int* labels, const long* targets, int* pred, int* rank, int Q,
                int k, int N, int C, float sigma, hipStream_t st) {
  if (Q < 0 || k < 1 || k > NTH || N < 1 || C < 1 || C > 8192 || !(sigma > 0.f)) return -1;
  if (Q == 0) return 0;
  knn_vote_kernel<<<Q, NTH, 0, st>>>(vals, idx, labels, targets, pred, rank, k, N, C, sigma);
  return 0;
}
