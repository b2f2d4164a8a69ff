// torch.library CUDA(=HIP) implementations of the `dedloc::` operators.
//
// The operator schemas are defined once, in Python (dedloc_amd/ops/_lib.py), together with the
// CPU implementations used only for the CPU plumbing configuration.  Loading this library adds
// the gfx950 kernels under the CUDA dispatch key, so on a GPU tensor the HIP kernel is the only
// implementation that can run (no silent eager fallback exists).
#include <torch/extension.h>
#include <torch/library.h>
#include <c10/hip/HIPStream.h>

#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>

#include "dl_kernels.h"

namespace {

inline hipStream_t cur_stream(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.get_device()).stream();
}

inline bf16_t* bf(const at::Tensor& t) { return reinterpret_cast<bf16_t*>(t.data_ptr()); }
inline const bf16_t* cbf(const at::Tensor& t) { return reinterpret_cast<const bf16_t*>(t.data_ptr()); }
inline float* f32(const at::Tensor& t) { return t.data_ptr<float>(); }

inline void check(int rc, const char* what) { TORCH_CHECK(rc == 0, "dedloc_amd: unsupported shape for ", what); }

inline void expect(const at::Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

inline int dtype_code(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return 0;
    case at::kHalf: return 1;
    case at::kBFloat16: return 2;
    default: TORCH_CHECK(false, "unsupported wire dtype ", t.scalar_type());
  }
  return -1;
}

// ------------------------------------------------------------------ layernorm
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> layernorm_fwd(const at::Tensor& x,
                                                                          const c10::optional<at::Tensor>& res,
                                                                          const at::Tensor& gamma,
                                                                          const at::Tensor& beta, double eps) {
  expect(x, at::kBFloat16, "x");
  expect(gamma, at::kFloat, "gamma");
  expect(beta, at::kFloat, "beta");
  const int64_t D = x.size(-1), rows = x.numel() / D;
  auto y = at::empty_like(x);
  auto mean = at::empty({rows}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  at::Tensor s = x;
  const bf16_t* rp = nullptr;
  if (res.has_value()) {
    expect(*res, at::kBFloat16, "res");
    TORCH_CHECK(res->numel() == x.numel(), "res shape mismatch");
    s = at::empty_like(x);
    rp = cbf(*res);
  }
  check(dl_layernorm_fwd(cbf(x), rp, f32(gamma), f32(beta), bf(y), rp ? bf(s) : nullptr, f32(mean), f32(rstd),
                         (int)rows, (int)D, (float)eps, cur_stream(x)),
        "layernorm_fwd");
  return {y, s, mean, rstd};
}

at::Tensor layernorm_bwd(const at::Tensor& dy, const at::Tensor& s, const at::Tensor& gamma, const at::Tensor& mean,
                         const at::Tensor& rstd, at::Tensor dgamma, at::Tensor dbeta, bool accumulate,
                         const c10::optional<at::Tensor>& dsum) {
  expect(dy, at::kBFloat16, "dy");
  expect(s, at::kBFloat16, "s");
  expect(dgamma, at::kFloat, "dgamma");
  expect(dbeta, at::kFloat, "dbeta");
  const int64_t D = dy.size(-1), rows = dy.numel() / D;
  constexpr int64_t max_parts = 512;  // grid cap of the LayerNorm backward's partial sums
  const int nparts = (int)std::min<int64_t>(max_parts, std::max<int64_t>(1, rows / 32));
  auto ds = at::empty_like(dy);
  if (!accumulate) {
    dgamma.zero_();
    dbeta.zero_();
  }
  float* dsp = nullptr;
  if (dsum.has_value()) {
    expect(*dsum, at::kFloat, "dsum");
    TORCH_CHECK(dsum->numel() == D, "dsum size mismatch");
    dsp = f32(*dsum);
  }
  check(dl_layernorm_bwd(cbf(dy), cbf(s), f32(gamma), f32(mean), f32(rstd), bf(ds), f32(dgamma), f32(dbeta), dsp,
                         (int)rows, (int)D, nparts, cur_stream(dy)),
        "layernorm_bwd");
  return ds;
}

// ------------------------------------------------------------------ elementwise
at::Tensor gelu_fwd(const at::Tensor& h) {
  expect(h, at::kBFloat16, "h");
  auto y = at::empty_like(h);
  check(dl_gelu_fwd(cbf(h), bf(y), h.numel(), cur_stream(h)), "gelu_fwd");
  return y;
}

at::Tensor gelu_bwd(const at::Tensor& dy, const at::Tensor& h, const c10::optional<at::Tensor>& dbias) {
  expect(dy, at::kBFloat16, "dy");
  expect(h, at::kBFloat16, "h");
  auto dh = at::empty_like(h);
  if (dbias.has_value()) {  // fused bias gradient of the producing Linear (accumulating)
    expect(*dbias, at::kFloat, "dbias");
    const int64_t N = h.size(-1);
    TORCH_CHECK(dbias->numel() == N, "dbias size mismatch");
    check(dl_gelu_bwd_colsum(cbf(dy), cbf(h), bf(dh), f32(*dbias), (int)(h.numel() / N), (int)N, cur_stream(h)),
          "gelu_bwd(colsum)");
    return dh;
  }
  check(dl_gelu_bwd(cbf(dy), cbf(h), bf(dh), h.numel(), cur_stream(h)), "gelu_bwd");
  return dh;
}

at::Tensor tanh_fwd(const at::Tensor& x) {
  expect(x, at::kBFloat16, "x");
  auto y = at::empty_like(x);
  check(dl_tanh_fwd(cbf(x), bf(y), x.numel(), cur_stream(x)), "tanh_fwd");
  return y;
}

at::Tensor tanh_bwd(const at::Tensor& dy, const at::Tensor& y) {
  expect(dy, at::kBFloat16, "dy");
  expect(y, at::kBFloat16, "y");
  auto dx = at::empty_like(y);
  check(dl_tanh_bwd(cbf(dy), cbf(y), bf(dx), y.numel(), cur_stream(y)), "tanh_bwd");
  return dx;
}

void bias_grad(const at::Tensor& dy, at::Tensor dbias, bool accumulate) {
  expect(dy, at::kBFloat16, "dy");
  expect(dbias, at::kFloat, "dbias");
  const int64_t N = dy.size(-1), rows = dy.numel() / N;
  TORCH_CHECK(dbias.numel() == N, "dbias size mismatch");
  const int nparts = (int)std::min<int64_t>(256, std::max<int64_t>(1, rows / 64));
  if (!accumulate) dbias.zero_();
  check(dl_colsum_bf16(cbf(dy), f32(dbias), (int)rows, (int)N, nparts, cur_stream(dy)), "bias_grad");
}

void cast_bf16(const at::Tensor& x, at::Tensor out) {
  expect(x, at::kFloat, "x");
  expect(out, at::kBFloat16, "out");
  TORCH_CHECK(x.numel() == out.numel(), "cast size mismatch");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0,
              "cast_bf16 needs 16-byte aligned buffers");
  dl_cast_f32_bf16(f32(x), bf(out), x.numel(), cur_stream(x));
}

// ------------------------------------------------------------------ optimizers
void lamb_step(at::Tensor p, const at::Tensor& g, at::Tensor m, at::Tensor v, const at::Tensor& chunk_tensor,
               const at::Tensor& chunk_start, const at::Tensor& chunk_len, const at::Tensor& tensor_wd,
               at::Tensor norms, double beta1, double beta2, double eps, double step_size, double clamp_value,
               double grad_scale) {
  for (auto* t : {&p, &m, &v, &norms}) expect(*t, at::kFloat, "lamb state");
  expect(g, at::kFloat, "g");
  check(dl_lamb_step(f32(p), f32(g), f32(m), f32(v), chunk_tensor.data_ptr<int>(), chunk_start.data_ptr<long>(),
                     chunk_len.data_ptr<int>(), (int)chunk_tensor.numel(), f32(tensor_wd), f32(norms),
                     (int)tensor_wd.numel(), beta1, beta2, (float)eps, (float)step_size,
                     (float)clamp_value, (float)grad_scale, nullptr, cur_stream(p)),
        "lamb_step");
}

void larc_sgd_step(at::Tensor p, const at::Tensor& g, at::Tensor buf, const at::Tensor& chunk_tensor,
                   const at::Tensor& chunk_start, const at::Tensor& chunk_len, const at::Tensor& tensor_wd,
                   at::Tensor norms, double lr, double momentum, double trust_coef, double eps, bool clip,
                   bool first_step, double grad_scale) {
  for (auto* t : {&p, &buf, &norms}) expect(*t, at::kFloat, "larc state");
  expect(g, at::kFloat, "g");
  check(dl_larc_sgd_step(f32(p), f32(g), f32(buf), chunk_tensor.data_ptr<int>(), chunk_start.data_ptr<long>(),
                         chunk_len.data_ptr<int>(), (int)chunk_tensor.numel(), f32(tensor_wd), f32(norms),
                         (int)tensor_wd.numel(), (float)lr, (float)momentum, (float)trust_coef, (float)eps,
                         clip ? 1 : 0, first_step ? 1 : 0, (float)grad_scale, cur_stream(p)),
        "larc_sgd_step");
}

void grad_norm_clip(at::Tensor g, double max_norm, at::Tensor part, at::Tensor out) {
  expect(g, at::kFloat, "g");
  expect(part, at::kFloat, "part");
  expect(out, at::kFloat, "out");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(g.data_ptr()) % 16 == 0, "grad buffer must be 16-byte aligned");
  check(dl_grad_norm_clip(f32(g), g.numel(), (float)max_norm, f32(part), (int)part.numel(), f32(out), (int)out.numel(),
                          cur_stream(g)),
        "grad_norm_clip");
}

void scale_by_(at::Tensor x, const at::Tensor& s) {
  expect(x, at::kBFloat16, "x");
  TORCH_CHECK(x.is_contiguous(), "scale_by_: x must be contiguous");
  TORCH_CHECK(s.is_cuda() && s.scalar_type() == at::kFloat && s.numel() == 1, "scale_by_: s must be one fp32 GPU scalar");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "scale_by_ needs a 16-byte aligned tensor");
  check(dl_scale_by(bf(x), x.numel(), f32(s.contiguous()), cur_stream(x)), "scale_by_");
}

// out += sum over the rows of slabs [S, out.numel()] (fp32), then slabs = 0: the concurrent SwAV
// passes' side gradient buffers folded into the flat gradient in one pass
void add_slabs_zero_(at::Tensor out, at::Tensor slabs) {
  expect(out, at::kFloat, "out");
  expect(slabs, at::kFloat, "slabs");
  TORCH_CHECK(out.is_contiguous() && slabs.is_contiguous() && slabs.dim() == 2 && slabs.size(1) == out.numel(),
              "add_slabs_zero_: slabs must be a contiguous [S, out.numel()] buffer");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(slabs.data_ptr()) % 16 == 0 && out.numel() % 4 == 0,
              "add_slabs_zero_ needs 16-byte aligned buffers and rows");
  check(dl_add_slabs_zero(f32(out), f32(slabs), (int)slabs.size(0), (size_t)out.numel(), cur_stream(out)),
        "add_slabs_zero_");
}

void axpby(at::Tensor y, const at::Tensor& x, double a, double b, const c10::optional<at::Tensor>& flag,
           const c10::optional<at::Tensor>& bdiv) {
  expect(y, at::kFloat, "y");
  expect(x, at::kFloat, "x");
  TORCH_CHECK(x.numel() == y.numel(), "axpby size mismatch");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(y.data_ptr()) % 16 == 0,
              "axpby needs 16-byte aligned buffers");
  const float* fp = flag.has_value() ? f32(*flag) : nullptr;
  const float* dp = nullptr;
  if (bdiv.has_value()) {
    expect(*bdiv, at::kFloat, "bdiv");
    TORCH_CHECK(bdiv->device() == y.device(), "axpby: bdiv must live with y");
    dp = f32(*bdiv);
  }
  dl_axpby(f32(y), f32(x), y.numel(), (float)a, (float)b, fp, dp, cur_stream(y));
}

// ------------------------------------------------------------------ averaging data plane
void pack(const at::Tensor& src, at::Tensor dst, double weight) {
  expect(src, at::kFloat, "src");
  TORCH_CHECK(dst.is_cuda() && dst.is_contiguous() && dst.numel() == src.numel(), "pack dst mismatch");
  check(dl_pack(f32(src), dst.data_ptr(), dtype_code(dst), src.numel(), (float)weight, cur_stream(src)), "pack");
}

void reduce_parts(const at::Tensor& parts, int64_t nparts, at::Tensor out, double inv_total) {
  TORCH_CHECK(parts.is_cuda() && parts.is_contiguous(), "parts must be contiguous GPU tensor");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous(), "out must be contiguous GPU tensor");
  const int64_t n = out.numel();
  TORCH_CHECK(parts.numel() == nparts * n, "parts size mismatch");
  check(dl_reduce_parts(parts.data_ptr(), dtype_code(parts), n, (int)nparts, out.data_ptr(), dtype_code(out), n,
                        (float)inv_total, cur_stream(out)),
        "reduce_parts");
}

void reduce_delta(const at::Tensor& parts, const at::Tensor& weights, at::Tensor deltas) {
  TORCH_CHECK(parts.is_cuda() && parts.is_contiguous() && parts.dim() == 2, "parts must be a contiguous [n, P] GPU tensor");
  TORCH_CHECK(deltas.is_cuda() && deltas.is_contiguous() && deltas.sizes() == parts.sizes() &&
                  deltas.scalar_type() == parts.scalar_type(),
              "deltas must match parts");
  expect(weights, at::kFloat, "weights");
  const int64_t nparts = parts.size(0), n = parts.size(1);
  TORCH_CHECK(weights.numel() == nparts, "one weight per part");
  check(dl_reduce_delta(parts.data_ptr(), deltas.data_ptr(), dtype_code(parts), n, (int)nparts, f32(weights), n,
                        cur_stream(parts)),
        "reduce_delta");
}

void unpack(const at::Tensor& src, at::Tensor dst, const c10::optional<at::Tensor>& snap, bool add) {
  expect(dst, at::kFloat, "dst");
  TORCH_CHECK(src.is_cuda() && src.is_contiguous() && src.numel() == dst.numel(), "unpack src mismatch");
  const float* sp = nullptr;
  if (snap.has_value()) {
    TORCH_CHECK(!add, "unpack: snap and add are exclusive");
    expect(*snap, at::kFloat, "snap");
    sp = f32(*snap);
  }
  check(dl_unpack(src.data_ptr(), dtype_code(src), f32(dst), sp, add ? 1 : 0, dst.numel(), cur_stream(dst)), "unpack");
}

// BLOCKWISE_8BIT wire codec: an encoded segment of n values is a 16-byte aligned uint8 [q8_bytes(n)]
inline void expect_q8(const at::Tensor& t, int64_t rows, int64_t n, const char* name) {
  expect(t, at::kByte, name);
  TORCH_CHECK(n >= 1, name, ": a segment holds at least one value");
  TORCH_CHECK(t.numel() == rows * (int64_t)dl_q8_bytes((size_t)n), name, " must hold ", rows, " x q8_bytes(", n,
              ") = ", rows * (int64_t)dl_q8_bytes((size_t)n), " bytes, has ", t.numel());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

void pack_q8(const at::Tensor& src, at::Tensor dst) {
  expect(src, at::kFloat, "src");
  expect_q8(dst, 1, src.numel(), "dst");
  check(dl_pack_q8(f32(src), dst.data_ptr(), src.numel(), cur_stream(src)), "pack_q8");
}

void reduce_delta_q8(const at::Tensor& parts, const at::Tensor& weights, at::Tensor deltas, int64_t n) {
  TORCH_CHECK(parts.dim() == 2 && deltas.dim() == 2 && deltas.sizes() == parts.sizes(), "deltas must match parts [k, bytes]");
  const int64_t nparts = parts.size(0);
  TORCH_CHECK(nparts >= 1 && nparts <= 64, "reduce_delta_q8: 1 to 64 senders");
  expect_q8(parts, nparts, n, "parts");
  expect_q8(deltas, nparts, n, "deltas");
  expect(weights, at::kFloat, "weights");
  TORCH_CHECK(weights.numel() == nparts, "one weight per part");
  check(dl_reduce_delta_q8(parts.data_ptr(), deltas.data_ptr(), (int)nparts, f32(weights), (size_t)n, cur_stream(parts)),
        "reduce_delta_q8");
}

void unpack_q8(const at::Tensor& src, at::Tensor dst, bool add) {
  expect(dst, at::kFloat, "dst");
  expect_q8(src, 1, dst.numel(), "src");
  check(dl_unpack_q8(src.data_ptr(), f32(dst), add ? 1 : 0, dst.numel(), cur_stream(dst)), "unpack_q8");
}

// ------------------------------------------------------------------ embeddings / loss
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> embed_ln_fwd(
    const at::Tensor& ids, const c10::optional<at::Tensor>& tt, const at::Tensor& wemb, const at::Tensor& pemb,
    const at::Tensor& temb, const at::Tensor& gamma, const at::Tensor& beta, int64_t S, double eps) {
  expect(ids, at::kLong, "ids");
  for (auto* t : {&wemb, &pemb, &temb, &gamma, &beta}) expect(*t, at::kFloat, "embedding table");
  const int64_t T = ids.numel(), E = wemb.size(1);
  auto opts = wemb.options();
  auto y = at::empty({T, E}, opts.dtype(at::kBFloat16));
  auto s = at::empty({T, E}, opts.dtype(at::kBFloat16));
  auto mean = at::empty({T}, opts);
  auto rstd = at::empty({T}, opts);
  const long* ttp = nullptr;
  if (tt.has_value()) {
    expect(*tt, at::kLong, "token_type_ids");
    ttp = tt->data_ptr<long>();
  }
  check(dl_embed_ln_fwd(ids.data_ptr<long>(), ttp, f32(wemb), f32(pemb), f32(temb), f32(gamma), f32(beta), bf(y), bf(s),
                        f32(mean), f32(rstd), (int)T, (int)S, (int)E, (float)eps, cur_stream(ids)),
        "embed_ln_fwd");
  return {y, s, mean, rstd};
}

void embed_bwd(const at::Tensor& ds, const at::Tensor& ids, const c10::optional<at::Tensor>& tt, at::Tensor dwemb,
               at::Tensor dpemb, at::Tensor dtemb, int64_t S) {
  expect(ds, at::kBFloat16, "ds");
  for (auto* t : {&dwemb, &dpemb, &dtemb}) expect(*t, at::kFloat, "embedding grad");
  expect(ids, at::kLong, "ids");
  const int64_t T = ids.numel(), E = ds.size(-1);
  // the kernels run B = T / S whole sequences: a partial one would silently lose its rows
  TORCH_CHECK(S > 0 && T % S == 0, "embed_bwd: ", T, " ids are not a whole number of sequences of S = ", S);
  TORCH_CHECK(ds.numel() == T * E, "embed_bwd: ds has ", ds.numel(), " elements, expected ", T, " ids x E = ", E);
  const long* ttp = nullptr;
  if (tt.has_value()) {
    expect(*tt, at::kLong, "token_type_ids");
    TORCH_CHECK(tt->numel() == T, "embed_bwd: one token type per id");
    ttp = tt->data_ptr<long>();
  }
  check(dl_embed_bwd(cbf(ds), ids.data_ptr<long>(), ttp, f32(dwemb), f32(dpemb), f32(dtemb), (int)(T / S), (int)S,
                     (int)E, (int)dtemb.size(0), cur_stream(ds)),
        "embed_bwd");
}

// packed batches: the position of each row is given (int32[T]) instead of derived as row % S
inline const int* pos_ptr(const at::Tensor& pos, int64_t T) {
  expect(pos, at::kInt, "pos");
  TORCH_CHECK(pos.numel() == T, "embed: pos must hold one position per row");
  TORCH_CHECK(T % 64 == 0, "embed: a packed token buffer is a whole number of 64-row tiles (got ", T, " rows)");
  return pos.data_ptr<int>();
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> embed_ln_pos_fwd(
    const at::Tensor& ids, const c10::optional<at::Tensor>& tt, const at::Tensor& pos, const at::Tensor& wemb,
    const at::Tensor& pemb, const at::Tensor& temb, const at::Tensor& gamma, const at::Tensor& beta, double eps) {
  expect(ids, at::kLong, "ids");
  for (auto* t : {&wemb, &pemb, &temb, &gamma, &beta}) expect(*t, at::kFloat, "embedding table");
  const int64_t T = ids.numel(), E = wemb.size(1);
  auto opts = wemb.options();
  auto y = at::empty({T, E}, opts.dtype(at::kBFloat16));
  auto s = at::empty({T, E}, opts.dtype(at::kBFloat16));
  auto mean = at::empty({T}, opts);
  auto rstd = at::empty({T}, opts);
  const long* ttp = nullptr;
  if (tt.has_value()) {
    expect(*tt, at::kLong, "token_type_ids");
    ttp = tt->data_ptr<long>();
  }
  check(dl_embed_ln_pos_fwd(ids.data_ptr<long>(), ttp, pos_ptr(pos, T), f32(wemb), f32(pemb), f32(temb),
                            f32(gamma), f32(beta), bf(y), bf(s), f32(mean), f32(rstd), (int)T, (int)E, (float)eps,
                            cur_stream(ids)),
        "embed_ln_pos_fwd");
  return {y, s, mean, rstd};
}

void embed_pos_bwd(const at::Tensor& ds, const at::Tensor& ids, const c10::optional<at::Tensor>& tt,
                   const at::Tensor& pos, at::Tensor dwemb, at::Tensor dpemb, at::Tensor dtemb) {
  expect(ds, at::kBFloat16, "ds");
  for (auto* t : {&dwemb, &dpemb, &dtemb}) expect(*t, at::kFloat, "embedding grad");
  const int64_t T = ids.numel(), E = ds.size(-1);
  const long* ttp = tt.has_value() ? tt->data_ptr<long>() : nullptr;
  check(dl_embed_pos_bwd(cbf(ds), ids.data_ptr<long>(), ttp, pos_ptr(pos, T), f32(dwemb), f32(dpemb),
                         f32(dtemb), (int)T, (int)E, (int)dtemb.size(0), cur_stream(ds)),
        "embed_pos_bwd");
}

std::tuple<at::Tensor, at::Tensor> xent_fwd_bwd(const at::Tensor& logits, const at::Tensor& labels, bool inplace,
                                                int64_t ignore_index) {
  expect(logits, at::kBFloat16, "logits");
  expect(labels, at::kLong, "labels");
  const int64_t V = logits.size(-1), M = logits.numel() / V;
  auto dl = inplace ? logits : at::empty_like(logits);
  auto ws = at::empty({3}, logits.options().dtype(at::kFloat));
  check(dl_xent_fwd_bwd(cbf(logits), labels.data_ptr<long>(), bf(dl), nullptr, f32(ws), f32(ws) + 1, (int)M, (int)V, V,
                        (int)ignore_index, cur_stream(logits)),
        "xent_fwd_bwd");
  return {ws.narrow(0, 0, 1).squeeze(0), dl};
}

// logits: contiguous [..., V], or a 2-D view whose rows are `stride(0)` elements apart (a slice of
// wider rows is read in place)
std::tuple<at::Tensor, at::Tensor> xent_eval(const at::Tensor& logits, const at::Tensor& labels,
                                             int64_t ignore_index) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16, "logits must be a bf16 GPU tensor");
  expect(labels, at::kLong, "labels");
  TORCH_CHECK(logits.dim() >= 1 && logits.size(-1) >= 1, "logits must be [..., V] with V >= 1");
  const int64_t V = logits.size(-1), M = logits.numel() / V;
  int64_t ld = V;
  if (logits.dim() == 2 && logits.stride(1) == 1 && logits.stride(0) >= V) ld = logits.stride(0);
  else TORCH_CHECK(logits.is_contiguous(), "logits must be contiguous or a 2-D view with unit column stride");
  TORCH_CHECK(labels.numel() == M, "labels has ", labels.numel(), " elements for ", M, " rows of logits");
  TORCH_CHECK(M <= INT32_MAX && V <= INT32_MAX, "xent_eval: too many rows or columns");
  auto row_loss = at::empty({M}, logits.options().dtype(at::kFloat));
  auto row_rank = at::empty({M}, logits.options().dtype(at::kInt));
  check(dl_xent_eval(cbf(logits), labels.data_ptr<long>(), f32(row_loss), row_rank.data_ptr<int>(), (int)M, (int)V, ld,
                     (int)ignore_index, cur_stream(logits)),
        "xent_eval");
  return {row_loss, row_rank};
}

// ------------------------------------------------------------------ kNN evaluation (knn.hip)
// Everything outside the kernels' domain raises here, before a launch.
std::tuple<at::Tensor, at::Tensor> knn_topk(const at::Tensor& q, const at::Tensor& bank, int64_t k, int64_t splits) {
  expect(q, at::kBFloat16, "q");
  expect(bank, at::kBFloat16, "bank");
  TORCH_CHECK(q.dim() == 2 && bank.dim() == 2 && q.size(1) == bank.size(1), "knn_topk: q [Q, D] and bank [N, D]");
  TORCH_CHECK(q.get_device() == bank.get_device(), "knn_topk: q and bank on different devices");
  const int64_t Q = q.size(0), N = bank.size(0), D = q.size(1);
  TORCH_CHECK(D % 16 == 0 && D >= 16 && D <= 4096, "knn_topk: D = ", D, " must be a multiple of 16 in 16 .. 4096");
  TORCH_CHECK(k >= 1 && k <= 256 && k <= N, "knn_topk: k = ", k, " must be in 1 .. min(256, N = ", N, ")");
  TORCH_CHECK(Q <= INT32_MAX && N <= INT32_MAX, "knn_topk: too many rows");
  const int max_splits = dl_knn_max_splits((int)N, (int)k);
  TORCH_CHECK(splits >= 0 && splits <= max_splits, "knn_topk: splits = ", splits, " must be 0 (automatic) or 1 .. ",
              max_splits, " for N = ", N, ", k = ", k);
  auto vals = at::empty({Q, k}, q.options().dtype(at::kFloat));
  auto idx = at::empty({Q, k}, q.options().dtype(at::kInt));
  if (Q == 0) return {vals, idx};
  int cus = 0;
  if (splits == 0)
    TORCH_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, q.get_device()) == hipSuccess,
                "knn_topk: cannot read the device's CU count");
  const int S = splits > 0 ? (int)splits : dl_knn_splits((int)Q, (int)N, (int)k, cus);
  auto lists = at::empty({dl_knn_list_entries((int)Q, (int)k, S)}, q.options().dtype(at::kLong));
  at::Tensor part;
  if (S > 1) part = at::empty({Q * S * k}, q.options().dtype(at::kLong));
  check(dl_knn_topk(cbf(q), cbf(bank), (int)Q, (int)N, (int)D, (int)k, S,
                    reinterpret_cast<unsigned long long*>(lists.data_ptr<int64_t>()),
                    S > 1 ? reinterpret_cast<unsigned long long*>(part.data_ptr<int64_t>()) : nullptr, f32(vals),
                    idx.data_ptr<int>(), cur_stream(q)),
        "knn_topk");
  return {vals, idx};
}

std::tuple<at::Tensor, at::Tensor> knn_vote(const at::Tensor& vals, const at::Tensor& idx, const at::Tensor& bank_labels,
                                            const at::Tensor& targets, int64_t num_classes, double sigma) {
  expect(vals, at::kFloat, "vals");
  expect(idx, at::kInt, "idx");
  expect(bank_labels, at::kInt, "bank_labels");
  expect(targets, at::kLong, "targets");
  TORCH_CHECK(vals.dim() == 2 && idx.sizes() == vals.sizes(), "knn_vote: vals and idx must both be [Q, k]");
  const int64_t Q = vals.size(0), k = vals.size(1), N = bank_labels.numel();
  TORCH_CHECK(k >= 1 && k <= 256, "knn_vote: k = ", k, " must be in 1 .. 256");
  TORCH_CHECK(targets.numel() == Q, "knn_vote: targets has ", targets.numel(), " elements for ", Q, " rows");
  TORCH_CHECK(N >= 1 && N <= INT32_MAX && Q <= INT32_MAX, "knn_vote: bank_labels must hold 1 .. 2^31 - 1 labels");
  TORCH_CHECK(num_classes >= 1 && num_classes <= 8192, "knn_vote: num_classes = ", num_classes, " must be in 1 .. 8192");
  TORCH_CHECK(sigma > 0, "knn_vote: sigma must be positive");
  auto pred = at::empty({Q}, vals.options().dtype(at::kInt));
  auto rank = at::empty({Q}, vals.options().dtype(at::kInt));
  check(dl_knn_vote(f32(vals), idx.data_ptr<int>(), bank_labels.data_ptr<int>(), targets.data_ptr<long>(),
                    pred.data_ptr<int>(), rank.data_ptr<int>(), (int)Q, (int)k, (int)N, (int)num_classes, (float)sigma,
                    cur_stream(vals)),
        "knn_vote");
  return {pred, rank};
}

// ------------------------------------------------------------------ attention
// Every fused call is one DlAttn descriptor (dl_kernels.h) handed to attn_route below, the only
// place that calls the launchers of attention.hip, attention_compact_q.hip and attention_hd128.hip.
inline const int* kvinfo_ptr(const c10::optional<at::Tensor>& kvinfo, int64_t B) {
  if (!kvinfo.has_value()) return nullptr;
  expect(*kvinfo, at::kInt, "kvinfo");
  TORCH_CHECK(kvinfo->numel() == B + 1, "kvinfo must be int32[B + 1] (lengths, prefix flag)");
  return kvinfo->data_ptr<int>();
}

// an optional fp32 tensor of n values (mbias [B, S], dbias [3*H*D]): its data, or null without one
inline float* opt_f32(const c10::optional<at::Tensor>& t, int64_t n, const char* name, const char* shape,
                      const char* what) {
  if (!t.has_value()) return nullptr;
  expect(*t, at::kFloat, name);
  TORCH_CHECK(t->numel() == n, what, ": ", name, " must be ", shape);
  return f32(*t);
}

// the fixed-S mask of a descriptor whose B and S are set
inline void fixed_mask(DlAttn& a, const c10::optional<at::Tensor>& mbias, const c10::optional<at::Tensor>& kvinfo,
                       const char* what) {
  a.mbias = opt_f32(mbias, (int64_t)a.B * a.S, "mbias", "[B, S]", what);
  a.kvinfo = kvinfo_ptr(kvinfo, a.B);
}

// The one place an attention kernel is chosen: head_dim 128 runs in attention_hd128.hip, head_dim
// 64 in attention.hip or, with compact queries, in attention_compact_q.hip.  There are no other
// fused kernels (ops.FUSED_HEAD_DIMS): every other head size goes through ops.attn_composed_*.
void attn_route(const DlAttn& a, bool bwd, const char* what, hipStream_t st) {
  if (a.q) {
    TORCH_CHECK(a.D == 64 && !a.seqinfo, "dedloc_amd: ", what,
                ": compact queries exist for head_dim 64 only, on the fixed-S layout");
    return check(bwd ? dl_attn_hd64q_bwd(a, st) : dl_attn_hd64q_fwd(a, st), what);
  }
  TORCH_CHECK((a.D == 64 || a.D == 128) && a.ld == 3L * a.H * a.D, "dedloc_amd: ", what, ": head_dim ", a.D,
              " (row length ", a.ld, ", ", a.H,
              " heads) is not supported by the fused attention kernels; supported head sizes are 64 and 128");
  if (a.D == 128) return check(bwd ? dl_attn_hd128_bwd(a, st) : dl_attn_hd128_fwd(a, st), what);
  check(bwd ? dl_attn_hd64_bwd(a, st) : dl_attn_hd64_fwd(a, st), what);
}

// the fused QKV buffer [rows, 3*H*D] of the forms without compact queries (attn_route checks the
// head size it implies) and the context's row length
inline DlAttn qkv_desc(const at::Tensor& qkv, int64_t H, double scale) {
  expect(qkv, at::kBFloat16, "qkv");
  DlAttn a;
  a.kv = cbf(qkv), a.ld = qkv.size(-1);
  a.H = (int)H, a.D = (int)(a.ld / (3 * H)), a.scale = (float)scale;
  a.ldo = H * a.D;
  return a;
}

// the backward's out / dout (`ctx` values each) and lse (`stats` values), as the forward returned them
inline void bwd_inputs(DlAttn& a, const at::Tensor& out, const at::Tensor& dout, const at::Tensor& lse, int64_t ctx,
                       int64_t stats, const char* what, const char* shapes) {
  expect(out, at::kBFloat16, "out");
  expect(dout, at::kBFloat16, "dout");
  expect(lse, at::kFloat, "lse");
  TORCH_CHECK(out.numel() == ctx && dout.numel() == ctx && lse.numel() == stats, what, ": out / dout must be ", shapes);
  a.out = bf(out), a.dout = cbf(dout), a.lse = f32(lse);
}

std::tuple<at::Tensor, at::Tensor> attn_fwd(const at::Tensor& qkv, const c10::optional<at::Tensor>& mbias, int64_t H,
                                            int64_t S, double scale, const c10::optional<at::Tensor>& kvinfo) {
  DlAttn a = qkv_desc(qkv, H, scale);
  const int64_t T = qkv.numel() / a.ld, B = T / S;
  auto out = at::empty({T, a.ldo}, qkv.options());
  auto lse = at::empty({B, H, S}, qkv.options().dtype(at::kFloat));
  a.B = (int)B, a.S = (int)S;
  fixed_mask(a, mbias, kvinfo, "attn_fwd");
  a.out = bf(out), a.lse = f32(lse);
  attn_route(a, false, "attn_fwd", cur_stream(qkv));
  return {out, lse};
}

at::Tensor attn_bwd(const at::Tensor& qkv, const c10::optional<at::Tensor>& mbias, const at::Tensor& out,
                    const at::Tensor& dout, const at::Tensor& lse, int64_t H, int64_t S, double scale,
                    const c10::optional<at::Tensor>& kvinfo, const c10::optional<at::Tensor>& dbias) {
  DlAttn a = qkv_desc(qkv, H, scale);
  const int64_t T = qkv.numel() / a.ld, B = T / S;
  bwd_inputs(a, out, dout, lse, T * a.ldo, B * H * S, "attn_bwd", "[B*S, H*D] and lse [B, H, S]");
  auto dqkv = at::empty_like(qkv);
  auto delta = at::empty({B, H, S}, qkv.options().dtype(at::kFloat));
  a.B = (int)B, a.S = (int)S;
  fixed_mask(a, mbias, kvinfo, "attn_bwd");
  a.delta = f32(delta), a.dqkv = bf(dqkv);
  a.dbias = opt_f32(dbias, a.ld, "dbias", "3*H*D values", "attn_bwd");
  attn_route(a, true, "attn_bwd", cur_stream(qkv));
  return dqkv;
}

// Compact queries: q [B*Sq, H*64] holds sequence b's queries in the first qcnt[b] rows of its slot of
// Sq rows; kv [B*S, 2*H*64] (K | V) may be a column slice of the fused QKV buffer (any row stride).
inline DlAttn compact_layout(const at::Tensor& q, const at::Tensor& kv, const at::Tensor& qcnt, int64_t H, int64_t S,
                             double scale, const char* what) {
  expect(q, at::kBFloat16, "q");
  expect(qcnt, at::kInt, "qcnt");
  TORCH_CHECK(kv.is_cuda() && kv.scalar_type() == at::kBFloat16 && kv.dim() == 2 && kv.stride(1) == 1, what,
              ": kv must be a 2-D bf16 GPU tensor with unit column stride");
  TORCH_CHECK(H >= 1 && S >= 64 && S % 64 == 0, what, ": S = ", S, " must be a positive multiple of 64");
  const int64_t T = kv.size(0), B = T / S, D = kv.size(1) / (2 * H), ld = kv.stride(0);
  TORCH_CHECK(D == 64 && kv.size(1) == 2 * H * D, "dedloc_amd: ", what, ": compact queries exist for head_dim 64 only (kv has ",
              kv.size(1), " columns for ", H, " heads)");
  TORCH_CHECK(B >= 1 && B * S == T, what, ": kv must have B*S rows");
  TORCH_CHECK(ld >= 2 * H * D && ld % 8 == 0 && reinterpret_cast<uintptr_t>(kv.data_ptr()) % 16 == 0, what,
              ": kv rows must be 16-byte aligned");
  TORCH_CHECK(q.dim() == 2 && q.size(1) == H * D && q.size(0) % B == 0, what, ": q must be [B*Sq, H*D]");
  const int64_t Sq = q.size(0) / B;
  TORCH_CHECK(Sq >= 64 && Sq % 64 == 0 && Sq <= S, what, ": the query slot Sq = ", Sq,
              " must be a multiple of 64 in 64 .. S = ", S);
  TORCH_CHECK(qcnt.numel() == B, what, ": qcnt must be int32[B]");
  DlAttn a;
  a.kv = reinterpret_cast<const bf16_t*>(kv.data_ptr()), a.ld = ld;
  a.q = cbf(q), a.qcnt = qcnt.data_ptr<int>(), a.Sq = (int)Sq;
  a.B = (int)B, a.H = (int)H, a.S = (int)S, a.D = (int)D, a.scale = (float)scale;
  a.ldo = H * D;
  return a;
}

std::tuple<at::Tensor, at::Tensor> attn_fwd_q(const at::Tensor& q, const at::Tensor& kv, const at::Tensor& qcnt,
                                              const c10::optional<at::Tensor>& mbias, int64_t H, int64_t S,
                                              double scale, const c10::optional<at::Tensor>& kvinfo) {
  DlAttn a = compact_layout(q, kv, qcnt, H, S, scale, "attn_fwd_q");
  fixed_mask(a, mbias, kvinfo, "attn_fwd_q");
  auto out = at::empty({(int64_t)a.B * a.Sq, a.ldo}, q.options());
  auto lse = at::empty({a.B, H, a.Sq}, q.options().dtype(at::kFloat));
  a.out = bf(out), a.lse = f32(lse);
  attn_route(a, false, "attn_fwd_q", cur_stream(q));
  return {out, lse};
}

// returns (dq [B*Sq, H*D], dkv [B*S, 2*H*D], delta [B, H, Sq]); past qcnt[b] dq rows are zero and
// delta entries are not written
std::tuple<at::Tensor, at::Tensor, at::Tensor> attn_bwd_q(const at::Tensor& q, const at::Tensor& kv,
                                                          const at::Tensor& qcnt,
                                                          const c10::optional<at::Tensor>& mbias,
                                                          const at::Tensor& out, const at::Tensor& dout,
                                                          const at::Tensor& lse, int64_t H, int64_t S, double scale,
                                                          const c10::optional<at::Tensor>& kvinfo,
                                                          const c10::optional<at::Tensor>& dbias) {
  DlAttn a = compact_layout(q, kv, qcnt, H, S, scale, "attn_bwd_q");
  fixed_mask(a, mbias, kvinfo, "attn_bwd_q");
  bwd_inputs(a, out, dout, lse, q.numel(), (int64_t)a.B * H * a.Sq, "attn_bwd_q", "[B*Sq, H*D] and lse [B, H, Sq]");
  auto dq = at::empty_like(q);
  auto dkv = at::empty({(int64_t)a.B * S, 2 * a.ldo}, q.options());
  auto delta = at::empty({a.B, H, a.Sq}, q.options().dtype(at::kFloat));
  a.delta = f32(delta), a.dq = bf(dq), a.dkv = bf(dkv);
  a.dbias = opt_f32(dbias, 3 * a.ldo, "dbias", "3*H*D values", "attn_bwd_q");
  attn_route(a, true, "attn_bwd_q", cur_stream(q));
  return {dq, dkv, delta};
}

// Packed variable-length batches.  seqinfo (device) = int32[2B + 1]: B + 1 row offsets, then B key
// lengths; seqinfo_host is the same array in host memory — the layout contract is checked on it, so
// a call costs no device synchronisation, and the largest slot (the grids' x extent) is read from it.
inline void packed_layout(DlAttn& a, const at::Tensor& seqinfo, const at::Tensor& seqinfo_host, int64_t T,
                          const char* what) {
  expect(seqinfo, at::kInt, "seqinfo");
  TORCH_CHECK(seqinfo_host.device().is_cpu() && seqinfo_host.scalar_type() == at::kInt && seqinfo_host.is_contiguous(),
              what, ": seqinfo_host must be a contiguous int32 CPU tensor");
  const int64_t n = seqinfo_host.numel();
  TORCH_CHECK(n >= 3 && n % 2 == 1 && seqinfo.numel() == n, what,
              ": seqinfo must be int32[2B + 1] (B + 1 row offsets, B lengths) on both sides");
  const int64_t B = (n - 1) / 2;
  const int* p = seqinfo_host.data_ptr<int>();
  TORCH_CHECK(p[0] == 0 && p[B] == T, what, ": row offsets must run from 0 to T = ", T, " (got ", p[0], " .. ", p[B],
              ")");
  int64_t max_slot = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t slot = (int64_t)p[b + 1] - p[b], len = p[B + 1 + b];
    TORCH_CHECK(p[b] % 64 == 0 && p[b + 1] % 64 == 0, what, ": row offset of sequence ", b,
                " is not a multiple of 64 (", p[b], ", ", p[b + 1], ")");
    TORCH_CHECK(slot >= 64, what, ": sequence ", b, " has an empty slot");
    TORCH_CHECK(len >= 1 && len <= slot, what, ": length ", len, " of sequence ", b, " is outside 1 .. its slot of ",
                slot, " rows");
    max_slot = std::max(max_slot, slot);
  }
  a.seqinfo = seqinfo.data_ptr<int>(), a.B = (int)B, a.T = (int)T, a.max_slot = (int)max_slot;
}

std::tuple<at::Tensor, at::Tensor> attn_varlen_fwd(const at::Tensor& qkv, const at::Tensor& seqinfo,
                                                   const at::Tensor& seqinfo_host, int64_t H, double scale) {
  DlAttn a = qkv_desc(qkv, H, scale);
  const int64_t T = qkv.numel() / a.ld;
  packed_layout(a, seqinfo, seqinfo_host, T, "attn_varlen_fwd");
  auto out = at::empty({T, a.ldo}, qkv.options());
  auto lse = at::empty({H, T}, qkv.options().dtype(at::kFloat));
  a.out = bf(out), a.lse = f32(lse);
  attn_route(a, false, "attn_varlen_fwd", cur_stream(qkv));
  return {out, lse};
}

at::Tensor attn_varlen_bwd(const at::Tensor& qkv, const at::Tensor& seqinfo, const at::Tensor& seqinfo_host,
                           const at::Tensor& out, const at::Tensor& dout, const at::Tensor& lse, int64_t H,
                           double scale, const c10::optional<at::Tensor>& dbias) {
  DlAttn a = qkv_desc(qkv, H, scale);
  const int64_t T = qkv.numel() / a.ld;
  packed_layout(a, seqinfo, seqinfo_host, T, "attn_varlen_bwd");
  bwd_inputs(a, out, dout, lse, T * a.ldo, H * T, "attn_varlen_bwd", "[T, H*D] and lse [H, T]");
  auto dqkv = at::empty_like(qkv);
  auto delta = at::empty({H, T}, qkv.options().dtype(at::kFloat));
  a.delta = f32(delta), a.dqkv = bf(dqkv);
  a.dbias = opt_f32(dbias, a.ld, "dbias", "3*H*D values", "attn_varlen_bwd");
  attn_route(a, true, "attn_varlen_bwd", cur_stream(qkv));
  return dqkv;
}

// composed attention (head sizes other than 64): row softmax over GEMM-produced fp32 scores
std::tuple<at::Tensor, at::Tensor> attn_softmax_fwd(const at::Tensor& s, const c10::optional<at::Tensor>& mbias,
                                                    int64_t H, double c) {
  expect(s, at::kFloat, "s");
  const int64_t S = s.size(-1), rows = s.numel() / S;
  TORCH_CHECK(rows % (H * S) == 0, "attn_softmax_fwd: scores must be [B*H*S, S]");
  const float* mb = nullptr;
  if (mbias.has_value()) {
    expect(*mbias, at::kFloat, "mbias");
    TORCH_CHECK(mbias->numel() == rows / H, "attn_softmax_fwd: mbias must be [B, S]");
    mb = f32(*mbias);
  }
  auto p = at::empty(s.sizes(), s.options().dtype(at::kBFloat16));
  auto lse = at::empty({rows}, s.options());
  check(dl_attn_softmax_fwd(f32(s), mb, bf(p), f32(lse), rows, (int)H, (int)S, (float)c, cur_stream(s)),
        "attn_softmax_fwd");
  return {p, lse};
}

std::tuple<at::Tensor, at::Tensor> attn_softmax_bwd(const at::Tensor& s, const at::Tensor& dp,
                                                    const c10::optional<at::Tensor>& mbias, const at::Tensor& lse,
                                                    const at::Tensor& delta, int64_t H, double c, double scale) {
  expect(s, at::kFloat, "s");
  expect(dp, at::kFloat, "dp");
  expect(lse, at::kFloat, "lse");
  expect(delta, at::kFloat, "delta");
  const int64_t S = s.size(-1), rows = s.numel() / S;
  TORCH_CHECK(dp.numel() == s.numel() && lse.numel() == rows && delta.numel() == rows && rows % (H * S) == 0,
              "attn_softmax_bwd: shape mismatch");
  const float* mb = nullptr;
  if (mbias.has_value()) {
    expect(*mbias, at::kFloat, "mbias");
    TORCH_CHECK(mbias->numel() == rows / H, "attn_softmax_bwd: mbias must be [B, S]");
    mb = f32(*mbias);
  }
  auto p = at::empty(s.sizes(), s.options().dtype(at::kBFloat16));
  auto ds = at::empty_like(p);
  check(dl_attn_softmax_bwd(f32(s), f32(dp), mb, f32(lse), f32(delta), bf(p), bf(ds), rows, (int)H, (int)S, (float)c,
                            (float)scale, cur_stream(s)),
        "attn_softmax_bwd");
  return {p, ds};
}

// ------------------------------------------------------------------ GEMM
// Every GPU GEMM runs on this repository's MFMA kernels (bf16 in, fp32 accumulation):
//   gemm8.hip      LDS-DMA 8-phase pipeline, 256x256 tiles — every ALBERT layer GEMM, fused
//                  epilogues (bias, residual, bias + GELU, GELU' + bias gradient, fp32 split-K slabs)
//   gemm.hip       register-staged 256x256 tiles — tiled shapes outside gemm8's contract
//                  (N % 256 != 0: the SwAV 1x1 convs with 64 / 128 outputs, the stem)
//   gemm_small.hip any shape and stride, 128x128 tiles with a slab-split reduction — the rest
//                  (N = 128 embedding GEMMs, the tied MLM decoder's gradients, SwAV prototypes)
// There is no vendor-library or ATen path: a shape no kernel takes is an error, not a fallback.
// The fp32-accumulating weight-gradient form writes straight into the fp32 gradient buffer, so the
// shared ALBERT layer's 24 weight-gradient contributions never round through bf16.
// Every call is one DlGemm descriptor (dl_kernels.h) handed to gemm_route below, the only place
// that calls the three launchers; docs/KERNELS.md "GEMM dispatch" has the rules per call site.

// Which kernel took each GEMM of this section: process-wide launch counts, bumped where a launcher
// returned 0 (host side only: no effect on dispatch, no synchronisation).  The tests read them
// before and after a call (`dedloc_ws::gemm_backend_counts()`), so a contract check that turns too
// strict and silently moves a shape to a slower kernel fails a test.
enum { kGemmNone = -1, kGemm8 = 0, kGemmTiled = 1, kGemmSmall = 2 };
std::atomic<int64_t> g_gemm_backend[3];

inline int took(int backend, int rc) {
  if (rc == 0) g_gemm_backend[backend].fetch_add(1, std::memory_order_relaxed);
  return rc;
}

std::vector<int64_t> gemm_backend_counts() {  // {gemm8.hip, gemm.hip, gemm_small.hip}
  return {g_gemm_backend[kGemm8].load(), g_gemm_backend[kGemmTiled].load(), g_gemm_backend[kGemmSmall].load()};
}

inline void expect_operands(const at::Tensor& a, const at::Tensor& b) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda(), "gemm operands must be GPU tensors");
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 && b.scalar_type() == at::kBFloat16, "gemm operands must be bf16");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.stride(1) == 1 && b.stride(1) == 1,
              "gemm operands must be 2-D with unit inner stride");
}

inline at::Tensor f32_bias(const c10::optional<at::Tensor>& bias, int64_t n) {
  if (!bias.has_value()) return at::Tensor();
  TORCH_CHECK(bias->numel() == n, "gemm bias must hold one value per output column");
  return bias->scalar_type() == at::kFloat ? bias->contiguous() : bias->to(at::kFloat).contiguous();
}

// The operands and extents of op(a) op(b) with its bf16 output; the caller names the epilogue and
// that epilogue's fields.  op(a) is [M, K]: a itself, or with trans_a its transpose (a is [K, M], a
// K-outer operand).  op(b) is [K, N]: with trans_b b is [N, K] (K-inner), else [K, N] (K-outer).
inline DlGemm gemm_desc(const at::Tensor& a, bool trans_a, const at::Tensor& b, bool trans_b, bf16_t* C = nullptr,
                        long ldc = 0) {
  DlGemm g;
  g.A = cbf(a), g.lda = a.stride(0), g.a_kouter = trans_a;
  g.B = cbf(b), g.ldb = b.stride(0), g.b_kouter = !trans_b;
  g.M = (int)a.size(trans_a ? 1 : 0), g.N = (int)b.size(trans_b ? 0 : 1), g.K = (int)a.size(trans_a ? 0 : 1);
  TORCH_CHECK(b.size(trans_b ? 1 : 0) == g.K, "gemm inner dimensions differ");
  g.C = C, g.ldc = ldc;
  return g;
}

// The one place a GEMM kernel is chosen.  Tries the kernels `allow` permits in the fixed order
// gemm8 -> gemm.hip -> gemm_small, each with the descriptor as the caller filled it, and returns the
// one that took the call (counted) or kGemmNone.  gemm_small's reduction split is its own
// (dl_gemm_small_splits, replacing g.splits), with the fp32 slab workspace from the caching
// allocator on `like`'s device when it splits; its split form has no statistics epilogue, so a
// descriptor with `stats` is refused there before anything is allocated.
enum : unsigned { kUse8 = 1, kUseTiled = 2, kUseSmall = 4 };
int gemm_route(const DlGemm& g, unsigned allow, const at::Tensor& like, hipStream_t st) {
  if ((allow & kUse8) && took(kGemm8, dl_gemm8(g, st)) == 0) return kGemm8;
  if ((allow & kUseTiled) && took(kGemmTiled, dl_gemm(g, st)) == 0) return kGemmTiled;
  if (!(allow & kUseSmall)) return kGemmNone;
  DlGemm s = g;
  s.splits = dl_gemm_small_splits(g.M, g.N, g.K);
  if (s.splits > 1 && g.stats) return kGemmNone;
  at::Tensor ws;
  if (s.splits > 1) ws = at::empty({(int64_t)s.splits * g.M * g.N}, like.options().dtype(at::kFloat));
  return took(kGemmSmall, dl_gemm_small(s, s.splits > 1 ? f32(ws) : nullptr, st)) == 0 ? kGemmSmall : kGemmNone;
}

// C (bf16) = op(A) op(B) (+ bias) (+ R): gemm8 where its contract holds; outputs of at most 192
// columns (1x1 convs with 64 / 128 channels, the stem, ALBERT's 128-wide embedding side) on
// gemm_small's 128x64 / 128x128 tiles (a 256-wide tile would waste half to three quarters of its
// MFMAs); the register-staged 256x256 gemm.hip for the remaining wide shapes; gemm_small last.
void gemm_store(const DlGemm& g, const at::Tensor& like, hipStream_t st) {
  TORCH_CHECK(gemm_route(g, kUse8 | (g.N > 192 ? kUseTiled : 0) | kUseSmall, like, st) != kGemmNone,
              "dedloc_amd: unsupported shape for gemm");
}

// gemm_store plus the BatchNorm statistics of the stored values (stats [M / stat_rows][2N], fp32,
// accumulated): in the GEMM epilogue where the kernel takes it (gemm8's STATS for N % 256 == 0,
// gemm_small's unsplit store for the narrow outputs), else one statistics pass over C afterwards
void gemm_store_stats(DlGemm g, float* stats, long stat_rows, const at::Tensor& like, hipStream_t st) {
  g.stats = stats, g.stat_rows = stat_rows;
  g.epi = DL_EPI_STATS;
  if (gemm_route(g, kUse8, like, st) != kGemmNone) return;
  g.epi = DL_EPI_STORE;
  if (g.N <= 192 && gemm_route(g, kUseSmall, like, st) != kGemmNone) return;
  g.stats = nullptr;
  gemm_store(g, like, st);
  TORCH_CHECK(g.ldc == g.N, "gemm_store_stats: the statistics pass needs a dense C");
  check(dl_bn_stats(g.C, stats, stat_rows, g.N, (int)(g.M / stat_rows), st), "bn_stats");
}

// out[b] = a[b] @ b[b] (torch.bmm semantics; any element strides, e.g. transposed views, read in
// place) on gemm_small's batched launch: bf16 out, or fp32 with out_f32 (the composed attention's
// scores).  One launch for the whole batch.
at::Tensor bmm(const at::Tensor& a, const at::Tensor& b, bool out_f32) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.scalar_type() == at::kBFloat16 && b.scalar_type() == at::kBFloat16,
              "bmm: bf16 GPU operands");
  TORCH_CHECK(a.dim() == 3 && b.dim() == 3 && a.size(0) == b.size(0) && a.size(2) == b.size(1), "bmm: shapes");
  const int64_t Bn = a.size(0), M = a.size(1), K = a.size(2), N = b.size(2);
  auto out = at::empty({Bn, M, N}, a.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
  if (Bn == 0 || M == 0 || N == 0) return out;
  if (K == 0) return out.zero_();
  check(took(kGemmSmall,
             dl_gemm_small_batched(out_f32 ? 1 : 0, cbf(a), a.stride(1), a.stride(2), a.stride(0), cbf(b), b.stride(2),
                                   b.stride(1), b.stride(0), (int)M, (int)N, (int)K, out_f32 ? nullptr : bf(out), N,
                                   out_f32 ? f32(out) : nullptr, N, M * N, (int)Bn, cur_stream(a))),
        "bmm");
  return out;
}

at::Tensor gemm(const at::Tensor& a, const at::Tensor& b, const c10::optional<at::Tensor>& bias,
                const c10::optional<at::Tensor>& residual, bool trans_a, bool trans_b, int64_t epilogue) {
  expect_operands(a, b);
  DlGemm g = gemm_desc(a, trans_a, b, trans_b);
  if (residual.has_value()) {
    TORCH_CHECK(residual->scalar_type() == at::kBFloat16 && residual->is_contiguous() &&
                    residual->size(0) == g.M && residual->size(1) == g.N,
                "gemm residual must be a contiguous bf16 [M, N] tensor");
  }
  auto c = at::empty({g.M, g.N}, a.options());
  const at::Tensor bias32 = f32_bias(bias, g.N);
  g.C = bf(c), g.ldc = g.N;
  if (bias32.defined()) g.bias = f32(bias32);
  if (residual.has_value()) g.R = cbf(*residual), g.ldr = g.N;
  gemm_store(g, a, cur_stream(a));
  if (epilogue == 1) check(dl_gelu_fwd(cbf(c), bf(c), c.numel(), cur_stream(c)), "gemm gelu epilogue");
  return c;
}

// fp32-accumulating weight gradient c += op(a) op(b) through gemm8: the token (reduction) dimension
// is split into S slices written as fp32 slabs and summed into c (no atomics).
// Weight gradients have few output tiles (48 for ALBERT's QKV) and a very long reduction (the
// tokens), so the reduction is split into S slices; S is chosen for whole waves of workgroups on
// the 256 CUs (one gemm8 workgroup per CU): 48 tiles x 8 slices = 384 workgroups would leave half
// the chip idle for the second half of the kernel, 48 x 16 = 768 = 3 full waves does not.  Among
// the splits with at least 1024 reduction rows per slice, the best wave efficiency wins, the
// smaller S on ties (fewer slab bytes to sum).
#ifndef DL_WGRAD_CUS
#define DL_WGRAD_CUS 256  // CUs one weight gradient is split to fill (a measurement build may override)
#endif
int wgrad_splits8(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = ((M + 255) / 256) * ((N + 255) / 256);
  // any S dividing the K-tile count, each slice at least 4 K-tiles (8 while S > 32).  SwAV's 14x14
  // maps: 25088 tokens = 392 K-tiles = 2^3 7^2 with one output tile get S = 49 (49 workgroups of 8
  // K-tiles, where powers of two stop at 32); S = 56 would leave 7 K-tiles per slice, below the floor
  constexpr int64_t kCUs = DL_WGRAD_CUS;
  const int64_t ktiles = K / 64;
  if (K % 64) return 1;
  int best = 1;
  double best_eff = 0.0;
  for (int S = 1; S <= 64; ++S) {
    if (ktiles % S) continue;
    if (S > 1 && ktiles / S < (S > 32 ? 8 : 4)) break;
    const int64_t wg = tiles * S;
    const double eff = (double)wg / (double)(kCUs * ((wg + kCUs - 1) / kCUs));
    if (eff > best_eff + 1e-9) {
      best_eff = eff;
      best = S;
    }
  }
  return best;
}

// the split count gemm8's weight gradient c [M, N] += over K tokens takes (host arithmetic only)
int64_t gemm_wgrad_splits(int64_t M, int64_t N, int64_t K) { return wgrad_splits8(M, N, K); }

// gemm8's weight-gradient form: reduction slice z of S writes (accumulate: adds to) slab z of the
// dense fp32 [S, M, N] at `out`.  False when gemm8 refuses the shape.
bool wgrad8(DlGemm g, float* out, int S, bool accumulate, const at::Tensor& like, hipStream_t st) {
  g.epi = DL_EPI_F32;
  g.Cf = out, g.ldcf = g.N, g.slab = S > 1 ? (long)g.M * g.N : 0, g.accumulate = accumulate;
  g.splits = S;
  return gemm_route(g, kUse8, like, st) == kGemm8;
}

void gemm_acc_f32(const at::Tensor& a, const at::Tensor& b, at::Tensor c, bool trans_a, bool trans_b) {
  expect_operands(a, b);
  TORCH_CHECK(c.is_cuda() && c.scalar_type() == at::kFloat && c.dim() == 2 && c.stride(1) == 1,
              "gemm_acc_f32: c must be an fp32 [M, N] GPU tensor with unit inner stride");
  DlGemm g = gemm_desc(a, trans_a, b, trans_b);
  TORCH_CHECK(c.size(0) == g.M && c.size(1) == g.N, "gemm_acc_f32: c shape mismatch");
  const hipStream_t st = cur_stream(a);
  if (c.is_contiguous()) {  // gemm8 writes dense slabs: c itself when it does not split
    const int S = wgrad_splits8(g.M, g.N, g.K);
    const at::Tensor slabs = S > 1 ? at::empty({S, g.M, g.N}, c.options()) : c;
    if (wgrad8(g, f32(slabs), S, S == 1, a, st)) {
      if (S > 1) check(dl_sum_slabs(f32(c), f32(slabs), S, (size_t)c.numel(), st), "sum_slabs");
      return;
    }
  }
  // gemm.hip: split the long reduction over ~2 workgroups per CU, fp32 atomics into c; gemm_small last
  const int64_t tiles = ((g.M + 255) / 256) * ((g.N + 255) / 256);
  g.epi = DL_EPI_F32;
  g.Cf = f32(c), g.ldcf = c.stride(0), g.accumulate = 1;
  g.splits = (int)std::max<int64_t>(1, std::min<int64_t>(g.K / 1024, (512 + tiles - 1) / tiles));
  TORCH_CHECK(gemm_route(g, kUseTiled | kUseSmall, a, st) != kGemmNone,
              "dedloc_amd: unsupported shape for gemm_acc_f32");
}

// Weight gradient of a weight that several consecutive backward calls share (ALBERT's one layer,
// applied 24 times): gemm8's token-split fp32 slabs persist across the calls — the first call
// writes them, later calls accumulate into them (the kernel's EPI_F32 accumulate form) — and are
// added into the gradient once, by the last call: one slab-sum pass per weight and micro-step
// instead of 24.  The slab workspace of one gradient tensor lives from the first to the last call,
// so it is keyed by the gradient (pointer, device, shape, split count); the cache is bounded: when a
// new key would exceed kMaxSlabSets entries (gradient buffers re-allocated, several models in one
// process) the least recently used workspace is freed; `dedloc_ws::clear_workspaces()` frees all.
struct SlabKey {
  const void* ptr;
  int64_t dev, S, M, N;
  bool operator==(const SlabKey& o) const {
    return ptr == o.ptr && dev == o.dev && S == o.S && M == o.M && N == o.N;
  }
};
struct SlabKeyHash {
  size_t operator()(const SlabKey& k) const {
    return std::hash<const void*>()(k.ptr) ^ (size_t)(k.S * 1000003 + k.M * 10007 + k.N * 31 + k.dev);
  }
};
constexpr size_t kMaxSlabSets = 16;
struct SlabSet {
  at::Tensor slabs;
  uint64_t used = 0;  // LRU clock
  bool live = false;  // holds partial sums of the current series (not yet added into c)
};
std::mutex g_slab_mu;
std::unordered_map<SlabKey, SlabSet, SlabKeyHash> g_slabs;
uint64_t g_slab_clock = 0;

SlabSet& shared_slabs(const at::Tensor& c, int64_t S) {
  std::lock_guard<std::mutex> lock(g_slab_mu);
  const SlabKey key{c.data_ptr(), (int64_t)c.get_device(), S, c.size(0), c.size(1)};
  auto it = g_slabs.find(key);
  if (it == g_slabs.end()) {
    while (g_slabs.size() >= kMaxSlabSets) {
      auto lru = g_slabs.begin();
      for (auto j = g_slabs.begin(); j != g_slabs.end(); ++j)
        if (j->second.used < lru->second.used) lru = j;
      g_slabs.erase(lru);
    }
    it = g_slabs.emplace(key, SlabSet{at::empty({S, c.size(0), c.size(1)}, c.options())}).first;
  }
  it->second.used = ++g_slab_clock;
  return it->second;
}

int64_t clear_workspaces() {
  std::lock_guard<std::mutex> lock(g_slab_mu);
  const int64_t n = (int64_t)g_slabs.size();
  g_slabs.clear();
  return n;
}

void gemm_acc_f32_shared(const at::Tensor& a, const at::Tensor& b, at::Tensor c, bool trans_a, bool trans_b,
                         bool first, bool last) {
  expect_operands(a, b);
  TORCH_CHECK(c.is_cuda() && c.scalar_type() == at::kFloat, "gemm_acc_f32_shared: c must be fp32");
  const DlGemm g = gemm_desc(a, trans_a, b, trans_b);
  TORCH_CHECK(c.size(0) == g.M && c.size(1) == g.N, "gemm_acc_f32_shared: shape mismatch");
  const int S = c.is_contiguous() ? wgrad_splits8(g.M, g.N, g.K) : 1;
  if (S > 1) {
    SlabSet& set = shared_slabs(c, S);
    if (first) set.live = false;
    // a shape gemm8 refuses (small heads, odd widths) falls through to the direct fp32 accumulation;
    // slabs that hold this series' earlier partial sums are still added by the last call
    if (wgrad8(g, f32(set.slabs), S, set.live, a, cur_stream(a))) set.live = true;
    else gemm_acc_f32(a, b, c, trans_a, trans_b);
    if (last && set.live) {
      check(dl_sum_slabs(f32(c), f32(set.slabs), S, (size_t)c.numel(), cur_stream(a)), "sum_slabs");
      set.live = false;
    }
    return;
  }
  gemm_acc_f32(a, b, c, trans_a, trans_b);
}

// fused FFN-up: h = bf16(x W^T + b), G = gelu_new(h), and for the backward either h itself
// (gemm_gelu) or, with `deriv`, D = gelu_new'(h) (gemm_gelu_d, gemm8 only: the backward then
// multiplies by D instead of evaluating gelu_new' — gemm_dmul).  trans_w: w holds W^T ([in, out]: a
// K-outer B operand) instead of W ([out, in], K-inner).  Returns (h or D, G).
std::tuple<at::Tensor, at::Tensor> ffn_up(const at::Tensor& x, const at::Tensor& w, const at::Tensor& bias,
                                          bool trans_w, bool deriv) {
  expect_operands(x, w);
  const int64_t nout = trans_w ? w.size(1) : w.size(0);
  auto H = at::empty({x.size(0), nout}, x.options());
  auto G = at::empty_like(H);
  const at::Tensor bias32 = f32_bias(bias, nout);
  const hipStream_t st = cur_stream(x);
  DlGemm g = gemm_desc(x, false, w, !trans_w, bf(G), nout);
  g.epi = deriv ? DL_EPI_GELUD : DL_EPI_GELU;
  g.bias = f32(bias32);
  g.H = bf(H), g.ldh = nout;
  if (gemm_route(g, deriv ? kUse8 : kUse8 | kUseTiled, x, st) != kGemmNone) return {H, G};
  const at::Tensor pre = deriv ? at::empty_like(H) : H;  // unfused: the plain store, then the elementwise kernel
  g.epi = DL_EPI_STORE;
  g.C = bf(pre), g.H = nullptr;
  gemm_store(g, x, st);
  if (deriv) check(dl_gelu_fwd_d(cbf(pre), bf(G), bf(H), pre.numel(), st), "gelu_fwd_d");
  else check(dl_gelu_fwd(cbf(pre), bf(G), pre.numel(), st), "gelu_fwd");
  return {H, G};
}
std::tuple<at::Tensor, at::Tensor> gemm_gelu(const at::Tensor& x, const at::Tensor& w, const at::Tensor& bias,
                                             bool trans_w) {
  return ffn_up(x, w, bias, trans_w, false);
}
std::tuple<at::Tensor, at::Tensor> gemm_gelu_d(const at::Tensor& x, const at::Tensor& w, const at::Tensor& bias,
                                               bool trans_w) {
  return ffn_up(x, w, bias, trans_w, true);
}

// fused FFN dgrad: C = bf16(dy W) * gelu_new'(F) (gemm_dgelu; F the pre-activation) or, with `deriv`,
// C = bf16(dy W) * F (gemm_dmul, gemm8 only; F the derivative gemm_gelu_d stored); dbias += colsum(C).
// trans_w: w holds W^T (the forward-layout copy, a K-inner operand for the tiled kernels)
at::Tensor ffn_dgrad(const char* op, const at::Tensor& dy, const at::Tensor& w, const at::Tensor& F, at::Tensor dbias,
                     bool trans_w, bool deriv) {
  expect_operands(dy, w);
  expect(F, at::kBFloat16, deriv ? "D" : "F");
  expect(dbias, at::kFloat, "dbias");
  const int64_t nout = trans_w ? w.size(0) : w.size(1);
  TORCH_CHECK(dbias.is_contiguous() && dbias.numel() == nout, op, ": dbias must hold one fp32 per output column");
  TORCH_CHECK(F.dim() == 2 && F.size(0) == dy.size(0) && F.size(1) == nout, op, ": ", deriv ? "D" : "F", " shape");
  auto C = at::empty({dy.size(0), nout}, dy.options());
  const hipStream_t st = cur_stream(dy);
  DlGemm g = gemm_desc(dy, false, w, trans_w, bf(C), nout);
  g.epi = deriv ? DL_EPI_DMUL : DL_EPI_DGELU;
  g.R = cbf(F), g.ldr = nout;
  g.dbias = f32(dbias);
  if (gemm_route(g, deriv ? kUse8 : kUse8 | kUseTiled, dy, st) != kGemmNone) return C;
  auto dg = at::empty_like(C);  // unfused: the plain store, then the elementwise kernel
  g.epi = DL_EPI_STORE;
  g.C = bf(dg), g.R = nullptr, g.dbias = nullptr;
  gemm_store(g, dy, st);
  const int M = (int)dg.size(0), N = (int)nout;
  if (deriv) check(dl_mul_colsum(cbf(dg), cbf(F), bf(C), f32(dbias), M, N, st), "mul_colsum");
  else check(dl_gelu_bwd_colsum(cbf(dg), cbf(F), bf(C), f32(dbias), M, N, st), "gelu_bwd");
  return C;
}
at::Tensor gemm_dgelu(const at::Tensor& dy, const at::Tensor& w, const at::Tensor& F, at::Tensor dbias,
                      bool trans_w) {
  return ffn_dgrad("gemm_dgelu", dy, w, F, dbias, trans_w, false);
}
at::Tensor gemm_dmul(const at::Tensor& dy, const at::Tensor& w, const at::Tensor& D, at::Tensor dbias, bool trans_w) {
  return ffn_dgrad("gemm_dmul", dy, w, D, dbias, trans_w, true);
}

// ------------------------------------------------------------------ SwAV
at::Tensor sinkhorn(const at::Tensor& scores, int64_t bs, double eps, int64_t iters) {
  expect(scores, at::kFloat, "scores");
  const int64_t n = scores.size(0), K = scores.size(1);
  TORCH_CHECK(bs <= n, "bs > rows");
  auto Q = at::empty({bs, K}, scores.options());
  auto ws = at::empty({(int64_t)dl_sinkhorn_ws((int)n, (int)K)}, scores.options());
  check(dl_sinkhorn(f32(scores), f32(Q), f32(ws), (int)n, (int)K, (int)bs, (float)eps, (int)iters,
                    cur_stream(scores)),
        "sinkhorn");
  return Q;
}

// every (assignment crop, other crop) pair of the SwAV loss in one launch: scores [num_crops * bs, K]
// (bf16 / fp32), q [n_assign, bs, K] fp32, crops = the assignments' crop ids; ds [num_crops * bs, K]
// fp32 is written, loss [1] accumulated
void swav_ce_multi(const at::Tensor& scores, const at::Tensor& q, at::IntArrayRef crops, at::Tensor dscores,
                   at::Tensor loss, double temperature, double scale) {
  TORCH_CHECK(scores.is_cuda() && scores.is_contiguous() && scores.dim() == 2, "scores: contiguous [rows, K] GPU");
  TORCH_CHECK(scores.scalar_type() == at::kFloat || scores.scalar_type() == at::kBFloat16, "scores dtype");
  expect(q, at::kFloat, "q");
  expect(dscores, at::kFloat, "dscores");
  expect(loss, at::kFloat, "loss");
  const int64_t K = scores.size(1), na = (int64_t)crops.size();
  TORCH_CHECK(na >= 1 && na <= 4 && q.dim() == 3 && q.size(0) == na && q.size(2) == K, "q: [n_assign <= 4, bs, K]");
  const int64_t bs = q.size(1);
  TORCH_CHECK(scores.size(0) % bs == 0 && dscores.numel() == scores.numel(), "scores / dscores shape");
  std::vector<int> cr(crops.begin(), crops.end());
  check(dl_swav_ce_multi(scores.data_ptr(), scores.scalar_type() == at::kBFloat16, f32(q), cr.data(), (int)na,
                         f32(dscores), f32(loss), (int)(scores.size(0) / bs), (int)bs, (int)K, (float)temperature,
                         (float)scale, cur_stream(scores)),
        "swav_ce_multi");
}

void swav_ce(const at::Tensor& scores, const at::Tensor& q, at::Tensor dscores, at::Tensor loss, double temperature,
             double scale) {
  TORCH_CHECK(scores.is_cuda() && scores.is_contiguous(), "scores must be a contiguous GPU tensor");
  TORCH_CHECK(scores.scalar_type() == at::kFloat || scores.scalar_type() == at::kBFloat16, "scores dtype");
  expect(q, at::kFloat, "q");
  expect(dscores, at::kFloat, "dscores");
  expect(loss, at::kFloat, "loss");
  const int64_t K = scores.size(-1), rows = scores.numel() / K;
  TORCH_CHECK(q.numel() == scores.numel(), "q shape mismatch");
  check(dl_swav_ce(scores.data_ptr(), scores.scalar_type() == at::kBFloat16, f32(q), f32(dscores), f32(loss), (int)rows,
                   (int)K, (float)temperature, (float)scale, cur_stream(scores)),
        "swav_ce");
}

void row_normalize_(at::Tensor w) {
  expect(w, at::kFloat, "w");
  check(dl_row_normalize(f32(w), (int)w.size(0), (int)w.size(1), cur_stream(w)), "row_normalize");
}

at::Tensor multicrop(const at::Tensor& pool, const at::Tensor& params, int64_t size, int64_t rad,
                     at::ArrayRef<double> mean, at::ArrayRef<double> std) {
  expect(pool, at::kFloat, "pool");
  expect(params, at::kFloat, "params");
  TORCH_CHECK(pool.dim() == 4 && pool.size(1) == 3, "pool must be [P, 3, H, W]");
  TORCH_CHECK(params.dim() == 2 && params.size(1) == 20, "params must be [nb, 20]");
  TORCH_CHECK(mean.size() == 3 && std.size() == 3, "mean/std need 3 channels");
  const int64_t nb = params.size(0), S = size;
  auto out = at::empty({nb, 3, S, S}, pool.options().dtype(at::kBFloat16), at::MemoryFormat::ChannelsLast);
  if (nb == 0) return out;
  auto ws = at::empty({nb * 3 * S * S + nb}, pool.options());
  const float m[3] = {(float)mean[0], (float)mean[1], (float)mean[2]};
  const float sd[3] = {(float)std[0], (float)std[1], (float)std[2]};
  check(dl_multicrop(f32(pool), (int)pool.size(0), (int)pool.size(2), (int)pool.size(3), f32(params), (int)nb, (int)S, (int)rad, m, sd,
                     f32(ws), bf(out), cur_stream(pool)),
        "multicrop (blur radius must be < crop size and <= 16)");
  return out;
}

at::Tensor multicrop_ragged(const at::Tensor& bytes, const at::Tensor& meta, const at::Tensor& params, int64_t size,
                            int64_t rad, at::ArrayRef<double> mean, at::ArrayRef<double> std) {
  expect(bytes, at::kByte, "bytes");
  expect(meta, at::kLong, "meta");
  expect(params, at::kFloat, "params");
  TORCH_CHECK(bytes.dim() == 1 && bytes.numel() > 0, "bytes must be a non-empty 1-D buffer");
  TORCH_CHECK(meta.dim() == 2 && meta.size(1) == 3 && meta.size(0) > 0, "meta must be [n > 0, 3] (offset, H, W)");
  TORCH_CHECK(params.dim() == 2 && params.size(1) == 20, "params must be [nb, 20]");
  TORCH_CHECK(meta.get_device() == bytes.get_device() && params.get_device() == bytes.get_device(),
              "bytes, meta and params must be on one device");
  TORCH_CHECK(mean.size() == 3 && std.size() == 3, "mean/std need 3 channels");
  TORCH_CHECK(size > 0 && size <= 4096, "crop size must be in [1, 4096]");
  const int64_t nb = params.size(0), S = size;
  auto out = at::empty({nb, 3, S, S}, params.options().dtype(at::kBFloat16), at::MemoryFormat::ChannelsLast);
  if (nb == 0) return out;
  auto ws = at::empty({nb * 3 * S * S + nb}, params.options());
  const float m[3] = {(float)mean[0], (float)mean[1], (float)mean[2]};
  const float sd[3] = {(float)std[0], (float)std[1], (float)std[2]};
  check(dl_multicrop_ragged(bytes.data_ptr<uint8_t>(), (long)bytes.numel(), meta.data_ptr<int64_t>(),
                            (int)meta.size(0), f32(params), (int)nb, (int)S, (int)rad, m, sd, f32(ws), bf(out),
                            cur_stream(bytes)),
        "multicrop_ragged (blur radius must be < crop size and <= 16)");
  return out;
}

// ------------------------------------------------------------------ BatchNorm (channels-last, fused act)
inline void expect_nhwc(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " has dtype ", t.scalar_type(), ", expected BFloat16");
  TORCH_CHECK(t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast), name,
              " must be a channels-last [N, C, H, W] tensor");
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> bn_fwd(const at::Tensor& x, const c10::optional<at::Tensor>& res,
                                                      const at::Tensor& gamma, const at::Tensor& beta,
                                                      const c10::optional<at::Tensor>& running_mean,
                                                      const c10::optional<at::Tensor>& running_var, double eps,
                                                      double momentum, bool relu, int64_t groups,
                                                      const c10::optional<at::Tensor>& sums, bool stats_ready) {
  expect_nhwc(x, "x");
  TORCH_CHECK(!stats_ready || sums.has_value(), "bn_fwd: stats_ready needs the sums tensor");
  if (res.has_value()) expect_nhwc(*res, "res");
  expect(gamma, at::kFloat, "gamma");
  expect(beta, at::kFloat, "beta");
  const int64_t C = x.size(1), G = groups;
  TORCH_CHECK(G >= 1 && x.size(0) % G == 0, "batch must split into `groups` equal statistics groups");
  const int64_t R = x.numel() / C / G;
  auto y = at::empty_like(x);
  auto stats = at::empty({4 * G * C}, gamma.options());  // sums[G,2C] | mean[G,C] | rstd[G,C]
  float* rm = running_mean.has_value() ? f32(*running_mean) : nullptr;
  float* rv = running_var.has_value() ? f32(*running_var) : nullptr;
  float* sp = f32(stats);
  if (sums.has_value()) {  // caller's pre-zeroed [G, 2C] slice: no memset per call
    expect(*sums, at::kFloat, "sums");
    TORCH_CHECK(sums->numel() == 2 * G * C, "sums must hold 2 * groups * C floats");
    sp = f32(*sums);
  }
  check(dl_bn_fwd(cbf(x), res.has_value() ? cbf(*res) : nullptr, bf(y), f32(gamma), f32(beta), sp,
                  f32(stats) + 2 * G * C, f32(stats) + 3 * G * C, rm, rv, R, (int)C, (int)G, (float)eps,
                  (float)momentum, relu, cur_stream(x), sums.has_value() ? 1 : 0, stats_ready ? 1 : 0),
        "bn_fwd (channels must be 64..2048, a power-of-two multiple of 8)");
  return {y, stats.narrow(0, 2 * G * C, G * C).view({G, C}), stats.narrow(0, 3 * G * C, G * C).view({G, C})};
}

at::Tensor bn_apply(const at::Tensor& x, const c10::optional<at::Tensor>& res, const at::Tensor& gamma,
                    const at::Tensor& beta, const at::Tensor& mean, const at::Tensor& rstd, bool relu,
                    int64_t groups) {
  expect_nhwc(x, "x");
  if (res.has_value()) {
    expect_nhwc(*res, "res");
    TORCH_CHECK(res->sizes() == x.sizes(), "bn_apply: res must have x's shape");
  }
  expect(gamma, at::kFloat, "gamma");
  expect(beta, at::kFloat, "beta");
  expect(mean, at::kFloat, "mean");
  expect(rstd, at::kFloat, "rstd");
  const int64_t C = x.size(1), G = groups;
  TORCH_CHECK(G >= 1 && x.size(0) % G == 0, "batch must split into `groups` equal statistics groups");
  TORCH_CHECK(gamma.numel() == C && beta.numel() == C, "bn_apply: gamma / beta must hold C floats");
  TORCH_CHECK(mean.numel() == G * C && rstd.numel() == G * C && mean.is_contiguous() && rstd.is_contiguous(),
              "bn_apply: mean / rstd must be contiguous [groups, C] (what bn_fwd returned)");
  const int64_t R = x.numel() / C / G;
  auto y = at::empty_like(x);
  check(dl_bn_apply(cbf(x), res.has_value() ? cbf(*res) : nullptr, bf(y), f32(gamma), f32(beta), f32(mean), f32(rstd),
                    R, (int)C, (int)G, relu, cur_stream(x)),
        "bn_apply (channels must be 64..2048, a power-of-two multiple of 8)");
  return y;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> bn_bwd(const at::Tensor& dy, const at::Tensor& y,
                                                                  const at::Tensor& x, const at::Tensor& mean,
                                                                  const at::Tensor& rstd, const at::Tensor& gamma,
                                                                  bool relu, bool want_dres,
                                                                  const c10::optional<at::Tensor>& sums,
                                                                  const c10::optional<at::Tensor>& dgamma_acc,
                                                                  const c10::optional<at::Tensor>& dbeta_acc,
                                                                  const c10::optional<at::Tensor>& beta,
                                                                  bool stats_ready) {
  const int64_t G = mean.dim() == 2 ? mean.size(0) : 1;
  // stats_ready: dy is already masked by the ReLU and `sums` holds the backward column sums (a
  // conv data-gradient epilogue prepared them, conv2d_dgrad_bn); the residual's gradient is then dy
  // itself, returned without a copy
  TORCH_CHECK(!stats_ready || sums.has_value(), "bn_bwd: stats_ready needs the sums tensor");
  expect_nhwc(x, "x");
  expect_nhwc(y, "y");
  const at::Tensor g = dy.is_contiguous(at::MemoryFormat::ChannelsLast) ? dy
                                                                        : dy.contiguous(at::MemoryFormat::ChannelsLast);
  expect_nhwc(g, "dy");
  const int64_t C = x.size(1), R = x.numel() / C / G;
  auto dx = at::empty_like(x);
  auto dres = want_dres && !stats_ready ? at::empty_like(x) : at::Tensor();
  auto ws = at::empty({2 * G * C + 2 * C}, gamma.options());  // sums[G,2C] | dgamma[C] | dbeta[C]
  float* sp = f32(ws);
  if (sums.has_value()) {  // caller's pre-zeroed [G, 2C] slice: no memset per call
    expect(*sums, at::kFloat, "sums");
    TORCH_CHECK(sums->numel() == 2 * G * C, "sums must hold 2 * groups * C floats");
    sp = f32(*sums);
  }
  // dgamma_acc / dbeta_acc: accumulate straight into the parameters' gradient buffers (then the
  // returned dgamma / dbeta are empty) instead of returning them for autograd to add
  const bool acc = dgamma_acc.has_value() && dbeta_acc.has_value();
  if (acc) {
    expect(*dgamma_acc, at::kFloat, "dgamma_acc");
    expect(*dbeta_acc, at::kFloat, "dbeta_acc");
    TORCH_CHECK(dgamma_acc->numel() == C && dbeta_acc->numel() == C, "parameter gradient size mismatch");
  }
  float* dgp = acc ? f32(*dgamma_acc) : f32(ws) + 2 * G * C;
  float* dbp = acc ? f32(*dbeta_acc) : f32(ws) + 2 * G * C + C;
  // beta (BatchNorm+ReLU without a residual branch only): the ReLU mask comes from x, y is not read
  const bool xmask = beta.has_value() && relu && !want_dres && !stats_ready;
  if (xmask) {
    expect(*beta, at::kFloat, "beta");
    TORCH_CHECK(beta->numel() == C, "beta size mismatch");
  }
  check(dl_bn_bwd(cbf(g), cbf(y), cbf(x), f32(mean), f32(rstd), f32(gamma), sp, bf(dx),
                  want_dres && !stats_ready ? bf(dres) : nullptr, dgp, dbp, R, (int)C, (int)G,
                  stats_ready ? 0 : relu, cur_stream(x), sums.has_value() ? 1 : 0, acc ? 1 : 0,
                  xmask ? f32(*beta) : nullptr, stats_ready ? 1 : 0),
        "bn_bwd");
  if (want_dres && stats_ready) dres = g;
  if (acc) return {dx, want_dres ? dres : at::empty({0}, x.options()), at::empty({0}, gamma.options()),
                   at::empty({0}, gamma.options())};
  return {dx, want_dres ? dres : at::empty({0}, x.options()), ws.narrow(0, 2 * G * C, C),
          ws.narrow(0, 2 * G * C + C, C)};
}

// ------------------------------------------------------------------ pools and head normalisation (pool.hip)
std::tuple<at::Tensor, at::Tensor> maxpool_fwd(const at::Tensor& x) {
  expect_nhwc(x, "x");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t P = (H - 1) / 2 + 1, Q = (W - 1) / 2 + 1;
  auto y = at::empty({N, C, P, Q}, x.options(), at::MemoryFormat::ChannelsLast);
  auto arg = at::empty({N, C, P, Q}, x.options().dtype(at::kByte), at::MemoryFormat::ChannelsLast);
  check(dl_maxpool_fwd(cbf(x), bf(y), arg.data_ptr<uint8_t>(), (int)N, (int)H, (int)W, (int)C, (int)P, (int)Q,
                       cur_stream(x)),
        "maxpool_fwd");
  return {y, arg};
}

at::Tensor maxpool_bwd(const at::Tensor& dy_in, const at::Tensor& arg, int64_t H, int64_t W) {
  const at::Tensor dy = dy_in.contiguous(at::MemoryFormat::ChannelsLast);
  expect_nhwc(dy, "dy");
  TORCH_CHECK(arg.sizes() == dy.sizes() && arg.is_contiguous(at::MemoryFormat::ChannelsLast), "maxpool_bwd: arg");
  const int64_t N = dy.size(0), C = dy.size(1), P = dy.size(2), Q = dy.size(3);
  auto dx = at::empty({N, C, H, W}, dy.options(), at::MemoryFormat::ChannelsLast);
  check(dl_maxpool_bwd(cbf(dy), arg.data_ptr<uint8_t>(), bf(dx), (int)N, (int)H, (int)W, (int)C, (int)P, (int)Q,
                       cur_stream(dy)),
        "maxpool_bwd");
  return dx;
}

at::Tensor avgpool_fwd(const at::Tensor& x) {
  expect_nhwc(x, "x");
  const int64_t N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  auto y = at::empty({N, C}, x.options());
  check(dl_avgpool_fwd(cbf(x), bf(y), (int)N, (int)HW, (int)C, cur_stream(x)), "avgpool_fwd");
  return y;
}

at::Tensor avgpool_bwd(const at::Tensor& dy_in, int64_t H, int64_t W) {
  const at::Tensor dy = dy_in.contiguous();
  expect(dy, at::kBFloat16, "dy");
  const int64_t N = dy.size(0), C = dy.size(1);
  auto dx = at::empty({N, C, H, W}, dy.options(), at::MemoryFormat::ChannelsLast);
  check(dl_avgpool_bwd(cbf(dy), bf(dx), (int)N, (int)(H * W), (int)C, cur_stream(dy)), "avgpool_bwd");
  return dx;
}

std::tuple<at::Tensor, at::Tensor> l2norm_fwd(const at::Tensor& x_in, double eps) {
  const at::Tensor x = x_in.contiguous();
  expect(x, at::kBFloat16, "x");
  const int64_t rows = x.size(0), D = x.size(1);
  auto y = at::empty_like(x);
  auto rinv = at::empty({rows}, x.options().dtype(at::kFloat));
  check(dl_l2norm_fwd(cbf(x), bf(y), f32(rinv), (int)rows, (int)D, (float)eps, cur_stream(x)), "l2norm_fwd");
  return {y, rinv};
}

at::Tensor l2norm_bwd(const at::Tensor& dy_in, const at::Tensor& y, const at::Tensor& rinv) {
  const at::Tensor dy = dy_in.contiguous().to(at::kBFloat16);
  expect(y, at::kBFloat16, "y");
  expect(rinv, at::kFloat, "rinv");
  auto dx = at::empty_like(y);
  check(dl_l2norm_bwd(cbf(dy), cbf(y), f32(rinv), bf(dx), (int)y.size(0), (int)y.size(1), cur_stream(y)),
        "l2norm_bwd");
  return dx;
}

// ------------------------------------------------------------------ implicit-GEMM convolution (NHWC, conv.hip)
// Weights arrive as [Cout, Cin, R, S] tensors whose memory is KRSC (channels_last), which is how the
// flat parameter buffer stores every conv weight; permute(0,2,3,1) is then a free view.
inline at::Tensor krsc_view(const at::Tensor& w) {
  at::Tensor k = w.permute({0, 2, 3, 1});
  return k.is_contiguous() ? k : k.contiguous();
}

inline int64_t conv_out(int64_t n, int64_t k, int64_t stride, int64_t pad) { return (n + 2 * pad - k) / stride + 1; }

// stem (Cin not a multiple of 64): explicit im2col matrix [N*P*Q, Kp], k = r*SCp + s*C + c (each
// filter row padded from S*C to SCp = roundup(S*C, 8) columns), zero padded to Kp = roundup(R*SCp, 64)
struct StemCols {
  int64_t SCp, Kp;
};
inline StemCols stem_cols(int64_t R, int64_t S, int64_t C, bool lt) {
  const int64_t SCp = (S * C + 7) / 8 * 8;  // hipBLASLt needs 16-byte rows only; conv.hip a multiple of BK
  return {SCp, lt ? R * SCp : (R * SCp + 63) / 64 * 64};
}
// The 7x7 stride-2 pad-3 stem over 3 channels (even H, W) runs as a 4x4 stride-1 conv over the
// space-to-depth image xs [N, H/2, W/2, 16] (dl_stem_s2d): tap (tr, ts) and xs channel
// (2a + b) * 3 + c carry the original tap r = 2 tr + a - 1, s = 2 ts + b - 1 (r or s of -1 or 7:
// a zero weight).  The "cols" tensor of im2col_stem is then xs as a [N*H/2*W/2, 16] matrix.
inline bool stem_s2d_ok(int64_t C, int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t H, int64_t W) {
  return C == 3 && R == 7 && S == 7 && stride == 2 && pad == 3 && H % 2 == 0 && W % 2 == 0;
}
// column of the [K, 256] s2d weight for each (r, s, c) of the KRSC weight's 147 columns
at::Tensor stem_s2d_index(const at::Device& dev) {
  static std::mutex mu;
  static std::unordered_map<int, at::Tensor> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(dev.index());
  if (it != cache.end()) return it->second;
  std::vector<int64_t> idx(147);
  for (int r = 0; r < 7; ++r)
    for (int s = 0; s < 7; ++s)
      for (int c = 0; c < 3; ++c) {
        const int tr = (r + 1) / 2, a = (r + 1) % 2, ts = (s + 1) / 2, b = (s + 1) % 2;
        idx[(r * 7 + s) * 3 + c] = (tr * 4 + ts) * 16 + (2 * a + b) * 3 + c;
      }
  at::Tensor t = at::tensor(idx, at::TensorOptions().dtype(at::kLong)).to(dev);
  cache.emplace(dev.index(), t);
  return t;
}
inline at::Tensor stem_s2d(const at::Tensor& x) {
  const int64_t N = x.size(0), H = x.size(2), W = x.size(3);
  auto xs = at::empty({N * (H / 2) * (W / 2), 16}, x.options());
  check(dl_stem_s2d(cbf(x), (int)N, (int)H, (int)W, bf(xs), cur_stream(x)), "stem_s2d");
  return xs;
}

inline at::Tensor stem_im2col(const at::Tensor& x, int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t P,
                              int64_t Q, const StemCols& sc) {
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  auto col = at::empty({N * P * Q, sc.Kp}, x.options());
  check(dl_im2col(cbf(x), (int)N, (int)H, (int)W, (int)C, (int)R, (int)S, (int)stride, (int)pad, (int)P, (int)Q,
                  (int)sc.SCp, (int)sc.Kp, bf(col), cur_stream(x)),
        "im2col");
  return col;
}

// Convolutions that are plain GEMMs run on the GEMM kernels (gemm8.hip / gemm_small.hip): 1x1
// stride-1 unpadded convs over NHWC tensors (x[N*H*W, C] x W[K, C]^T; dgrad dY[N*H*W, K] x W
// with the KRSC weight as a K-outer operand) and the stem's column-matrix GEMM; their
// weight gradients use gemm8's split-K slabs where both channel counts are multiples of 256 and the
// implicit-GEMM conv.hip wgrad otherwise.
constexpr bool conv_gemm() { return true; }
inline bool is_pointwise(int64_t R, int64_t S, int64_t stride, int64_t pad) {
  return R == 1 && S == 1 && stride == 1 && pad == 0;
}
// 1x1 convs whose GEMM output has at most this many columns (forward: output channels; data
// gradient: input channels) run on conv.hip's implicit-GEMM kernel (256x64 / 128x128 tiles, 2-deep
// register prefetch) instead of gemm_small: 128 won the round-3 A/B over 0 / 64 / 256 / 512
// (SwAV b=64: 2087 / 2128 / 2205 / 2197 / 2190 samples/s, profiles/README.md)
constexpr int64_t narrow_1x1_max() { return 128; }
// 1x1 forward convs whose gemm8 grid (256 x 256 tiles) has fewer than this many workgroups run on
// conv.hip's 128 x 128 tiles instead (4x the workgroups, lower latency): SwAV's layer-3/4 convs of the
// 96-crop pass, which with the 224 crops split into passes of their own is the iteration's critical
// path (a measurement build may override)
#ifndef DL_FEW_TILE_1X1
#define DL_FEW_TILE_1X1 128
#endif
inline bool few_tile_gemm(int64_t M, int64_t N) { return ((M + 255) / 256) * ((N + 255) / 256) < DL_FEW_TILE_1X1; }
inline at::Tensor rows2d(const at::Tensor& t) {  // channels-last [N, C, H, W] -> [N*H*W, C] view
  return t.permute({0, 2, 3, 1}).reshape({-1, t.size(1)});
}
inline DlConvGeom geom(const bf16_t* img, int64_t N, int64_t H, int64_t W, int64_t C, int64_t I, int64_t J,
                       int64_t sh, int64_t sw, int64_t TR, int64_t TS, int64_t dh0, int64_t dhs, int64_t dw0,
                       int64_t dws) {
  return DlConvGeom{img, (int)N, (int)H, (int)W, (int)C, (int)I, (int)J, (int)sh, (int)sw,
                    (int)TR, (int)TS, (int)dh0, (int)dhs, (int)dw0, (int)dws};
}

// stats (optional, fp32 [groups][2 Cout], accumulated): the BatchNorm statistics of the output per
// statistics group of the batch (the producing epilogue computes them where the kernel allows,
// otherwise one statistics pass runs after the conv)
// cols (optional): the stem's column matrix from im2col_stem (computed once per pass and kept for the
// weight gradient instead of being rebuilt there)
// af (optional, excludes stats): the inference epilogue of conv2d_bn_act
struct ConvAffine {
  const float* scale;
  const float* shift;
  const bf16_t* res;
  bool relu;
};
at::Tensor conv2d_fwd_impl(const at::Tensor& x, const at::Tensor& w, int64_t stride, int64_t pad, float* stats,
                           int64_t groups, const c10::optional<at::Tensor>& cols, const ConvAffine* af = nullptr);

at::Tensor conv2d_fwd(const at::Tensor& x, const at::Tensor& w, int64_t stride, int64_t pad,
                      const c10::optional<at::Tensor>& cols) {
  return conv2d_fwd_impl(x, w, stride, pad, nullptr, 1, cols);
}

at::Tensor conv2d_fwd_stats(const at::Tensor& x, const at::Tensor& w, int64_t stride, int64_t pad, at::Tensor sums,
                            int64_t groups, const c10::optional<at::Tensor>& cols) {
  expect(sums, at::kFloat, "sums");
  TORCH_CHECK(groups >= 1 && x.size(0) % groups == 0, "conv2d_fwd_stats: batch must split into `groups`");
  TORCH_CHECK(sums.numel() == 2 * groups * w.size(0), "conv2d_fwd_stats: sums must hold 2 * groups * Cout floats");
  return conv2d_fwd_impl(x, w, stride, pad, f32(sums), groups, cols);
}

// the stem's column matrix [N*P*Q, Kp] (see stem_cols) for conv2d_fwd / conv2d_wgrad(cols=...)
at::Tensor im2col_stem(const at::Tensor& x, int64_t R, int64_t S, int64_t stride, int64_t pad) {
  expect_nhwc(x, "x");
  if (stem_s2d_ok(x.size(1), R, S, stride, pad, x.size(2), x.size(3))) return stem_s2d(x);
  const int64_t P = conv_out(x.size(2), R, stride, pad), Q = conv_out(x.size(3), S, stride, pad);
  return stem_im2col(x, R, S, stride, pad, P, Q, stem_cols(R, S, x.size(1), false));
}

inline at::Tensor stem_cols_checked(const c10::optional<at::Tensor>& cols, const at::Tensor& x, int64_t R, int64_t S,
                                    int64_t stride, int64_t pad, int64_t P, int64_t Q, const StemCols& sc) {
  if (!cols.has_value()) return stem_im2col(x, R, S, stride, pad, P, Q, sc);
  TORCH_CHECK(cols->scalar_type() == at::kBFloat16 && cols->is_contiguous() && cols->dim() == 2 &&
                  cols->size(0) == x.size(0) * P * Q && cols->size(1) == sc.Kp,
              "cols must be the stem's im2col_stem matrix for this input");
  return *cols;
}

// fp32 zeros / ones [2, C] per device: the mean / rstd with which dl_bn_apply computes
// fmaf(x, gamma, beta) exactly (sc = gamma * 1, sh = beta - 0 * sc)
at::Tensor affine_identity_stats(const at::Device& dev, int64_t C) {
  static std::mutex mu;
  static std::map<std::pair<int, int64_t>, at::Tensor> cache;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_pair((int)dev.index(), C);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  at::Tensor t = at::cat({at::zeros({1, C}, at::kFloat), at::ones({1, C}, at::kFloat)}).to(dev);
  cache.emplace(key, t);
  return t;
}
// the GEMM routes of conv2d_bn_act: one streaming pass over the GEMM's stored output
inline at::Tensor affine_pass(const at::Tensor& c, const ConvAffine& af) {
  const int64_t K = c.size(1);
  const at::Tensor id = affine_identity_stats(c.device(), K);
  auto y = at::empty_like(c);
  check(dl_bn_apply(cbf(c), af.res, bf(y), af.scale, af.shift, f32(id), f32(id) + K, c.numel() / K, (int)K, 1,
                    af.relu, cur_stream(c)),
        "conv2d_bn_act (a GEMM-routed conv needs 64..2048 output channels, a power-of-two multiple of 8)");
  return y;
}

at::Tensor conv2d_fwd_impl(const at::Tensor& x, const at::Tensor& w, int64_t stride, int64_t pad, float* stats,
                           int64_t groups, const c10::optional<at::Tensor>& cols, const ConvAffine* af) {
  expect_nhwc(x, "x");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 && w.dim() == 4, "w must be a bf16 [Cout,Cin,R,S] GPU tensor");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t K = w.size(0), R = w.size(2), S = w.size(3);
  TORCH_CHECK(w.size(1) == C, "conv2d_fwd: weight/input channel mismatch");
  const int64_t P = conv_out(H, R, stride, pad), Q = conv_out(W, S, stride, pad);
  auto y = at::empty({N, K, P, Q}, x.options(), at::MemoryFormat::ChannelsLast);
  const at::Tensor wk = krsc_view(w);
  const long stat_rows = N / groups * P * Q;  // output rows per statistics group
  if (is_pointwise(R, S, stride, pad) && conv_gemm() && !(K <= narrow_1x1_max() && C % 64 == 0) &&
      !(C % 64 == 0 && few_tile_gemm(N * P * Q, K))) {
    const at::Tensor xr = rows2d(x), wr = wk.view({K, C});
    const DlGemm g = gemm_desc(xr, false, wr, true, bf(y), K);  // y[M, K] = x[M, C] w[K, C]^T
    if (stats) gemm_store_stats(g, stats, stat_rows, xr, cur_stream(x));
    else gemm_store(g, xr, cur_stream(x));
    return af ? affine_pass(y, *af) : y;
  }
  if (C % 64 == 0) {
    const DlConvGeom gm = geom(cbf(x), N, H, W, C, P, Q, stride, stride, R, S, -pad, 1, -pad, 1);
    if (af) {
      check(dl_conv_fwd_affine(gm, cbf(wk), R * S * C, (int)K, bf(y), (int)P, (int)Q, K, af->scale, af->shift, af->res,
                               af->relu, cur_stream(x)),
            "conv2d_bn_act");
      return y;
    }
    if (stats && dl_conv_fwd(gm, cbf(wk), R * S * C, (int)K, bf(y), (int)P, (int)Q, 1, 1, 0, 0, K, cur_stream(x),
                             stats, stat_rows) == 0)
      return y;
    check(dl_conv_fwd(gm, cbf(wk), R * S * C, (int)K, bf(y), (int)P, (int)Q, 1, 1, 0, 0, K, cur_stream(x)),
          "conv2d_fwd");
    if (stats) check(dl_bn_stats(cbf(y), stats, stat_rows, (int)K, (int)groups, cur_stream(x)), "bn_stats");
    return y;
  }
  if (stem_s2d_ok(C, R, S, stride, pad, H, W)) {
    at::Tensor xs;
    if (cols.has_value()) {
      TORCH_CHECK(cols->scalar_type() == at::kBFloat16 && cols->is_contiguous() && cols->dim() == 2 &&
                      cols->size(0) == N * P * Q && cols->size(1) == 16,
                  "cols must be the stem's im2col_stem (space-to-depth) matrix for this input");
      xs = *cols;
    } else {
      xs = stem_s2d(x);
    }
    auto w2 = at::zeros({K, 256}, w.options());
    w2.index_copy_(1, stem_s2d_index(w.device()), wk.reshape({K, 147}));
    const DlConvGeom gs = geom(cbf(xs), N, H / 2, W / 2, 16, P, Q, 1, 1, 4, 4, -2, 1, -2, 1);
    if (af) {
      check(dl_conv_fwd_affine(gs, cbf(w2), 256, (int)K, bf(y), (int)P, (int)Q, K, af->scale, af->shift, af->res,
                               af->relu, cur_stream(x)),
            "conv2d_bn_act(stem)");
      return y;
    }
    if (stats && dl_conv_fwd(gs, cbf(w2), 256, (int)K, bf(y), (int)P, (int)Q, 1, 1, 0, 0, K, cur_stream(x), stats,
                             stat_rows) == 0)
      return y;
    check(dl_conv_fwd(gs, cbf(w2), 256, (int)K, bf(y), (int)P, (int)Q, 1, 1, 0, 0, K, cur_stream(x)),
          "conv2d_fwd(stem)");
    if (stats) check(dl_bn_stats(cbf(y), stats, stat_rows, (int)K, (int)groups, cur_stream(x)), "bn_stats");
    return y;
  }
  // other small-channel convs: im2col into a column matrix padded to a multiple of 64 columns, then
  // one GEMM against the equally padded weight rows
  const StemCols sc = stem_cols(R, S, C, false);
  const at::Tensor col = stem_cols_checked(cols, x, R, S, stride, pad, P, Q, sc);
  auto wp = at::zeros({K, sc.Kp}, w.options());
  wp.narrow(1, 0, R * sc.SCp).view({K, R, sc.SCp}).narrow(2, 0, S * C).copy_(wk.reshape({K, R, S * C}));
  // the column-matrix GEMM as a 1x1 conv over the [N*P*Q, 1, 1, Kp] "image" on conv.hip (its
  // 256x64 tiles for the 64 stem channels, with the statistics epilogue; +2% over the tiled GEMM
  // kernels in round 3), the tiled GEMM kernels for a column width conv.hip does not take
  const int64_t Mc = col.size(0);
  if (sc.Kp % 64 == 0) {
    const DlConvGeom gc = geom(cbf(col), Mc, 1, 1, sc.Kp, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1);
    if (af && dl_conv_fwd_affine(gc, cbf(wp), sc.Kp, (int)K, bf(y), 1, 1, K, af->scale, af->shift, af->res, af->relu,
                                 cur_stream(x)) == 0)
      return y;
    if (stats && dl_conv_fwd(gc, cbf(wp), sc.Kp, (int)K, bf(y), 1, 1, 1, 1, 0, 0, K, cur_stream(x), stats,
                             stat_rows) == 0)
      return y;
    if (dl_conv_fwd(gc, cbf(wp), sc.Kp, (int)K, bf(y), 1, 1, 1, 1, 0, 0, K, cur_stream(x)) == 0) {
      if (stats) check(dl_bn_stats(cbf(y), stats, stat_rows, (int)K, (int)groups, cur_stream(x)), "bn_stats");
      return y;
    }
  }
  const DlGemm g = gemm_desc(col, false, wp, true, bf(y), K);
  if (stats) gemm_store_stats(g, stats, stat_rows, col, cur_stream(x));
  else gemm_store(g, col, cur_stream(x));
  return af ? affine_pass(y, *af) : y;
}

// Inference conv with a frozen BatchNorm folded into the epilogue:
//   y = bf16(act(fmaf(float(bf16(conv(x, w))), scale[ch], shift[ch]) [+ res]))
// i.e. conv2d_fwd followed by bn_apply(gamma = scale, beta = shift, mean = 0, rstd = 1), bit for bit.
// Routed as conv2d_fwd: the conv.hip routes apply the expression in the kernel's epilogue, the
// GEMM routes run the GEMM and one bn_apply pass.
at::Tensor conv2d_bn_act(const at::Tensor& x, const at::Tensor& w, const at::Tensor& scale, const at::Tensor& shift,
                         const c10::optional<at::Tensor>& res, bool relu, int64_t stride, int64_t pad) {
  expect_nhwc(x, "x");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 && w.dim() == 4, "w must be a bf16 [Cout,Cin,R,S] GPU tensor");
  expect(scale, at::kFloat, "scale");
  expect(shift, at::kFloat, "shift");
  const int64_t K = w.size(0);
  TORCH_CHECK(scale.dim() == 1 && shift.dim() == 1 && scale.numel() == K && shift.numel() == K,
              "conv2d_bn_act: scale / shift must be fp32 [Cout]");
  TORCH_CHECK(K % 8 == 0, "conv2d_bn_act: Cout must be a multiple of 8");
  TORCH_CHECK(stride >= 1 && pad >= 0, "conv2d_bn_act: stride / pad");
  TORCH_CHECK(x.size(2) + 2 * pad >= w.size(2) && x.size(3) + 2 * pad >= w.size(3), "conv2d_bn_act: empty output");
  if (res.has_value()) {
    expect_nhwc(*res, "res");
    const int64_t P = conv_out(x.size(2), w.size(2), stride, pad), Q = conv_out(x.size(3), w.size(3), stride, pad);
    TORCH_CHECK(res->dim() == 4 && res->size(0) == x.size(0) && res->size(1) == K && res->size(2) == P &&
                    res->size(3) == Q,
                "conv2d_bn_act: res must have the output's shape");
  }
  const ConvAffine af{f32(scale), f32(shift), res.has_value() ? cbf(*res) : nullptr, relu};
  return conv2d_fwd_impl(x, w, stride, pad, nullptr, 1, c10::nullopt, &af);
}

// Tap-transposed data-gradient weights of every parity class of a strided conv, in (a, b) order:
// [C, TR, TS, K] per class (an empty tensor for a class with no contributing tap).  The SwAV
// model computes them once per iteration and passes them to every data-gradient call of that conv
// (both trunk passes), instead of one copy kernel per class per call.
std::vector<at::Tensor> conv2d_dgrad_weights(const at::Tensor& w, int64_t stride, int64_t pad) {
  const at::Tensor wk = krsc_view(w);
  const int64_t R = wk.size(1), S = wk.size(2);
  std::vector<at::Tensor> out;
  for (int64_t a = 0; a < stride; ++a)
    for (int64_t b = 0; b < stride; ++b) {
      const int64_t r0 = (a + pad) % stride, s0 = (b + pad) % stride;
      if (r0 < R && s0 < S) out.push_back(wk.slice(1, r0, R, stride).slice(2, s0, S, stride).permute({3, 1, 2, 0}).contiguous());
      else out.push_back(at::empty({0}, w.options()));  // no contributing tap
    }
  return out;
}

// conv2d_dgrad_weights of several convs at once: the concatenation of their per-class lists (stride^2
// tensors per conv, empty for a class with no contributing tap), views of ONE buffer filled by one
// batched transpose launch (weights: channels-last bf16, both channel counts multiples of 64)
std::vector<at::Tensor> conv2d_dgrad_weights_batched(const std::vector<at::Tensor>& ws, std::vector<int64_t> strides,
                                                     std::vector<int64_t> pads) {
  TORCH_CHECK(!ws.empty() && ws.size() == strides.size() && ws.size() == pads.size(),
              "conv2d_dgrad_weights_batched: one stride and pad per weight");
  struct Cls { int64_t conv, r0, s0, TR, TS, off; };
  std::vector<Cls> cls;
  int64_t total = 0;
  for (size_t i = 0; i < ws.size(); ++i) {
    const at::Tensor& w = ws[i];
    TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 && w.dim() == 4 &&
                    w.is_contiguous(at::MemoryFormat::ChannelsLast) && w.size(0) % 64 == 0 && w.size(1) % 64 == 0 &&
                    w.device() == ws[0].device(),
                "conv2d_dgrad_weights_batched: channels-last bf16 weights with 64-multiple channel counts on one GPU");
    const int64_t R = w.size(2), S = w.size(3), st = strides[i], pd = pads[i];
    TORCH_CHECK(st >= 1 && pd >= 0, "conv2d_dgrad_weights_batched: stride / pad");
    for (int64_t a = 0; a < st; ++a)
      for (int64_t b = 0; b < st; ++b) {
        const int64_t r0 = (a + pd) % st, s0 = (b + pd) % st;
        const int64_t TR = r0 < R ? (R - 1 - r0) / st + 1 : 0, TS = s0 < S ? (S - 1 - s0) / st + 1 : 0;
        cls.push_back(Cls{(int64_t)i, r0, s0, TR, TS, total});
        total += TR * TS * w.size(0) * w.size(1);
      }
  }
  auto buf = at::empty({std::max<int64_t>(total, 1)}, ws[0].options());
  std::vector<at::Tensor> out;
  std::vector<DlWtJob> jobs;
  for (const Cls& c : cls) {
    const at::Tensor& w = ws[c.conv];
    const int64_t K = w.size(0), C = w.size(1);
    if (c.TR == 0 || c.TS == 0) {
      out.push_back(at::empty({0}, w.options()));
      continue;
    }
    out.push_back(buf.narrow(0, c.off, c.TR * c.TS * K * C).view({C, c.TR, c.TS, K}));
    jobs.push_back(DlWtJob{cbf(w), bf(buf) + c.off, (int)K, (int)C, (int)w.size(2), (int)w.size(3), (int)c.r0, (int)c.s0,
                           (int)strides[c.conv], (int)c.TR, (int)c.TS});
  }
  check(dl_conv_dgrad_weights_batched(jobs.data(), (int)jobs.size(), cur_stream(ws[0])), "conv2d_dgrad_weights_batched");
  return out;
}

// The implicit-GEMM data gradient dX[n, h, w, c] of a conv (dy NHWC, wk the KRSC weight view): a
// stride-s conv splits into s^2 parity classes (h = i*s + a), each a dense stride-1 sub-convolution
// over its contributing taps.  bn (with sums [groups][2C]): conv.hip's BN-backward epilogue on every
// class; returns false without launching anything when a class's rows do not split into whole
// 256-row tiles per statistics group.
bool conv_dgrad_classes(const at::Tensor& dy, const at::Tensor& wk, int64_t stride, int64_t pad, int64_t H, int64_t W,
                        at::Tensor& dx, const c10::optional<std::vector<at::Tensor>>& wds, float* sums,
                        int64_t groups, const DlBnBwdEpi* bn) {
  const int64_t N = dy.size(0), K = dy.size(1), P = dy.size(2), Q = dy.size(3);
  const int64_t R = wk.size(1), S = wk.size(2), C = wk.size(3);
  if (bn) {
    if (groups < 1 || N % groups || C % 8) return false;
    for (int64_t a = 0; a < stride; ++a)
      for (int64_t b = 0; b < stride; ++b) {
        const int64_t I = (H - a + stride - 1) / stride, J = (W - b + stride - 1) / stride;
        if (I > 0 && J > 0 && (N / groups * I * J) % 256) return false;
      }
  }
  std::vector<DlConvFwdJob> jobs;
  std::vector<at::Tensor> keep;  // per-class weights alive until the launch
  for (int64_t a = 0; a < stride; ++a) {
    const int64_t I = (H - a + stride - 1) / stride;
    const int64_t r0 = (a + pad) % stride, TR = r0 < R ? (R - 1 - r0) / stride + 1 : 0;
    const int64_t dh0 = (a + pad - r0) / stride;
    for (int64_t b = 0; b < stride; ++b) {
      const int64_t J = (W - b + stride - 1) / stride;
      const int64_t s0 = (b + pad) % stride, TS = s0 < S ? (S - 1 - s0) / stride + 1 : 0;
      const int64_t dw0 = (b + pad - s0) / stride;
      if (I <= 0 || J <= 0) continue;
      // [C, TR, TS, K] tap-transposed weights of this parity class (precomputed ones when given); a
      // class with no contributing tap runs the kernel's zero-tile path, which reads no weights
      at::Tensor wd = wk;
      if (TR > 0 && TS > 0) {
        const size_t cls = (size_t)(a * stride + b);
        if (wds.has_value() && cls < wds->size() && (*wds)[cls].numel() > 0) {
          wd = (*wds)[cls];
          TORCH_CHECK(wd.is_contiguous() && wd.numel() == C * TR * TS * K, "conv2d_dgrad: wds shape");
        } else {
          wd = wk.slice(1, r0, R, stride).slice(2, s0, S, stride).permute({3, 1, 2, 0}).contiguous();
        }
      }
      keep.push_back(wd);
      jobs.push_back(DlConvFwdJob{geom(cbf(dy), N, P, Q, K, I, J, 1, 1, TR, TS, dh0, -1, dw0, -1), cbf(wd),
                                  std::max<int64_t>(8, TR * TS * K), (int)a, (int)b, bn ? N / groups * I * J : 0});
    }
  }
  // every parity class in one launch (the classes' grids back to back left most CUs idle: stride-2
  // 3x3 data gradients ran at half the forward's speed); per-class launches when the classes need
  // different kernel variants
  const hipStream_t st = cur_stream(dy);
  if (!jobs.empty() && dl_conv_fwd_multi(jobs.data(), (int)jobs.size(), (int)C, bf(dx), (int)H, (int)W, (int)stride,
                                         (int)stride, C, st, bn ? sums : nullptr, bn) != 0) {
    for (const DlConvFwdJob& jb : jobs)
      check(dl_conv_fwd(jb.g, jb.w, jb.ldw, (int)C, bf(dx), (int)H, (int)W, (int)stride, (int)stride, jb.oh0, jb.ow0, C,
                        st, bn ? sums : nullptr, jb.stat_rows, bn),
            "conv2d_dgrad");
  }
  return true;
}

// dX = conv^T(dY): for each output parity class (a, b) of the stride, a dense sub-convolution over
// the taps r = r0, r0 + stride, ... that reach it (dY row = i + dh0 - tr), weights [Cin][tr][ts][Cout]
// residual (optional, [N, C, H, W] channels-last bf16): added to dX — in the GEMM epilogue on the
// 1x1 stride-1 path (a Bottleneck's conv1 taking the identity branch's gradient), afterwards otherwise
at::Tensor conv2d_dgrad(const at::Tensor& dy_in, const at::Tensor& w, int64_t stride, int64_t pad, int64_t H,
                        int64_t W, const c10::optional<at::Tensor>& residual,
                        const c10::optional<std::vector<at::Tensor>>& wds) {
  const at::Tensor dy = dy_in.is_contiguous(at::MemoryFormat::ChannelsLast)
                            ? dy_in
                            : dy_in.contiguous(at::MemoryFormat::ChannelsLast);
  expect_nhwc(dy, "dy");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 && w.dim() == 4, "w must be a bf16 [Cout,Cin,R,S] GPU tensor");
  const int64_t N = dy.size(0), K = dy.size(1), P = dy.size(2), Q = dy.size(3);
  const int64_t C = w.size(1), R = w.size(2), S = w.size(3);
  TORCH_CHECK(w.size(0) == K, "conv2d_dgrad: weight/grad channel mismatch");
  TORCH_CHECK(K % 64 == 0, "conv2d_dgrad needs Cout % 64 == 0");
  auto dx = at::empty({N, C, H, W}, dy.options(), at::MemoryFormat::ChannelsLast);
  if (residual.has_value()) {
    expect_nhwc(*residual, "residual");
    TORCH_CHECK(residual->sizes() == dx.sizes(), "conv2d_dgrad: residual must have the input's shape");
  }
  const at::Tensor wk = krsc_view(w);  // [K, R, S, C]
  if (is_pointwise(R, S, stride, pad) && H == P && W == Q && conv_gemm() &&
      !(C <= narrow_1x1_max() && K % 64 == 0)) {
    // dX[M, C] = dY[M, K] W[K, C] (+ residual): the weight as a K-outer B operand, no transposed copy
    const at::Tensor dyr = rows2d(dy), wkc = wk.view({K, C});
    DlGemm g = gemm_desc(dyr, false, wkc, false, bf(dx), C);
    if (residual.has_value()) g.R = cbf(*residual), g.ldr = C;
    gemm_store(g, dyr, cur_stream(dy));
    return dx;
  }
  conv_dgrad_classes(dy, wk, stride, pad, H, W, dx, wds, nullptr, 1, nullptr);
  if (residual.has_value()) dx.add_(*residual);
  return dx;
}

// The data gradient of a conv whose input is the output of a BatchNorm+ReLU, prepared for that BN's
// backward (which then skips its statistics pass, bn_bwd(stats_ready)): returns g = dX (+ residual)
// masked by the ReLU — mask from y > 0 when y is given (the BN had a residual branch), else from
// the forward's pre-activation over x (the BN input) — and adds sums[grp][c] += g, sums[grp][C + c]
// += g * (x - mean) * rstd, in the GEMM epilogue of a 1x1 stride-1 data gradient (gemm8 DL_EPI_BNBWD)
// or in conv.hip's epilogue on every
// parity class of the others (no residual; whole 256-row tiles per statistics group).  Returns
// (dx, fused): where the epilogue cannot take it, dx is the plain data gradient (+ residual), unmasked, and fused is false —
// the BN backward then runs its own statistics pass (a separate preparation pass here would cost
// more than that pass: it writes the masked gradient too).
std::tuple<at::Tensor, bool> conv2d_dgrad_bn(const at::Tensor& dy, const at::Tensor& w, int64_t stride, int64_t pad, int64_t H,
                           int64_t W, const c10::optional<at::Tensor>& residual, const at::Tensor& x,
                           const c10::optional<at::Tensor>& y, const at::Tensor& mean, const at::Tensor& rstd,
                           const at::Tensor& gamma, const at::Tensor& beta, at::Tensor sums, int64_t groups,
                           const c10::optional<std::vector<at::Tensor>>& wds) {
  expect_nhwc(x, "x");
  if (y.has_value()) expect_nhwc(*y, "y");
  expect(mean, at::kFloat, "mean");
  expect(rstd, at::kFloat, "rstd");
  expect(gamma, at::kFloat, "gamma");
  expect(beta, at::kFloat, "beta");
  expect(sums, at::kFloat, "sums");
  const int64_t N = x.size(0), C = x.size(1);
  TORCH_CHECK(groups >= 1 && N % groups == 0 && mean.numel() == groups * C && rstd.numel() == groups * C &&
                  sums.numel() == 2 * groups * C,
              "conv2d_dgrad_bn: statistics shapes");
  TORCH_CHECK(x.size(2) == H && x.size(3) == W && w.size(1) == C, "conv2d_dgrad_bn: x must be the conv input");
  const long stat_rows = N / groups * H * W;
  const DlBnBwdEpi bn{cbf(x), y.has_value() ? cbf(*y) : nullptr, (long)C, f32(mean), f32(rstd), f32(gamma),
                      f32(beta)};
  const at::Tensor gdy = dy.is_contiguous(at::MemoryFormat::ChannelsLast) ? dy
                                                                           : dy.contiguous(at::MemoryFormat::ChannelsLast);
  const int64_t K = w.size(0), R = w.size(2), S = w.size(3);
  if (is_pointwise(R, S, stride, pad) && gdy.size(2) == H && gdy.size(3) == W && conv_gemm()) {
    expect_nhwc(gdy, "dy");
    if (residual.has_value()) {
      expect_nhwc(*residual, "residual");
      TORCH_CHECK(residual->sizes() == x.sizes(), "conv2d_dgrad_bn: residual must have the input's shape");
    }
    auto dx = at::empty_like(x);
    const at::Tensor wk = krsc_view(w);
    const at::Tensor dyr = rows2d(gdy), wkc = wk.view({K, C});
    DlGemm g = gemm_desc(dyr, false, wkc, false, bf(dx), C);
    g.epi = DL_EPI_BNBWD;
    if (residual.has_value()) g.R = cbf(*residual), g.ldr = C;
    g.stats = f32(sums), g.stat_rows = stat_rows;
    g.bn = &bn;
    if (gemm_route(g, kUse8, dyr, cur_stream(dy)) != kGemmNone) return {dx, true};
  }
  // 3x3 / strided data gradients (Bottleneck conv2 <- bn1) and the 1x1 ones gemm8 does not take
  // (at most 128 input channels: conv3 <- bn2 in the first stages): conv.hip's epilogue
  if (!residual.has_value() && K % 64 == 0) {
    expect_nhwc(gdy, "dy");
    auto dx = at::empty_like(x);
    if (conv_dgrad_classes(gdy, krsc_view(w), stride, pad, H, W, dx, wds, f32(sums), groups, &bn)) return {dx, true};
  }
  return {conv2d_dgrad(gdy, w, stride, pad, H, W, residual, wds), false};
}

// the preparation as its own pass (tests; the fallback the fused epilogues are checked against)
at::Tensor bn_bwd_prep(at::Tensor g, const at::Tensor& x, const c10::optional<at::Tensor>& y, const at::Tensor& mean,
                       const at::Tensor& rstd, const at::Tensor& gamma, const at::Tensor& beta, at::Tensor sums,
                       int64_t groups) {
  expect_nhwc(g, "g");
  expect_nhwc(x, "x");
  const int64_t C = x.size(1);
  check(dl_bn_bwd_prep(bf(g), y.has_value() ? cbf(*y) : nullptr, cbf(x), f32(mean), f32(rstd), f32(gamma), f32(beta),
                       f32(sums), x.numel() / C / groups, (int)C, (int)groups, cur_stream(g)),
        "bn_bwd_prep");
  return g;
}

// dW (fp32 [Cout, Cin, R, S] with KRSC memory, e.g. the flat-buffer grad view) += conv wgrad
void conv2d_wgrad(const at::Tensor& dy_in, const at::Tensor& x, at::Tensor dw, int64_t stride, int64_t pad,
                  const c10::optional<at::Tensor>& cols) {
  const at::Tensor dy = dy_in.is_contiguous(at::MemoryFormat::ChannelsLast)
                            ? dy_in
                            : dy_in.contiguous(at::MemoryFormat::ChannelsLast);
  expect_nhwc(dy, "dy");
  if (!cols.has_value()) expect_nhwc(x, "x");  // with the stem's cols only x's shape is read
  TORCH_CHECK(dw.is_cuda() && dw.scalar_type() == at::kFloat && dw.dim() == 4, "dw must be an fp32 4-D GPU tensor");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t K = dy.size(1), P = dy.size(2), Q = dy.size(3), R = dw.size(2), S = dw.size(3);
  TORCH_CHECK(dw.size(0) == K && dw.size(1) == C, "conv2d_wgrad: dw shape mismatch");
  TORCH_CHECK(!cols.has_value() || C % 64 != 0, "conv2d_wgrad: cols are the stem's (C not a multiple of 64) only");
  at::Tensor dk = dw.permute({0, 2, 3, 1});  // [K, R, S, C]
  const bool direct = dk.is_contiguous();
  at::Tensor acc = direct ? dk : at::zeros({K, R, S, C}, dw.options());
  int rc;
  if (is_pointwise(R, S, stride, pad) && conv_gemm() && K % 256 == 0 && C % 256 == 0) {
    gemm_acc_f32(rows2d(dy), rows2d(x), acc.view({K, C}), true, false);
  } else if (C % 8 == 0 && C >= 8 && C % 64 == 0) {
    const DlConvGeom gm = geom(cbf(x), N, H, W, C, P, Q, stride, stride, R, S, -pad, 1, -pad, 1);
    // split partials accumulate with fp32 atomics (the slab-and-sum form measured no consistent
    // gain in round 3 and was removed)
    rc = dl_conv_wgrad(gm, cbf(dy), K, (int)K, f32(acc), R * S * C, (int)(R * S * C), cur_stream(dy));
    check(rc, "conv2d_wgrad");
  } else if (stem_s2d_ok(C, R, S, stride, pad, H, W)) {
    // stem: 4x4 wgrad over the space-to-depth image into [K, 256], folded back onto the 7x7 taps
    at::Tensor xs;
    if (cols.has_value()) {
      TORCH_CHECK(cols->scalar_type() == at::kBFloat16 && cols->is_contiguous() && cols->dim() == 2 &&
                      cols->size(0) == N * P * Q && cols->size(1) == 16,
                  "cols must be the stem's im2col_stem (space-to-depth) matrix for this input");
      xs = *cols;
    } else {
      xs = stem_s2d(x);
    }
    auto slab = at::zeros({K, 256}, dw.options());
    rc = dl_conv_wgrad(geom(cbf(xs), N, H / 2, W / 2, 16, P, Q, 1, 1, 4, 4, -2, 1, -2, 1), cbf(dy), K, (int)K,
                       f32(slab), 256, 256, cur_stream(dy));
    check(rc, "conv2d_wgrad(stem)");
    acc.view({K, R * S * C}).add_(slab.index_select(1, stem_s2d_index(dw.device())));
  } else {
    // other small-channel convs: wgrad over the padded column matrix into a [K, R, SCp] slab, then
    // the real columns
    const StemCols sc = stem_cols(R, S, C, false);
    const int64_t M = N * P * Q;
    const at::Tensor col = stem_cols_checked(cols, x, R, S, stride, pad, P, Q, sc);
    auto slab = at::zeros({K, R, sc.SCp}, dw.options());
    rc = dl_conv_wgrad(geom(cbf(col), M, 1, 1, sc.Kp, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1), cbf(dy), K, (int)K,
                       f32(slab), R * sc.SCp, (int)(R * sc.SCp), cur_stream(dy));
    check(rc, "conv2d_wgrad(stem)");
    acc.view({K, R, S * C}).add_(slab.narrow(2, 0, S * C));
  }
  if (!direct) dk.add_(acc);
}

}  // namespace

TORCH_LIBRARY_IMPL(dedloc, CUDA, m) {
  m.impl("conv2d_fwd", &conv2d_fwd);
  m.impl("conv2d_bn_act", &conv2d_bn_act);
  m.impl("conv2d_fwd_stats", &conv2d_fwd_stats);
  m.impl("im2col_stem", &im2col_stem);
  m.impl("conv2d_dgrad_bn", &conv2d_dgrad_bn);
  m.impl("conv2d_dgrad_weights", &conv2d_dgrad_weights);
  m.impl("conv2d_dgrad_weights_batched", &conv2d_dgrad_weights_batched);
  m.impl("bn_bwd_prep", &bn_bwd_prep);
  m.impl("conv2d_dgrad", &conv2d_dgrad);
  m.impl("conv2d_wgrad", &conv2d_wgrad);
  m.impl("bn_fwd", &bn_fwd);
  m.impl("bn_apply", &bn_apply);
  m.impl("bn_bwd", &bn_bwd);
  m.impl("sinkhorn", &sinkhorn);
  m.impl("swav_ce", &swav_ce);
  m.impl("swav_ce_multi", &swav_ce_multi);
  m.impl("row_normalize_", &row_normalize_);
  m.impl("maxpool_fwd", &maxpool_fwd);
  m.impl("maxpool_bwd", &maxpool_bwd);
  m.impl("avgpool_fwd", &avgpool_fwd);
  m.impl("avgpool_bwd", &avgpool_bwd);
  m.impl("l2norm_fwd", &l2norm_fwd);
  m.impl("l2norm_bwd", &l2norm_bwd);
  m.impl("multicrop", &multicrop);
  m.impl("multicrop_ragged", &multicrop_ragged);
  m.impl("layernorm_fwd", &layernorm_fwd);
  m.impl("layernorm_bwd", &layernorm_bwd);
  m.impl("gelu_fwd", &gelu_fwd);
  m.impl("gelu_bwd", &gelu_bwd);
  m.impl("tanh_fwd", &tanh_fwd);
  m.impl("tanh_bwd", &tanh_bwd);
  m.impl("bias_grad", &bias_grad);
  m.impl("cast_bf16", &cast_bf16);
  m.impl("lamb_step", &lamb_step);
  m.impl("larc_sgd_step", &larc_sgd_step);
  m.impl("grad_norm_clip", &grad_norm_clip);
  m.impl("axpby", &axpby);
  m.impl("add_slabs_zero_", &add_slabs_zero_);
  m.impl("scale_by_", &scale_by_);
  m.impl("pack", &pack);
  m.impl("reduce_parts", &reduce_parts);
  m.impl("unpack", &unpack);
  m.impl("reduce_delta", &reduce_delta);
  m.impl("pack_q8", &pack_q8);
  m.impl("reduce_delta_q8", &reduce_delta_q8);
  m.impl("unpack_q8", &unpack_q8);
  m.impl("embed_ln_fwd", &embed_ln_fwd);
  m.impl("embed_bwd", &embed_bwd);
  m.impl("xent_fwd_bwd", &xent_fwd_bwd);
  m.impl("xent_eval", &xent_eval);
  m.impl("knn_topk", &knn_topk);
  m.impl("knn_vote", &knn_vote);
  m.impl("attn_fwd", &attn_fwd);
  m.impl("attn_bwd", &attn_bwd);
  m.impl("attn_fwd_q", &attn_fwd_q);
  m.impl("attn_bwd_q", &attn_bwd_q);
  m.impl("attn_varlen_fwd", &attn_varlen_fwd);
  m.impl("attn_varlen_bwd", &attn_varlen_bwd);
  m.impl("embed_ln_pos_fwd", &embed_ln_pos_fwd);
  m.impl("embed_pos_bwd", &embed_pos_bwd);
  m.impl("attn_softmax_fwd", &attn_softmax_fwd);
  m.impl("attn_softmax_bwd", &attn_softmax_bwd);
  m.impl("gemm", &gemm);
  m.impl("bmm", &bmm);
  m.impl("gemm_acc_f32", &gemm_acc_f32);
  m.impl("gemm_acc_f32_shared", &gemm_acc_f32_shared);
  m.impl("gemm_gelu", &gemm_gelu);
  m.impl("gemm_dgelu", &gemm_dgelu);
  m.impl("gemm_gelu_d", &gemm_gelu_d);
  m.impl("gemm_dmul", &gemm_dmul);
}

// a tiny C entry point so that the loader can verify the library really is the gfx950 build
extern "C" int dedloc_amd_native_abi_version() { return 1; }

TORCH_LIBRARY(dedloc_ws, m) {
  m.def("clear_workspaces() -> int", &clear_workspaces);
  m.def("gemm_backend_counts() -> int[]", &gemm_backend_counts);
  m.def("gemm_wgrad_splits(int M, int N, int K) -> int", &gemm_wgrad_splits);
}
