// Bindings of the attention kernels: training forward / backward (attention.hip,
// attention128.hip) and the KV-cache decode steps (attn_decode.hip, attn_decode_block.hip,
// attn_decode_fp8.hip).
#include "bind_util.h"

static std::vector<at::Tensor> attn_fwd(const at::Tensor& qkv, int64_t heads, double p, bool causal,
                                        int64_t seed, int64_t offset, bool head_major) {
  CHECK_DEV(qkv); CHECK_BF16(qkv); CHECK_CONTIG(qkv);
  TORCH_CHECK(qkv.dim() == 3, "qkv must be [B, L, 3*H*D]");
  const int B = (int)qkv.size(0), L = (int)qkv.size(1), H = (int)heads;
  TORCH_CHECK(H > 0 && qkv.size(2) % (3LL * H) == 0, "attn: qkv width must be 3*H*D");
  const int D = (int)(qkv.size(2) / (3LL * H));
  TORCH_CHECK(D == 64 || D == 128, "attn: head_dim must be 64 or 128");
  TORCH_CHECK(L % 64 == 0, "attn: L must be a multiple of 64");
  const c10::DeviceGuard guard(qkv.device());
  at::Tensor out = at::empty({B, L, (int64_t)H * D}, qkv.options());
  at::Tensor lse = at::empty({B, H, L}, qkv.options().dtype(at::kFloat));
  TORCH_CHECK(!head_major || dpa::attn128_supports(L, D, causal),
              "attn_fwd: the head-major qkv layout needs L == 128, head_dim 64, bidirectional");
  const bool ok = dpa::launch_attn_fwd(bf_ptr(qkv), bf_mut(out), lse.data_ptr<float>(), B, L, H, D, (float)p,
                                       causal, (uint32_t)seed, (uint32_t)offset, cur_stream(), head_major);
  TORCH_CHECK(ok, "attn_fwd: no kernel for this shape");
  return {out, lse};
}

static void attn_colpart_reduce(const at::Tensor& part, int64_t R, int64_t H, int64_t D, at::Tensor db) {
  CHECK_DEV(part);
  TORCH_CHECK(part.scalar_type() == at::kFloat && db.scalar_type() == at::kFloat && part.is_contiguous() &&
                  db.is_contiguous() && part.numel() >= R * H * 3 * D && db.numel() == 3 * H * D &&
                  D % 64 == 0 && R > 0,
              "attn_colpart_reduce: fp32 part [R*H][3D], db [3HD]");
  const c10::DeviceGuard guard(part.device());
  dpa::launch_colpart_reduce(part.data_ptr<float>(), db.data_ptr<float>(), (int)R, (int)H, (int)D, cur_stream());
}

static std::vector<at::Tensor> attn_bwd(const at::Tensor& dout, const at::Tensor& qkv,
                                        const at::Tensor& out, const at::Tensor& lse, int64_t heads,
                                        double p, bool causal, int64_t seed, int64_t offset,
                                        bool want_db, bool head_major, c10::optional<at::Tensor> db_acc,
                                        c10::optional<at::Tensor> part_out) {
  CHECK_DEV(dout); CHECK_BF16(dout); CHECK_CONTIG(dout); CHECK_CONTIG(out); CHECK_CONTIG(qkv);
  const int B = (int)qkv.size(0), L = (int)qkv.size(1), H = (int)heads;
  TORCH_CHECK(dout.sizes() == out.sizes(), "dout shape");
  TORCH_CHECK(H > 0 && qkv.size(2) % (3LL * H) == 0, "attn: qkv width must be 3*H*D");
  const int D = (int)(qkv.size(2) / (3LL * H));
  TORCH_CHECK(D == 64 || D == 128, "attn: head_dim must be 64 or 128");
  TORCH_CHECK(L % 64 == 0 && out.size(2) == (int64_t)H * D, "attn_bwd: shapes");
  TORCH_CHECK(lse.numel() == (int64_t)B * H * L, "attn_bwd: lse shape");
  TORCH_CHECK(!head_major || dpa::attn128_supports(L, D, causal),
              "attn_bwd: the head-major qkv layout needs L == 128, head_dim 64, bidirectional");
  const c10::DeviceGuard guard(qkv.device());
  at::Tensor dqkv = at::empty_like(qkv);
  auto f32 = qkv.options().dtype(at::kFloat);
  at::Tensor delta = at::empty({B, H, L}, f32);
  at::Tensor dq, colpart, db;
  if (dpa::attn_bwd_needs_dq_acc(L)) dq = at::zeros({B, L, H, D}, f32);
  // db_acc: the qkv bias gradient accumulated straight onto this fp32 .grad (returned undefined)
  const bool acc = want_db && usable_acc(db_acc, 3LL * H * D, qkv.device());
  // part_out: a caller-owned fp32 slot of attn_colpart_rows * 3 D floats; the bias-gradient
  // partials are left there for a later colpart_reduce (deferral window), db is not produced
  const int64_t cp_n = dpa::attn_colpart_rows(B, L, H, D, causal) * 3 * D;
  const bool defer = want_db && acc && usable_acc(part_out, -1, qkv.device()) && part_out->numel() >= cp_n;
  if (want_db) {
    colpart = defer ? *part_out : at::empty({cp_n}, f32);
    db = acc ? *db_acc : at::empty({3 * H * D}, f32);
  }
  bool got = dpa::launch_attn_bwd(
      bf_ptr(qkv), bf_ptr(out), bf_ptr(dout), lse.data_ptr<float>(), delta.data_ptr<float>(), bf_mut(dqkv),
      dq.defined() ? dq.data_ptr<float>() : nullptr, want_db ? colpart.data_ptr<float>() : nullptr,
      want_db ? db.data_ptr<float>() : nullptr, B, L, H, D, (float)p, causal, (uint32_t)seed, (uint32_t)offset,
      cur_stream(), head_major, acc, defer);
  if (defer) {
    TORCH_CHECK(got, "attn_bwd: deferred column sums on a path without partials");
    return {dqkv, at::Tensor()};
  }
  if (want_db && !got) {
    // no fused column sums on this path (L != 128): one column-sum pass over the bf16 dqkv,
    // accumulated onto db (zeroed unless it is the parameter's .grad)
    if (!acc) db.zero_();
    const int Nq = (int)(3LL * H * D);
    at::Tensor ws = at::empty({dpa::bias_act_bwd_ws_floats((int64_t)B * L, Nq)}, db.options());
    dpa::launch_bias_act_bwd(bf_ptr(dqkv), nullptr, nullptr, db.data_ptr<float>(), (int64_t)B * L, Nq, 0,
                             cur_stream(), ws.data_ptr<float>());
    got = true;
  }
  // contract: with a usable db_acc the bias gradient is always accumulated (result undefined)
  return {dqkv, got && !acc ? db : at::Tensor()};
}

// One decode step's cache append + single-query attention (csrc/attn_decode.hip): qkv_new [B, 3 H D]
// bf16, k_cache / v_cache [B, H, Lmax, D] bf16 (updated in place; batch and head strides free, so
// views into a larger buffer work), lens [B] int32 -> out [B, H D] bf16, or None for a case the
// kernel does not cover (dtype, D, CPU tensors, row layout): the caller's PyTorch path takes it.
//
// With `src` (attn_decode_beam): the rows are groups of `beams` slots and src uint8 [B, Lmax] names the
// slot of the row's group that holds each cached key (launchers.h has the semantics and the caller's
// contract).
static c10::optional<at::Tensor> attn_decode_any(const at::Tensor& qkv_new, at::Tensor& k_cache, at::Tensor& v_cache,
                                                 const at::Tensor& lens, int64_t n_heads, const at::Tensor* src,
                                                 int64_t beams) {
  TORCH_CHECK(qkv_new.dim() == 2 && k_cache.dim() == 4 && v_cache.dim() == 4 && lens.dim() == 1 && n_heads > 0,
              "attn_decode: qkv_new [B, 3 H D], caches [B, H, Lmax, D], lens [B]");
  const int64_t B = k_cache.size(0), H = k_cache.size(1), Lmax = k_cache.size(2), D = k_cache.size(3);
  TORCH_CHECK(H == n_heads && v_cache.sizes() == k_cache.sizes() && qkv_new.size(0) == B &&
                  qkv_new.size(1) == 3 * H * D && lens.size(0) == B,
              "attn_decode: shapes of qkv_new, the caches, lens and n_heads do not agree");
  TORCH_CHECK(lens.scalar_type() == at::kInt, "attn_decode: lens must be int32");
  if (src) {
    TORCH_CHECK(src->scalar_type() == at::kByte, "attn_decode_beam: src must be uint8");
    TORCH_CHECK(src->dim() == 2 && src->size(0) == B && src->size(1) == Lmax, "attn_decode_beam: src must be [R, Lmax]");
    TORCH_CHECK(src->stride(1) == 1 || Lmax <= 1, "attn_decode_beam: src must have last stride 1");
    TORCH_CHECK(beams >= 1 && beams <= 255, "attn_decode_beam: beams must be in 1 .. 255");
    TORCH_CHECK(B % beams == 0, "attn_decode_beam: the rows must be whole groups of `beams`");
    if (!src->is_cuda() || src->device() != qkv_new.device() || (B > 1 && src->stride(0) < Lmax)) return c10::nullopt;
  }
  for (const at::Tensor* t : {&qkv_new, (const at::Tensor*)&k_cache, (const at::Tensor*)&v_cache, &lens})
    if (!t->is_cuda() || t->device() != qkv_new.device()) return c10::nullopt;
  if (qkv_new.scalar_type() != at::kBFloat16 || k_cache.scalar_type() != at::kBFloat16 ||
      v_cache.scalar_type() != at::kBFloat16)
    return c10::nullopt;
  if ((D != 64 && D != 128) || B == 0 || Lmax == 0 || Lmax > 0x7fffffffLL || B * H > 0x7fffffffLL) return c10::nullopt;
  auto rows_ok = [&](const at::Tensor& c) {  // packed rows of D; 16-byte row starts
    return c.stride(3) == 1 && c.stride(2) == D && c.stride(0) % 8 == 0 && c.stride(1) % 8 == 0 &&
           reinterpret_cast<uintptr_t>(c.data_ptr()) % 16 == 0;
  };
  if (!rows_ok(k_cache) || !rows_ok(v_cache) || !lens.is_contiguous()) return c10::nullopt;
  if (qkv_new.stride(1) != 1 || qkv_new.stride(0) % 8 != 0 || reinterpret_cast<uintptr_t>(qkv_new.data_ptr()) % 16 != 0)
    return c10::nullopt;
  const c10::DeviceGuard guard(qkv_new.device());
  at::Tensor out = at::empty({B, H * D}, qkv_new.options());
  const bool ok =
      src ? dpa::launch_attn_decode_beam(bf_ptr(qkv_new), qkv_new.stride(0), bf_mut(k_cache), bf_mut(v_cache),
                                         k_cache.stride(0), k_cache.stride(1), v_cache.stride(0), v_cache.stride(1),
                                         lens.data_ptr<int>(), src->data_ptr<uint8_t>(), B > 1 ? src->stride(0) : Lmax,
                                         (int)beams, (int)B, (int)H, (int)Lmax, (int)D, bf_mut(out), cur_stream())
          : dpa::launch_attn_decode(bf_ptr(qkv_new), qkv_new.stride(0), bf_mut(k_cache), bf_mut(v_cache),
                                    k_cache.stride(0), k_cache.stride(1), v_cache.stride(0), v_cache.stride(1),
                                    lens.data_ptr<int>(), (int)B, (int)H, (int)Lmax, (int)D, bf_mut(out), cur_stream());
  if (!ok) return c10::nullopt;
  return out;
}

static c10::optional<at::Tensor> attn_decode(const at::Tensor& qkv_new, at::Tensor& k_cache, at::Tensor& v_cache,
                                             const at::Tensor& lens, int64_t n_heads) {
  return attn_decode_any(qkv_new, k_cache, v_cache, lens, n_heads, nullptr, 1);
}

static c10::optional<at::Tensor> attn_decode_beam(const at::Tensor& qkv_new, at::Tensor& k_cache,
                                                  at::Tensor& v_cache, const at::Tensor& lens, int64_t n_heads,
                                                  const at::Tensor& src, int64_t beams) {
  return attn_decode_any(qkv_new, k_cache, v_cache, lens, n_heads, &src, beams);
}

// A block of T new tokens per row (csrc/attn_decode_block.hip): qkv_new [B, T, 3 H D] bf16, counts
// int32 [B] or None (= T) -> out [B, T, H D] bf16: T successive attn_decode calls in one pass over the
// caches (launchers.h has the definition), or None for a case the kernel does not cover.
static c10::optional<at::Tensor> attn_decode_block(const at::Tensor& qkv_new, at::Tensor& k_cache, at::Tensor& v_cache,
                                                   const at::Tensor& lens, int64_t n_heads,
                                                   c10::optional<at::Tensor> counts) {
  TORCH_CHECK(qkv_new.dim() == 3 && k_cache.dim() == 4 && v_cache.dim() == 4 && lens.dim() == 1 && n_heads > 0,
              "attn_decode_block: qkv_new [B, T, 3 H D], caches [B, H, Lmax, D], lens [B]");
  const int64_t B = k_cache.size(0), H = k_cache.size(1), Lmax = k_cache.size(2), D = k_cache.size(3);
  const int64_t T = qkv_new.size(1);
  TORCH_CHECK(H == n_heads && v_cache.sizes() == k_cache.sizes() && qkv_new.size(0) == B &&
                  qkv_new.size(2) == 3 * H * D && lens.size(0) == B,
              "attn_decode_block: shapes of qkv_new, the caches, lens and n_heads do not agree");
  TORCH_CHECK(T >= 1 && T <= 8, "attn_decode_block: T must be in 1 .. 8, got ", T);
  TORCH_CHECK(lens.scalar_type() == at::kInt, "attn_decode_block: lens must be int32");
  const bool has_counts = counts.has_value() && counts->defined();
  if (has_counts)
    TORCH_CHECK(counts->scalar_type() == at::kInt && counts->dim() == 1 && counts->size(0) == B,
                "attn_decode_block: counts must be int32 [B]");
  for (const at::Tensor* t : {&qkv_new, (const at::Tensor*)&k_cache, (const at::Tensor*)&v_cache, &lens})
    if (!t->is_cuda() || t->device() != qkv_new.device()) return c10::nullopt;
  if (has_counts && (!counts->is_cuda() || counts->device() != qkv_new.device() || !counts->is_contiguous()))
    return c10::nullopt;
  if (qkv_new.scalar_type() != at::kBFloat16 || k_cache.scalar_type() != at::kBFloat16 ||
      v_cache.scalar_type() != at::kBFloat16)
    return c10::nullopt;
  if ((D != 64 && D != 128) || B == 0 || Lmax == 0 || Lmax > 0x7fffffffLL || B * H > 0x7fffffffLL) return c10::nullopt;
  auto rows_ok = [&](const at::Tensor& c) {  // packed rows of D; 16-byte row starts
    return c.stride(3) == 1 && c.stride(2) == D && c.stride(0) % 8 == 0 && c.stride(1) % 8 == 0 &&
           reinterpret_cast<uintptr_t>(c.data_ptr()) % 16 == 0;
  };
  if (!rows_ok(k_cache) || !rows_ok(v_cache) || !lens.is_contiguous()) return c10::nullopt;
  if (qkv_new.stride(2) != 1 || qkv_new.stride(0) % 8 != 0 || qkv_new.stride(1) % 8 != 0 ||
      reinterpret_cast<uintptr_t>(qkv_new.data_ptr()) % 16 != 0)
    return c10::nullopt;
  const c10::DeviceGuard guard(qkv_new.device());
  at::Tensor out = at::empty({B, T, H * D}, qkv_new.options());
  const bool ok = dpa::launch_attn_decode_block(
      bf_ptr(qkv_new), qkv_new.stride(0), qkv_new.stride(1), bf_mut(k_cache), bf_mut(v_cache), k_cache.stride(0),
      k_cache.stride(1), v_cache.stride(0), v_cache.stride(1), lens.data_ptr<int>(),
      has_counts ? counts->data_ptr<int>() : nullptr, (int)B, (int)T, (int)H, (int)Lmax, (int)D, bf_mut(out),
      cur_stream());
  if (!ok) return c10::nullopt;
  return out;
}

// The decode step over a one-byte cache (csrc/attn_decode_fp8.hip): qkv_new [B, 3 H D] bf16, k8 / v8 uint8
// [B, H, Lmax, D], ke / ve int8 [B, H, Lmax] (all four updated in place at row lens[b]), lens [B] int32
// -> out [B, H D] bf16, or None for a case the kernel does not cover: the caller's PyTorch path takes it.
static c10::optional<at::Tensor> attn_decode_fp8(const at::Tensor& qkv_new, at::Tensor& k8, at::Tensor& ke,
                                                 at::Tensor& v8, at::Tensor& ve, const at::Tensor& lens,
                                                 int64_t n_heads) {
  TORCH_CHECK(qkv_new.dim() == 2 && lens.dim() == 1 && n_heads > 0, "attn_decode_fp8: qkv_new [B, 3 H D], lens [B]");
  const bool k_ok = fp8_cache_usable(k8, ke, qkv_new.device(), "attn_decode_fp8 (k)");
  const bool v_ok = fp8_cache_usable(v8, ve, qkv_new.device(), "attn_decode_fp8 (v)");
  const int64_t B = k8.size(0), H = k8.size(1), Lmax = k8.size(2), D = k8.size(3);
  TORCH_CHECK(H == n_heads && v8.sizes() == k8.sizes() && qkv_new.size(0) == B && qkv_new.size(1) == 3 * H * D &&
                  lens.size(0) == B,
              "attn_decode_fp8: shapes of qkv_new, the caches, lens and n_heads do not agree");
  TORCH_CHECK(lens.scalar_type() == at::kInt, "attn_decode_fp8: lens must be int32");
  if (!k_ok || !v_ok || !qkv_new.is_cuda() || !lens.is_cuda() || lens.device() != qkv_new.device()) return c10::nullopt;
  if (qkv_new.scalar_type() != at::kBFloat16 || !lens.is_contiguous()) return c10::nullopt;
  if ((D != 64 && D != 128) || B == 0 || Lmax == 0 || Lmax > 0x7fffffffLL || B * H > 0x7fffffffLL) return c10::nullopt;
  if (qkv_new.stride(1) != 1 || qkv_new.stride(0) % 8 != 0 || reinterpret_cast<uintptr_t>(qkv_new.data_ptr()) % 16 != 0)
    return c10::nullopt;
  const c10::DeviceGuard guard(qkv_new.device());
  at::Tensor out = at::empty({B, H * D}, qkv_new.options());
  const bool ok = dpa::launch_attn_decode_fp8(
      bf_ptr(qkv_new), qkv_new.stride(0), k8.data_ptr<uint8_t>(), ke.data_ptr<int8_t>(), v8.data_ptr<uint8_t>(),
      ve.data_ptr<int8_t>(), k8.stride(0), k8.stride(1), ke.stride(0), ke.stride(1), v8.stride(0), v8.stride(1),
      ve.stride(0), ve.stride(1), lens.data_ptr<int>(), (int)B, (int)H, (int)Lmax, (int)D, bf_mut(out), cur_stream());
  if (!ok) return c10::nullopt;
  return out;
}

// The prefill's quantizing store: qkv [B, L, 3 H D] bf16 (last stride 1, any batch and position stride),
// lens [B] int32; K and V of the positions l < lens[b] go to cache row l -> false for a case the kernel
// does not cover (nothing written).
static bool kv8_store(const at::Tensor& qkv, const at::Tensor& lens, at::Tensor& k8, at::Tensor& ke, at::Tensor& v8,
                      at::Tensor& ve) {
  TORCH_CHECK(qkv.dim() == 3 && lens.dim() == 1, "kv_store: qkv [B, L, 3 H D], lens [B]");
  const bool k_ok = fp8_cache_usable(k8, ke, qkv.device(), "kv_store (k)");
  const bool v_ok = fp8_cache_usable(v8, ve, qkv.device(), "kv_store (v)");
  const int64_t B = k8.size(0), H = k8.size(1), Lmax = k8.size(2), D = k8.size(3), L = qkv.size(1);
  TORCH_CHECK(v8.sizes() == k8.sizes() && qkv.size(0) == B && qkv.size(2) == 3 * H * D && lens.size(0) == B,
              "kv_store: shapes of qkv, the caches and lens do not agree");
  TORCH_CHECK(L <= Lmax, "kv_store: ", L, " positions do not fit a cache of ", Lmax);
  TORCH_CHECK(lens.scalar_type() == at::kInt, "kv_store: lens must be int32");
  if (!k_ok || !v_ok || !qkv.is_cuda() || !lens.is_cuda() || lens.device() != qkv.device()) return false;
  if (qkv.scalar_type() != at::kBFloat16 || !lens.is_contiguous()) return false;
  if ((D != 64 && D != 128) || B == 0 || L == 0 || B > 0x7fffffffLL || Lmax > 0x7fffffffLL) return false;
  if (qkv.stride(2) != 1 || qkv.stride(0) % 8 != 0 || qkv.stride(1) % 8 != 0 ||
      reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 != 0)
    return false;
  const c10::DeviceGuard guard(qkv.device());
  return dpa::launch_kv8_store(bf_ptr(qkv), qkv.stride(0), qkv.stride(1), lens.data_ptr<int>(), k8.data_ptr<uint8_t>(),
                               ke.data_ptr<int8_t>(), v8.data_ptr<uint8_t>(), ve.data_ptr<int8_t>(), k8.stride(0),
                               k8.stride(1), ke.stride(0), ke.stride(1), v8.stride(0), v8.stride(1), ve.stride(0),
                               ve.stride(1), (int)B, (int)L, (int)H, (int)Lmax, (int)D, cur_stream());
}

// x [R, D] bf16 -> (codes uint8 [R, D], exponents int8 [R]), or None for a case the kernel does not cover.
static c10::optional<std::vector<at::Tensor>> kv8_quantize(const at::Tensor& x) {
  TORCH_CHECK(x.dim() == 2, "kv_quantize: x must be [R, D]");
  const int64_t R = x.size(0), D = x.size(1);
  if (!x.is_cuda() || x.scalar_type() != at::kBFloat16 || !x.is_contiguous() || (D != 64 && D != 128) || R == 0 ||
      reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 != 0)
    return c10::nullopt;
  const c10::DeviceGuard guard(x.device());
  at::Tensor codes = at::empty({R, D}, x.options().dtype(at::kByte));
  at::Tensor exps = at::empty({R}, x.options().dtype(at::kChar));
  if (!dpa::launch_kv8_quantize(bf_ptr(x), R, (int)D, codes.data_ptr<uint8_t>(), exps.data_ptr<int8_t>(), cur_stream()))
    return c10::nullopt;
  return std::vector<at::Tensor>{codes, exps};
}

void dpa::register_attention(pybind11::module& m) {
  m.def("attn128_supports", &dpa::attn128_supports, "the persistent L = 128 attention covers (L, D, causal)");
  m.def("attn_fwd", &attn_fwd, "fused attention forward (head_dim 64/128) -> (out, lse)", py::arg("qkv"),
        py::arg("heads"), py::arg("p"), py::arg("causal"), py::arg("seed"), py::arg("offset"),
        py::arg("head_major") = false);
  m.def("attn_bwd", &attn_bwd, "fused attention backward -> (dqkv, colsum(dqkv) or None)",
        py::arg("dout"), py::arg("qkv"), py::arg("out"), py::arg("lse"), py::arg("heads"), py::arg("p"),
        py::arg("causal"), py::arg("seed"), py::arg("offset"), py::arg("want_db") = false,
        py::arg("head_major") = false, py::arg("db_acc") = py::none(), py::arg("part_out") = py::none());
  m.def("attn_colpart_rows", &dpa::attn_colpart_rows,
        "rows of attn_bwd's bias-gradient partials ([rows][3 D] fp32) for (B, L, H, D, causal)");
  m.def("attn_colpart_reduce", &attn_colpart_reduce,
        "db[3 H D] += column sums of R x H rows of attn_bwd partials (deferred bias gradient)");
  m.def("attn_decode", &attn_decode,
        "KV-cache append + single-query attention of one decode step (caches updated in place) -> out [B, H D] bf16 | None (case not covered)",
        py::arg("qkv_new"), py::arg("k_cache"), py::arg("v_cache"), py::arg("lens"), py::arg("n_heads"));
  m.def("attn_decode_beam", &attn_decode_beam,
        "attn_decode through a cache indirection table: rows in groups of `beams`, src uint8 [R, Lmax] names the group slot holding each cached key -> out [R, H D] bf16 | None (case not covered)",
        py::arg("qkv_new"), py::arg("k_cache"), py::arg("v_cache"), py::arg("lens"), py::arg("n_heads"),
        py::arg("src"), py::arg("beams"));
  m.def("attn_decode_block", &attn_decode_block,
        "KV-cache append + attention of a block of T <= 8 new tokens per row, as T successive attn_decode calls in one pass over the caches -> out [B, T, H D] bf16 | None (case not covered)",
        py::arg("qkv_new"), py::arg("k_cache"), py::arg("v_cache"), py::arg("lens"), py::arg("n_heads"),
        py::arg("counts") = py::none());
  m.def("attn_decode_fp8", &attn_decode_fp8,
        "attn_decode over a one-byte cache (e4m3fn codes + one int8 exponent per row): quantizing append + single-query attention -> out [B, H D] bf16 | None (case not covered)",
        py::arg("qkv_new"), py::arg("k8"), py::arg("ke"), py::arg("v8"), py::arg("ve"), py::arg("lens"),
        py::arg("n_heads"));
  m.def("kv8_store", &kv8_store,
        "quantize K and V of qkv [B, L, 3 H D] bf16 into the one-byte cache for the positions below lens -> bool (False: case not covered, nothing written)",
        py::arg("qkv"), py::arg("lens"), py::arg("k8"), py::arg("ke"), py::arg("v8"), py::arg("ve"));
  m.def("kv8_quantize", &kv8_quantize,
        "x [R, D] bf16 -> (codes uint8 [R, D], exponents int8 [R]) of the one-byte cache format | None (case not covered)",
        py::arg("x"));
}
