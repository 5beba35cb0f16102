// Bindings of the DiffuSeq diffusion kernels (diffusion.hip, reverse_step.hip), the embedding
// gradient with its id sort (sort.hip) and the device-side Philox offset base.
#include "bind_util.h"

// ---- id sort and embedding gradient -----------------------------------------------------
// (sorted ids, permutation) with equal ids adjacent in index order: the stable counting sort of
// csrc/sort.hip (block histograms, scans, ordered scatter) for vocabularies up to 81919, else a
// stable at::sort.
static std::tuple<at::Tensor, at::Tensor> bucket_sort_ids(const at::Tensor& ids, int64_t V) {
  const at::Tensor flat = ids.reshape({-1}).contiguous();
  const int64_t n = flat.numel();
  auto i64 = flat.options().dtype(at::kLong);
  at::Tensor sorted = at::empty({n}, i64), perm = at::empty({n}, i64);
  const int Vc = (int)std::min<int64_t>(V, 1 << 20);
  at::Tensor ws = at::empty({dpa::id_sort_workspace_ints(n, Vc)}, flat.options().dtype(at::kInt));
  if (V < (1 << 17) &&
      dpa::launch_id_bucket_sort(flat.data_ptr<int64_t>(), n, (int)V, ws.data_ptr<int>(),
                                 sorted.data_ptr<int64_t>(), perm.data_ptr<int64_t>(), cur_stream()))
    return {sorted, perm};
  return at::sort(flat, /*stable=*/true, 0, false);
}

static std::vector<at::Tensor> id_sort(const at::Tensor& ids, int64_t V) {
  CHECK_DEV(ids);
  TORCH_CHECK(ids.scalar_type() == at::kLong && V > 0, "id_sort: int64 ids, V > 0");
  const c10::DeviceGuard guard(ids.device());
  if (ids.numel() == 0) return {ids.reshape({-1}), ids.reshape({-1})};
  at::Tensor s, p;
  std::tie(s, p) = bucket_sort_ids(ids, V);
  return {s, p};
}

// order of a 0/1 (any nonzero = 1) int64 mask: nonzero entries first, both parts in index order
static at::Tensor partition01(const at::Tensor& mask) {
  CHECK_DEV(mask);
  TORCH_CHECK(mask.scalar_type() == at::kLong, "partition01: int64 mask");
  const c10::DeviceGuard guard(mask.device());
  const at::Tensor flat = mask.reshape({-1}).contiguous();
  const int64_t n = flat.numel();
  at::Tensor order = at::empty({n}, flat.options());
  if (n == 0) return order;
  at::Tensor ws = at::empty({dpa::partition01_workspace_ints(n)}, flat.options().dtype(at::kInt));
  TORCH_CHECK(dpa::launch_partition01(flat.data_ptr<int64_t>(), n, ws.data_ptr<int>(), order.data_ptr<int64_t>(),
                                      cur_stream()),
              "partition01: unsupported size ", n);
  return order;
}

// dW[ids[i]] += dy[i] (fp32 accumulate): counting sort of the ids, then one wave per run
// of equal ids sums its rows in registers and adds once (csrc/diffusion.hip) - the
// token-embedding backward without ATen's index_add.
void dpa::emb_grad(const at::Tensor& ids, const at::Tensor& dy, at::Tensor& dW) {
  CHECK_DEV(ids); CHECK_DEV(dy); CHECK_DEV(dW); CHECK_CONTIG(dy); CHECK_CONTIG(dW); CHECK_F32(dW);
  TORCH_CHECK(ids.scalar_type() == at::kLong, "emb_grad: int64 ids");
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 || dy.scalar_type() == at::kFloat, "emb_grad: bf16/fp32 dy");
  const int64_t NT = ids.numel(), E = dW.size(1);
  TORCH_CHECK(dy.numel() == NT * E, "emb_grad: dy [ids..., E]");
  if (NT == 0) return;
  const c10::DeviceGuard guard(dW.device());
  at::Tensor sorted, perm;
  std::tie(sorted, perm) = bucket_sort_ids(ids, dW.size(0));
  const bool b16 = dy.scalar_type() == at::kBFloat16;
  at::Tensor part = at::empty({dpa::emb_grad_part_floats(NT, (int)E, false)}, dW.options());
  TORCH_CHECK(dpa::launch_emb_grad(sorted.data_ptr<int64_t>(), perm.data_ptr<int64_t>(),
                                   b16 ? nullptr : dy.data_ptr<float>(), b16 ? bf_ptr(dy) : nullptr, NT, (int)E,
                                   (int)dW.size(0), dW.data_ptr<float>(), part.data_ptr<float>(), cur_stream()),
              "emb_grad: unsupported embedding width ", E);
}

// ---- DiffuSeq diffusion kernels ------------------------------------------------------------
static void check_diffusion_common(const at::Tensor& ids, const at::Tensor& t, const at::Tensor& W) {
  check_i64(ids, "ids");
  check_i64(t, "t");
  CHECK_DEV(W); CHECK_F32(W); CHECK_CONTIG(W); CHECK_ALIGNED(W);
  TORCH_CHECK(ids.dim() == 2 && t.dim() == 1 && t.size(0) == ids.size(0), "ids [B, L], t [B]");
  TORCH_CHECK(W.dim() == 2 && W.size(1) % 4 == 0, "W [V, E] with E % 4 == 0");
}

static std::vector<at::Tensor> emb_qsample_fwd(const at::Tensor& ids, const at::Tensor& mask,
                                               const at::Tensor& t, const at::Tensor& W,
                                               const at::Tensor& sa, const at::Tensor& s1a, double std0,
                                               int64_t seed, int64_t offset, bool want_x16) {
  check_diffusion_common(ids, t, W);
  check_i64(mask, "mask");
  TORCH_CHECK(mask.sizes() == ids.sizes(), "mask [B, L]");
  CHECK_DEV(sa); CHECK_F32(sa); CHECK_CONTIG(sa); CHECK_DEV(s1a); CHECK_F32(s1a); CHECK_CONTIG(s1a);
  TORCH_CHECK(sa.numel() == s1a.numel() && sa.numel() > 0, "schedule tables [T]");
  const int64_t B = ids.size(0), L = ids.size(1), E = W.size(1);
  const c10::DeviceGuard guard(W.device());
  auto bf = W.options().dtype(at::kBFloat16);
  at::Tensor xs = at::empty({B, L, E}, W.options()), xt = at::empty({B, L, E}, bf), x16;
  if (want_x16) x16 = at::empty({B, L, E}, bf);
  if (B * L > 0)
    dpa::launch_emb_qsample_fwd(ids.data_ptr<int64_t>(), mask.data_ptr<int64_t>(), t.data_ptr<int64_t>(),
                                W.data_ptr<float>(), sa.data_ptr<float>(), s1a.data_ptr<float>(), B * L,
                                (int)L, (int)E, (int)W.size(0), (float)std0, (uint32_t)seed,
                                (uint32_t)offset, xs.data_ptr<float>(), want_x16 ? bf_mut(x16) : nullptr,
                                bf_mut(xt), cur_stream());
  return {xs, x16, xt};
}

static void emb_qsample_bwd(const at::Tensor& ids, const at::Tensor& mask, const at::Tensor& t,
                            const at::Tensor& sa, c10::optional<at::Tensor> d_xs,
                            c10::optional<at::Tensor> d_xs16, c10::optional<at::Tensor> d_xt,
                            at::Tensor& dW) {
  check_diffusion_common(ids, t, dW);
  check_i64(mask, "mask");
  CHECK_DEV(sa); CHECK_F32(sa); CHECK_CONTIG(sa);
  const int64_t B = ids.size(0), L = ids.size(1), E = dW.size(1), n = B * L * E;
  const float* p_xs = opt_f32_ptr(d_xs, n, "d_x_start size", /*contig=*/true);
  const uint16_t* p_xs16 = opt_bf_ptr(d_xs16, n, "d_x_start16 size");
  const uint16_t* p_xt16 = nullptr;
  const float* p_xt32 = nullptr;
  if (has(d_xt)) {
    CHECK_CONTIG((*d_xt));
    TORCH_CHECK(d_xt->numel() == n, "d_x_t size");
    if (d_xt->scalar_type() == at::kBFloat16) p_xt16 = bf_ptr(*d_xt);
    else { CHECK_F32((*d_xt)); p_xt32 = d_xt->data_ptr<float>(); }
  }
  const c10::DeviceGuard guard(dW.device());
  if (n > 0) {
    // stable counting sort of the token ids -> runs of equal ids summed in registers, one
    // writer per gradient row (deterministic; csrc/sort.hip, csrc/diffusion.hip)
    at::Tensor sorted, perm, part;
    if (E == 128 || E == 256) {
      std::tie(sorted, perm) = bucket_sort_ids(ids, dW.size(0));
      part = at::empty({dpa::emb_grad_part_floats(B * L, (int)E, true)}, dW.options());
    }
    dpa::launch_emb_qsample_bwd(ids.data_ptr<int64_t>(), mask.data_ptr<int64_t>(), t.data_ptr<int64_t>(),
                                sa.data_ptr<float>(), p_xs, p_xs16, p_xt16, p_xt32, B * L, (int)L, (int)E,
                                (int)dW.size(0), dW.data_ptr<float>(), cur_stream(),
                                sorted.defined() ? sorted.data_ptr<int64_t>() : nullptr,
                                perm.defined() ? perm.data_ptr<int64_t>() : nullptr,
                                part.defined() ? part.data_ptr<float>() : nullptr);
  };
}

static void check_loss_inputs(const at::Tensor& xs, const at::Tensor& out, const at::Tensor& ids,
                              const at::Tensor& t, const at::Tensor& W) {
  check_diffusion_common(ids, t, W);
  CHECK_DEV(xs); CHECK_F32(xs); CHECK_CONTIG(xs); CHECK_ALIGNED(xs);
  CHECK_DEV(out); CHECK_CONTIG(out);
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 || out.scalar_type() == at::kFloat,
              "model output must be bf16 or fp32");
  TORCH_CHECK(xs.dim() == 3 && xs.size(0) == ids.size(0) && xs.size(1) == ids.size(1) &&
                  xs.size(2) == W.size(1) && out.sizes() == xs.sizes(),
              "x_start / output [B, L, E] matching ids and W");
}

static std::vector<at::Tensor> diff_loss_fwd(const at::Tensor& xs, const at::Tensor& out,
                                             const at::Tensor& ids, const at::Tensor& t,
                                             const at::Tensor& W, double sa_last) {
  check_loss_inputs(xs, out, ids, t, W);
  const int64_t B = xs.size(0), L = xs.size(1), E = xs.size(2);
  const c10::DeviceGuard guard(xs.device());
  at::Tensor mse = at::empty({B}, xs.options()), tT = at::empty({B}, xs.options());
  if (B > 0)
    dpa::launch_diff_loss_fwd(xs.data_ptr<float>(), out.data_ptr(), out.scalar_type() == at::kBFloat16,
                              ids.data_ptr<int64_t>(), t.data_ptr<int64_t>(), W.data_ptr<float>(), (int)B,
                              (int)L, (int)E, (int)W.size(0), (float)sa_last, mse.data_ptr<float>(),
                              tT.data_ptr<float>(), cur_stream());
  return {mse, tT};
}

static std::vector<at::Tensor> diff_loss_bwd(const at::Tensor& xs, const at::Tensor& out,
                                             const at::Tensor& ids, const at::Tensor& t,
                                             const at::Tensor& W, c10::optional<at::Tensor> dmse,
                                             c10::optional<at::Tensor> dtT, double sa_last, bool need_dout,
                                             bool need_dxs, c10::optional<at::Tensor> dW, bool fold_t0) {
  check_loss_inputs(xs, out, ids, t, W);
  const int64_t B = xs.size(0), L = xs.size(1), E = xs.size(2);
  const float* pm = opt_f32_ptr(dmse, B, "dmse [B]", /*contig=*/true);
  const float* pt = opt_f32_ptr(dtT, B, "dtT [B]", /*contig=*/true);
  float* pw = nullptr;
  if (has(dW)) {
    CHECK_F32((*dW)); CHECK_CONTIG((*dW)); TORCH_CHECK(dW->sizes() == W.sizes(), "dW like W");
    pw = dW->data_ptr<float>();
  }
  const c10::DeviceGuard guard(xs.device());
  at::Tensor d_out, d_xs;
  if (need_dout) d_out = at::empty_like(out);
  if (need_dxs) d_xs = at::empty_like(xs);
  if (B > 0 && (need_dout || need_dxs || pw))
    dpa::launch_diff_loss_bwd(xs.data_ptr<float>(), out.data_ptr(), out.scalar_type() == at::kBFloat16,
                              ids.data_ptr<int64_t>(), t.data_ptr<int64_t>(), W.data_ptr<float>(), pm, pt,
                              (int)B, (int)L, (int)E, (int)W.size(0), (float)sa_last,
                              need_dout ? d_out.data_ptr() : nullptr,
                              need_dxs ? d_xs.data_ptr<float>() : nullptr, pw, cur_stream(), fold_t0 && need_dxs);
  return {d_out, d_xs};
}

// One reverse-process update (csrc/reverse_step.hip).  `like` fixes the device; every given
// tensor must hold exactly N rows (of E columns) on it.  pred_prev / idx_prev are looked at only
// when a_prev != 0.
static std::vector<at::Tensor> reverse_step(const at::Tensor& like, int64_t N, int64_t E,
                                            c10::optional<at::Tensor> x, c10::optional<at::Tensor> pred,
                                            c10::optional<at::Tensor> idx, c10::optional<at::Tensor> W,
                                            c10::optional<at::Tensor> x_start, c10::optional<at::Tensor> mask,
                                            double scale, double a, double b, double s, int64_t seed,
                                            int64_t step, int64_t row_base, double tau, double erf_tau,
                                            bool want_bf16, c10::optional<at::Tensor> pred_prev,
                                            c10::optional<at::Tensor> idx_prev, double a_prev) {
  CHECK_DEV(like);
  TORCH_CHECK(N >= 0 && E > 0 && E % 4 == 0 && E <= 65536, "reverse_step: N >= 0, E % 4 == 0, E <= 65536");
  TORCH_CHECK(step >= 0 && step <= 0xffffffffLL && row_base >= 0, "reverse_step: step in [0, 2^32), row_base >= 0");
  const float af = (float)a, bf = (float)b, sf = (float)s, apf = (float)a_prev;
  auto rows_f32 = [&](const at::Tensor& t, const char* name) -> const float* {
    TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == at::kFloat && t.is_contiguous() &&
                    t.numel() == N * E && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                name, " must be a contiguous, 16-byte aligned fp32 [N, E] tensor on the op's device");
    return t.data_ptr<float>();
  };
  auto rows_i64 = [&](const at::Tensor& t, const char* name) -> const int64_t* {
    check_i64(t, name);
    TORCH_CHECK(t.device() == like.device() && t.numel() == N, name, " must hold N entries on the op's device");
    return t.data_ptr<int64_t>();
  };
  const float* xp = has(x) ? rows_f32(*x, "x") : nullptr;
  const float* xsp = has(x_start) ? rows_f32(*x_start, "x_start") : nullptr;
  const int64_t* mp = has(mask) ? rows_i64(*mask, "mask") : nullptr;
  auto rows_bf16 = [&](const at::Tensor& t, const char* name) -> const uint16_t* {
    TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == at::kBFloat16 && t.is_contiguous() &&
                    t.numel() == N * E && reinterpret_cast<uintptr_t>(t.data_ptr()) % 8 == 0,
                name, " must be a contiguous, 8-byte aligned bf16 [N, E] tensor on the op's device");
    return bf_ptr(t);
  };
  const uint16_t *pp = nullptr, *ppp = nullptr;
  const int64_t *ip = nullptr, *ipp = nullptr;
  const float* wp = nullptr;
  int64_t V = 0;
  if (has(pred)) {
    pp = rows_bf16(*pred, "pred");
  } else if (has(idx)) {
    TORCH_CHECK(has(W), "reverse_step: idx needs the embedding table W");
    ip = rows_i64(*idx, "idx");
  }
  if (apf != 0.f) {
    if (has(pred_prev)) {
      ppp = rows_bf16(*pred_prev, "pred_prev");
    } else if (has(idx_prev)) {
      TORCH_CHECK(has(W), "reverse_step: idx_prev needs the embedding table W");
      ipp = rows_i64(*idx_prev, "idx_prev");
    }
  }
  if (ip || ipp) {
    CHECK_DEV((*W)); CHECK_F32((*W)); CHECK_CONTIG((*W)); CHECK_ALIGNED((*W));
    TORCH_CHECK(W->dim() == 2 && W->size(1) == E && W->device() == like.device(), "W [V, E] fp32 on the op's device");
    TORCH_CHECK(W->size(0) <= 0x7fffffffLL, "W: too many rows");
    wp = W->data_ptr<float>();
    V = W->size(0);
  }
  TORCH_CHECK(bf == 0.f || xp, "reverse_step: b != 0 needs x");
  TORCH_CHECK(af == 0.f || pp || ip, "reverse_step: a != 0 needs pred or idx + W");
  TORCH_CHECK(apf == 0.f || ppp || ipp, "reverse_step: a_prev != 0 needs pred_prev or idx_prev + W");
  TORCH_CHECK(!mp || xsp, "reverse_step: mask needs x_start");
  const c10::DeviceGuard guard(like.device());
  auto f32 = at::TensorOptions().device(like.device()).dtype(at::kFloat);
  at::Tensor out = at::empty({N, E}, f32), out16;
  if (want_bf16) out16 = at::empty({N, E}, f32.dtype(at::kBFloat16));
  if (N > 0) {
    const bool ok = dpa::launch_reverse_step(
        xp, pp, ip, wp, xsp, mp, N, (int)E, (int)V, (float)scale, af, bf, sf, (uint64_t)seed, (uint32_t)step,
        (uint64_t)row_base, (float)tau, (float)erf_tau, out.data_ptr<float>(), want_bf16 ? bf_mut(out16) : nullptr,
        cur_stream(), ppp, ipp, apf);
    TORCH_CHECK(ok, "reverse_step: unsupported arguments");
  }
  return {out, out16};
}

// Bump the device-side Philox offset base of every kernel translation unit that draws noise
// or dropout (common.h g_rng_base): a replayed HIP graph's baked offsets + the base = fresh
// numbers per replay.  Stream-ordered on the current stream.
static void rng_base_add(int64_t d) {
  const auto s = cur_stream();
  dpa::rng_base_add_attention((uint32_t)d, s);
  dpa::rng_base_add_attention128((uint32_t)d, s);
  dpa::rng_base_add_diffusion((uint32_t)d, s);
  dpa::rng_base_add_norm((uint32_t)d, s);
  dpa::rng_base_add_gemm256((uint32_t)d, s);
}

static at::Tensor timestep_emb(const at::Tensor& ts, int64_t dim, double max_period) {
  CHECK_DEV(ts); CHECK_F32(ts); CHECK_CONTIG(ts);
  TORCH_CHECK(ts.dim() == 1 && dim > 0, "timesteps [B]");
  const c10::DeviceGuard guard(ts.device());
  at::Tensor out = at::empty({ts.size(0), dim}, ts.options().dtype(at::kBFloat16));
  if (ts.numel() > 0)
    dpa::launch_timestep_emb(ts.data_ptr<float>(), (int)ts.size(0), (int)dim, (float)max_period, bf_mut(out),
                             cur_stream());
  return out;
}

void dpa::register_diffusion(pybind11::module& m) {
  m.def("emb_grad", &dpa::emb_grad, "dW[ids] += dy (sorted segment sum, fp32)");
  m.def("id_sort", &id_sort, "counting sort of int64 ids into V + 1 buckets -> (sorted ids, permutation)");
  m.def("partition01", &partition01, "stable partition order of an int64 0/1 mask (nonzero first)");
  m.def("emb_qsample_fwd", &emb_qsample_fwd,
        "DiffuSeq embedding gather + x_start noise + masked q_sample -> (x_start, x_start bf16, x_t bf16)");
  m.def("emb_qsample_bwd", &emb_qsample_bwd, "scatter-add of the q_sample gradients into dW (fp32)");
  m.def("diff_loss_fwd", &diff_loss_fwd, "DiffuSeq per-sample (mse, tT) losses");
  m.def("diff_loss_bwd", &diff_loss_bwd, "backward of diff_loss_fwd -> (d_out, d_x_start)", py::arg("xs"),
        py::arg("out"), py::arg("ids"), py::arg("t"), py::arg("W"), py::arg("dmse"), py::arg("dtT"),
        py::arg("sa_last"), py::arg("need_dout"), py::arg("need_dxs"), py::arg("dW"), py::arg("fold_t0") = false);
  m.def("reverse_step", &reverse_step,
        "DiffuSeq reverse update a x0 + a_prev x0_prev + b x + s z (in-kernel Philox noise; source rows kept) -> (out fp32, out bf16 | None)",
        py::arg("like"), py::arg("N"), py::arg("E"), py::arg("x") = py::none(), py::arg("pred") = py::none(),
        py::arg("idx") = py::none(), py::arg("W") = py::none(), py::arg("x_start") = py::none(),
        py::arg("mask") = py::none(), py::arg("scale") = 1.0, py::arg("a") = 0.0, py::arg("b") = 0.0,
        py::arg("s") = 0.0, py::arg("seed") = 0, py::arg("step") = 0, py::arg("row_base") = 0,
        py::arg("tau") = 0.0, py::arg("erf_tau") = 0.0, py::arg("want_bf16") = false,
        py::arg("pred_prev") = py::none(), py::arg("idx_prev") = py::none(), py::arg("a_prev") = 0.0);
  m.def("rng_base_add", &rng_base_add, "advance the device-side Philox offset base (graph replays)");
  m.def("timestep_emb", &timestep_emb, "sinusoidal timestep embedding [cos | sin] -> bf16");
}
