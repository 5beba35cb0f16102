// Bindings of the vocabulary heads: fused linear + cross-entropy (xent.hip), fused linear +
// arg-max (linear_argmax.hip) and the row softmax cross-entropy (xent_rows.hip).
#include "bind_util.h"

// ---- fused linear + cross-entropy ---------------------------------------------
static void check_lxent(const at::Tensor& x, const at::Tensor& W, const c10::optional<at::Tensor>& b,
                        const at::Tensor& tgt) {
  CHECK_DEV(x); CHECK_DEV(W); CHECK_DEV(tgt);
  CHECK_BF16(x); CHECK_BF16(W); CHECK_CONTIG(x); CHECK_CONTIG(W); CHECK_CONTIG(tgt);
  TORCH_CHECK(x.dim() == 2 && W.dim() == 2 && x.size(1) == W.size(1), "x [N,E], W [V,E]");
  TORCH_CHECK(x.size(1) == 128 || x.size(1) == 256, "lxent: E must be 128 or 256");
  TORCH_CHECK(tgt.scalar_type() == at::kLong && tgt.numel() == x.size(0), "target [N] int64");
  opt_bf_ptr(b, W.size(0), "bias [V]");
}

static std::vector<at::Tensor> lxent_fwd(const at::Tensor& x, const at::Tensor& W,
                                         c10::optional<at::Tensor> b, const at::Tensor& tgt) {
  check_lxent(x, W, b, tgt);
  const c10::DeviceGuard guard(x.device());
  const int N = (int)x.size(0), V = (int)W.size(0), E = (int)x.size(1);
  auto f32 = x.options().dtype(at::kFloat);
  at::Tensor loss = at::empty({N}, f32), lse = at::empty({N}, f32);
  at::Tensor ws = at::empty({dpa::lxent_workspace_floats(N, V)}, f32);
  if (N > 0)
    dpa::launch_lxent_fwd(bf_ptr(x), bf_ptr(W), opt_bf_ptr(b), tgt.data_ptr<int64_t>(), N, V, E,
                          loss.data_ptr<float>(), lse.data_ptr<float>(), ws.data_ptr<float>(),
                          cur_stream());
  return {loss, lse};
}

static std::vector<at::Tensor> lxent_fwd_dx(const at::Tensor& x, const at::Tensor& W,
                                            c10::optional<at::Tensor> b, const at::Tensor& tgt) {
  check_lxent(x, W, b, tgt);
  const c10::DeviceGuard guard(x.device());
  const int N = (int)x.size(0), V = (int)W.size(0), E = (int)x.size(1);
  auto f32 = x.options().dtype(at::kFloat);
  at::Tensor loss = at::empty({N}, f32), lse = at::empty({N}, f32), dxu = at::empty({N, E}, f32);
  const int64_t wsn = N > 0 ? dpa::lxent_fwd_dx_workspace_floats(N, V, E) : 0;
  at::Tensor ws = at::empty({wsn}, f32);
  if (N > 0)
    dpa::launch_lxent_fwd_dx(bf_ptr(x), bf_ptr(W), opt_bf_ptr(b), tgt.data_ptr<int64_t>(), N, V, E,
                             loss.data_ptr<float>(), lse.data_ptr<float>(), dxu.data_ptr<float>(), cur_stream(),
                             wsn ? ws.data_ptr<float>() : nullptr);
  return {loss, lse, dxu};
}

// onehot_scatter: the dW kernel leaves out the target one-hot (softmax only) and it is added
// here as dW[t] -= g x_t, db[t] -= g over the valid targets, by the sorted segment-sum scatter
// of the embedding backward - a compare, subtract and select less per logit in the kernel
// dw_acc / db_acc: fp32 buffers of W's / b's shape (the parameters' flat .grad views) the kernel
// accumulates into directly (its token splits' partials go through a scratch summed in split
// order); the matching results are then undefined - no zero-filled [V, E] result and no
// autograd-side add per call
static std::vector<at::Tensor> lxent_bwd(const at::Tensor& dloss, const at::Tensor& x,
                                         const at::Tensor& W, c10::optional<at::Tensor> b,
                                         const at::Tensor& tgt, const at::Tensor& lse, bool need_dx,
                                         bool need_dw, bool need_db, bool onehot_scatter,
                                         c10::optional<at::Tensor> dw_acc, c10::optional<at::Tensor> db_acc) {
  check_lxent(x, W, b, tgt);
  CHECK_F32(dloss); CHECK_F32(lse); CHECK_CONTIG(dloss); CHECK_CONTIG(lse);
  const c10::DeviceGuard guard(x.device());
  const int N = (int)x.size(0), V = (int)W.size(0), E = (int)x.size(1);
  auto f32 = x.options().dtype(at::kFloat);
  at::Tensor dx, dW, db;
  if (need_dx) {
    dx = at::empty_like(x);
    at::Tensor acc;
    if (dpa::lxent_dx_needs_acc(N)) acc = at::zeros({(int64_t)N * E}, f32);
    if (N > 0)
      dpa::launch_lxent_dx(bf_ptr(x), bf_ptr(W), opt_bf_ptr(b), tgt.data_ptr<int64_t>(),
                           lse.data_ptr<float>(), dloss.data_ptr<float>(), N, V, E, bf_mut(dx),
                           acc.defined() ? acc.data_ptr<float>() : nullptr, cur_stream());
  }
  const bool ext_w = need_dw && usable_acc(dw_acc, (int64_t)V * E, x.device());
  const bool ext_b = need_db && usable_acc(db_acc, V, x.device());
  if (need_dw || need_db) {
    dW = ext_w ? *dw_acc : at::zeros({V, E}, f32);
    if (need_db) db = ext_b ? *db_acc : at::zeros({V}, f32);
    const bool scatter = onehot_scatter && need_dw && (E == 128 || E == 256);
    if (N > 0) {
      const int64_t wsn = dpa::lxent_dw_ws_floats(N, V, E);
      at::Tensor ws = wsn > 0 ? at::empty({wsn}, f32) : at::Tensor();
      dpa::launch_lxent_dw(bf_ptr(x), bf_ptr(W), opt_bf_ptr(b), tgt.data_ptr<int64_t>(),
                           lse.data_ptr<float>(), dloss.data_ptr<float>(), N, V, E,
                           dW.data_ptr<float>(), need_db ? db.data_ptr<float>() : nullptr,
                           cur_stream(), !scatter, wsn > 0 ? ws.data_ptr<float>() : nullptr);
    }
    if (scatter && N > 0) {
      const at::Tensor valid = tgt.ge(0).logical_and(tgt.lt(V));
      const at::Tensor ng = at::where(valid, dloss.neg(), at::zeros({}, dloss.options()));
      dpa::emb_grad(tgt, x.to(at::kFloat).mul_(ng.unsqueeze(1)), dW);  // ids outside [0, V) are skipped
      if (need_db) db.index_add_(0, tgt.clamp(0, V - 1), ng);
    }
    if (!need_dw || ext_w) dW = at::Tensor();
    if (ext_b) db = at::Tensor();
  }
  return {dx, dW, db};
}

// ---- fused linear + arg-max (decoding) -------------------------------------------
static void check_argmax_w(const at::Tensor& W) {
  CHECK_DEV(W); CHECK_BF16(W); CHECK_CONTIG(W);
  TORCH_CHECK(W.dim() == 2 && W.size(0) > 0, "W [V,E] with V > 0");
  TORCH_CHECK(W.size(1) == 128 || W.size(1) == 256, "linear_argmax: E must be 128 or 256");
}

static std::vector<at::Tensor> linear_argmax(const at::Tensor& x, const at::Tensor& W,
                                             c10::optional<at::Tensor> c) {
  check_argmax_w(W);
  CHECK_DEV(x); CHECK_BF16(x); CHECK_CONTIG(x);
  TORCH_CHECK(x.dim() == 2 && x.size(1) == W.size(1), "x [N,E], W [V,E]");
  TORCH_CHECK(x.device() == W.device(), "x and W must be on one device");
  const float* cp = nullptr;
  if (has(c)) {
    CHECK_DEV((*c)); CHECK_F32((*c)); CHECK_CONTIG((*c));
    TORCH_CHECK(c->numel() == W.size(0) && c->device() == W.device(), "c [V] fp32 on W's device");
    cp = c->data_ptr<float>();
  }
  const c10::DeviceGuard guard(x.device());
  const int N = (int)x.size(0), V = (int)W.size(0), E = (int)x.size(1);
  at::Tensor idx = at::empty({N}, x.options().dtype(at::kLong));
  at::Tensor best = at::empty({N}, x.options().dtype(at::kFloat));
  if (N == 0) return {idx, best};
  const int64_t wsn = dpa::linear_argmax_workspace_floats(N, V);
  at::Tensor ws = at::empty({wsn}, x.options().dtype(at::kFloat));
  dpa::launch_linear_argmax(bf_ptr(x), bf_ptr(W), cp, N, V, E, idx.data_ptr<int64_t>(),
                            best.data_ptr<float>(), wsn ? ws.data_ptr<float>() : nullptr, cur_stream());
  return {idx, best};
}

static at::Tensor row_half_sqnorm(const at::Tensor& W) {
  check_argmax_w(W);
  const c10::DeviceGuard guard(W.device());
  at::Tensor c = at::empty({W.size(0)}, W.options().dtype(at::kFloat));
  dpa::launch_row_half_sqnorm(bf_ptr(W), (int)W.size(0), (int)W.size(1), c.data_ptr<float>(), cur_stream());
  return c;
}

// ---- row softmax cross-entropy (chunked wide-E linear-CE) ------------------------------
static void check_xent_rows(const at::Tensor& lg, int64_t V, const at::Tensor& tgt) {
  CHECK_DEV(lg); CHECK_BF16(lg); CHECK_CONTIG(lg); CHECK_ALIGNED(lg);
  check_i64(tgt, "target");
  TORCH_CHECK(lg.dim() == 2 && lg.size(1) % 8 == 0 && V > 0 && V <= lg.size(1),
              "logits [R, ld] with ld % 8 == 0 and V <= ld");
  TORCH_CHECK(tgt.numel() == lg.size(0), "target [R]");
}

// (loss, lse) outputs: the caller's [R] fp32 slices when given (a chunk of the whole
// batch's vectors: no per-chunk copy), else fresh tensors
static std::pair<at::Tensor, at::Tensor> xent_rows_outs(const at::Tensor& lg, const c10::optional<at::Tensor>& loss_out,
                                                        const c10::optional<at::Tensor>& lse_out) {
  auto f32 = lg.options().dtype(at::kFloat);
  at::Tensor loss = loss_out.has_value() ? *loss_out : at::empty({lg.size(0)}, f32);
  at::Tensor lse = lse_out.has_value() ? *lse_out : at::empty({lg.size(0)}, f32);
  for (const at::Tensor* t : {&loss, &lse})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == lg.size(0),
                "loss / lse outputs must be contiguous fp32 [R] HIP tensors");
  return {loss, lse};
}

static std::vector<at::Tensor> xent_rows_fwd(const at::Tensor& lg, int64_t V, const at::Tensor& tgt,
                                             const c10::optional<at::Tensor>& loss_out,
                                             const c10::optional<at::Tensor>& lse_out) {
  check_xent_rows(lg, V, tgt);
  const c10::DeviceGuard guard(lg.device());
  auto [loss, lse] = xent_rows_outs(lg, loss_out, lse_out);
  dpa::launch_xent_rows_fwd(bf_ptr(lg), lg.size(1), (int)V, tgt.data_ptr<int64_t>(), lg.size(0),
                            loss.data_ptr<float>(), lse.data_ptr<float>(), cur_stream());
  return {loss, lse};
}

// in place: logits -> softmax - onehot (unscaled); returns (loss, lse) (empty list if refused)
static std::vector<at::Tensor> xent_rows_fwd_grad_(at::Tensor& lg, int64_t V, const at::Tensor& tgt,
                                                   const c10::optional<at::Tensor>& loss_out,
                                                   const c10::optional<at::Tensor>& lse_out) {
  check_xent_rows(lg, V, tgt);
  const c10::DeviceGuard guard(lg.device());
  auto [loss, lse] = xent_rows_outs(lg, loss_out, lse_out);
  if (!dpa::launch_xent_rows_fwd_grad(bf_mut(lg), lg.size(1), (int)V, tgt.data_ptr<int64_t>(), lg.size(0),
                                      loss.data_ptr<float>(), lse.data_ptr<float>(), cur_stream()))
    return {};
  return {loss, lse};
}

static void xent_rows_bwd_(at::Tensor& lg, int64_t V, const at::Tensor& tgt, const at::Tensor& lse,
                           const at::Tensor& dloss) {
  check_xent_rows(lg, V, tgt);
  CHECK_F32(lse); CHECK_F32(dloss); CHECK_CONTIG(lse); CHECK_CONTIG(dloss);
  const int64_t R = lg.size(0);
  TORCH_CHECK(lse.numel() == R && dloss.numel() == R, "per-row tensors [R]");
  const c10::DeviceGuard guard(lg.device());
  dpa::launch_xent_rows_bwd(bf_mut(lg), lg.size(1), (int)V, tgt.data_ptr<int64_t>(), lse.data_ptr<float>(),
                            dloss.data_ptr<float>(), R, cur_stream());
}

void dpa::register_heads(pybind11::module& m) {
  m.def("lxent_fwd", &lxent_fwd, "fused linear + cross-entropy forward -> (loss, lse)");
  m.def("lxent_fwd_dx", &lxent_fwd_dx,
        "fused linear-CE forward + unscaled input gradient -> (loss, lse, dxu fp32 [N, E])");
  m.def("lxent_bwd", &lxent_bwd, "fused linear + cross-entropy backward -> (dx, dW fp32, db fp32)",
        py::arg("dloss"), py::arg("x"), py::arg("W"), py::arg("b"), py::arg("tgt"), py::arg("lse"),
        py::arg("need_dx"), py::arg("need_dw"), py::arg("need_db"), py::arg("onehot_scatter") = false,
        py::arg("dw_acc") = py::none(), py::arg("db_acc") = py::none());
  m.def("linear_argmax", &linear_argmax,
        "row-wise arg-max of x W^T + c without the scores -> (idx int64, best fp32); ties: lowest index",
        py::arg("x"), py::arg("W"), py::arg("c") = py::none());
  m.def("row_half_sqnorm", &row_half_sqnorm, "c[v] = -1/2 ||W[v]||^2 in fp32 from a bf16 W");
  m.def("xent_rows_fwd", &xent_rows_fwd, "row softmax-CE over bf16 logits [R, ld] -> (loss, lse)",
        py::arg("lg"), py::arg("V"), py::arg("tgt"), py::arg("loss_out") = py::none(),
        py::arg("lse_out") = py::none());
  m.def("xent_rows_bwd_", &xent_rows_bwd_, "in place: logits -> dloss * (softmax - onehot)");
  m.def("xent_rows_fwd_grad_", &xent_rows_fwd_grad_,
        "in place: logits -> softmax - onehot (unscaled), returns (loss, lse) or [] if the row is too long",
        py::arg("lg"), py::arg("V"), py::arg("tgt"), py::arg("loss_out") = py::none(),
        py::arg("lse_out") = py::none());
}
