// Bindings of the memory-bound kernels around the GEMMs: fused dropout + residual + LayerNorm and
// its column sums (norm.hip), the bias + activation epilogues (elementwise.hip) and the
// flat-buffer optimizer (optim.hip).
#include "bind_util.h"

// ---- optimizer --------------------------------------------------------------
static void sqnorm(const at::Tensor& g, at::Tensor& partial, at::Tensor& out, double scale,
                   double max_norm) {
  CHECK_DEV(g); CHECK_CONTIG(g); CHECK_ALIGNED(g);
  CHECK_DEV(partial); CHECK_F32(partial); CHECK_CONTIG(partial);
  CHECK_DEV(out); CHECK_F32(out); CHECK_CONTIG(out);
  TORCH_CHECK(g.numel() % 4 == 0, "flat grad buffer must be padded to a multiple of 4");
  // the grid is capped at partial.numel() blocks: an empty one would be a 0-block launch
  TORCH_CHECK(partial.numel() >= 1, "partial needs at least 1 float");
  TORCH_CHECK(out.numel() >= 3, "out needs 3 floats");
  const bool bf = g.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf || g.scalar_type() == at::kFloat, "grad must be fp32 or bf16");
  const c10::DeviceGuard guard(g.device());
  dpa::launch_sqnorm(g.data_ptr(), bf, g.numel(), partial.data_ptr<float>(), (int)partial.numel(),
                     (float)scale, (float)max_norm, out.data_ptr<float>(), cur_stream());
}

static void adamw_ema(at::Tensor& p, const at::Tensor& g, at::Tensor& m, at::Tensor& v,
                      c10::optional<at::Tensor> p16, std::vector<at::Tensor> emas,
                      std::vector<double> rates, double lr, double beta1, double beta2, double eps,
                      double wd, int64_t step, double grad_scale, c10::optional<at::Tensor> clip,
                      c10::optional<at::Tensor> skip) {
  for (auto* t : {&p, &m, &v}) { CHECK_DEV((*t)); CHECK_CONTIG((*t)); CHECK_F32((*t)); CHECK_ALIGNED((*t)); }
  CHECK_DEV(g); CHECK_CONTIG(g); CHECK_ALIGNED(g);
  TORCH_CHECK(g.device() == p.device(), "g must be on the device of p");
  const int64_t n = p.numel();
  TORCH_CHECK(n % 4 == 0, "flat buffers must be padded to a multiple of 4");
  TORCH_CHECK(g.numel() == n && m.numel() == n && v.numel() == n, "size mismatch");
  TORCH_CHECK(emas.size() == rates.size(), "ema/rates mismatch");
  const bool bf = g.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf || g.scalar_type() == at::kFloat, "grad must be fp32 or bf16");
  std::vector<float*> bufs;
  std::vector<float> r;
  for (size_t i = 0; i < emas.size(); ++i) {
    CHECK_DEV(emas[i]); CHECK_F32(emas[i]); CHECK_CONTIG(emas[i]); CHECK_ALIGNED(emas[i]);
    TORCH_CHECK(emas[i].numel() == n, "ema size mismatch");
    bufs.push_back(emas[i].data_ptr<float>());
    r.push_back((float)rates[i]);
  }
  uint16_t* p16p = nullptr;
  if (has(p16)) {
    CHECK_DEV((*p16)); CHECK_BF16((*p16)); CHECK_CONTIG((*p16));
    TORCH_CHECK(p16->numel() == n, "bf16 shadow size mismatch");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(p16->data_ptr()) % 8 == 0, "bf16 shadow must be 8B aligned");
    p16p = bf_mut(*p16);
  }
  const float* clipp = nullptr;
  if (has(clip)) {
    // [norm, coef, norm * coef] of sqnorm: the kernel reads clip[1]
    CHECK_DEV((*clip)); CHECK_F32((*clip)); CHECK_CONTIG((*clip));
    TORCH_CHECK(clip->numel() >= 2, "clip needs at least 2 floats");
    clipp = clip->data_ptr<float>();
  }
  const int* skipp = nullptr;
  if (has(skip)) {
    CHECK_DEV((*skip));
    TORCH_CHECK(skip->scalar_type() == at::kInt && skip->numel() >= 1, "skip flag: int32 device tensor");
    skipp = skip->data_ptr<int>();
  }
  const c10::DeviceGuard guard(p.device());
  dpa::launch_adamw_ema(p.data_ptr<float>(), g.data_ptr(), bf, m.data_ptr<float>(),
                        v.data_ptr<float>(), p16p, bufs.data(), r.data(), (int)bufs.size(), n,
                        (float)lr, beta1, beta2, (float)eps, (float)wd, step,
                        (float)grad_scale, clipp, cur_stream(), skipp);
}

static void ema_update(at::Tensor& e, const at::Tensor& p, double rate) {
  CHECK_DEV(e); CHECK_DEV(p); CHECK_CONTIG(e); CHECK_CONTIG(p);
  CHECK_F32(e); CHECK_F32(p); CHECK_ALIGNED(e); CHECK_ALIGNED(p);
  TORCH_CHECK(e.numel() == p.numel() && e.numel() % 4 == 0, "ema size");
  const c10::DeviceGuard guard(p.device());
  dpa::launch_ema(e.data_ptr<float>(), p.data_ptr<float>(), e.numel(), (float)rate, cur_stream());
}

static void cast_bf16(const at::Tensor& src, at::Tensor& dst) {
  CHECK_DEV(src); CHECK_DEV(dst); CHECK_CONTIG(src); CHECK_CONTIG(dst);
  CHECK_F32(src); CHECK_BF16(dst); CHECK_ALIGNED(src);
  TORCH_CHECK(src.numel() == dst.numel() && src.numel() % 4 == 0, "cast size");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(dst.data_ptr()) % 8 == 0, "dst must be 8B aligned");
  const c10::DeviceGuard guard(src.device());
  dpa::launch_cast_bf16(src.data_ptr<float>(), bf_mut(dst), src.numel(), cur_stream());
}

// ---- fused dropout + residual + LayerNorm ------------------------------------------
static std::vector<at::Tensor> add_ln_fwd(const at::Tensor& y, c10::optional<at::Tensor> res,
                                          const at::Tensor& g, const at::Tensor& b, double p,
                                          double eps, int64_t seed, int64_t offset,
                                          c10::optional<at::Tensor> pos, c10::optional<at::Tensor> temb,
                                          int64_t L, bool post, bool save_h, bool h_guard) {
  CHECK_DEV(y); CHECK_BF16(y); CHECK_CONTIG(y); CHECK_BF16(g); CHECK_BF16(b);
  TORCH_CHECK(y.dim() == 2, "y must be [R, D]");
  const int64_t R = y.size(0);
  const int D = (int)y.size(1);
  TORCH_CHECK(g.numel() == D && b.numel() == D, "gamma/beta size");
  const uint16_t* rp = nullptr;
  if (has(res)) {
    CHECK_BF16((*res)); CHECK_CONTIG((*res));
    TORCH_CHECK(res->sizes() == y.sizes(), "residual shape");
    rp = bf_ptr(*res);
  }
  // row-broadcast terms: pos [L, D] (row % L), temb [R / L, D] (row / L)
  const uint16_t* pp = nullptr;
  const uint16_t* tp = nullptr;
  if (has(pos)) {
    CHECK_BF16((*pos)); CHECK_CONTIG((*pos));
    TORCH_CHECK(L > 0 && R % L == 0 && pos->numel() == L * D, "pos must be [L, D] with R % L == 0");
    pp = bf_ptr(*pos);
  }
  if (has(temb)) {
    CHECK_BF16((*temb)); CHECK_CONTIG((*temb));
    TORCH_CHECK(L > 0 && R % L == 0 && temb->numel() == (R / L) * D, "temb must be [R / L, D]");
    tp = bf_ptr(*temb);
  }
  const c10::DeviceGuard guard(y.device());
  // save_h = false: no bf16 copy of h.  h_guard: the copy is written only for a gamma with
  // some |gamma| < 0.125 (norm.hip LN_XO_GMIN) - add_ln_bwd(beta=, hcopy=) reads it then and
  // reconstructs xhat from the output otherwise
  at::Tensor out = at::empty_like(y), hs = save_h ? at::empty_like(y) : at::Tensor();
  auto f32 = y.options().dtype(at::kFloat);
  at::Tensor mean = at::empty({R}, f32), rstd = at::empty({R}, f32);
  bool ok = dpa::launch_add_ln_fwd(bf_ptr(y), rp, bf_ptr(g), bf_ptr(b), bf_mut(out),
                                   save_h ? bf_mut(hs) : nullptr, mean.data_ptr<float>(),
                                   rstd.data_ptr<float>(), R, D, (float)p, (float)eps,
                                   (uint32_t)seed, (uint32_t)offset, cur_stream(), pp, tp, (int)L, post,
                                   save_h && h_guard);
  TORCH_CHECK(ok, "add_ln_fwd: unsupported hidden size ", D);
  return {out, hs, mean, rstd};
}

static std::vector<at::Tensor> add_ln_bwd(const at::Tensor& dout, const at::Tensor& hs,
                                          const at::Tensor& mean, const at::Tensor& rstd,
                                          const at::Tensor& g, double p, int64_t seed,
                                          int64_t offset, bool need_dres, bool need_dy,
                                          bool want_dyb, c10::optional<at::Tensor> dh_in, bool post,
                                          c10::optional<at::Tensor> dg_acc, c10::optional<at::Tensor> db_acc,
                                          c10::optional<at::Tensor> dyb_acc, c10::optional<at::Tensor> part_buf,
                                          bool part_acc, c10::optional<at::Tensor> beta,
                                          c10::optional<at::Tensor> hcopy, bool pair_hash) {
  CHECK_DEV(dout); CHECK_BF16(dout); CHECK_CONTIG(dout); CHECK_BF16(hs); CHECK_CONTIG(hs);
  TORCH_CHECK(hs.sizes() == dout.sizes(), "add_ln_bwd: hsave/out shape");
  // beta given: `hs` is the LN output (forward with save_h=false), xhat = (out - beta) / gamma
  const uint16_t* btp = nullptr;
  if (has(beta)) {
    CHECK_BF16((*beta)); CHECK_CONTIG((*beta));
    TORCH_CHECK(beta->numel() == dout.size(1) && !post, "add_ln_bwd: beta [D], pre-dropout placement only");
    TORCH_CHECK(has(hcopy) && hcopy->sizes() == dout.sizes(),
                "add_ln_bwd: beta needs hcopy (the forward's guarded h copy)");
    CHECK_BF16((*hcopy)); CHECK_CONTIG((*hcopy));
    btp = bf_ptr(*beta);
  }
  const uint16_t* hcp = btp ? bf_ptr(*hcopy) : nullptr;
  const uint16_t* dhp = nullptr;
  if (has(dh_in)) {
    CHECK_BF16((*dh_in)); CHECK_CONTIG((*dh_in));
    TORCH_CHECK(dh_in->sizes() == dout.sizes(), "dh_in shape");
    dhp = bf_ptr(*dh_in);
  }
  const int64_t R = dout.size(0);
  const int D = (int)dout.size(1);
  const c10::DeviceGuard guard(dout.device());
  at::Tensor dres, dy;
  if (need_dres) dres = at::empty_like(dout);
  if (need_dy) dy = at::empty_like(dout);
  auto f32 = dout.options().dtype(at::kFloat);
  // dgamma, dbeta and colsum(dy) as consecutive rows of one scratch buffer (one memset),
  // or accumulated straight onto given fp32 .grad buffers (returned undefined then: no
  // autograd-side add and no memset)
  at::Tensor acc3 = at::empty({3, D}, f32);
  at::Tensor dg = acc3[0], db = acc3[1], dyb;
  if (need_dy && want_dyb) dyb = acc3[2];
  int zero_mask = 7;
  const bool ext_g = usable_acc(dg_acc, D, dout.device()), ext_b = usable_acc(db_acc, D, dout.device()),
             ext_y = dyb.defined() && usable_acc(dyb_acc, D, dout.device());
  if (ext_g) { dg = *dg_acc; zero_mask &= ~1; }
  if (ext_b) { db = *db_acc; zero_mask &= ~2; }
  if (ext_y) { dyb = *dyb_acc; zero_mask &= ~4; }
  const int64_t wsn = dpa::ln_bwd_ws_floats(R, D);
  at::Tensor ws;
  int part_mode = 0;
  if (has(part_buf)) {
    // deferred column sums (caller-owned partials, reduced later by ln_colreduce): only
    // when every accumulator is a caller buffer - nothing is returned for them
    TORCH_CHECK(wsn > 0 && usable_acc(part_buf, wsn, dout.device()),
                "add_ln_bwd: part_buf must be fp32 [ln_bwd_partials(R, D)] on the device");
    TORCH_CHECK(ext_g && ext_b && (!dyb.defined() || ext_y), "add_ln_bwd: part_buf needs dg/db/dyb_acc");
    ws = *part_buf;
    part_mode = part_acc ? 2 : 1;
  } else if (wsn > 0) {
    ws = at::empty({wsn}, f32);
  }
  bool ok = dpa::launch_add_ln_bwd(
      bf_ptr(dout), bf_ptr(hs), mean.data_ptr<float>(), rstd.data_ptr<float>(), bf_ptr(g),
      need_dres ? bf_mut(dres) : nullptr, need_dy ? bf_mut(dy) : nullptr,
      dyb.defined() ? dyb.data_ptr<float>() : nullptr,
      dg.data_ptr<float>(), db.data_ptr<float>(), R, D, (float)p, (uint32_t)seed, (uint32_t)offset,
      cur_stream(), dhp, post, zero_mask, wsn > 0 ? ws.data_ptr<float>() : nullptr, part_mode, btp, hcp,
      pair_hash);
  TORCH_CHECK(ok, "add_ln_bwd: unsupported hidden size ", D);
  return {dres, dy, ext_g ? at::Tensor() : dg, ext_b ? at::Tensor() : db, ext_y ? at::Tensor() : dyb};
}

// floats of the caller-owned partial buffer add_ln_bwd(part_buf=...) takes for R x D (0: the
// shape has no two-stage column sums, no deferral)
static int64_t ln_bwd_partials(int64_t R, int64_t D) { return dpa::ln_bwd_ws_floats(R, (int)D); }

// (dpos [L][H] fp32 or empty, dtemb [B][H] fp32 or empty) of d [B * L][H] bf16 in one read;
// empty list if the shape is not supported
static std::vector<at::Tensor> seq_pos_sums(const at::Tensor& d, int64_t L, bool need_pos, bool need_temb) {
  CHECK_DEV(d); CHECK_BF16(d); CHECK_CONTIG(d);
  TORCH_CHECK(d.dim() == 2 && L > 0 && d.size(0) % L == 0, "d [B * L, H]");
  const int64_t B = d.size(0) / L, H = d.size(1);
  const c10::DeviceGuard guard(d.device());
  auto f32 = d.options().dtype(at::kFloat);
  at::Tensor dpos = need_pos ? at::zeros({L, H}, f32) : at::Tensor();
  at::Tensor dtemb = need_temb ? at::empty({B, H}, f32) : at::Tensor();
  at::Tensor part = need_pos ? at::empty({(int64_t)dpa::seq_pos_groups((int)B) * L * H}, f32) : at::Tensor();
  if (!dpa::launch_seq_pos_sums(bf_ptr(d), (int)B, (int)L, (int)H,
                                need_pos ? dpos.data_ptr<float>() : nullptr,
                                need_temb ? dtemb.data_ptr<float>() : nullptr,
                                need_pos ? part.data_ptr<float>() : nullptr, cur_stream()))
    return {};
  return {dpos, dtemb};
}

// dg += colsum, db += colsum (, dyb += colsum) of partials accumulated by add_ln_bwd(part_buf=...)
static void ln_colreduce(const at::Tensor& part, int64_t R, int64_t D, at::Tensor& dg, at::Tensor& db,
                         c10::optional<at::Tensor> dyb) {
  CHECK_DEV(part); CHECK_F32(part); CHECK_CONTIG(part); CHECK_F32(dg); CHECK_F32(db);
  TORCH_CHECK(part.numel() == dpa::ln_bwd_ws_floats(R, (int)D) && dg.numel() == D && db.numel() == D,
              "ln_colreduce shapes");
  float* yp = opt_f32_ptr(dyb, D, "ln_colreduce dyb", /*contig=*/false);
  const c10::DeviceGuard guard(part.device());
  TORCH_CHECK(dpa::launch_ln_colreduce(part.data_ptr<float>(), R, (int)D, dg.data_ptr<float>(),
                                       db.data_ptr<float>(), yp, cur_stream()),
              "ln_colreduce: no two-stage shape");
}

// dst += column sums of fp32 partials [rows, cols] (the kept gemm_nn_dact partials)
static void colsum_acc(const at::Tensor& part, at::Tensor& dst) {
  CHECK_DEV(part); CHECK_F32(part); CHECK_CONTIG(part); CHECK_F32(dst); CHECK_CONTIG(dst);
  TORCH_CHECK(part.dim() == 2 && dst.numel() == part.size(1), "colsum_acc shapes");
  const c10::DeviceGuard guard(part.device());
  if (!dpa::launch_colsum_acc(part.data_ptr<float>(), (int)part.size(0), (int)part.size(1), dst.data_ptr<float>(),
                              cur_stream()))
    dst.add_(part.sum(0));
}

// ---- bias + activation epilogues ------------------------------------------------------
static std::vector<at::Tensor> bias_act_fwd(at::Tensor& z, c10::optional<at::Tensor> b, int64_t act) {
  CHECK_DEV(z); CHECK_BF16(z); CHECK_CONTIG(z);
  TORCH_CHECK(z.dim() == 2 && z.size(1) % 8 == 0, "z must be [R, N] with N % 8 == 0");
  const int64_t R = z.size(0);
  const int N = (int)z.size(1);
  const uint16_t* bp = opt_bf_ptr(b);
  if (bp) TORCH_CHECK(b->numel() == N, "bias size");
  const c10::DeviceGuard guard(z.device());
  at::Tensor y = act == 0 ? z : at::empty_like(z);
  if (bp || act != 0)
    dpa::launch_bias_act_fwd(bf_mut(z), bp, act == 0 ? nullptr : bf_mut(y), R, N, (int)act, cur_stream());
  return {z, y};
}

static std::vector<at::Tensor> bias_act_bwd(const at::Tensor& dy, const at::Tensor& zy, int64_t act,
                                            bool want_db) {
  CHECK_DEV(dy); CHECK_BF16(dy); CHECK_CONTIG(dy);
  const int64_t R = dy.size(0);
  const int N = (int)dy.size(1);
  TORCH_CHECK(N % 8 == 0, "N % 8");
  const c10::DeviceGuard guard(dy.device());
  at::Tensor dz = act == 0 ? dy : at::empty_like(dy);
  at::Tensor db;
  if (want_db) db = at::zeros({N}, dy.options().dtype(at::kFloat));
  if (act != 0 || want_db) {
    CHECK_CONTIG(zy);
    at::Tensor ws = want_db ? at::empty({dpa::bias_act_bwd_ws_floats(R, N)}, dy.options().dtype(at::kFloat))
                            : at::Tensor();
    dpa::launch_bias_act_bwd(bf_ptr(dy), bf_ptr(zy), act == 0 ? nullptr : bf_mut(dz),
                             want_db ? db.data_ptr<float>() : nullptr, R, N, (int)act, cur_stream(),
                             want_db ? ws.data_ptr<float>() : nullptr);
  }
  return {dz, db};
}

void dpa::register_elementwise(pybind11::module& m) {
  m.def("sqnorm", &sqnorm, "flat grad L2 norm + clip coefficient (device)");
  m.def("adamw_ema", &adamw_ema, "fused AdamW + EMA + bf16 shadow refresh");
  m.def("ema_update", &ema_update, "flat EMA update");
  m.def("cast_bf16", &cast_bf16, "flat fp32->bf16");
  m.def("add_ln_fwd", &add_ln_fwd,
        "LN(dropout(y [+pos] [+temb]) + res) (post: dropout(LN(...))) -> (out, hsave, mean, rstd)",
        py::arg("y"), py::arg("res"), py::arg("gamma"), py::arg("beta"), py::arg("p"), py::arg("eps"),
        py::arg("seed"), py::arg("offset"), py::arg("pos") = py::none(), py::arg("temb") = py::none(),
        py::arg("L") = 1, py::arg("post") = false, py::arg("save_h") = true, py::arg("h_guard") = false);
  m.def("add_ln_bwd", &add_ln_bwd, "backward of add_ln_fwd -> (dres, dy, dgamma, dbeta, colsum(dy))",
        py::arg("dout"), py::arg("hsave"), py::arg("mean"), py::arg("rstd"), py::arg("gamma"),
        py::arg("p"), py::arg("seed"), py::arg("offset"), py::arg("need_dres"), py::arg("need_dy"),
        py::arg("want_dy_colsum") = false, py::arg("dh_in") = py::none(), py::arg("post") = false,
        py::arg("dg_acc") = py::none(), py::arg("db_acc") = py::none(), py::arg("dyb_acc") = py::none(),
        py::arg("part_buf") = py::none(), py::arg("part_acc") = false, py::arg("beta") = py::none(),
        py::arg("hcopy") = py::none(), py::arg("pair_hash") = false);
  m.def("ln_bwd_partials", &ln_bwd_partials, "floats of add_ln_bwd's deferred partial buffer (0: none)");
  m.def("ln_colreduce", &ln_colreduce, "dg/db(/dyb) += column sums of add_ln_bwd partials",
        py::arg("part"), py::arg("R"), py::arg("D"), py::arg("dg"), py::arg("db"), py::arg("dyb") = py::none());
  m.def("seq_pos_sums", &seq_pos_sums, "(sum over b, sum over l) of a [B*L, H] bf16 gradient in one read",
        py::arg("d"), py::arg("L"), py::arg("need_pos"), py::arg("need_temb"));
  m.def("colsum_acc", &colsum_acc, "dst += colsum(part) (fp32 partials [rows, cols])");
  m.def("bias_act_fwd", &bias_act_fwd, "z += bias (in place); y = act(z) -> (z, y)");
  m.def("bias_act_bwd", &bias_act_bwd, "dz = dy*act'(zy); db = colsum(dz) -> (dz, db)");
}
