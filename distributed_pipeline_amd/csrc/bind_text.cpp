// Bindings of the generation and text-metric kernels: token sampling (sample.hip), the beam-search
// step (beam_step.hip), the logit processors (logit_penalty.hip), teacher-forced scoring
// (token_stats.hip) and the per-group n-gram / LCS counts (ngram_match.hip, ngram_distinct.hip, lcs.hip).
#include <limits.h>

#include "bind_util.h"

// One next-token draw per row of logits [B, V] (csrc/sample.hip; the definition is in ops/decode.py):
// -> [tokens int64 [B]], with return_stats also thr fp32 [B] and kept int32 [B]; None for a case the
// kernel does not cover (CPU tensor, dtype, V > 65536, a last stride other than 1, B == 0).  seed and
// row_base carry 64 bits in their two's complement; step is used modulo 2^32.
static c10::optional<std::vector<at::Tensor>> sample_tokens(const at::Tensor& logits, double temperature,
                                                            int64_t top_k, double top_p, int64_t seed, int64_t step,
                                                            int64_t row_base, bool return_stats) {
  TORCH_CHECK(logits.dim() == 2, "sample_tokens: logits [B, V]");
  TORCH_CHECK(temperature > 0, "sample_tokens: temperature must be > 0");
  const int64_t B = logits.size(0), V = logits.size(1);
  if (!logits.is_cuda() || (logits.scalar_type() != at::kFloat && logits.scalar_type() != at::kBFloat16))
    return c10::nullopt;
  if (B < 1 || B > 0x7fffffffLL || V < 1 || V > 65536 || logits.stride(1) != 1 || logits.stride(0) < 0)
    return c10::nullopt;
  const c10::DeviceGuard guard(logits.device());
  auto opt = at::TensorOptions().device(logits.device());
  std::vector<at::Tensor> out{at::empty({B}, opt.dtype(at::kLong))};
  if (return_stats) {
    out.push_back(at::empty({B}, opt.dtype(at::kFloat)));
    out.push_back(at::empty({B}, opt.dtype(at::kInt)));
  }
  const int k = (top_k > 0 && top_k < V) ? (int)top_k : 0;
  const bool ok = dpa::launch_sample_tokens(
      logits.data_ptr(), logits.scalar_type() == at::kBFloat16, logits.stride(0), B, (int)V, (float)temperature, k,
      (float)top_p, (uint64_t)seed, (uint32_t)step, (uint64_t)row_base, out[0].data_ptr<int64_t>(),
      return_stats ? out[1].data_ptr<float>() : nullptr, return_stats ? out[2].data_ptr<int>() : nullptr,
      cur_stream());
  if (!ok) return c10::nullopt;
  return out;
}

// The uniforms sample_tokens draws with -> fp32 [B, V] on `like`'s device, or None (a CPU tensor, a
// shape the kernel does not cover).
static c10::optional<at::Tensor> sample_uniforms(const at::Tensor& like, int64_t seed, int64_t step,
                                                 int64_t row_base, int64_t B, int64_t V) {
  if (!like.is_cuda() || B < 1 || V < 1 || V > 65536 || B > 0x7fffffffLL) return c10::nullopt;
  const c10::DeviceGuard guard(like.device());
  at::Tensor out = at::empty({B, V}, at::TensorOptions().device(like.device()).dtype(at::kFloat));
  if (!dpa::launch_sample_uniforms(out.data_ptr<float>(), B, (int)V, (uint64_t)seed, (uint32_t)step,
                                   (uint64_t)row_base, cur_stream()))
    return c10::nullopt;
  return out;
}

// One beam-search step (csrc/beam_step.hip; the definition is in ops/decode.py): logits [B, W, V] fp32 or
// bf16 (last stride 1, any batch / beam stride >= 0), scores fp32 [B, W], finished bool [B, W] ->
// [new_scores fp32, parent int32, token int64, new_finished bool, logp fp32], all [B, W] (logp: a live
// pick's own log-probability term, 0 for a finished beam's candidate and an empty slot); None for a case the
// kernel does not cover (CPU tensor, dtype, V > 65536, W > 8, a last stride other than 1, B == 0).
static c10::optional<std::vector<at::Tensor>> beam_step(const at::Tensor& logits, const at::Tensor& scores,
                                                        const at::Tensor& finished, int64_t eos_id, int64_t fill) {
  TORCH_CHECK(logits.dim() == 3, "beam_step: logits [B, W, V]");
  const int64_t B = logits.size(0), W = logits.size(1), V = logits.size(2);
  TORCH_CHECK(scores.dim() == 2 && scores.size(0) == B && scores.size(1) == W && finished.sizes() == scores.sizes(),
              "beam_step: scores and finished must be [B, W]");
  TORCH_CHECK(scores.scalar_type() == at::kFloat, "beam_step: scores must be float32");
  TORCH_CHECK(finished.scalar_type() == at::kBool, "beam_step: finished must be bool");
  if (!logits.is_cuda() || (logits.scalar_type() != at::kFloat && logits.scalar_type() != at::kBFloat16))
    return c10::nullopt;
  if (scores.device() != logits.device() || finished.device() != logits.device() || !scores.is_contiguous() ||
      !finished.is_contiguous())
    return c10::nullopt;
  if (B < 1 || W < 1 || W > 8 || V < 1 || V > 65536 || B * W > 0x7fffffffLL || (V > 1 && logits.stride(2) != 1) ||
      logits.stride(0) < 0 || logits.stride(1) < 0 || fill < INT_MIN || fill > INT_MAX)
    return c10::nullopt;
  const c10::DeviceGuard guard(logits.device());
  auto opt = at::TensorOptions().device(logits.device());
  std::vector<at::Tensor> out{at::empty({B, W}, opt.dtype(at::kFloat)), at::empty({B, W}, opt.dtype(at::kInt)),
                              at::empty({B, W}, opt.dtype(at::kLong)), at::empty({B, W}, opt.dtype(at::kBool)),
                              at::empty({B, W}, opt.dtype(at::kFloat))};
  at::Tensor ws_c = at::empty({B, W, W + 2}, opt.dtype(at::kFloat)), ws_v = at::empty({B, W, W}, opt.dtype(at::kInt));
  const int eos = (eos_id < 0 || eos_id > INT_MAX) ? -1 : (int)eos_id;
  const bool ok = dpa::launch_beam_step(
      logits.data_ptr(), logits.scalar_type() == at::kBFloat16, logits.stride(0), logits.stride(1), B, (int)W, (int)V,
      scores.data_ptr<float>(), reinterpret_cast<const uint8_t*>(finished.data_ptr<bool>()), eos, (int)fill,
      ws_c.data_ptr<float>(), ws_v.data_ptr<int>(), out[0].data_ptr<float>(), out[1].data_ptr<int>(),
      out[2].data_ptr<int64_t>(), reinterpret_cast<uint8_t*>(out[3].data_ptr<bool>()), out[4].data_ptr<float>(),
      cur_stream());
  if (!ok) return c10::nullopt;
  return out;
}

// The logit processors of generation, in place (csrc/logit_penalty.hip; the definition is in ops/decode.py):
// logits [R, V] fp32 or bf16 (last stride 1, rows that do not overlap), hist [R, Lh] int32 or int64 (any
// strides), n and start (optional) int32 [R] -> true when the kernel ran, false for a case it does not
// cover (CPU tensor, dtype, Lh > 2048, a last stride other than 1, n or start not contiguous int32).
static bool penalize_logits(at::Tensor& logits, const at::Tensor& hist, const at::Tensor& n,
                            const c10::optional<at::Tensor>& start, double theta, double alpha_p, double alpha_f,
                            int64_t ngram) {
  TORCH_CHECK(logits.dim() == 2 && hist.dim() == 2 && n.dim() == 1, "penalize_logits: logits [R, V], hist [R, Lh], n [R]");
  const int64_t R = logits.size(0), V = logits.size(1), Lh = hist.size(1);
  TORCH_CHECK(hist.size(0) == R && n.size(0) == R, "penalize_logits: hist and n must have logits' R rows");
  TORCH_CHECK(!has(start) || (start->dim() == 1 && start->size(0) == R), "penalize_logits: start must be [R]");
  TORCH_CHECK(theta > 0 && ngram >= 0, "penalize_logits: repetition_penalty must be > 0 and no_repeat_ngram >= 0");
  TORCH_CHECK(R <= 1 || logits.stride(0) >= V, "penalize_logits: the rows of logits overlap");
  if (R == 0 || V == 0 || Lh == 0) return true;
  if (!logits.is_cuda() || (logits.scalar_type() != at::kFloat && logits.scalar_type() != at::kBFloat16))
    return false;
  if (hist.scalar_type() != at::kInt && hist.scalar_type() != at::kLong) return false;
  auto i32 = [&](const at::Tensor& t) {
    return t.scalar_type() == at::kInt && t.is_contiguous() && t.device() == logits.device();
  };
  if (hist.device() != logits.device() || !i32(n) || (has(start) && !i32(*start))) return false;
  if (R > 0x7fffffffLL || V > 0x7fffffffLL || Lh > dpa::LP_MAX_L || (V > 1 && logits.stride(1) != 1)) return false;
  const c10::DeviceGuard guard(logits.device());
  return dpa::launch_logit_penalty(logits.data_ptr(), logits.scalar_type() == at::kBFloat16, logits.stride(0), R,
                                   (int)V, hist.data_ptr(), hist.scalar_type() == at::kLong, hist.stride(0),
                                   hist.stride(1), (int)Lh, n.data_ptr<int>(),
                                   has(start) ? start->data_ptr<int>() : nullptr, (float)theta, (float)alpha_p,
                                   (float)alpha_f, (int)std::min<int64_t>(ngram, INT_MAX), cur_stream());
}

// Teacher-forced statistics of logits [R, V] against targets [R] (csrc/token_stats.hip; the definition is in
// ops/decode.py): logits fp32 or bf16 (last stride 1, any row stride >= 0), targets int32 or int64 (any
// stride) -> [logp fp32, rank int32, entropy fp32, top1 int32], all [R]; None for a case the kernel does
// not cover (CPU tensor, dtype, V > 65536, V < 1, a last stride other than 1, R == 0).
static c10::optional<std::vector<at::Tensor>> token_stats(const at::Tensor& logits, const at::Tensor& targets) {
  TORCH_CHECK(logits.dim() == 2 && targets.dim() == 1 && targets.size(0) == logits.size(0),
              "token_stats: logits [R, V], targets [R]");
  const int64_t R = logits.size(0), V = logits.size(1);
  if (!logits.is_cuda() || (logits.scalar_type() != at::kFloat && logits.scalar_type() != at::kBFloat16))
    return c10::nullopt;
  if (targets.device() != logits.device() || (targets.scalar_type() != at::kInt && targets.scalar_type() != at::kLong))
    return c10::nullopt;
  if (R < 1 || R > 0x7fffffffLL || V < 1 || V > 65536 || (V > 1 && logits.stride(1) != 1) || logits.stride(0) < 0)
    return c10::nullopt;
  const c10::DeviceGuard guard(logits.device());
  auto opt = at::TensorOptions().device(logits.device());
  std::vector<at::Tensor> out{at::empty({R}, opt.dtype(at::kFloat)), at::empty({R}, opt.dtype(at::kInt)),
                              at::empty({R}, opt.dtype(at::kFloat)), at::empty({R}, opt.dtype(at::kInt))};
  const bool ok = dpa::launch_token_stats(
      logits.data_ptr(), logits.scalar_type() == at::kBFloat16, logits.stride(0), R, (int)V, targets.data_ptr(),
      targets.scalar_type() == at::kLong, targets.stride(0), out[0].data_ptr<float>(), out[1].data_ptr<int>(),
      out[2].data_ptr<float>(), out[3].data_ptr<int>(), cur_stream());
  if (!ok) return c10::nullopt;
  return out;
}

// ---- per-group token ops: tokens [G, K, L] int32 / int64, lens [G, K] int32 -> int32 counts ----
static void check_token_group(const at::Tensor& tokens, const at::Tensor& lens, const char* op) {
  CHECK_DEV(tokens); CHECK_CONTIG(tokens); CHECK_DEV(lens); CHECK_CONTIG(lens);
  TORCH_CHECK(tokens.scalar_type() == at::kInt || tokens.scalar_type() == at::kLong, op,
              ": tokens must be int32 or int64");
  TORCH_CHECK(lens.scalar_type() == at::kInt, op, ": lens must be int32");
  TORCH_CHECK(tokens.dim() == 3 && lens.dim() == 2 && lens.size(0) == tokens.size(0) &&
                  lens.size(1) == tokens.size(1) && lens.device() == tokens.device(),
              op, ": tokens [G, K, L], lens [G, K] on one device");
}

using TokenGroupLauncher = bool (*)(const void*, bool, const int*, int64_t, int, int, int*, hipStream_t);

// the int32 result of `shape` from checked inputs, or None for a shape the kernel does not cover
static c10::optional<at::Tensor> run_token_group(const at::Tensor& tokens, const at::Tensor& lens,
                                                 at::IntArrayRef shape, TokenGroupLauncher launch) {
  const int64_t G = tokens.size(0), K = tokens.size(1), L = tokens.size(2);
  const c10::DeviceGuard guard(tokens.device());
  at::Tensor out = at::empty(shape, tokens.options().dtype(at::kInt));
  if (G == 0) return out;
  if (K > 0x7fffffffLL || L > 0x7fffffffLL) return c10::nullopt;
  if (!launch(tokens.data_ptr(), tokens.scalar_type() == at::kLong, lens.data_ptr<int>(), G, (int)K, (int)L,
              out.data_ptr<int>(), cur_stream()))
    return c10::nullopt;
  return out;
}

// Clipped n-gram match counts of every pair of a group's K sequences (csrc/ngram_match.hip):
// -> int32 [G, K, K, 4]
static c10::optional<at::Tensor> ngram_matches(const at::Tensor& tokens, const at::Tensor& lens) {
  check_token_group(tokens, lens, "ngram_matches");
  const int64_t G = tokens.size(0), K = tokens.size(1);
  return run_token_group(tokens, lens, {G, K, K, 4}, dpa::launch_ngram_match);
}

// Distinct n-gram counts of a group's K sequences and of their union (csrc/ngram_distinct.hip):
// -> int32 [G, K + 1, 4]
static c10::optional<at::Tensor> ngram_distinct(const at::Tensor& tokens, const at::Tensor& lens) {
  check_token_group(tokens, lens, "ngram_distinct");
  const int64_t G = tokens.size(0), K = tokens.size(1);
  return run_token_group(tokens, lens, {G, K + 1, 4}, dpa::launch_ngram_distinct);
}

// LCS length of every pair of a group's K sequences (csrc/lcs.hip): -> int32 [G, K, K]
static c10::optional<at::Tensor> lcs_lengths(const at::Tensor& tokens, const at::Tensor& lens) {
  check_token_group(tokens, lens, "lcs_lengths");
  const int64_t G = tokens.size(0), K = tokens.size(1);
  return run_token_group(tokens, lens, {G, K, K}, dpa::launch_lcs_lengths);
}

void dpa::register_text(pybind11::module& m) {
  m.def("sample_tokens", &sample_tokens,
        "temperature / top-k / top-p next-token draw with counter-based noise -> [tokens] or [tokens, thr, kept] | None (case not covered)",
        py::arg("logits"), py::arg("temperature"), py::arg("top_k"), py::arg("top_p"), py::arg("seed"),
        py::arg("step"), py::arg("row_base"), py::arg("return_stats") = false);
  m.def("sample_uniforms", &sample_uniforms,
        "the uniforms of sample_tokens -> fp32 [B, V] | None (case not covered)", py::arg("like"), py::arg("seed"),
        py::arg("step"), py::arg("row_base"), py::arg("B"), py::arg("V"));
  m.def("beam_step", &beam_step,
        "one beam-search step: log-softmax + cumulative score + the W best of W V candidates -> [new_scores, parent, token, new_finished, logp] | None (case not covered)",
        py::arg("logits"), py::arg("scores"), py::arg("finished"), py::arg("eos_id") = -1, py::arg("fill") = 0);
  m.def("penalize_logits", &penalize_logits,
        "repetition / presence / frequency penalty and no-repeat-n-gram ban on logits, in place -> True | False (case not covered)",
        py::arg("logits"), py::arg("hist"), py::arg("n"), py::arg("start"), py::arg("theta"), py::arg("alpha_p"),
        py::arg("alpha_f"), py::arg("ngram"));
  m.def("token_stats", &token_stats,
        "log-probability and rank of a target id, entropy and arg-max of every logits row -> [logp, rank, entropy, top1] | None (case not covered)",
        py::arg("logits"), py::arg("targets"));
  m.def("ngram_matches", &ngram_matches,
        "clipped 1..4-gram match counts of every sequence pair of a group -> int32 [G, K, K, 4] | None (shape not covered)",
        py::arg("tokens"), py::arg("lens"));
  m.def("ngram_distinct", &ngram_distinct,
        "distinct 1..4-gram counts of every sequence of a group and of their union -> int32 [G, K + 1, 4] | None (shape not covered)",
        py::arg("tokens"), py::arg("lens"));
  m.def("lcs_lengths", &lcs_lengths,
        "longest-common-subsequence length of every sequence pair of a group -> int32 [G, K, K] | None (shape not covered)",
        py::arg("tokens"), py::arg("lens"));
}
