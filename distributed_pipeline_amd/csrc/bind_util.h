// Shared by the binding translation units (bindings.cpp, bind_*.cpp): the argument-check macros,
// the current stream, raw-pointer helpers and the checks that several kernel families repeat.
// The only header of csrc/ that includes ATen - the kernel TUs never see it.
#pragma once
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>

#include <vector>

#include "launchers.h"

#define CHECK_DEV(x) TORCH_CHECK((x).is_cuda(), #x " must be a HIP tensor")
#define CHECK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")
#define CHECK_F32(x) TORCH_CHECK((x).scalar_type() == at::kFloat, #x " must be float32")
#define CHECK_BF16(x) TORCH_CHECK((x).scalar_type() == at::kBFloat16, #x " must be bfloat16")
#define CHECK_ALIGNED(x) \
  TORCH_CHECK(reinterpret_cast<uintptr_t>((x).data_ptr()) % 16 == 0, #x " must be 16-byte aligned")

// Every op launches on the *current* HIP stream of the tensor's device, so it composes with
// torch's stream semantics and with HIP-graph capture.
static inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

// bf16 storage as the launchers take it (no dtype check: the caller has made it)
static inline const uint16_t* bf_ptr(const at::Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }
static inline uint16_t* bf_mut(const at::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

// an optional tensor argument that was given (not None, not an undefined tensor)
static inline bool has(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); }

// nullptr when absent; unchecked (e.g. the GEMM biases)
static inline const uint16_t* opt_bf_ptr(const c10::optional<at::Tensor>& t) { return has(t) ? bf_ptr(*t) : nullptr; }
// nullptr when absent, else a contiguous bf16 tensor of numel elements (msg names the size)
static inline const uint16_t* opt_bf_ptr(const c10::optional<at::Tensor>& t, int64_t numel, const char* msg) {
  if (!has(t)) return nullptr;
  TORCH_CHECK(t->scalar_type() == at::kBFloat16, msg, ": must be bfloat16");
  TORCH_CHECK(t->is_contiguous(), msg, ": must be contiguous");
  TORCH_CHECK(t->numel() == numel, msg);
  return bf_ptr(*t);
}
// nullptr when absent, else an fp32 tensor of numel elements (msg names the size), contiguous
// where the op asks for it
static inline float* opt_f32_ptr(const c10::optional<at::Tensor>& t, int64_t numel, const char* msg, bool contig) {
  if (!has(t)) return nullptr;
  TORCH_CHECK(t->scalar_type() == at::kFloat, msg, ": must be float32");
  TORCH_CHECK(!contig || t->is_contiguous(), msg, ": must be contiguous");
  TORCH_CHECK(t->numel() == numel, msg);
  return t->data_ptr<float>();
}

// A caller-owned fp32 accumulator (a parameter's flat .grad view, a partial slot) the op can write
// straight into: given, fp32, contiguous, numel elements (< 0: any length), on the op's device.
// An unusable one is ignored, never refused - the op returns its result as without it.
static inline bool usable_acc(const c10::optional<at::Tensor>& t, int64_t numel, const c10::Device& dev) {
  return has(t) && t->scalar_type() == at::kFloat && t->is_contiguous() && (numel < 0 || t->numel() == numel) &&
         t->device() == dev;
}

// The one-byte K/V cache of csrc/attn_decode_fp8.hip: codes uint8 [B, H, Lmax, D] and exponents int8
// [B, H, Lmax] (views into larger buffers work).  Wrong dtypes or shapes are refused; -> whether the
// kernels can take the layout (packed rows of D bytes on 16 bytes, packed exponent rows, on `dev`).
static inline bool fp8_cache_usable(const at::Tensor& codes, const at::Tensor& exps, const c10::Device& dev,
                                    const char* name) {
  TORCH_CHECK(codes.scalar_type() == at::kByte && exps.scalar_type() == at::kChar, name,
              ": codes must be uint8 and exponents int8");
  TORCH_CHECK(codes.dim() == 4 && exps.dim() == 3 && exps.size(0) == codes.size(0) && exps.size(1) == codes.size(1) &&
                  exps.size(2) == codes.size(2),
              name, ": codes must be [B, H, Lmax, D] and exponents [B, H, Lmax]");
  if (!codes.is_cuda() || !exps.is_cuda() || codes.device() != dev || exps.device() != dev) return false;
  const int64_t D = codes.size(3);
  return codes.stride(3) == 1 && codes.stride(2) == D && codes.stride(0) % 16 == 0 && codes.stride(1) % 16 == 0 &&
         reinterpret_cast<uintptr_t>(codes.data_ptr()) % 16 == 0 && (exps.stride(2) == 1 || exps.size(2) <= 1);
}

static inline void check_i64(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kLong && t.is_contiguous(), name,
              " must be a contiguous int64 HIP tensor");
}

namespace dpa {
// the one binding another family calls (bind_diffusion.cpp): lxent_bwd scatters its one-hot term
// through it
void emb_grad(const at::Tensor& ids, const at::Tensor& dy, at::Tensor& dW);

void register_comm(pybind11::module& m);     // comm/reducer.cpp
void register_runtime(pybind11::module& m);  // runtime/streams.cpp
void register_elementwise(pybind11::module& m);
void register_heads(pybind11::module& m);
void register_attention(pybind11::module& m);
void register_gemm(pybind11::module& m);
void register_diffusion(pybind11::module& m);
void register_text(pybind11::module& m);
}  // namespace dpa
