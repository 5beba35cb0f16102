// The Python module of the gfx950 kernels.  Each kernel family binds its ops (torch tensors ->
// raw launchers) in a translation unit of its own, bind_<family>.cpp, next to the checks they
// make; bind_util.h holds what they share.
#include "bind_util.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "distributed_pipeline_amd native gfx950 kernels";
  dpa::register_comm(m);
  dpa::register_runtime(m);
  dpa::register_elementwise(m);
  dpa::register_heads(m);
  dpa::register_attention(m);
  dpa::register_gemm(m);
  dpa::register_diffusion(m);
  dpa::register_text(m);
}
