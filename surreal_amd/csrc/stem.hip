// stem.hip — the pixel stem behind one entry point (stem_plan.hpp): the fused
// kernels of cnn_kernels.hip where stem_fused_ok holds, else one general
// convolution launch per layer and direction (conv_kernels.hip) and the Linear
// layer on the GEMM engine, as the fused path runs it.  Both forms honour the
// device stop flag and write the same outputs: the activations, feat at ldf
// and the whole flat gradient.  Host code only; arguments checked by the caller.
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "stem_plan.hpp"

namespace smi {

int stem_forward(const StemPlan& p, const float* prm, const PixRows& pr, int64_t rows,
                 float* const* A, float* feat, int64_t ldf, hipStream_t st, const int* skip) {
  if (p.fused)
    return cnn_forward(prm, pr, p.C, p.H, p.W, p.F, rows, A[0], A[1], feat, ldf, st, skip);
  if (rows < 1) return SMI_OK;
  for (int i = 0; i < p.n; ++i) {
    if (i == 0)
      RC_CHECK(conv2d_forward(nullptr, 1, 1, rows, p.g[0], prm + p.oW[0], prm + p.ob[0], ACT_RELU,
                              A[0], st, skip, &pr));
    else
      RC_CHECK(conv2d_forward(A[i - 1], 0, 0, rows, p.g[i], prm + p.oW[i], prm + p.ob[i], ACT_RELU,
                              A[i], st, skip));
  }
  return launch_linear_fwd(A[p.n - 1], p.flat, (int)rows, (int)p.flat, prm + p.oWf, p.flat,
                           prm + p.obf, p.F, ACT_RELU, feat, ldf, st, skip);
}

int stem_backward(const StemPlan& p, const float* prm, const PixRows& pr, int64_t rows,
                  const float* const* A, const float* dz, int64_t lddz, float* grad,
                  float* const* dA, float* part, hipStream_t st, const int* skip) {
  if (p.fused)
    return cnn_backward(prm, pr, p.C, p.H, p.W, p.F, rows, A[0], A[1], dz, lddz, grad, dA[1], part,
                        st, skip);
  if (rows < 1) return SMI_OK;
  const int n = p.n;
  const float* An = A[n - 1];
  RC_CHECK(launch_linear_bwd_dw(dz, lddz, (int)rows, p.F, An, p.flat, (int)p.flat, grad + p.oWf,
                                p.flat, grad + p.obf, 0, st, skip));
  RC_CHECK(launch_linear_bwd_dx(dz, lddz, (int)rows, p.F, prm + p.oWf, p.flat, (int)p.flat, An,
                                p.flat, dA[n - 1], p.flat, st, skip));
  // dA_{i-1} = [A_{i-1} > 0] convT(dA_i, w_i); layer 1 has no input gradient
  for (int i = n - 1; i >= 0; --i) {
    if (i == 0)
      RC_CHECK(conv2d_backward_weight(dA[0], nullptr, 1, 1, rows, p.g[0], grad + p.oW[0],
                                      grad + p.ob[0], part, st, skip, &pr));
    else {
      RC_CHECK(conv2d_backward_weight(dA[i], A[i - 1], 0, 0, rows, p.g[i], grad + p.oW[i],
                                      grad + p.ob[i], part, st, skip));
      RC_CHECK(conv2d_backward_input(dA[i], rows, p.g[i], prm + p.oW[i], A[i - 1], dA[i - 1], st,
                                     skip));
    }
  }
  return SMI_OK;
}

}  // namespace smi
