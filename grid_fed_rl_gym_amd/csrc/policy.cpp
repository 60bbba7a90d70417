// policy.cpp -- host side of the MLP policy: the rules of gs_policy_mlp and the weight layout gs_k_policy_mlp reads (policy.h).
#include "policy.h"

#include <cmath>
#include <cstdio>

namespace {
std::string fmt(const char* f, int a = 0, int b = 0, int c = 0) {
  char buf[256];
  snprintf(buf, sizeof buf, f, a, b, c);
  return buf;
}
}  // namespace

std::string gs_policy_check(const gs_policy_mlp* p, int32_t obs_dim, int32_t action_dim) {
  if (!p) return "policy is NULL";
  if (p->struct_size != (int32_t)sizeof(gs_policy_mlp)) return fmt("gs_policy_mlp struct_size %d != %d", p->struct_size, (int)sizeof(gs_policy_mlp));
  if (action_dim <= 0) return fmt("a policy needs action_dim > 0 (have %d)", action_dim);
  if (p->n_layers < 1 || p->n_layers > GS_POLICY_MAX_LAYERS) return fmt("n_layers %d outside 1 .. %d", p->n_layers, GS_POLICY_MAX_LAYERS);
  if (p->activation != GS_ACT_RELU && p->activation != GS_ACT_TANH && p->activation != GS_ACT_ELU) return fmt("unknown activation %d", p->activation);
  if (p->head != GS_HEAD_TANH && p->head != GS_HEAD_GAUSSIAN_TANH) return fmt("unknown head %d", p->head);
  if (p->stochastic != 0 && p->stochastic != 1) return fmt("stochastic must be 0 or 1 (have %d)", p->stochastic);
  if (p->stochastic && p->head != GS_HEAD_GAUSSIAN_TANH) return "stochastic needs the Gaussian head (GS_HEAD_GAUSSIAN_TANH)";
  if (p->dims[0] != obs_dim) return fmt("dims[0] = %d != obs_dim %d", p->dims[0], obs_dim);
  for (int l = 1; l <= p->n_layers; ++l)
    if (p->dims[l] < 1 || p->dims[l] > GS_POL_MAX_WIDTH) return fmt("dims[%d] = %d outside 1 .. %d", l, p->dims[l], GS_POL_MAX_WIDTH);
  const int want = p->head == GS_HEAD_GAUSSIAN_TANH ? 2 * action_dim : action_dim;
  if (p->dims[p->n_layers] != want) return fmt("the last width %d does not match the head (%d for action_dim %d)", p->dims[p->n_layers], want, action_dim);
  for (int l = 0; l < p->n_layers; ++l) {
    if (!p->weights[l] || !p->biases[l]) return fmt("weights[%d] / biases[%d] is NULL", l, l);
    const size_t nw = (size_t)p->dims[l + 1] * p->dims[l];
    for (size_t i = 0; i < nw; ++i)
      if (!std::isfinite(p->weights[l][i])) return fmt("weights[%d] holds a non-finite value (row %d, column %d)", l, (int)(i / p->dims[l]), (int)(i % p->dims[l]));
    for (int i = 0; i < p->dims[l + 1]; ++i)
      if (!std::isfinite(p->biases[l][i])) return fmt("biases[%d][%d] is not finite", l, i);
  }
  return "";
}

GsPolicyImage gs_policy_pack(const gs_policy_mlp& p) {
  GsPolicyImage im;
  size_t total = 0;
  for (int l = 0; l < p.n_layers; ++l) {
    im.kb[l] = 2 * ((p.dims[l] + 15) / 16);
    im.nt[l] = (p.dims[l + 1] + 15) / 16;
    im.w_off[l] = total; total += (size_t)im.nt[l] * im.kb[l] * 128;
    im.b_off[l] = total; total += (size_t)im.nt[l] * 16;
  }
  im.blob.assign(total, 0.0);
  for (int l = 0; l < p.n_layers; ++l) {
    const int K = p.dims[l], N = p.dims[l + 1];
    double* w = im.blob.data() + im.w_off[l];
    for (int nt = 0; nt < im.nt[l]; ++nt)
      for (int kb = 0; kb < im.kb[l]; ++kb)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 2; ++j) {
            const int n = 16 * nt + (lane & 15), k = 8 * kb + 2 * (lane >> 4) + j;
            if (n < N && k < K) w[(((size_t)nt * im.kb[l] + kb) * 64 + lane) * 2 + j] = p.weights[l][(size_t)n * K + k];
          }
    for (int n = 0; n < N; ++n) im.blob[im.b_off[l] + n] = p.biases[l][n];
  }
  return im;
}
