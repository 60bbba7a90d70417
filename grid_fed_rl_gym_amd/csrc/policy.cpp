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

std::string gs_policy_check_opts(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim, int32_t action_dim) {
  const std::string why = gs_policy_check(p, obs_dim, action_dim);
  if (!why.empty() || !o) return why;
  if (o->struct_size != (int32_t)sizeof(gs_policy_mlp_opts)) return fmt("gs_policy_mlp_opts struct_size %d != %d", o->struct_size, (int)sizeof(gs_policy_mlp_opts));
  if (o->compute != GS_COMPUTE_F64 && o->compute != GS_COMPUTE_F32) return fmt("unknown compute %d", o->compute);
  if (o->compute == GS_COMPUTE_F64) {
    if (o->obs_shift || o->obs_scale)
      return "obs_shift / obs_scale need GS_COMPUTE_F32: the float64 path takes raw observations, fold the normalisation into the first layer (as MLPPolicy does)";
    return "";
  }
  for (int i = 0; i < p->dims[0]; ++i) {
    if (o->obs_shift && !std::isfinite(o->obs_shift[i])) return fmt("obs_shift[%d] is not finite", i);
    if (o->obs_scale && !std::isfinite(o->obs_scale[i])) return fmt("obs_scale[%d] is not finite", i);
  }
  // the largest double that still rounds to a finite float32: anything at or beyond FLT_MAX + half an ulp rounds to infinity
  const double limit = 0x1.ffffffp127;
  for (int l = 0; l < p->n_layers; ++l) {
    const size_t nw = (size_t)p->dims[l + 1] * p->dims[l];
    for (size_t i = 0; i < nw; ++i)
      if (std::fabs(p->weights[l][i]) >= limit) return fmt("weights[%d] holds a value that is not finite in float32 (row %d, column %d)", l, (int)(i / p->dims[l]), (int)(i % p->dims[l]));
    for (int i = 0; i < p->dims[l + 1]; ++i)
      if (std::fabs(p->biases[l][i]) >= limit) return fmt("biases[%d][%d] is not finite in float32", l, i);
  }
  return "";
}

std::string gs_value_check(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim) {
  if (!p) return "value network is NULL";
  if (p->struct_size != (int32_t)sizeof(gs_policy_mlp)) return fmt("gs_policy_mlp struct_size %d != %d", p->struct_size, (int)sizeof(gs_policy_mlp));
  if (p->head != GS_HEAD_LINEAR) return fmt("a value network needs head GS_HEAD_LINEAR (have %d)", p->head);
  if (p->stochastic != 0) return fmt("a value network is not stochastic (have %d)", p->stochastic);
  if (p->n_layers < 1 || p->n_layers > GS_POLICY_MAX_LAYERS) return fmt("n_layers %d outside 1 .. %d", p->n_layers, GS_POLICY_MAX_LAYERS);
  if (p->dims[p->n_layers] != 1) return fmt("a value network's last width must be 1 (have %d)", p->dims[p->n_layers]);
  if (!o || o->compute != GS_COMPUTE_F32) return "a value network needs gs_policy_mlp_opts with compute = GS_COMPUTE_F32 (the precision of torch critics)";
  // every other rule is the policy's: a plain head of one output
  gs_policy_mlp q = *p;
  q.head = GS_HEAD_TANH;
  return gs_policy_check_opts(&q, o, obs_dim, 1);
}

GsPolicyImageF32 gs_policy_pack_f32(const gs_policy_mlp& p, const gs_policy_mlp_opts& o) {
  GsPolicyImageF32 im;
  size_t total = 0;
  for (int l = 0; l < p.n_layers; ++l) {
    im.kb[l] = (p.dims[l] + 15) / 16;
    im.nt[l] = (p.dims[l + 1] + 15) / 16;
    im.w_off[l] = total; total += (size_t)im.nt[l] * im.kb[l] * 256;
    im.b_off[l] = total; total += (size_t)im.nt[l] * 16;
  }
  im.blob.assign(total, 0.0f);
  for (int l = 0; l < p.n_layers; ++l) {
    const int K = p.dims[l], N = p.dims[l + 1];
    float* w = im.blob.data() + im.w_off[l];
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) w[gs_pol32_slot(n, k, im.kb[l])] = (float)p.weights[l][(size_t)n * K + k];
    for (int n = 0; n < N; ++n) im.blob[im.b_off[l] + n] = (float)p.biases[l][n];
  }
  const int D = p.dims[0], D16 = 16 * im.kb[0];
  im.norm.assign(2 * (size_t)D16, 0.0);
  for (int i = 0; i < D; ++i) {
    im.norm[i] = o.obs_shift ? o.obs_shift[i] : 0.0;
    im.norm[D16 + i] = o.obs_scale ? o.obs_scale[i] : 1.0;
  }
  return im;
}

void gs_policy_unpack_f32(const GsPolicyLayerF32& L, int n_out, int n_in, float* dst, float* wt) {
  for (int o = 0; o < n_out; ++o)
    for (int k = 0; k < n_in; ++k) {
      const float x = L.w[gs_pol32_slot(o, k, L.kb)];
      dst[(size_t)o * n_in + k] = x;
      if (wt) wt[gs_pol32_slot(k, o, L.nt)] = x;
    }
  for (int o = 0; o < n_out; ++o) dst[(size_t)n_out * n_in + o] = L.b[o];
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
