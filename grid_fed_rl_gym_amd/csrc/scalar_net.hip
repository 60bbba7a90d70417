// scalar_net.hip -- what the row networks share on the host (handle.h "what the scalar-output networks share on the host"; DESIGN.md
// section 28): the install and the grid of the two scalar-output networks, and the ONE launch of each kernel that runs a network over
// rows of float64 observations -- gs_k_value_mlp_f32, gs_k_q_mlp_f32 / _rows_f32, gs_k_policy_rows_f32.  Every entry that evaluates
// a network over rows (abi_onpolicy.hip, abi_q.hip, abi_q_next.hip, abi_refresh.hip) launches it from here.
#include "handle.h"

namespace gsi __attribute__((visibility("hidden"))) {

int scalar_net_install(gs_handle* h, gs_handle::Value& val, const void* kernel, const gs_policy_mlp& p, const gs_policy_mlp_opts& o, ScalarNet& net) {
  net.im = gs_policy_pack_f32(p, o);
  val.lds = gs_val_lds_bytes(net.im.kb[0]);
  HIPCHK(h, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GS_VAL_LDS_MAX));
  if (int rc = upload_image_f32(h, val.blob, net.im, &net.image, &net.norm)) return rc;
  for (int l = 0; l <= p.n_layers; ++l) val.dims[l] = p.dims[l];
  val.h_norm = net.im.norm;
  return GS_OK;
}

int scalar_net_grid(gs_handle* h, long long rows, const char* kernel, unsigned* blocks) {
  if (rows > 0x7fffffffLL - GS_VAL_ROWS) return fail(h, GS_E_INVALID, "%lld rows exceed the %s kernel's 32-bit row index", rows, kernel);
  *blocks = (unsigned)((rows + GS_VAL_ROWS - 1) / GS_VAL_ROWS);
  return GS_OK;
}

int launch_value_rows(gs_handle* h, const gs_handle::Value& val, const double* obs, double* out, long long rows, const int32_t* rows_dev, const int32_t* scatter_idx,
                      double* scatter_out, int scatter_T) {
  if (rows <= 0) return GS_OK;
  unsigned blocks = 0;
  if (int rc = scalar_net_grid(h, rows, "value", &blocks)) return rc;
  GsValueArgs a = val.args;
  a.obs = obs; a.out = out; a.rows = (int32_t)rows; a.rows_dev = rows_dev;
  a.scatter_idx = scatter_idx; a.scatter_out = scatter_out; a.scatter_T = scatter_T; a.scatter_B = h->B;
  hipLaunchKernelGGL(gs_k_value_mlp_f32, dim3(blocks), dim3(64 * GS_POL_WAVES), val.lds, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

int launch_q_rows(gs_handle* h, const gs_handle::QNet& Q, const GsPolicyLayerF32* L, const double* obs, const double* act, long long rows, const int32_t* rows_dev,
                  double* out) {
  unsigned blocks = 0;
  if (int rc = scalar_net_grid(h, rows, "Q", &blocks)) return rc;
  GsQArgs a = Q.qargs;
  a.obs = obs; a.act = act; a.out = out; a.rows = (int32_t)rows;
  for (int l = 0; l < a.n_layers; ++l) a.L[l] = L[l];
  if (rows_dev) hipLaunchKernelGGL(gs_k_q_mlp_rows_f32, dim3(blocks), dim3(64 * GS_POL_WAVES), Q.net.lds, h->stream, a, rows_dev);
  else hipLaunchKernelGGL(gs_k_q_mlp_f32, dim3(blocks), dim3(64 * GS_POL_WAVES), Q.net.lds, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

int launch_policy_rows(gs_handle* h, const PolicyNoise& noise, const double* obs, long long rows, const int32_t* rows_dev, const int32_t* idx, uint32_t tag,
                       float* pre, double* act, double* eps, double* lp) {
  unsigned blocks = 0;
  if (int rc = scalar_net_grid(h, rows, "policy-rows", &blocks)) return rc;
  const GsPolicyArgsF32& p = h->pol.args32;
  GsPolicyRowsArgs a{};
  a.obs = obs; a.rows_dev = rows_dev; a.idx = idx; a.shift = p.shift; a.scale = p.scale;
  a.pre_head = pre; a.act = act; a.noise = eps; a.logp = lp;
  a.rows = (int32_t)rows; a.B = h->B; a.D = p.D; a.A = p.A; a.n_layers = p.n_layers; a.activation = p.activation;
  a.obs_stride = gs_val_obs_stride(p.L[0].kb); a.panel_kb = gs_val_panel_kb(p.L[0].kb);
  a.stochastic = noise.stochastic; a.draw = noise.draw; a.tag = tag; a.seed = noise.seed;
  for (int l = 0; l < p.n_layers; ++l) a.L[l] = p.L[l];
  hipLaunchKernelGGL(gs_k_policy_rows_f32, dim3(blocks), dim3(64 * GS_POL_WAVES), gs_qn_lds_bytes(p.L[0].kb, p.A), h->stream, a);
  HIPCHK(h, hipGetLastError());
  return GS_OK;
}

int rows_kernels_lds_cap(gs_handle* h) {
  // (the cap on a kernel's dynamic LDS is a setting of the FUNCTION: always the most, policy.h GS_POL_LDS_MAX)
  HIPCHK(h, hipFuncSetAttribute((const void*)gs_k_policy_rows_f32, hipFuncAttributeMaxDynamicSharedMemorySize, GS_VAL_LDS_MAX));
  HIPCHK(h, hipFuncSetAttribute((const void*)gs_k_q_mlp_rows_f32, hipFuncAttributeMaxDynamicSharedMemorySize, GS_VAL_LDS_MAX));
  return GS_OK;
}

}  // namespace gsi
