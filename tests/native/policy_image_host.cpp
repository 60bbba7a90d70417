// Host check of the packed float32 image of csrc/policy.h (tests/test_policy_image.py builds it together with csrc/policy.cpp by the
// Makefile's host compiler line and runs it; no device).  For every network below: gs_policy_pack_f32 places every weight where the
// layout's description says ([nt][kb][64 lanes][4]: W[16 nt + (lane & 15)][16 kb + 4 (lane >> 4) + j]) and leaves every other slot
// zero; gs_policy_unpack_f32 gives every layer's float32 values back exactly, in torch order; the transposed image it fills for a
// layer l >= 1 is the pack of W_l^T.  Prints one line per network; exit status 0 exactly when every check holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "policy.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what, int l, long at) {
  if (ok) return;
  if (++failures <= 20) fprintf(stderr, "FAILED: %s (layer %d, at %ld)\n", what, l, at);
}

// distinct, nonzero, exactly representable in float32: a padded slot that received one, or a weight that went astray, shows
double value(int l, long i, bool bias) { return (double)(float)((bias ? -1.0 : 1.0) * (double)(1 + i + 100000L * l) / 1024.0); }

void check(const std::vector<int>& dims) {
  const int n_layers = (int)dims.size() - 1;
  std::vector<std::vector<double>> W(n_layers), B(n_layers);
  gs_policy_mlp p{};
  p.struct_size = (int32_t)sizeof(gs_policy_mlp); p.n_layers = n_layers; p.activation = GS_ACT_RELU; p.head = GS_HEAD_LINEAR;
  for (int l = 0; l <= n_layers; ++l) p.dims[l] = dims[l];
  for (int l = 0; l < n_layers; ++l) {
    W[l].resize((size_t)dims[l + 1] * dims[l]); B[l].resize(dims[l + 1]);
    for (size_t i = 0; i < W[l].size(); ++i) W[l][i] = value(l, (long)i, false);
    for (size_t i = 0; i < B[l].size(); ++i) B[l][i] = value(l, (long)i, true);
    p.weights[l] = W[l].data(); p.biases[l] = B[l].data();
  }
  gs_policy_mlp_opts o{};
  o.struct_size = (int32_t)sizeof(gs_policy_mlp_opts); o.compute = GS_COMPUTE_F32;
  const GsPolicyImageF32 im = gs_policy_pack_f32(p, o);

  size_t total = 0;
  for (int l = 0; l < n_layers; ++l) {
    const int n_in = dims[l], n_out = dims[l + 1], kb = im.kb[l], nt = im.nt[l];
    expect(kb == (n_in + 15) / 16 && nt == (n_out + 15) / 16, "block counts", l, 0);
    expect(im.w_off[l] == total, "the layers lie behind one another", l, (long)total);
    total = im.b_off[l] + 16 * (size_t)nt;
    const float* w = im.blob.data() + im.w_off[l];
    const float* b = im.blob.data() + im.b_off[l];
    // the image against the layout's description, slot by slot: a weight or, beyond the layer's shape, zero
    for (int t = 0; t < nt; ++t)
      for (int q = 0; q < kb; ++q)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j) {
            const int n = 16 * t + (lane & 15), k = 16 * q + 4 * (lane >> 4) + j;
            const long at = (((long)t * kb + q) * 64 + lane) * 4 + j;
            const float want = n < n_out && k < n_in ? (float)W[l][(size_t)n * n_in + k] : 0.0f;
            expect(memcmp(&w[at], &want, sizeof(float)) == 0, n < n_out && k < n_in ? "a weight's slot" : "a padded slot is zero", l, at);
          }
    for (int n = 0; n < 16 * nt; ++n) {
      const float want = n < n_out ? (float)B[l][n] : 0.0f;
      expect(memcmp(&b[n], &want, sizeof(float)) == 0, n < n_out ? "a bias" : "a padded bias is zero", l, n);
    }
    // the way back, and the transposed image
    const size_t wt_floats = (size_t)kb * nt * 256;
    std::vector<float> flat((size_t)n_out * (n_in + 1), -1.0f), wt(wt_floats, 0.0f);
    gs_policy_unpack_f32(GsPolicyLayerF32{w, b, kb, nt}, n_out, n_in, flat.data(), l ? wt.data() : nullptr);
    for (size_t i = 0; i < W[l].size(); ++i) {
      const float want = (float)W[l][i];
      expect(memcmp(&flat[i], &want, sizeof(float)) == 0, "an unpacked weight", l, (long)i);
    }
    for (int n = 0; n < n_out; ++n) {
      const float want = (float)B[l][n];
      expect(memcmp(&flat[W[l].size() + n], &want, sizeof(float)) == 0, "an unpacked bias", l, n);
    }
    if (!l) continue;
    std::vector<double> WT((size_t)n_in * n_out), zero(n_in, 0.0);
    for (int n = 0; n < n_out; ++n)
      for (int k = 0; k < n_in; ++k) WT[(size_t)k * n_out + n] = W[l][(size_t)n * n_in + k];
    gs_policy_mlp pt{};
    pt.struct_size = (int32_t)sizeof(gs_policy_mlp); pt.n_layers = 1; pt.activation = GS_ACT_RELU; pt.head = GS_HEAD_LINEAR;
    pt.dims[0] = n_out; pt.dims[1] = n_in; pt.weights[0] = WT.data(); pt.biases[0] = zero.data();
    const GsPolicyImageF32 it = gs_policy_pack_f32(pt, o);
    expect(it.kb[0] == nt && it.nt[0] == kb && it.b_off[0] - it.w_off[0] == wt_floats, "the transposed image's block counts", l, 0);
    if (it.b_off[0] - it.w_off[0] == wt_floats)
      for (size_t i = 0; i < wt_floats; ++i)
        expect(memcmp(&wt[i], &it.blob[it.w_off[0] + i], sizeof(float)) == 0, "the transposed image is the pack of W^T", l, (long)i);
  }
  expect(im.blob.size() == total, "the image's length", n_layers, (long)total);
  printf("dims");
  for (int d : dims) printf(" %d", d);
  printf(": %s\n", failures ? "FAILED" : "ok");
}

}  // namespace

int main() {
  check({71, 96, 40, 6});
  check({3, 1});
  return failures ? 1 : 0;
}
