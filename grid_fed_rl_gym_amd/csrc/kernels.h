// kernels.h -- host-visible declarations of the HIP kernels (defined in kernels_*.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <array>

#include "gs_internal.h"
#include "members.h"
#include "policy.h"
#include "train.h"
#include "q.h"
#include "q_next.h"
#include "pathwise.h"
#include "conservative.h"
#include "anchor.h"
#include "refresh.h"
#include "rollout_load.h"
#include "rollout_window.h"

// The launch tables: host function pointers of the kernel members, indexed by their enum (members.h); nullptr where a member has no
// such kernel.  The first generation (kernels_solve.hip): solve, step, stepc per SolveMember (nr_dense_mfma / nr_sparse_lds: none,
// they launch the gs_k_*_nr_dmfma kernels below around their solver); the second (kernels_flow2.hip): per StepMember, step and
// stepc of each of its forms.  A form is an index, not a type: every second-generation step kernel has the one signature
// GsF2StepFn, whose two trailing pointers are the per-instance line impedances (pz) and load powers (pl); a form reads the ones
// it is built for and is launched with null for the others.
typedef void (*GsSolveFn)(GsTables T, GsRows R, GsSolveCfg C, double* slab, int B);
typedef void (*GsStepFn)(GsTables T, GsRows R, GsSolveCfg C, GsEnvCfg E, double* slab, int B, const double* actions, double total_load,
                         GsPackArgs PA, GsFusedChecks FC);
typedef void (*GsF2StepFn)(GsTables T, GsF2Tables F, GsRows R, GsSolveCfg C, GsEnvCfg E, double* slab, int B, const double* actions,
                           double total_load, GsPackArgs PA, GsFusedChecks FC, GsRolloutStep RS, const double* pz, const double* pl);
template <class Fn> struct GsStepFns { Fn step = nullptr, stepc = nullptr; };      // the plain step and the step with the checks
struct GsSolveKernels { GsSolveFn solve; GsStepFns<GsStepFn> step; };
// form[pz][pl]: the kernels that read per-instance line impedances (pz = 1) and / or per-instance load powers (pl = 1);
// {nullptr, nullptr} where the member has no such form
struct GsStepKernels { GsStepFns<GsF2StepFn> form[2][2]; };
extern const std::array<GsSolveKernels, (size_t)SolveMember::nr_sparse_lds + 1> gs_solve_kernels;
extern const std::array<GsStepKernels, kStepMemberCount> gs_step_kernels;

extern "C" {
__global__ void gs_k_line_params(GsLineParamArgs A);
__global__ void gs_k_load_params(GsLoadParamArgs A);
__global__ void gs_k_load_columns(const double* __restrict__ pl, double* __restrict__ out, int B, int obs_dim, int c0, int n_loads);
__global__ void gs_k_pre_nr_dmfma(GsTables T, GsRows R, GsSolveCfg C, GsEnvCfg E, double* __restrict__ slab, int B,
                                  const double* __restrict__ actions, double total_load, GsPackArgs PA, GsFusedChecks FC);
__global__ void gs_k_post_nr_dmfma(GsTables T, GsRows R, GsSolveCfg C, GsEnvCfg E, double* __restrict__ slab, int B,
                                   const double* __restrict__ actions, double total_load, GsPackArgs PA, GsFusedChecks FC);
__global__ void gs_k_postc_nr_dmfma(GsTables T, GsRows R, GsSolveCfg C, GsEnvCfg E, double* __restrict__ slab, int B,
                                    const double* __restrict__ actions, double total_load, GsPackArgs PA, GsFusedChecks FC);
__global__ void gs_k_posts_nr_dmfma(GsTables T, GsRows R, GsSolveCfg C, double* __restrict__ slab, int B);
__global__ void gs_k_nr_dense_mfma(GsDenseArgs A, double* __restrict__ slab, int B);
__global__ void gs_k_nr_dense_mfma2(GsDenseArgs A, double* __restrict__ slab, int B);
__global__ void gs_k_nr_sparse_lds(GsSparseArgs A, double* __restrict__ slab, int B);
__global__ void gs_k_env_reset(GsTables T, GsRows R, GsEnvCfg E, double* __restrict__ slab, int B,
                               const uint64_t* __restrict__ seeds, const uint8_t* __restrict__ mask);
__global__ void gs_k_polar_to_rect(GsTables T, GsRows R, double* __restrict__ slab, int B);
__global__ void gs_k_rollout_actions(double* __restrict__ act, int T, int B, int A, uint64_t seed, int64_t first_instance, uint32_t t0);
__global__ void gs_k_fill_const_columns(double* __restrict__ out, long long rows, int obs_dim, int skip0, int skip1,
                                        const int32_t* __restrict__ map, const double* __restrict__ cst);
__global__ void gs_k_policy_mlp(GsPolicyArgs P);
__global__ void gs_k_policy_mlp_f32(GsPolicyArgsF32 P);
__global__ void gs_k_value_mlp_f32(GsValueArgs P);
__global__ void gs_k_gae(GsGaeArgs G);
__global__ void gs_k_costs(GsCostArgs A);
__global__ void gs_k_ep_count(GsEpisodeArgs E);
__global__ void gs_k_ep_offsets(GsEpisodeArgs E);
__global__ void gs_k_ep_accumulate(GsEpisodeArgs E);
__global__ void gs_k_ep_accumulate_costs(GsEpisodeArgs E);
__global__ void gs_k_ep_stats(GsEpisodeArgs E);
__global__ void gs_k_opb_combine(GsOpbCombineArgs A);
__global__ void gs_k_opb_index(GsOpbIndexArgs A);
__global__ void gs_k_opb_mbstats(const double* __restrict__ stage, int n, double* __restrict__ adv_stats);
__global__ void gs_k_opb_gather_f64(GsOpbGatherArgs G);
__global__ void gs_k_opb_gather_f32(GsOpbGatherArgs G);
__global__ void gs_k_train_forward(GsTrainFwdArgs P);
__global__ void gs_k_train_head(GsTrainHeadArgs H);
__global__ void gs_k_train_bwd_data(GsTrainBwdArgs P);
__global__ void gs_k_train_grad(GsTrainGradArgs P);
__global__ void gs_k_train_reduce(GsTrainReduceArgs A);
__global__ void gs_k_train_stats(GsTrainStatArgs S);
__global__ void gs_k_train_adam(GsTrainAdamArgs A);
__global__ void gs_k_train_head_awr(GsTrainAwrHeadArgs H);
__global__ void gs_k_train_head_expectile(GsTrainExpectileArgs H);
__global__ void gs_k_train_stats_awr(GsTrainAwrStatArgs S);
__global__ void gs_k_q_mlp_f32(GsQArgs P);
__global__ void gs_k_q_mlp_rows_f32(GsQArgs P, const int32_t* rows_dev);
__global__ void gs_k_policy_rows_f32(GsPolicyRowsArgs P);
__global__ void gs_k_q_next_td(GsQNextTdArgs G);
__global__ void gs_k_q_combine(GsQCombineArgs C);
__global__ void gs_k_q_td(GsQTdArgs G);
__global__ void gs_k_q_gather(GsQGatherArgs G);
__global__ void gs_k_q_polyak(GsQPolyakArgs A);
__global__ void gs_k_pw_sample(GsPwSampleArgs S);
__global__ void gs_k_pw_rows(GsPwRowsArgs R);
__global__ void gs_k_pw_seed(GsPwSeedArgs S);
__global__ void gs_k_pw_input_grad(GsPwInputGradArgs P);
__global__ void gs_k_pw_head(GsPwHeadArgs H);
__global__ void gs_k_pw_stats(GsPwStatArgs S);
__global__ void gs_k_cql_rows(GsCqlRowsArgs R);
__global__ void gs_k_cql_lse(GsCqlLseArgs L);
__global__ void gs_k_cql_head(GsCqlHeadArgs H);
__global__ void gs_k_cql_stats(GsCqlStatArgs S);
__global__ void gs_k_train_anchor(GsAnchorArgs A);
__global__ void gs_k_train_grad_sq(GsTrainGradArgs P);
__global__ void gs_k_fisher_accumulate(GsFisherAccArgs A);
__global__ void gs_k_fisher_commit(GsFisherCommitArgs C);
__global__ void gs_k_refresh_terms(GsRefreshTermsArgs G);
__global__ void gs_k_refresh_rows(GsRefreshRowsArgs G);
__global__ void gs_k_refresh_td_policy(GsRefreshTdPolicyArgs G);
__global__ void gs_k_refresh_td_value(GsRefreshTdValueArgs G);
__global__ void gs_k_refresh_combine(GsRefreshCombineArgs C);
__global__ void gs_k_load_widen(const float* __restrict__ src, double* __restrict__ dst, long long n);
__global__ void gs_k_load_next_f64(GsLoadNextArgs G);
__global__ void gs_k_load_next_f32(GsLoadNextArgs G);
__global__ void gs_k_window_shift(GsWindowShiftArgs G);
__global__ void gs_k_window_terms(GsWindowTermsArgs G);
__global__ void gs_k_window_term_rows(GsWindowTermRowsArgs G);
__global__ void gs_k_ds_chunk_stats(GsDsStatArgs A);
__global__ void gs_k_ds_merge(double* __restrict__ part, long long chunks, int Ct, long long stride, long long N,
                              const GsDsMatrix m0, const GsDsMatrix m1, const GsDsMatrix m2, double* __restrict__ fin_mean, double* __restrict__ fin_std);
__global__ void gs_k_ds_map_fill(int32_t* __restrict__ map, long long n);
__global__ void gs_k_ds_map_scatter(int32_t* __restrict__ map, const int32_t* __restrict__ term_count, const int32_t* __restrict__ term_idx,
                                    int term_cap, int T, int B);
__global__ void gs_k_ds_draw(int32_t* __restrict__ idx, int n, long long N, uint64_t seed, uint64_t draw);
__global__ void gs_k_ds_gather_f64(GsDsGatherArgs G);
__global__ void gs_k_ds_gather_f32(GsDsGatherArgs G);
__global__ void gs_k_rollout_post(GsTables T, GsRows R, GsEnvCfg E, double* __restrict__ slab, GsRolloutPostArgs A);
__global__ void gs_k_pack(const int32_t* __restrict__ src, const double* __restrict__ cst, int C, int rows_total,
                          const double* __restrict__ slab, double* __restrict__ out, int B);
__global__ void gs_k_unpack(const int32_t* __restrict__ dst, int C, int rows_total, double* __restrict__ slab,
                            const double* __restrict__ in, int B, int stride);
__global__ void gs_k_obs_compact(const double* __restrict__ src, double* __restrict__ dst, long long rows, int D, int skip0, int skip1, int expand);
__global__ void gs_k_obs_to_f32(const double* __restrict__ src, float* __restrict__ dst, long long n);
__global__ void gs_k_gather_lane(int row0, int count, int lane, const double* __restrict__ slab, double* __restrict__ out);
__global__ void gs_k_fill_rows(int row0, int stride, int count, int rows_total, double* __restrict__ slab, double value);
__global__ void gs_k_scalars(const int32_t* __restrict__ rf, int nf, const int32_t* __restrict__ ri, int ni,
                             const int32_t* __restrict__ ru, int nu, int rows_total, const double* __restrict__ slab,
                             double* __restrict__ of, int32_t* __restrict__ oi, uint8_t* __restrict__ ou, int Bp, uint32_t* __restrict__ ov4, int vf0);
__global__ void gs_k_checks(GsChecksCfg C, const double* __restrict__ slab, const double* __restrict__ freq_override,
                            double* __restrict__ prev, int32_t* __restrict__ state, int32_t* __restrict__ out_i,
                            double* __restrict__ out_f, uint8_t* __restrict__ bus_mask, uint8_t* __restrict__ line_mask, int B, int Bp);
__global__ void gs_k_fallback_linear(GsTables T, GsRows R, GsFallbackArgs A, double* __restrict__ slab, int B);
__global__ void gs_k_checks_reset(int32_t* __restrict__ state, const uint8_t* __restrict__ mask, int B, int Bp);
}
