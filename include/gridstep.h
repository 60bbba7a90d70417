/* gridstep.h -- C ABI of libgridstep.so: MI355X-native batched AC power flow + env.step().
 *
 * This is the drop-in boundary for the hot path of danieleschmidt/grid-fed-rl-gym.  The
 * reference has no FFI layer: the path sits behind two duck-typed Python plug points, and
 * each entry point below names the reference interface it replaces (file:line relative to
 * /root/reference/grid_fed_rl/).  The Python binding a maintainer would add is a ctypes
 * stub; grid_fed_rl_gym_amd/_lib.py is that stub.
 *
 * Conventions
 *  - plain pointers and sizes only; every array is caller-owned, dense, C order, float64
 *    unless stated; batch axis first:  P_spec[B][n], obs[B][obs_dim], actions[B][action_dim].
 *  - every function returns 0 (GS_OK) or a negative GS_E* code; gs_last_error() gives text.
 *  - per-INSTANCE numerical failure never fails the call: it sets status[b]
 *    (0 converged, 1 iteration cap, 2 singular Jacobian, 3 non-finite mismatch), mirroring
 *    the reference's "return converged=False" convention (environments/power_flow.py:186-190).
 *  - one handle = one device = one HIP stream.  A handle is not thread-safe; distinct
 *    handles are independent.
 *  - there is no CPU fallback: gs_create fails with GS_E_NO_DEVICE when no GPU is present.
 */
#ifndef GRIDSTEP_H
#define GRIDSTEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 2

enum {
  GS_OK = 0,
  GS_E_INVALID = -1,     /* bad argument / shape / enum value                       */
  GS_E_NO_DEVICE = -2,   /* no HIP device, or device index out of range             */
  GS_E_HIP = -3,         /* a HIP runtime call failed                               */
  GS_E_TOPOLOGY = -4,    /* network unusable for the requested solver (e.g. FBS on a mesh) */
  GS_E_STATE = -5,       /* call sequence error (e.g. step before reset)            */
  GS_E_COMM = -6,        /* RCCL not loadable / communicator failure                */
  GS_E_NOMEM = -7
};

enum { GS_BUS_PQ = 0, GS_BUS_PV = 1, GS_BUS_SLACK = 2 };          /* base.py:210 bus_type   */
enum { GS_JACOBIAN_AS_CODED = 0, GS_JACOBIAN_EXACT = 1 };         /* power_flow.py:247-248  */
enum { GS_ZERO_Z_OPEN = 0, GS_ZERO_Z_EPSILON = 1 };               /* power_flow.py:63       */
enum { GS_SOLVER_NR = 0, GS_SOLVER_FBS = 1 };
/* AUTO: exact Jacobian -> TREE on radial networks, SPARSE_LU on meshed ones (2x2-block pivots,
 * no row exchanges: safe because the exact diagonal blocks are rotation-like);
 * as-coded Jacobian -> DENSE_PIVOT (partial pivoting like LAPACK dgesv, power_flow.py:187),
 * because the as-coded diagonal blocks can be exactly singular (e.g. a leaf fed through r = x). */
enum { GS_LINSOLVE_AUTO = 0, GS_LINSOLVE_TREE = 1, GS_LINSOLVE_SPARSE_LU = 2, GS_LINSOLVE_DENSE_PIVOT = 3,
       /* dense block LU on the matrix cores, one workgroup per instance (exact Jacobian, at most 128 non-slack buses);
        * what AUTO takes for a meshed network whose sparse LU would fill in (more than a quarter of all blocks) */
       GS_LINSOLVE_DENSE_MFMA = 4,
       /* sparse 2x2-block LU with all blocks of an instance in LDS, one wavefront per instance (meshed networks of at most 256
        * buses whose blocks fit 32 KB).  An alternative to SPARSE_LU that moves 1/20 of its bytes and is slower on the feeders
        * measured: never AUTO's choice */
       GS_LINSOLVE_SPARSE_LDS = 5 };
enum { GS_GEN_SOLAR = 0, GS_GEN_WIND = 1 };
enum { GS_STATUS_OK = 0, GS_STATUS_MAX_ITER = 1, GS_STATUS_SINGULAR = 2, GS_STATUS_NAN = 3,
       GS_STATUS_FALLBACK_LINEAR = 4 /* answer replaced by gs_fallback_linear; converged = 1 as the reference's linear solver reports */ };

/* Network + devices, flattened.  Replaces the Bus/Line/Load object lists the reference
 * passes to solve() (environments/base.py:197-295, power_flow.py:38-46) and the feeder
 * containers (feeders/base.py:44-47).  Bus references are 0-based list positions (the
 * reference's bus_map, power_flow.py:54). */
typedef struct gs_topology {
  int32_t struct_size;            /* = sizeof(gs_topology) */
  int32_t n, m;
  const int32_t* from_bus;        /* [m] */
  const int32_t* to_bus;          /* [m] */
  const double* r;                /* [m] per unit */
  const double* x;                /* [m] per unit */
  const double* rating;           /* [m] VA, as the reference stores it */
  const uint8_t* bus_type;        /* [n] GS_BUS_* */
  const double* v_set;            /* [n] magnitude set-point of slack / pv buses */
  int32_t n_loads;
  const int32_t* load_bus;        /* [n_loads] */
  const double* load_base;        /* [n_loads] base_power (base.py:280) */
  const double* load_pf;          /* [n_loads] power factor (base.py:281) */
  int32_t n_gens;
  const int32_t* gen_bus;         /* [n_gens] */
  const int32_t* gen_kind;        /* [n_gens] GS_GEN_* */
  const double* gen_cap;          /* [n_gens] capacity */
  const double* gen_p0;           /* solar: efficiency   | wind: cut-in speed  (dynamics.py:116,150) */
  const double* gen_p1;           /* solar: panel area   | wind: rated speed   */
  const double* gen_p2;           /* solar: unused       | wind: cut-out speed */
  int32_t n_bats;
  const int32_t* bat_bus;         /* [n_bats] injection bus (reference hard-codes id 2, grid_env.py:714) */
  const double* bat_cap;          /* [n_bats] dynamics.py:178 */
  const double* bat_rating;       /* [n_bats] dynamics.py:179 */
  const double* bat_eff;          /* [n_bats] dynamics.py:180 */
  /* Per-instance line impedances (domain randomisation of the network): [batch][m] per unit, or both NULL.  Both non-NULL makes a
   * per-instance-impedance handle: instance b solves on its own Ybus (power_flow.py:48-73) and reports its own line flows
   * (:329-358), built from line_r_inst[b] / line_x_inst[b]; exactly one non-NULL is GS_E_INVALID.  r / x above stay mandatory:
   * they define the topology and which lines are zero-impedance.  Every value must be finite with r >= 0; a line whose nominal
   * hypot(r, x) <= 1e-12 must keep its nominal values in every instance (it keeps its open-circuit / epsilon treatment,
   * power_flow.py:63), every other line needs hypot(r, x) > 1e-12 -- so islanding never depends on the instance.  Only a
   * second-generation radial step member serves such a handle (gs_describe "kernel": fbs_flow2s / fbs_flow2h / fbs_flow2x /
   * nr_flow2s / nr_flow2, "per_instance_z": 1); anything else is GS_E_TOPOLOGY.  gs_solve / gs_solve_device are GS_E_STATE on it. */
  const double* line_r_inst;
  const double* line_x_inst;
  /* Per-instance load powers (domain randomisation of the loading): [batch][n_loads] watts, or NULL.  Non-NULL makes a
   * per-instance-loads handle: instance b behaves as the reference environment whose loads have base_power = load_base_inst[b][l] --
   * its realised load powers (dynamics.py:54-75, into the injections of grid_env.py:683-720), the sum of load.active_power in its
   * frequency update (grid_env.py:744) and the static [P_l, Q_l] columns of its observation (grid_env.py:769-770, Q_l = P_l *
   * tan(acos(load_pf[l])) with the shared power factor) all follow the instance.  load_base above stays mandatory (the nominal
   * values).  Every value must be finite and >= 0, and n_loads > 0 (GS_E_INVALID).  Only a second-generation step member serves
   * such a handle (gs_describe "kernel": fbs_flow2s / fbs_flow2h / fbs_flow2x / nr_flow2s / nr_flow2 / nr_mesh2,
   * "per_instance_loads": 1); anything else is GS_E_TOPOLOGY.  Combines with line_r_inst / line_x_inst on the radial members. */
  const double* load_base_inst;
} gs_topology;

/* Solver + environment configuration.  Replaces the constructor kwargs of
 * NewtonRaphsonSolver (power_flow.py:79-87) and GridEnvironment (grid_env.py:161-174) and
 * GridDynamics (dynamics.py:233-238). */
typedef struct gs_config {
  int32_t struct_size;            /* = sizeof(gs_config) */
  int32_t solver_kind;            /* GS_SOLVER_* */
  int32_t jacobian_mode;          /* GS_JACOBIAN_* */
  int32_t zero_z_mode;            /* GS_ZERO_Z_* */
  int32_t linear_solver;          /* GS_LINSOLVE_* */
  int32_t max_iterations;         /* power_flow.py:82 (default 50) */
  int32_t episode_length;         /* grid_env.py:165 */
  int32_t stochastic_loads;       /* grid_env.py:166 (Philox stream) */
  int32_t weather_variation;      /* grid_env.py:168 */
  int32_t waves_per_group;        /* 0 = auto; 1,2,4,8,16: waves cooperating on one 64-instance group */
  int32_t fbs_warm_start;         /* 0 (default): every step solves from the flat start, as the reference's solve() does
                                     (power_flow.py:125-134); 1: the sweep solver starts from the previous step's voltages --
                                     same tolerance, fewer sweeps; an option, never the measured headline */
  double tolerance;               /* power_flow.py:81 (default 1e-6).  Sweep solver: the summed mismatch is held against
                                     tolerance / 2; below 1e-10 a handle runs the first-generation sweep kernels (double-precision
                                     comparison; the second generation keeps the sum in 2^-44 pu fixed point), gs_describe says so */
  double acceleration_factor;     /* power_flow.py:83 (default 1.0) */
  double timestep;                /* grid_env.py:164 */
  double v_min, v_max;            /* grid_env.py:170 */
  double f_min, f_max;            /* grid_env.py:171 */
  double safety_penalty;          /* grid_env.py:172 */
  double inertia_H, damping_D, f_nominal;   /* dynamics.py:235-237 */
  double power_base;              /* injections are divided by this before the solve; 1.0 = as coded (F4) */
} gs_config;

/* Host destination pointers for one batched solution; any pointer may be NULL (skipped).
 * Field-for-field the reference's PowerFlowSolution (power_flow.py:12-22) with a batch axis. */
typedef struct gs_solution_view {
  double* bus_voltages;           /* [B][n] */
  double* bus_angles;             /* [B][n] rad, wrapped to (-pi, pi] like np.angle */
  double* line_flows;             /* [B][m] P from->to */
  double* line_loadings;          /* [B][m] |S|/rating */
  double* losses;                 /* [B] */
  double* max_mismatch;           /* [B] */
  int32_t* iterations;            /* [B] last loop index + 1 (power_flow.py:204) */
  uint8_t* converged;             /* [B] */
  int32_t* status;                /* [B] GS_STATUS_* */
} gs_solution_view;

/* Host destination pointers for the per-step info dict (grid_env.py:610-617); NULLs skipped. */
typedef struct gs_info_view {
  uint8_t* power_flow_converged;  /* [B] */
  double* max_voltage;            /* [B] */
  double* min_voltage;            /* [B] */
  double* total_losses;           /* [B] solution.losses of this step */
  uint8_t* violations;            /* [B][4] voltage_high, voltage_low, frequency_high, frequency_low (base.py:153-167) */
  int32_t* constraint_violations; /* [B] running count (grid_env.py:586) */
  int32_t* current_step;          /* [B] */
  double* episode_reward;         /* [B] */
  int32_t* iterations;            /* [B] */
  int32_t* status;                /* [B] */
} gs_info_view;

typedef struct gs_handle gs_handle;

/* ---- library ------------------------------------------------------------------------- */
int gs_version(void);
/* 1 if the library was built with `make EXPERIMENTS=1`: the kernel members and environment switches that exist to measure
 * alternatives (linear_solver sparse_lds, the 32-instance sweep member, table-layout and launch-shape switches) are present.
 * The default build carries what AUTO can reach and the switches the parity tests compare handles with (csrc/gs_internal.h). */
int gs_build_experiments(void);
int gs_device_count(void);
/* text of the last error on this thread (handle may be NULL for creation errors) */
const char* gs_last_error(const gs_handle* h);

/* ---- lifetime ------------------------------------------------------------------------ */
/* Compiles the topology (Ybus CSR, elimination schedule), allocates all device memory for
 * `batch` instances on `device`.  Replaces solver/env construction (power_flow.py:79,
 * grid_env.py:161-241).  `first_instance` is the global index of this handle's instance 0
 * (rank * B_local when a batch is sharded over GPUs); it only feeds the RNG counters. */
int gs_create(const gs_topology* topo, const gs_config* cfg, int32_t batch, int32_t device,
              int64_t first_instance, gs_handle** out);
void gs_destroy(gs_handle* h);
int gs_dims(const gs_handle* h, int32_t* n, int32_t* m, int32_t* obs_dim, int32_t* action_dim,
            int32_t* state_dim, int32_t* batch);
/* how the topology was compiled: linear solver chosen, tree depth, fill, waves per group; "flow2" / "mesh2": "on", or why the
 * second-generation member does not take the handle (a network with a bus that has no path to the slack: "island without a path
 * to the slack" -- it stays with a kernel that tests every pivot and reports GS_STATUS_SINGULAR) */
int gs_describe(const gs_handle* h, char* buf, int32_t buflen);
/* the same JSON for a handle that gs_create would build from these arguments on a device of `cus` compute units, planned on the
 * host alone (no device needed; the GS_* switches as for gs_create) */
int gs_plan_describe(const gs_topology* topo, const gs_config* cfg, int32_t batch, int32_t cus, char* buf, int32_t buflen);
int gs_synchronize(gs_handle* h);
/* Per-instance line impedances of a handle created with gs_topology::line_r_inst / line_x_inst (else GS_E_STATE): r / x [B][m] per
 * unit, mask [B] (!= 0: take this instance's row) or NULL (all).  The selected instances solve on the new values from the next
 * gs_step / rollout step on; the rules of gs_topology apply (GS_E_INVALID, handle unchanged).  The values are not environment
 * state: gs_reset, the in-place resets of gs_rollout and gs_set_state leave them alone. */
int gs_set_line_impedances(gs_handle* h, const double* r, const double* x, const uint8_t* mask);
/* the values the handle holds, [B][m] each (either pointer may be NULL); GS_E_STATE on a handle without per-instance impedances */
int gs_get_line_impedances(const gs_handle* h, double* r, double* x);
/* Per-instance load powers of a handle created with gs_topology::load_base_inst (else GS_E_STATE): base [B][n_loads] watts, mask [B]
 * (!= 0: take this instance's row) or NULL (all).  The selected instances draw, sum and report the new values from the next gs_step /
 * rollout step on (grid_env.py:683-720, 744, 769-770); the rules of gs_topology apply (GS_E_INVALID, handle unchanged).  The values
 * are not environment state: gs_reset, the in-place resets of gs_rollout and gs_set_state leave them alone. */
int gs_set_load_powers(gs_handle* h, const double* base, const uint8_t* mask);
/* the values the handle holds, [B][n_loads]; GS_E_STATE on a handle without per-instance load powers */
int gs_get_load_powers(const gs_handle* h, double* base);

/* ---- solver plug point: NewtonRaphsonSolver.solve (power_flow.py:89-211) ---------------
 * P_spec[B][n] is the net specified injection (generation - load, what :112-121 builds from
 * the two dicts); Q_spec may be NULL (the reference never injects reactive power, :107). */
int gs_solve(gs_handle* h, const double* P_spec, const double* Q_spec, const gs_solution_view* out);
/* device-resident variant for measurement: upload once, solve many times, download once */
int gs_upload_injections(gs_handle* h, const double* P_spec, const double* Q_spec);
int gs_solve_device(gs_handle* h);
int gs_download_solution(gs_handle* h, const gs_solution_view* out);

/* ---- fallback for rejected load flows: LinearApproximationSolver.solve (robust_power_flow.py:336-398), the
 * "linear_approximation" stage of AdvancedRobustPowerFlowSolver.solve (:523-613) ------------------------------
 * Overwrites the solution rows (voltages, angles, flows, loadings, losses, converged = 1, iterations = 1,
 * max_mismatch = 0, status = GS_STATUS_FALLBACK_LINEAR) of the instances selected by mask[B] (!= 0), or, with
 * mask == NULL, of the instances whose last solve / step did not converge; every other instance keeps its rows.
 * load_w / gen_w: [B][n] totals of the reference's `loads` / `generation` dicts per bus (0 = no entry), in the
 * reference's units (W); both NULL = take them from the environment state on the device (load powers, curtailed
 * renewables, battery powers: grid_env.py:683-720).  total_load / total_gen: [B] sums of the dict values in the
 * caller's dict order, or NULL = summed over the buses in index order (host arrays) / in the order the
 * reference's dicts are filled (device state).  applied_out: NULL or [B], 1 where the answer was replaced;
 * n_applied: NULL or their count.  Follow with gs_download_solution / gs_checks_run / gs_download_step as usual.
 * On a per-instance-impedance handle every instance's angles use its own line reactances (gs_set_line_impedances). */
int gs_fallback_linear(gs_handle* h, const double* load_w, const double* gen_w, const double* total_load,
                       const double* total_gen, const uint8_t* mask, uint8_t* applied_out, int32_t* n_applied);

/* ---- env plug point: GridEnvironment.reset/step (grid_env.py:360-408, 410-619) and their
 * batched form VectorizedEnvironment.reset/step (utils/parallel_environment.py:309-355) --- */
/* seeds: [B] per-instance RNG seeds, or NULL = the stream runs on, as the reference's reset(seed=None) leaves its
 * global generators running (grid_env.py:366-369): every reset instance gets the next seed of its chain, one Philox
 * call keyed by the seed it holds (0 on a fresh handle) with counter (global instance, 0, 'RSED') -- so consecutive
 * episodes differ while gs_reset(seeds) stays exactly reproducible; mask: NULL (all) or [B] (reset where != 0);
 * obs_out: NULL or [B][obs_dim]. */
int gs_reset(gs_handle* h, const uint64_t* seeds, const uint8_t* mask, double* obs_out);
int gs_step(gs_handle* h, const double* actions, double* obs, double* reward,
            uint8_t* terminated, uint8_t* truncated, const gs_info_view* info);
/* Page-locked host memory for the arrays gs_step / gs_download_step / gs_reset / gs_rollout_download fill.  The reference's
 * step() returns fresh NumPy arrays every call (grid_env.py:563-619); at [8192][684] doubles that is 45 MB of first-touch
 * page faults plus a staged copy per step.  A caller that hands gs_step buffers from gs_host_alloc gets the copy at the
 * link's rate and asynchronously (measured: DESIGN.md section 5, `with_host_io`).  Plain host allocations, owned by the
 * caller: gs_host_free releases them; they outlive any handle. */
int gs_host_alloc(void** out, size_t bytes);
int gs_host_free(void* p);

/* device-resident variant: K action batches [K][B][action_dim] staged in HBM, stepped by index */
int gs_upload_actions(gs_handle* h, const double* actions, int32_t n_batches);
int gs_step_device(gs_handle* h, int32_t action_batch_index);
int gs_download_step(gs_handle* h, double* obs, double* reward, uint8_t* terminated,
                     uint8_t* truncated, const gs_info_view* info);
/* The same with the observation block as FLOAT32 [B][obs_dim] -- the dtype the reference declares for its observation space
 * (grid_env.py:346, `Box(..., dtype=np.float32)`; the values its step() returns are Python floats, which is what gs_step hands out).
 * Rounded to nearest on the device; every other output as in gs_step / gs_download_step.  Opt-in: half the bytes over the link. */
int gs_step_f32(gs_handle* h, const double* actions, float* obs, double* reward, uint8_t* terminated,
                uint8_t* truncated, const gs_info_view* info);
int gs_download_step_f32(gs_handle* h, float* obs, double* reward, uint8_t* terminated,
                         uint8_t* truncated, const gs_info_view* info);
/* Host observation arrays that are handed to gs_step / gs_download_step again and again (the recycled page-locked sets of the
 * Python environment): gs_host_obs_bind writes the constant columns of the observation -- the static load powers of
 * grid_env.py:769-770, a third of the row on the 123-bus feeder -- into `obs` once and remembers the address; later downloads
 * into that address move the changing columns only (one pitched copy: in memory order the changing columns of row r behind the
 * constants and those of row r + 1 in front of them are one run), the same bytes as a whole-row download would leave.
 * The caller must not modify the constant columns of a bound array (bind again if it did).  After gs_reset. */
int gs_host_obs_bind(gs_handle* h, double* obs);
int gs_host_obs_unbind(gs_handle* h, double* obs);

/* A consumer that lives on the same GPU (a policy network) steps the environment without any host copy: it reads the
 * observation block and the reward / flag arrays through device pointers and hands back a device pointer to its actions.
 * Streams are passed as `hipStream_t` cast to `void*`; NULL means "the caller synchronises itself"; the legacy default
 * stream (handle 0 -- PyTorch's current stream unless the caller created one) is passed as hipStreamLegacy, (void*)1.
 *   gs_step_device_ptr   one env step with actions[B][action_dim] (float64, C order) in DEVICE memory of the handle's GPU; when
 *                        `producer_stream` is given, the step waits (on the device) for the work queued on it so far.
 *   gs_step_device_view  device pointers to what the last step left: observations[B][obs_dim] (one of the handle's two
 *                        observation buffers: valid until the next-but-one step), reward[B], terminated[B], truncated[B]
 *                        (refreshed by this call; valid until the next call); when `consumer_stream` is given it is made to
 *                        wait (on the device) for the step, otherwise the call returns after the step has finished. */
typedef struct gs_step_device_out {
  double* observations;
  double* reward;
  uint8_t* terminated;
  uint8_t* truncated;
  int32_t B, obs_dim;
} gs_step_device_out;
int gs_step_device_ptr(gs_handle* h, const double* d_actions, void* producer_stream);
int gs_step_device_view(gs_handle* h, gs_step_device_out* out, void* consumer_stream);

/* ---- device-resident rollout collection: collect_random_data(env, num_steps) and the five arrays GridDataset is
 * built from (algorithms/base.py:268-298, 180-205) ------------------------------------------------------------
 * T env steps back to back on the device -- no host round trip between them: the step kernel of step t writes its
 * observation block straight into slot t + 1 of obs_seq[T + 1][B][obs_dim], a small kernel behind it files reward and
 * done flags and resets the instances that finished (terminated or truncated) in place, exactly where the reference
 * calls env.reset() (base.py:289-290); their seed is the next one of the instance's chain (see gs_reset).
 * policy: GS_POLICY_RANDOM -- uniform actions in (-1, 1) drawn on the device (the reference samples
 * env.action_space; here Philox keyed by policy_seed, counter (global instance, t, action / 4, 'ACTN'), word k of a
 * call = action 4 q + k = 2 (r + 1/2) 2^-32 - 1); GS_POLICY_UPLOADED -- actions[T][B][action_dim] from the caller.
 * The call is asynchronous; the environment afterwards stands where T calls of gs_step (+ resets) would have left it. */
enum { GS_POLICY_UPLOADED = 0, GS_POLICY_RANDOM = 1 };
int gs_rollout(gs_handle* h, int32_t T, int32_t policy, uint64_t policy_seed, const double* actions);
/* host copies in the reference's layout, transition index = t * B + b; any pointer may be NULL */
typedef struct gs_rollout_view {
  double* observations;           /* [T][B][obs_dim] what each step started from */
  double* actions;                /* [T][B][action_dim] */
  double* rewards;                /* [T][B] */
  double* next_observations;      /* [T][B][obs_dim] (the terminal observation where the transition ended an episode) */
  uint8_t* terminals;             /* [T][B] bit 0 terminated, bit 1 truncated; != 0 is the reference's `terminated or truncated` */
  double* final_observation;      /* [B][obs_dim] what step T would start from */
  int32_t* n_terminal;            /* [1] number of finished episodes in the rollout */
} gs_rollout_view;
int gs_rollout_download(gs_handle* h, const gs_rollout_view* out);
/* the same data where it lies, for a consumer on the GPU (valid until the next gs_rollout on the handle; waits for the
 * rollout to finish).  observations = obs_seq[0 .. T-1], next_observations = obs_seq[1 .. T] except for the n_terminal
 * transitions (t, b) = terminal_index[k], whose next observation is terminal_obs[k] (obs_seq[t + 1][b] being the fresh
 * observation after the reset). */
typedef struct gs_rollout_device {
  int32_t T, B, obs_dim, action_dim;
  const double* obs_seq;          /* [T + 1][B][obs_dim] */
  const double* actions;          /* [T][B][action_dim] */
  const double* rewards;          /* [T][B] */
  const uint8_t* terminals;       /* [T][B] */
  int32_t n_terminal, reserved;
  const int32_t* terminal_index;  /* [n_terminal][2] (t, b), in no particular order */
  const double* terminal_obs;     /* [n_terminal][obs_dim] */
} gs_rollout_device;
int gs_rollout_device_view(gs_handle* h, gs_rollout_device* out);

/* ---- a recorded dataset as the handle's rollout: the inverse of gs_rollout_download -------------
 * GridDataset(observations, actions, rewards, next_observations, terminals) (algorithms/base.py:180-205) takes five arrays from
 * anywhere.  gs_rollout_load installs such arrays -- host memory, transition index = t * B + b, B / obs_dim / action_dim the
 * handle's -- as the handle's rollout: the state is what a gs_rollout would have left had it produced these transitions, and every
 * entry that reads "the last rollout" (gs_dataset_*, gs_rollout_evaluate*, gs_rollout_costs, gs_rollout_episodes, gs_onpolicy_*,
 * gs_learner_*, gs_learner_refresh, gs_fed_*) runs on them unchanged.
 *   obs_seq[t] = observations[t], obs_seq[T] = final_observation (NULL: next_observations[T - 1]); actions, rewards and flags as
 *   given; every transition with terminals != 0 has an entry in the terminal list with its next_observations row, the list in
 *   ASCENDING t * B + b order (deterministic, where gs_rollout promises no particular order); log-probabilities count as recorded
 *   exactly when log_probs is given.  The rollout counts as a new one: whatever was computed over the previous one (critic values, Q
 *   arrays, policy-action targets, costs, the episode list, the dataset's map, the refresh map, prepared minibatches) is stale by the
 *   gates those entries have; installed dataset statistics stay, as after gs_rollout.
 *   The ENVIRONMENT is not touched -- state, current observation, random chains, whether it was reset -- and a handle that was never
 *   reset may load.  The next gs_rollout puts the constant observation columns back before it steps.
 * Continuity: a transition with terminals == 0 has no room for a next observation of its own, so next_observations[t][b] must equal
 * observations[t + 1][b] (t < T - 1) or, with final_observation given, final_observation[b] (t = T - 1) -- by the BITS of the source
 * element (a NaN equals the same NaN; float32 sources are compared after their exact widening, which tells all values apart and
 * every NaN but a signalling from the quiet one of its payload).  Checked on the device while next_observations streams through:
 * GS_E_INVALID with the number of offending transitions and the first one's (t, b) in ascending order, and the handle then holds NO
 * rollout (as before its first gs_rollout), never half of one.  Observations are not tested for finiteness: the simulator itself
 * records NaN rows for unsolved instances.
 * GS_E_INVALID before anything is allocated or launched (gs_rollout_load_check: the same checks on the host alone, no handle, no
 * device): a wrong struct_size, an unknown dtype, T <= 0, chunk_rows < 0, non-zero flags, a NULL required pointer, T * B beyond what
 * int32 row indices hold, a terminals value above 3.  out (may be NULL): n = T * B, n_terminal, and the capacity of the terminal
 * list the load needs (a recorded dataset may end an episode at every transition; gs_rollout's own bound is B (T / min(episode_length,
 * 11) + 1)).
 * The source is staged through two page-locked buffers of chunk_rows rows of next_observations (0: the library's choice, 16 MiB),
 * the copy of one chunk under the kernel of the one before; next_observations is never resident as a whole.  float32 sources are
 * widened once, exactly.  The call synchronises before it returns: the source arrays are the caller's again. */
typedef struct gs_rollout_source {
  int32_t struct_size;            /* = sizeof(gs_rollout_source) */
  int32_t dtype;                  /* GS_COMPUTE_F64 / GS_COMPUTE_F32: element type of every floating array below */
  int32_t T;                      /* > 0; B, obs_dim, action_dim are the handle's */
  int32_t chunk_rows;             /* 0: the library's choice; > 0: rows per staging chunk */
  uint32_t flags;                 /* 0; reserved */
  const void* observations;       /* host [T][B][obs_dim] */
  const void* actions;            /* host [T][B][action_dim]; may be NULL only when action_dim == 0 */
  const void* rewards;            /* host [T][B] */
  const void* next_observations;  /* host [T][B][obs_dim] */
  const uint8_t* terminals;       /* host [T][B]: 0, or bit 0 terminated | bit 1 truncated, as gs_rollout_view */
  const void* final_observation;  /* host [B][obs_dim], or NULL: next_observations[T - 1] */
  const void* log_probs;          /* host [T][B], or NULL: the rollout then "recorded none" */
} gs_rollout_source;
typedef struct gs_rollout_load_info { int64_t n; int32_t n_terminal, term_cap_needed; } gs_rollout_load_info;
int gs_rollout_load_check(const gs_rollout_source* s, int32_t B, int32_t obs_dim, int32_t action_dim, gs_rollout_load_info* out);  /* host only */
int gs_rollout_load(gs_handle* h, const gs_rollout_source* s);

/* ---- a sliding window over consecutive rollouts: the last `keep` steps stay, T fresh ones follow ---------
 * gs_rollout_continue keeps steps T_old - keep .. T_old - 1 of the rollout the handle holds, moves them to the front ON THE DEVICE
 * and collects T new steps behind them; the handle's rollout then has keep + T steps and every entry that reads "the last rollout"
 * runs on that window unchanged -- a replay window for the off-policy learners with no transition crossing the host.
 *   steps 0 .. keep - 1 are, by bits, steps T_old - keep .. T_old - 1 of the previous rollout (obs_seq slots 0 .. keep, actions,
 *   rewards, flags, log-probabilities where recorded); slot keep is the previous slot T_old, where the environment stands; steps
 *   keep .. keep + T - 1 are what gs_rollout(h, T, policy, policy_seed, actions) would have produced, except that new step i draws
 *   with the index t0 + i wherever gs_rollout draws with its step index t (the random actions' counter, the policy's noise): after
 *   gs_rollout(T1), continue(T2, keep, t0 = T1) holds the last keep + T2 steps of one gs_rollout(T1 + T2), by bits.
 *   The terminal list holds the previous entries with t >= T_old - keep, renumbered t -= T_old - keep, each with its row, in the
 *   order the previous list had them (a stable compaction); the new steps' entries follow.
 *   Log-probabilities count as recorded when the kept steps had them (or keep == 0) and the new steps record them.
 *   The window counts as a new rollout: whatever was computed over the previous one is stale, as after gs_rollout.
 * GS_E_INVALID: a NULL handle or config, a wrong struct_size, T <= 0, keep < 0 or keep beyond the current rollout's T, an unknown
 * policy, GS_POLICY_UPLOADED without actions.  GS_E_STATE: keep > 0 without a rollout; GS_POLICY_MLP without a policy; before
 * gs_reset; keep > 0 on a rollout that gs_rollout_load installed (the environment does not stand at its last slot) or after the
 * environment was moved since the rollout ended (gs_reset, gs_set_state, gs_step*, an upload of state, gs_solve*).  Every check
 * runs before anything is queued: a refused call leaves the rollout and everything computed over it as they were.  keep == 0 is
 * gs_rollout with the draw origin t0.
 * Asynchronous, like gs_rollout; the host waits only where the window outgrows the buffers' capacity and they are made again (the
 * kept part is carried over).  gs_rollout_episodes(GS_EPISODES_CONTINUE) on a window with kept steps is GS_E_STATE: it would
 * count them twice.
 * gs_rollout_window_info: host state, no wait.  T: steps of the handle's rollout (0: none); kept: the steps at its front that
 * came from before the last gs_rollout_continue (0 after gs_rollout or a load); t0_next: t0 + T of the last continue, T after a
 * plain gs_rollout -- the t0 that makes the next continue draw on; T_cap: the steps the buffers hold. */
typedef struct gs_rollout_continue_config {
  int32_t struct_size;            /* = sizeof(gs_rollout_continue_config) */
  int32_t T;                      /* new steps, > 0 */
  int32_t keep;                   /* steps kept from the end of the current rollout, 0 <= keep <= its T */
  int32_t policy;                 /* GS_POLICY_* as gs_rollout */
  uint64_t policy_seed;
  uint32_t t0;                    /* the step index the first NEW step draws with */
  uint32_t reserved;
  const double* actions;          /* GS_POLICY_UPLOADED: host [T][B][action_dim], the new steps only */
} gs_rollout_continue_config;
typedef struct gs_rollout_window_info_out { int32_t T, kept; uint32_t t0_next; int32_t T_cap; } gs_rollout_window_info_out;
int gs_rollout_continue(gs_handle* h, const gs_rollout_continue_config* cfg);
int gs_rollout_window_info(gs_handle* h, gs_rollout_window_info_out* out);

/* ---- closed-loop rollouts: an MLP policy evaluated on the device between two steps of gs_rollout ---------------
 * The reference's actors are plain MLPs (algorithms/base.py:157-177 `_build_mlp`: Linear + relu / tanh / elu) whose head is
 * tanh(mean) or tanh(mean + exp(clamp(log_std, -20, 2)) * eps) (algorithms/offline.py:69-76, 114-136).
 *   weights[l]  [dims[l + 1]][dims[l]] row-major float64 -- torch's Linear.weight --, biases[l] [dims[l + 1]]
 *   activation  between the layers (not behind the last one)
 *   head        GS_HEAD_TANH: dims[n_layers] = action_dim, a = tanh(out); GS_HEAD_GAUSSIAN_TANH: dims[n_layers] = 2 * action_dim,
 *               out = [mean | log_std] as torch.chunk(out, 2, dim=-1) splits it, log_std clamped to [-20, 2]
 *   stochastic  0: a = tanh(mean); 1 (Gaussian head only): a = tanh(mean + exp(log_std) * eps), eps for action a of instance b at
 *               rollout step t = component a & 3 of the four normals of ONE Philox call keyed by policy_seed with counter
 *               (global instance, t, a / 4, 'PNOI' = 0x504E4F49): Box-Muller cosine and sine on words (0, 1) and (2, 3),
 *               u = (r + 1/2) 2^-32 -- so sharded handles (first_instance) draw what one handle would.
 * Rules (GS_E_INVALID with a message): 1 <= n_layers <= 4; dims[0] = obs_dim; action_dim > 0; the last width matches the head;
 * every width behind the first is in 1 .. 256; stochastic only with the Gaussian head; every weight and bias finite. */
enum { GS_ACT_RELU = 0, GS_ACT_TANH = 1, GS_ACT_ELU = 2 };
enum { GS_HEAD_TANH = 0, GS_HEAD_GAUSSIAN_TANH = 1 };
enum { GS_POLICY_MLP = 2 };       /* gs_rollout's third policy: the one gs_policy_mlp_set installed */
#define GS_POLICY_MAX_LAYERS 4
typedef struct gs_policy_mlp {
  int32_t struct_size;            /* = sizeof(gs_policy_mlp) */
  int32_t n_layers;               /* linear layers, 1 .. GS_POLICY_MAX_LAYERS */
  int32_t dims[GS_POLICY_MAX_LAYERS + 1];
  int32_t activation;             /* GS_ACT_* */
  int32_t head;                   /* GS_HEAD_* */
  int32_t stochastic;
  const double* weights[GS_POLICY_MAX_LAYERS];
  const double* biases[GS_POLICY_MAX_LAYERS];
} gs_policy_mlp;
/* the rules above, on the host alone (no device needed) */
int gs_policy_mlp_check(const gs_policy_mlp* p, int32_t obs_dim, int32_t action_dim);
/* Checks `p` against the handle's obs_dim / action_dim and uploads it (the handle keeps its own copy, in the operand order of the
 * matrix cores); NULL removes the policy.  The policy is not environment state: gs_reset, gs_set_state and the in-place resets of
 * gs_rollout leave it alone. */
int gs_policy_mlp_set(gs_handle* h, const gs_policy_mlp* p);
/* The policy's actions [B][action_dim] on the observation the environment stands at (after gs_reset / a step / a rollout); does not
 * step.  policy_seed / t: the noise of a stochastic policy, as rollout step t would draw it.  GS_E_STATE without a policy. */
int gs_policy_mlp_eval(gs_handle* h, uint64_t policy_seed, int32_t t, double* actions_host);
/* gs_rollout(h, T, GS_POLICY_MLP, policy_seed, NULL): before step t one kernel reads obs_seq[t] and writes actions[t] -- the
 * observation of an instance that finished at step t - 1 being the fresh one after its in-place reset, as the reference calls
 * env.reset() and then the policy (algorithms/base.py:289-290).  GS_E_STATE without a policy; everything else as above. */

/* ---- the float32 compute path of the MLP policy ------------------------------------------------------------------
 * gs_policy_mlp_set_opts installs `p` like gs_policy_mlp_set, with options.  o == NULL, or compute == GS_COMPUTE_F64 without
 * obs_shift / obs_scale, IS gs_policy_mlp_set(h, p): same kernel, same bits.  GS_COMPUTE_F32 (the precision of the reference's
 * torch actors):
 *   - weights and biases are rounded to the nearest float32 once, at install;
 *   - the observation is normalised in float64, z = (obs - obs_shift) * obs_scale, and z is rounded to float32 once (a raw
 *     1e5-watt column rounded to float32 first would lose 2.4e-3 W, which a folded first layer multiplies and sums);
 *   - the layer products run on the f32 matrix instructions with f32 accumulation; bias, activation and the hidden activations
 *     are float32;
 *   - the head is evaluated in float64 on the float32 pre-head values: the log_std clamp, exp, the 'PNOI' noise and tanh are
 *     those of the float64 path, draw for draw, so the stochastic contract above holds unchanged; actions are float64.
 * gs_policy_mlp_eval, gs_rollout(GS_POLICY_MLP) and the "not environment state" rule apply to whichever variant is installed.
 * Rules beyond those of gs_policy_mlp (GS_E_INVALID with a message; the installed policy stays): struct_size matches; compute is
 * a GS_COMPUTE_* value; obs_shift / obs_scale only with GS_COMPUTE_F32 (for float64, fold the normalisation into the first
 * layer); every obs_shift / obs_scale entry finite; every weight and bias still finite after rounding to float32. */
enum { GS_COMPUTE_F64 = 0, GS_COMPUTE_F32 = 1 };
typedef struct gs_policy_mlp_opts {
  int32_t struct_size;            /* = sizeof(gs_policy_mlp_opts) */
  int32_t compute;                /* GS_COMPUTE_* */
  const double* obs_shift;        /* [dims[0]] or NULL (0) */
  const double* obs_scale;        /* [dims[0]] or NULL (1): z = (obs - shift) * scale in float64, then rounded to float32 */
} gs_policy_mlp_opts;
/* the rules of gs_policy_mlp and of the options, on the host alone (no device needed); o == NULL: gs_policy_mlp_check */
int gs_policy_mlp_check_opts(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim, int32_t action_dim);
int gs_policy_mlp_set_opts(gs_handle* h, const gs_policy_mlp* p, const gs_policy_mlp_opts* o);

/* ---- on-policy rollouts: log-probabilities, a value network, advantages and returns ---------------------
 * What a policy-gradient learner needs from gs_rollout(GS_POLICY_MLP) beyond the five arrays, computed where the collection lies.
 * Additive to ABI 2.
 *
 * Log-probabilities.  A rollout under a STOCHASTIC policy (Gaussian head) records log_probs[T][B], float64, written by the policy
 * kernel's head with the action:
 *   logp[b] = sum over a = 0 .. A-1 of  -0.5 eps^2 - ls - 0.5 log(2 pi) - log((1 - act^2) + 1e-6)
 * ls the clamped log_std, eps the 'PNOI' draw, act the action written: the reference's Normal(mean, std).log_prob(x) minus its tanh
 * correction (algorithms/offline.py:114-136) with (x - mean)^2 / (2 std^2) written as eps^2 / 2.  The sum runs in action order.
 * Deterministic and GS_HEAD_TANH policies record none (the view's pointer is NULL).  gs_rollout_set_log_probs(h, 0) switches the
 * recording off (on by default); the actions and everything else the rollout leaves are the same bits either way.
 *
 * The value network.  gs_value_mlp_set installs a critic: the reference's `_build_mlp` with a scalar output (IQL's and AWR's value
 * functions), described by gs_policy_mlp with head = GS_HEAD_LINEAR.  Rules beyond those of gs_policy_mlp / gs_policy_mlp_opts
 * (GS_E_INVALID with a message; the installed network stays): head = GS_HEAD_LINEAR, dims[n_layers] = 1, stochastic = 0, and
 * compute = GS_COMPUTE_F32 (the precision of torch critics; obs_shift / obs_scale as for the policy).  gs_policy_mlp_set* keeps
 * refusing GS_HEAD_LINEAR.  NULL removes the network.  Like the policy it is not environment state.  gs_value_mlp_check: the
 * rules on the host alone.  gs_value_mlp_eval: values[B] on the observation the environment stands at (the twin of
 * gs_policy_mlp_eval; GS_E_STATE without a network or before gs_reset).  A row's value depends on that row alone: the same
 * observation gives the same bits wherever it lies in a batch.
 *
 * gs_rollout_evaluate (asynchronous, on the handle's stream, over the LAST rollout; no host synchronisation behind gs_rollout)
 * computes values[T + 1][B] over obs_seq, terminal_values[k] over terminal_obs in the order of terminal_index, and, t running
 * from T - 1 down to 0 with every operation IEEE float64 and none contracted,
 *   done  = terminals[t][b] != 0
 *   vnext = done ? ((terminals[t][b] & bootstrap_mask) ? terminal_value(t, b) : 0.0) : values[t + 1][b]
 *   delta = (r' + gamma * vnext) - values[t][b]                  r' = (rewards[t][b] - reward_shift) * reward_scale
 *   adv   = done ? delta : delta + (gamma * lambda) * adv_next   adv_next = 0 at t = T - 1
 *   ret   = adv + values[t][b]
 * so the tail of an unfinished episode bootstraps from values[T].  GS_E_STATE without a rollout or without a value network;
 * GS_E_INVALID for a wrong struct_size, bootstrap_mask outside 0 .. 3 or a non-finite parameter.
 * gs_rollout_onpolicy_view: device pointers, valid until the next gs_rollout (consumer_stream as gs_step_device_view; the call
 * waits for the number of finished episodes).  gs_rollout_onpolicy_download: host copies, any pointer may be NULL.  Both return
 * GS_E_STATE unless gs_rollout_evaluate has run on the last rollout -- in particular after a further gs_rollout --, except that the
 * download of log_probs alone needs no evaluation (GS_E_STATE if the last rollout recorded none). */
enum { GS_HEAD_LINEAR = 2 };      /* gs_policy_mlp.head of a value network: the last layer's output as it is */
int gs_rollout_set_log_probs(gs_handle* h, int32_t on);
int gs_value_mlp_check(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim);
int gs_value_mlp_set(gs_handle* h, const gs_policy_mlp* p, const gs_policy_mlp_opts* o);
int gs_value_mlp_eval(gs_handle* h, double* values_host /* [B] */);
typedef struct gs_gae_config {
  int32_t struct_size;            /* = sizeof(gs_gae_config) */
  int32_t bootstrap_mask;         /* done-flag bits whose episode end bootstraps from V(terminal observation): bit 0 terminated
                                     (here: the time limit), bit 1 truncated (too many violations); 0 = the reference's (1 - terminals) */
  double gamma, lambda;
  double reward_shift, reward_scale;   /* r' = (r - shift) * scale; 0, 1 = raw */
} gs_gae_config;
int gs_rollout_evaluate(gs_handle* h, const gs_gae_config* cfg);
typedef struct gs_rollout_onpolicy {
  int32_t T, B, n_terminal, rows_per_tile;   /* rows_per_tile: the rows one workgroup of the value kernel evaluates */
  const double* log_probs;        /* [T][B], or NULL: the last rollout recorded none */
  const double* values;           /* [T + 1][B] */
  const double* terminal_values;  /* [n_terminal], in the order of gs_rollout_device.terminal_index */
  const double* advantages;       /* [T][B] */
  const double* returns;          /* [T][B] */
} gs_rollout_onpolicy;
int gs_rollout_onpolicy_view(gs_handle* h, gs_rollout_onpolicy* out, void* consumer_stream);
typedef struct gs_rollout_onpolicy_host {
  double* log_probs;              /* [T][B] */
  double* values;                 /* [T + 1][B] */
  double* terminal_values;        /* [n_terminal] (room for as many as gs_rollout_download reported) */
  double* advantages;             /* [T][B] */
  double* returns;                /* [T][B] */
} gs_rollout_onpolicy_host;
int gs_rollout_onpolicy_download(gs_handle* h, const gs_rollout_onpolicy_host* out);

/* ---- constraint costs of a rollout: margins, violation counts, costs, cost critics and cost advantages ----
 * What the reference's constrained learners (algorithms/safe.py: SafeRL, ConstrainedPolicyOptimization) need beside the reward:
 * a constraint value per transition (>= 0 is safe, safe.py:26-32), violation flags and rates (:282, :74-80) and a penalty on
 * max(0, -value) (:459-474), computed where the collection lies.  Additive to ABI 2.
 *
 * One observation row o is read at the positions of the real layout (grid_env.py:753-783; the reference's own constraint functions
 * read placeholder positions, safe.py:519): Vm_i = o[2 i], i < n; L_k = |o[2 n + 2 k + 1]|, k < m; f = o[2 n + 2 m]; no other column.
 * Three channels with the limits (vlo, vhi), (flo, fhi) and lim:
 *   margin[V] = min_i min(Vm_i - vlo, vhi - Vm_i)   safe.py:513-522        count[V] = #{i : Vm_i < vlo or Vm_i > vhi}   base.py:153-167
 *   margin[F] = min(f - flo, fhi - f)               safe.py:534-542        count[F] = (f < flo or f > fhi)
 *   margin[T] = lim - max_k L_k  (m = 0: lim)       safe.py:554-561        count[T] = #{k : L_k > lim}
 * margins are float64, counts int32.  A NaN among a channel's own inputs makes that channel's margin NaN (as np.min / np.max do) and
 * counts as nothing (the comparisons are strict); a NaN anywhere else in the row changes nothing.  cost (float64) by the channel's kind:
 *   GS_COSTKIND_EXCESS     margin < 0 ? -margin : 0.0   (safe.py:471; a NaN margin gives 0)
 *   GS_COSTKIND_INDICATOR  margin < 0 ? 1.0 : 0.0       (safe.py:282)
 *   GS_COSTKIND_COUNT      (double)count
 * Every quantity is a minimum, a maximum, a count or one rounded subtraction: the results do not depend on how the device maps lanes.
 *
 * gs_cost_config_default: the handle's own v_min / v_max and f_min / f_max, 0.8 (get_reward's threshold, grid_env.py:785-826, and
 * thermal_constraint's default) and GS_COSTKIND_EXCESS.  gs_cost_config_check: the rules on the host alone (GS_E_INVALID with a
 * message: a wrong struct_size, a kind outside 0 .. 2, a non-finite limit, lo > hi).
 * gs_rollout_costs (asynchronous, on the handle's stream, over the LAST rollout; c == NULL: the default) fills margins, counts and
 * costs [3][T][B], channel-major, each channel indexed like rewards by t * B + b, and n_violating[3], the number of transitions with
 * margin < 0.  The row of transition (t, b) is the observation its reward was computed on: obs_seq[t + 1][b] unless
 * terminals[t][b] != 0, then terminal_obs[k] with terminal_index[k] = (t, b).  GS_E_STATE without a rollout.
 * gs_costs_eval: the same three results [rows][3] for `rows` observation rows on the host (any output may be NULL); GS_E_INVALID for
 * rows <= 0 or a NULL obs_host.
 *
 * Cost critics.  gs_cost_value_mlp_set installs a value network for one channel exactly as gs_value_mlp_set accepts it
 * (GS_HEAD_LINEAR, scalar output, GS_COMPUTE_F32; the same rules, GS_E_INVALID also for a channel outside 0 .. 2; NULL removes it; a
 * refused network leaves the installed one in place).  gs_rollout_evaluate_costs (asynchronous) runs, for every channel that has a
 * critic, the value kernel over obs_seq and over the terminal observations and the recurrence of gs_rollout_evaluate with
 * rewards = costs[c] and the channel's own gamma, lambda, cost_shift and cost_scale; the bootstrap mask is shared.  GS_E_STATE
 * without a rollout, before gs_rollout_costs on the last rollout, or with no cost critic installed; GS_E_INVALID as gs_rollout_evaluate.
 * gs_rollout_costs_view: device pointers, valid until the next gs_rollout (consumer_stream as gs_step_device_view).  The pointers
 * of a channel that had no critic at the last evaluation -- or of every channel, before the evaluation -- are NULL.
 * gs_rollout_costs_download: host copies, any pointer may be NULL; asking for values, terminal_values, advantages or returns of a
 * channel that was not evaluated on the last rollout is GS_E_STATE.  Both return GS_E_STATE unless gs_rollout_costs has run on the
 * last rollout -- in particular after a further gs_rollout. */
enum { GS_COST_VOLTAGE = 0, GS_COST_FREQUENCY = 1, GS_COST_THERMAL = 2, GS_COST_CHANNELS = 3 };
enum { GS_COSTKIND_EXCESS = 0, GS_COSTKIND_INDICATOR = 1, GS_COSTKIND_COUNT = 2 };
typedef struct gs_cost_config {
  int32_t struct_size;            /* = sizeof(gs_cost_config) */
  int32_t kind[3];                /* GS_COSTKIND_* per channel */
  double voltage_limits[2];       /* (vlo, vhi), per unit */
  double frequency_limits[2];     /* (flo, fhi), Hz */
  double line_loading_limit;      /* lim, |S| / rating */
} gs_cost_config;
int gs_cost_config_default(const gs_handle* h, gs_cost_config* out);
int gs_cost_config_check(const gs_cost_config* c);
int gs_rollout_costs(gs_handle* h, const gs_cost_config* c);
int gs_costs_eval(gs_handle* h, const gs_cost_config* c, const double* obs_host /* [rows][obs_dim] */, int32_t rows,
                  double* margins_host, int32_t* counts_host, double* costs_host /* [rows][3] each */);
int gs_cost_value_mlp_set(gs_handle* h, int32_t channel, const gs_policy_mlp* p, const gs_policy_mlp_opts* o);
typedef struct gs_cost_gae_config {
  int32_t struct_size;            /* = sizeof(gs_cost_gae_config) */
  int32_t bootstrap_mask;         /* as gs_gae_config, shared by the channels */
  double gamma[3], lambda[3];
  double cost_shift[3], cost_scale[3];   /* c' = (cost - shift) * scale; 0, 1 = raw */
} gs_cost_gae_config;
int gs_rollout_evaluate_costs(gs_handle* h, const gs_cost_gae_config* c);
typedef struct gs_rollout_costs_dev {
  int32_t T, B;
  const double* margins;          /* [3][T][B] */
  const int32_t* counts;          /* [3][T][B] */
  const double* costs;            /* [3][T][B] */
  const int64_t* n_violating;     /* [3] */
  const double* values[3];        /* [T + 1][B] per channel, or NULL */
  const double* terminal_values[3];   /* [n_terminal], in the order of gs_rollout_device.terminal_index */
  const double* advantages[3];    /* [T][B] */
  const double* returns[3];       /* [T][B] */
} gs_rollout_costs_dev;
int gs_rollout_costs_view(gs_handle* h, gs_rollout_costs_dev* out, void* consumer_stream);
typedef struct gs_rollout_costs_host {
  double* margins;                /* [3][T][B] */
  int32_t* counts;                /* [3][T][B] */
  double* costs;                  /* [3][T][B] */
  int64_t* n_violating;           /* [3] */
  double* values[3];              /* [T + 1][B] */
  double* terminal_values[3];     /* [n_terminal] (room for as many as gs_rollout_download reported) */
  double* advantages[3];          /* [T][B] */
  double* returns[3];             /* [T][B] */
} gs_rollout_costs_host;
int gs_rollout_costs_download(gs_handle* h, const gs_rollout_costs_host* out);

/* ---- episode accounting: returns, lengths and episodic costs of the episodes a rollout finished ----------
 * What the reference's evaluation loop (benchmarking/benchmark_suite.py:360-429) keeps per episode -- `episode_return += reward`
 * until done, the steps, the violating steps -- kept per instance on the device ACROSS rollouts, so that an episode that straddles
 * a rollout boundary is one episode.  Additive to ABI 2.
 *
 * Per-instance carries (device arrays of the handle's episode track): ep_return[B] float64, ep_length[B], ep_ordinal[B] int32 (the
 * episodes the instance has finished since the track started), ep_partial[B] uint8 (the open episode's start was not seen), and with
 * costs ep_cost[3][B] float64, ep_violating[3][B], ep_any_violating[B] int32.
 * gs_rollout_episodes (asynchronous, on the handle's stream, over the LAST rollout) runs, per instance b and t = 0 .. T-1 in order,
 *   ret = ret + rewards[t][b]          one rounded float64 addition per step, never contracted or reassociated
 *   len = len + 1
 *   with costs, per channel c:  cost[c] = cost[c] + costs[c][t][b];  viol[c] += margins[c][t][b] < 0  (a NaN margin counts as nothing);
 *                               any += (margins[c][t][b] < 0 for some c)
 *   terminals[t][b] != 0:  file the record (t, b, ret, len, ordinal, flags, cost, viol, any), flags = (terminals[t][b] & 3) |
 *                          (partial ? GS_EPISODE_PARTIAL : 0); then ret = 0, len = 0, cost = viol = any = 0, ordinal += 1, partial = 0
 * and stores the carries.  The records of the rollout form a list of n_episodes == n_terminal entries sorted by (b, t_end):
 * instance-major, chronological within an instance; every record's place follows from a prefix sum of the instances' counts, no
 * atomic decides it.  cfg == NULL: GS_EPISODES_CONTINUE, no costs, success_return = -1000.
 *
 * start.  GS_EPISODES_FRESH: the caller states that every instance stood at the start of an episode when the last rollout began
 * (gs_reset came directly before it); the carries start from zero and nothing is partial.  GS_EPISODES_UNKNOWN: the carries start
 * from zero and every instance's open episode is partial: its record covers the seen part only.  GS_EPISODES_CONTINUE: the carries
 * are those the previous accounted rollout left.
 *
 * gs_episode_stats, over the rollout's COMPLETE episodes (those without GS_EPISODE_PARTIAL): count and count_partial; mean,
 * population standard deviation (np.std), minimum and maximum of the return; mean, minimum and maximum of the length; with costs
 * the mean cost and the total of violating steps per channel; n_success = the complete episodes with return > success_return and
 * (with costs) no step violating in any channel.  One workgroup reduces the list in a fixed order (DESIGN.md section 17 states the
 * order and its error bound): no floating-point atomics, the same list gives the same bits.  count == 0: the means, the standard
 * deviation and the extremes are NaN, the counts 0.  Without costs cost_mean is NaN and violating 0.
 *
 * GS_E_STATE (with a message; nothing launched, the carries untouched): no rollout yet; the last rollout was already accounted;
 * CONTINUE without a track, or when the rollout before the last one was not accounted, or when the environment was moved outside
 * gs_rollout since the accounted one (gs_reset, gs_set_state, gs_step*, gs_upload_injections, gs_solve*), or with a with_costs
 * other than the track was started with; with_costs before gs_rollout_costs on the last rollout.  GS_E_INVALID: a wrong
 * struct_size, an unknown start, a success_return that is NaN or +inf (-inf: no floor on the return).
 * gs_rollout_episodes_view: device pointers, the list valid until the next gs_rollout_episodes or gs_rollout, the carries until
 * gs_episodes_clear (consumer_stream as gs_step_device_view; the call waits for the number of finished episodes).  Channel c of
 * episode_cost / episode_violating lies at c * cost_stride; all three cost pointers and the cost carries are NULL without costs.
 * gs_rollout_episodes_download: host copies, any pointer may be NULL; episode_cost / episode_violating packed [3][n_episodes].
 * Both return GS_E_STATE unless gs_rollout_episodes has run on the last rollout.  gs_episodes_clear drops the track. */
enum { GS_EPISODES_CONTINUE = 0, GS_EPISODES_FRESH = 1, GS_EPISODES_UNKNOWN = 2 };
enum { GS_EPISODE_TERMINATED = 1, GS_EPISODE_TRUNCATED = 2, GS_EPISODE_PARTIAL = 4 };   /* bits 0, 1: the done flag's own */
typedef struct gs_episode_config {
  int32_t struct_size, start;        /* = sizeof(gs_episode_config); GS_EPISODES_* */
  int32_t with_costs, reserved;      /* != 0: also accumulate gs_rollout_costs' costs and violating steps */
  double success_return;             /* an episode succeeds with no violating step and return > this (reference: -1000) */
} gs_episode_config;
typedef struct gs_episode_stats {
  int64_t count, count_partial;
  double return_mean, return_std, return_min, return_max;
  double length_mean, length_min, length_max;
  double cost_mean[3];
  int64_t violating[3];
  int64_t n_success;
} gs_episode_stats;
typedef struct gs_rollout_episodes_dev {
  int32_t n_episodes, B, with_costs, cost_stride;
  const int32_t* episode_index;          /* [n_episodes][2] (t_end, b) */
  const double* episode_return;          /* [n_episodes] */
  const int32_t* episode_length;         /* [n_episodes] */
  const int32_t* episode_ordinal;        /* [n_episodes] */
  const int32_t* episode_flags;          /* [n_episodes] GS_EPISODE_* */
  const double* episode_cost;            /* channel c at c * cost_stride, or NULL */
  const int32_t* episode_violating;      /* channel c at c * cost_stride, or NULL */
  const int32_t* episode_any_violating;  /* [n_episodes], or NULL */
  const gs_episode_stats* stats;
  const double* ep_return;               /* [B] */
  const int32_t* ep_length;              /* [B] */
  const int32_t* ep_ordinal;             /* [B] */
  const uint8_t* ep_partial;             /* [B] */
  const double* ep_cost;                 /* [3][B], or NULL */
  const int32_t* ep_violating;           /* [3][B], or NULL */
  const int32_t* ep_any_violating;       /* [B], or NULL */
} gs_rollout_episodes_dev;
typedef struct gs_rollout_episodes_host {
  int32_t* n_episodes;                   /* [1] */
  int32_t* episode_index;                /* [n_episodes][2] (room for as many as gs_rollout_download reported) */
  double* episode_return;
  int32_t* episode_length;
  int32_t* episode_ordinal;
  int32_t* episode_flags;
  double* episode_cost;                  /* [3][n_episodes] */
  int32_t* episode_violating;            /* [3][n_episodes] */
  int32_t* episode_any_violating;
  gs_episode_stats* stats;
  double* ep_return;                     /* [B] */
  int32_t* ep_length;
  int32_t* ep_ordinal;
  uint8_t* ep_partial;
  double* ep_cost;                       /* [3][B] */
  int32_t* ep_violating;                 /* [3][B] */
  int32_t* ep_any_violating;
} gs_rollout_episodes_host;
int gs_rollout_episodes(gs_handle* h, const gs_episode_config* cfg);
int gs_rollout_episodes_view(gs_handle* h, gs_rollout_episodes_dev* out, void* consumer_stream);
int gs_rollout_episodes_download(gs_handle* h, const gs_rollout_episodes_host* out);
int gs_episodes_clear(gs_handle* h);

/* ---- the device-resident dataset: statistics of the last rollout and normalised minibatches ----------------------------
 * What the reference's GridDataset (algorithms/base.py:180-266) does on the host, done where gs_rollout left the collection:
 * the per-column normalisation statistics over its N = T * B transitions (transition index = t * B + b), and minibatches
 * gathered by index with the terminal observations put in their place.  Additive to ABI 2.
 *
 * gs_dataset_build (asynchronous, on the handle's stream, over the LAST rollout) computes per-column mean and population
 * standard deviation (np.std, ddof 0) of obs_seq[0 .. T-1] and of actions, the scalar pair of rewards, and the [T][B] int32 map
 * from a transition to its row of terminal_obs (-1: the transition ended no episode).  The reduction is a fixed tree (shifted
 * sums per chunk of rows_per_chunk rows, Chan's pairwise merge above them): no atomics, the same rollout
 * gives the same bits, and a column whose values are all equal comes out as that value and a standard deviation of exactly 0.
 * flags: GS_DATASET_KEEP_STATS builds the map only and keeps the statistics the handle holds (GS_E_STATE if it holds none).
 * GS_E_STATE without a rollout; GS_E_INVALID if N >= 2^31.  The handle remembers which rollout the dataset was built on: after a
 * further gs_rollout, gs_dataset_stats and gs_dataset_sample return GS_E_STATE until gs_dataset_build has run again. */
enum { GS_DATASET_KEEP_STATS = 1 };
int gs_dataset_build(gs_handle* h, uint32_t flags);
/* The statistics as host copies (waits for the build); any pointer may be NULL.  The standard deviations are the raw ones: the
 * reference's + 1e-6 (base.py:207-224) is applied where values are normalised, x_n = (x - mean) / (std + 1e-6).
 * gs_dataset_stats fills n, obs_dim, action_dim and rows_per_chunk (the rows one partial reduction covers).
 * gs_dataset_set_stats installs the caller's statistics in place of the computed ones (a normalisation that stays fixed over
 * several rollouts; the map still needs gs_dataset_build(GS_DATASET_KEEP_STATS) after every rollout).  It needs no build.  Rules
 * (GS_E_INVALID, the handle unchanged): struct_size, obs_dim and action_dim match the handle; every pointer set (act_* may be
 * NULL where action_dim = 0); every value finite, every standard deviation >= 0.  n and rows_per_chunk are ignored. */
typedef struct gs_dataset_stats_view {
  int32_t struct_size;            /* = sizeof(gs_dataset_stats_view) */
  int32_t rows_per_chunk;
  int64_t n;                      /* transitions the dataset was built on */
  int32_t obs_dim, action_dim;
  double* obs_mean;               /* [obs_dim] */
  double* obs_std;                /* [obs_dim] */
  double* act_mean;               /* [action_dim] */
  double* act_std;                /* [action_dim] */
  double* reward_mean;            /* [1] */
  double* reward_std;             /* [1] */
} gs_dataset_stats_view;
int gs_dataset_stats(gs_handle* h, gs_dataset_stats_view* view);
int gs_dataset_set_stats(gs_handle* h, const gs_dataset_stats_view* view);
/* One minibatch of n transitions, gathered by ONE kernel into five row-major arrays of `dtype` (GS_COMPUTE_F64 / GS_COMPUTE_F32):
 *   observations [n][obs_dim], actions [n][action_dim], rewards [n], next_observations [n][obs_dim], terminals [n]
 * terminals = 1.0 where bit 0 or bit 1 of the done flag is set (the reference's terminals.astype(float)); next_observations =
 * terminal_obs[map[t][b]] where the map is >= 0, obs_seq[t + 1][b] otherwise.  normalize != 0: exactly (x - mean) / (std + 1e-6),
 * IEEE subtraction, addition and division in float64 (next_observations with the observation statistics, rewards with the scalar
 * pair), rounded ONCE to float32 for GS_COMPUTE_F32; normalize == 0: the raw values.
 * indices: host int64[n], any value outside [0, N) refusing the call (GS_E_INVALID) before anything is launched; or NULL: drawn
 * on the device with replacement (the reference's rng.integers(0, size, batch_size)): sample i of call `draw` is word i & 3 of
 * ONE Philox-4x32 call keyed by `seed` with counter (i >> 2, draw low word, draw high word, 'SMPL' = 0x534D504C), mapped by
 * idx = (uint64(word) * N) >> 32.  (That mapping gives every index floor(2^32 / N) or ceil(2^32 / N) of the 2^32 words: its
 * probability differs from 1 / N by less than 2^-32, a relative bias below N / 2^32 -- 1.2e-4 at N = 524 288.)
 * out: each pointer is the caller's device memory or NULL; for NULL the handle supplies a buffer of its own and writes the address
 * back, valid until the next gs_dataset_sample or gs_rollout on the handle.  consumer_stream: as gs_step_device_view (made to wait
 * on the device for the batch; NULL: the call returns when the batch is complete).  GS_E_STATE without a current build. */
typedef struct gs_dataset_batch {
  void* observations;
  void* actions;
  void* rewards;
  void* next_observations;
  void* terminals;
} gs_dataset_batch;
int gs_dataset_sample(gs_handle* h, int32_t n, const int64_t* indices, uint64_t seed, uint64_t draw, int32_t dtype, int32_t normalize,
                      gs_dataset_batch* out, void* consumer_stream);

/* ---- on-policy minibatch epochs: a keyed permutation of the last rollout and one gather per minibatch ----
 * What a clipped-surrogate (PPO) learner does first with an evaluated rollout -- shuffle its N = T * B transitions, visit every one
 * exactly once per epoch in minibatches, normalise observations and advantages -- done where the collection lies.  gs_dataset_sample
 * draws WITH replacement (the reference's offline GridDataset); this visits without.  Additive to ABI 2.
 *
 * The epoch permutation perm(seed, epoch) of [0, N), N < 2^31, is a stateless keyed bijection evaluated per position (no stored
 * permutation, no sort).  h = the smallest integer >= 1 with 2^(2 h) >= N, m = 2^h - 1.  One PASS over a value x < 2^(2 h):
 *   L = x >> h, R = x & m;  for round = 0, 1, 2, 3:  (L, R) <- (R, L ^ (w & m)),
 *   w = word 0 of Philox-4x32-10 with counter (R, round, epoch, 'PERM' = 0x5045524D) and key (seed low word, seed high word);
 *   the result is (L << h) | R
 * -- a four-round Feistel network, a bijection of [0, 2^(2 h)).  perm[x] = the first of pass(x), pass(pass(x)), ... below N (cycle
 * walking: x < N lies on a cycle of the bijection, so the walk returns below N at the latest at x itself).  epoch is a uint32, seed a
 * uint64.
 *
 * gs_onpolicy_prepare (asynchronous, on the handle's stream, over the LAST rollout) combines the advantage per transition in float64,
 * nothing contracted:  comb = advantages;  for c = 0, 1, 2 with lambda[c] != 0:  comb = comb - lambda[c] * cost_advantages[c]  (the
 * product rounded, then the difference); reduces mean and population standard deviation of comb over N in the fixed tree of
 * gs_dataset_build (no atomics: a second call gives the same bits); and uploads obs_shift / obs_scale.  With every lambda 0 and no
 * cost field asked for it needs nothing of gs_rollout_costs.
 *   GS_E_STATE (with a message): gs_rollout_evaluate has not run on the last rollout; lambda[c] != 0 or a cost field asked for while
 *     gs_rollout_evaluate_costs left channel c unevaluated on the last rollout (a cost field needs at least one evaluated channel and
 *     covers every evaluated one); GS_ONPOLICY_LOG_PROBS on a rollout that recorded none.
 *   GS_E_INVALID: a wrong struct_size; an unknown adv_norm, dtype or field bit; a non-finite lambda, adv_eps, shift or scale;
 *     adv_eps < 0; exactly one of obs_shift and obs_scale; N >= 2^31.
 * gs_onpolicy_stats: host copies of N and of the combined advantage's mean and RAW standard deviation; waits for the prepare.
 *
 * gs_onpolicy_batch: the minibatch of positions first .. first + n - 1 of perm(seed, epoch), row-major arrays of cfg.dtype.  Sample
 * i is transition j = perm[first + i] = t * B + b:
 *   observations [n][obs_dim]   (obs_seq[t][b] - obs_shift) * obs_scale in float64, subtraction then multiplication, not contracted
 *                               (the formula of the float32 policy and value kernels); the raw row without shift / scale
 *   actions [n][action_dim], log_probs [n], returns [n]   as stored;   values [n] = values[t][b]
 *   advantages [n]              GS_ADVNORM_NONE: comb[j];  GS_ADVNORM_ROLLOUT: (comb[j] - mean_N) / (std_N + adv_eps);
 *                               GS_ADVNORM_MINIBATCH: the same with mean and population standard deviation of the minibatch's n values
 *   cost_advantages[c] [n], cost_returns[c] [n]   per evaluated channel (the pointers of the others are left alone)
 *   indices [n]                 int32 j
 *   adv_stats [2]               float64 (mean, raw std) the advantages were normalised with, NaN for GS_ADVNORM_NONE; written with
 *                               GS_ONPOLICY_ADVANTAGES
 * every value computed in float64 and rounded ONCE to float32 for GS_COMPUTE_F32.  The minibatch statistics are reduced by one
 * workgroup of 1024 threads in the fixed order of the episode statistics (thread i over entries i, i + 1024, ...; a butterfly over
 * the threads; a second pass for the squared deviations; DESIGN.md sections 17 and 18).
 * out: each pointer of a field in cfg.fields is the caller's device memory, or NULL for a buffer of the handle's, whose address is
 * written back and stays valid until the next gs_onpolicy_batch, gs_onpolicy_prepare or gs_rollout; the pointer of a field not in
 * cfg.fields is left alone.  consumer_stream: as gs_dataset_sample.  GS_E_INVALID (before any launch) for n <= 0, first < 0 or
 * first + n > N; GS_E_STATE unless gs_onpolicy_prepare has run on the last rollout. */
enum { GS_ADVNORM_NONE = 0, GS_ADVNORM_ROLLOUT = 1, GS_ADVNORM_MINIBATCH = 2 };
enum { GS_ONPOLICY_OBSERVATIONS = 1, GS_ONPOLICY_ACTIONS = 2, GS_ONPOLICY_LOG_PROBS = 4, GS_ONPOLICY_ADVANTAGES = 8,
       GS_ONPOLICY_RETURNS = 16, GS_ONPOLICY_VALUES = 32, GS_ONPOLICY_COST_ADVANTAGES = 64, GS_ONPOLICY_COST_RETURNS = 128,
       GS_ONPOLICY_INDICES = 256, GS_ONPOLICY_ALL_FIELDS = 511 };
typedef struct gs_onpolicy_batch_config {
  int32_t struct_size;            /* = sizeof(gs_onpolicy_batch_config) */
  int32_t adv_norm;               /* GS_ADVNORM_* */
  int32_t dtype;                  /* GS_COMPUTE_F64 / GS_COMPUTE_F32 */
  uint32_t fields;                /* GS_ONPOLICY_* bits */
  double lambda[3];               /* the multiplier of each cost channel */
  double adv_eps;                 /* 1e-8 is the usual choice */
  const double* obs_shift;        /* host [obs_dim], or NULL */
  const double* obs_scale;        /* host [obs_dim], or NULL: both or neither */
} gs_onpolicy_batch_config;
typedef struct gs_onpolicy_stats_out {
  int64_t n;                      /* N = T * B */
  double adv_mean, adv_std;       /* of the combined advantage over N; the raw standard deviation */
} gs_onpolicy_stats_out;
typedef struct gs_onpolicy_batch_out {
  void* observations;
  void* actions;
  void* log_probs;
  void* advantages;
  void* returns;
  void* values;
  void* cost_advantages[3];
  void* cost_returns[3];
  int32_t* indices;
  double* adv_stats;
} gs_onpolicy_batch_out;
int gs_onpolicy_prepare(gs_handle* h, const gs_onpolicy_batch_config* cfg);
int gs_onpolicy_stats(gs_handle* h, gs_onpolicy_stats_out* out);
int gs_onpolicy_batch(gs_handle* h, uint64_t seed, uint32_t epoch, int64_t first, int32_t n, gs_onpolicy_batch_out* out,
                      void* consumer_stream);

/* ---- the learner: one clipped-surrogate (PPO) or critic update per minibatch, where the networks lie ----
 * The networks that gs_policy_mlp_set_opts, gs_value_mlp_set and gs_cost_value_mlp_set installed become trainable in place: one
 * gs_learner_step per network and minibatch runs the forward pass with saved activations, the loss and its gradient at the head, the
 * backward pass, a deterministic gradient reduction and Adam, which also rewrites the packed image the rollout and critic kernels
 * read -- the next gs_rollout acts with the updated policy and no weight crosses the host.  Additive to ABI 2.
 *
 * net: GS_LEARNER_POLICY, GS_LEARNER_VALUE (the reward critic) or GS_LEARNER_COST_VALUE + c (the critic of cost channel c).
 * gs_learner_create snapshots the installed network's float32 weights and biases as the master parameters -- P float32 values, flat
 * in torch order: W_0 row-major [out][in], b_0, W_1, b_1, ... -- and zeroes Adam's m, v and step count.  GS_E_STATE: the network is
 * not installed, or the policy is not GS_COMPUTE_F32 with GS_HEAD_GAUSSIAN_TANH.  GS_E_INVALID: a wrong struct_size, an unknown
 * net, or a hyper-parameter that is not finite or outside lr >= 0, 0 <= beta1 < 1, 0 <= beta2 < 1, eps >= 0, weight_decay >= 0,
 * max_grad_norm >= 0 (0: no clipping), clip >= 0.  Creating again starts afresh from the installed image (which holds the trained
 * parameters).  Installing a network again with a *_set* entry drops that network's learner: a step is GS_E_STATE until
 * gs_learner_create has run again.
 *
 * gs_learner_step (asynchronous, on the handle's stream): one update on the minibatch of n samples that gs_onpolicy_batch just left
 * in `batch`.  It needs gs_onpolicy_prepare on the last rollout with dtype GS_COMPUTE_F32 and with obs_shift / obs_scale bit-equal,
 * compared on the host, to the network's own normalisation (none given: the network's must be shift 0, scale 1); GS_E_STATE
 * otherwise, and for the policy also when the last rollout recorded no log-probabilities.  The policy reads observations [n][obs_dim]
 * (float32, normalised), advantages [n] and indices [n] of `batch`, and THROUGH the indices the rollout's float64 actions and
 * log-probabilities: a float32 copy of a saturated action loses 1 - a^2, and importance ratios of up to 5.5 at unchanged
 * parameters were measured with it.  A critic reads observations and returns (cost_returns[c]).  A missing pointer or n <= 0 (or more
 * than 2^24 samples) is GS_E_INVALID.  Every check runs before anything is launched.  consumer_stream: as gs_onpolicy_batch.
 *
 * The loss.  Layers in float32 (float32 products and sums on the matrix cores, float32 activations), the head in float64 on the
 * float32 pre-head values (mean_k | log_std_k), its gradient rounded once to float32, the backward pass in float32.
 *   policy, sample i with stored action a (float64), old log-probability lp_old and advantage A:
 *     ls_k = clamp(log_std_k, -20, 2);  x_k = atanh(clamp(a_k, -(1 - 1e-7), 1 - 1e-7));  e_k = (x_k - mean_k) exp(-ls_k)
 *     lp = sum_k (((-0.5 e_k) e_k - ls_k) - 0.5 log(2 pi)) - log((1 - a_k a_k) + 1e-6)      in action order from k = 0
 *     r = exp(lp - lp_old);   s_i = min(r A, clamp(r, 1 - clip, 1 + clip) A);   h_i = sum_k (ls_k + 0.5 log(2 pi e))
 *     L = -(1/n) sum_i s_i - ent_coef (1/n) sum_i h_i
 *     clipped_i = (A > 0 and r > 1 + clip) or (A < 0 and r < 1 - clip);   dL/dlp = 0 if clipped_i, else -(r A) / n
 *     dL/dmean_k = dL/dlp  e_k exp(-ls_k)
 *     dL/dlog_std_k = dL/dlp (e_k e_k - 1) - ent_coef / n   where -20 <= log_std_k <= 2, and 0 outside (as torch.clamp)
 *   critic:  L = (1/n) sum_i (v_i - ret_i)^2,   dL/dv_i = 2 (v_i - ret_i) / n
 *   hidden layers: delta_l = (delta_{l+1} W_{l+1}) * act'(y_l), act' from the saved output y: relu y > 0, tanh 1 - y^2, elu
 *     y > 0 ? 1 : y + 1;  dW_l = delta_l^T a_{l-1},  db_l = the column sums of delta_l.
 * Determinism.  dW and db are summed over segments of rows_per_segment rows (a compile-time constant): within a segment in an order
 * fixed by the layer's shape, the segments' partial results in ascending order; no floating-point atomics.  The gradient's bits are
 * a function of the parameters, the minibatch's contents and n alone.  grad_norm = sqrt of the float64 sum of the squares of the
 * float32 gradient, in a fixed tree (four per thread in order, a butterfly over 256 threads; then ONE workgroup of 1024 threads
 * over those sums in the order of gs_episode_stats).
 * Adam, per parameter p with gradient g, all float32, every operation rounded, nothing contracted (t = the step's number from 1):
 *     max_grad_norm > 0:   g = g * float32(min(1, max_grad_norm / (grad_norm + 1e-6)))        the scale computed in float64
 *     weight_decay != 0:   g = g + wd * p
 *     m = b1 * m + omb1 * g;   v = b2 * v + (omb2 * g) * g;   denom = sqrt(v) / bc2s + eps;   p = p - step * (m / denom)
 *   with the scalars computed on the host in float64 and rounded ONCE to float32: wd = weight_decay, b1 = beta1, omb1 = 1 - beta1,
 *   b2 = beta2, omb2 = 1 - beta2, bc2s = sqrt(1 - beta2^t), eps, step = lr / (1 - beta1^t).  That is torch.optim.Adam with
 *   weight_decay as L2 on the gradient, behind torch.nn.utils.clip_grad_norm_.  The same thread stores p into the master
 *   parameters, the installed image and (layers >= 1) the transposed image of the backward pass; padding stays zero.
 *
 * gs_learner_stats waits for the step: loss = L; policy: surrogate = (1/n) sum s_i, entropy = (1/n) sum h_i, approx_kl = (1/n)
 * sum (lp_old - lp), clip_fraction = (1/n) sum clipped_i, value_loss NaN; critic: value_loss = L, the four policy figures NaN;
 * grad_norm (before clipping); step = the steps taken.  Reduced by ONE workgroup in the order of gs_episode_stats.  GS_E_STATE
 * before the first step.  gs_learner_info: the network's shape (any time after create).  gs_learner_download: host float32 copies
 * [param_count], any pointer may be NULL (grads: the last step's, before clipping and weight decay).  gs_learner_view: device
 * pointers of the last step's per-sample arrays, valid until the learner's next step or the next gs_rollout that grows the
 * rollout's buffers; consumer_stream as gs_onpolicy_batch. */
enum { GS_LEARNER_POLICY = 0, GS_LEARNER_VALUE = 1, GS_LEARNER_COST_VALUE = 2 /* + channel */ };
typedef struct gs_learner_config {
  int32_t struct_size;            /* = sizeof(gs_learner_config) */
  int32_t reserved;
  double lr, beta1, beta2, eps, weight_decay, max_grad_norm;
  double clip, ent_coef;          /* the policy's; ignored for a critic */
} gs_learner_config;
typedef struct gs_learner_stats_out {
  double loss, surrogate, entropy, approx_kl, clip_fraction, value_loss, grad_norm, step;
} gs_learner_stats_out;
typedef struct gs_learner_info_out {
  int32_t n_layers, activation;   /* GS_ACT_* */
  int32_t dims[5];                /* widths, dims[0] = obs_dim */
  int32_t rows_per_segment;
  int64_t param_count, step;
} gs_learner_info_out;
typedef struct gs_learner_view_out {
  int32_t n, reserved;
  const double* log_probs_new;    /* [n]; NULL for a critic, like ratio, clipped and entropy_terms */
  const double* ratio;            /* [n] */
  const int32_t* clipped;         /* [n] */
  const double* loss_terms;       /* [n] policy: s_i; critic: (v_i - ret_i)^2 */
  const double* entropy_terms;    /* [n] h_i */
} gs_learner_view_out;
int gs_learner_create(gs_handle* h, int32_t net, const gs_learner_config* cfg);
int gs_learner_step(gs_handle* h, int32_t net, const gs_onpolicy_batch_out* batch, int32_t n, void* consumer_stream);
int gs_learner_stats(gs_handle* h, int32_t net, gs_learner_stats_out* out);
int gs_learner_info(gs_handle* h, int32_t net, gs_learner_info_out* out);
int gs_learner_download(gs_handle* h, int32_t net, float* params, float* grads, float* m, float* v);
int gs_learner_view(gs_handle* h, int32_t net, gs_learner_view_out* out, void* consumer_stream);

/* ---- the learner's loss: advantage-weighted log-likelihood and expectile regression ----
 * The two in-sample losses of offline RL, as other heads behind the learner's unchanged matrix kernels.  Additive to ABI 2;
 * gs_learner_config is as it was.  A learner has ONE loss: GS_LOSS_DEFAULT (the policy's clipped surrogate, a critic's mean squared
 * error: everything "the learner" states), GS_LOSS_AWR (the policy only) or GS_LOSS_EXPECTILE (critics only).
 *
 * gs_learner_set_loss applies from the learner's next gs_learner_step.  It touches neither the parameters nor Adam's m, v and step
 * count nor the learner's generation number: a federation on the learner stays valid.  gs_learner_create resets the loss to
 * GS_LOSS_DEFAULT, and a *_set* entry that drops the learner drops its loss with it.  gs_learner_get_loss: the loss in force
 * (struct_size is written; fields the kind does not use hold what was last given, 0 after gs_learner_create).
 * GS_E_STATE: no live learner for `net`.  GS_E_INVALID, before anything changes: a wrong struct_size, an unknown net or kind,
 * GS_LOSS_AWR on a critic, GS_LOSS_EXPECTILE on the policy, NaN in any field, and for the kind's own fields temperature <= 0,
 * weight_max <= 0 (+inf is allowed for both) or expectile outside (0, 1).  Fields the kind does not use are otherwise ignored.
 *
 * GS_LOSS_AWR.  Sample i has the stored float64 action a, read through `indices` as the clipped surrogate reads it, and the batch's
 * float32 advantage A under whichever adv_norm the minibatches were prepared with.  ls_k, x_k, e_k, lp and h_i are the formulas of
 * "the learner", in the same order, nothing contracted.  In float64:
 *     u_i = exp(A / temperature);   w_i = fmin(u_i, weight_max);   capped_i = u_i > weight_max;   s_i = w_i lp
 *     L = -(1/n) sum_i s_i - ent_coef (1/n) sum_i h_i;      dL/dlp = -(w_i (1/n))
 *     dL/dmean_k and dL/dlog_std_k from dL/dlp as in "the learner": the clamp rule, - ent_coef / n, one rounding to float32.
 *   A / +inf = 0, so temperature = +inf gives w_i = 1 exactly: with weight_max = +inf that is behaviour cloning, L = -mean lp.  The
 *   weight is a constant of the gradient (no derivative through A).  ent_coef is gs_learner_config's; clip is ignored.  The rollout's
 *   log-probabilities are NOT read for the gradient: the step's refusal of a rollout that recorded none holds for GS_LOSS_DEFAULT
 *   only, so a random-action or uploaded-action rollout trains the policy.
 *   gs_learner_stats: surrogate = (1/n) sum s_i, entropy as before, clip_fraction = (1/n) sum capped_i, approx_kl = (1/n) sum
 *   (lp_old - lp) when the last rollout recorded log-probabilities and NaN otherwise, value_loss NaN.  gs_learner_view: ratio holds
 *   w_i, clipped holds capped_i, loss_terms holds s_i.
 *   Deviation from the reference: its AWR.update and IQL._update_actor weight the log-probability of an action freshly SAMPLED from
 *   the current policy (_get_action_and_log_prob(states)), not of the dataset's action.  This is the published algorithm, which
 *   weights the stored action's log-probability.
 * GS_LOSS_EXPECTILE (IQL's value loss), in float64 on the float32 value v_i and return ret_i:
 *     d = v_i - ret_i   (the reference's diff is -d);   q_i = (d < 0) ? tau : 1 - tau;   term0_i = q_i (d d)
 *     L = (1/n) sum_i term0_i;      dL/dv_i = q_i ((2.0 d) (1/n)), rounded once to float32
 *   At tau = 0.5 every head gradient is exactly half of the mean squared error's (a product with 0.5 is exact away from underflow),
 *   and so is the loss.  gs_learner_stats: loss = value_loss = L; gs_learner_view: loss_terms holds term0_i.
 * Both reduce their statistics in the order of gs_learner_stats, ONE workgroup of 1024 threads.  Everything else of a step -- forward
 * pass, backward pass, gradient reduction, Adam, determinism -- is "the learner"'s, by the same kernels. */
enum { GS_LOSS_DEFAULT = 0,       /* policy: clipped surrogate; critic: mean squared error */
       GS_LOSS_AWR = 1,           /* policy only */
       GS_LOSS_EXPECTILE = 2 };   /* critics only */
typedef struct gs_learner_loss {
  int32_t struct_size, kind;      /* = sizeof(gs_learner_loss); GS_LOSS_* */
  double temperature;             /* AWR: > 0, +inf allowed (unit weights: behaviour cloning) */
  double weight_max;              /* AWR: > 0, +inf allowed (no cap) */
  double expectile;               /* EXPECTILE: 0 < tau < 1 */
} gs_learner_loss;
int gs_learner_set_loss(gs_handle* h, int32_t net, const gs_learner_loss* loss);
int gs_learner_get_loss(gs_handle* h, int32_t net, gs_learner_loss* out);

/* ---- state-action critics: twin Q networks, target networks, TD targets, Q-based signals ----
 * The critic over concat(state, action) that the reference's value-based learners need (algorithms/offline.py: TwinCritic, IQL.update,
 * lines 454-545), beside the policy and the state critics.  Additive to ABI 2: no struct above changes, and a handle that calls none
 * of these entries computes what it computed before.
 *
 * The network.  gs_q_mlp_set(h, which, p, o) installs twin `which` (0 or 1): a gs_policy_mlp with head = GS_HEAD_LINEAR, dims[0] =
 * obs_dim + action_dim, dims[n_layers] = 1, stochastic = 0 and o->compute = GS_COMPUTE_F32, under the layer and width limits of
 * gs_value_mlp_set (GS_E_INVALID with a message otherwise, also for `which` outside 0 .. 1 and for action_dim = 0; the installed
 * network stays).  o->obs_shift / obs_scale have obs_dim entries and apply to the observation columns, in float64 and rounded once
 * as for the policy; the action columns enter as the stored float64 action rounded once to float32.  Installing packs the float32
 * image and makes a second copy of it, the TARGET image; it drops that network's learner.  NULL removes the network.
 * gs_q_mlp_check: the rules on the host alone.
 *
 * gs_rollout_evaluate_q (asynchronous, on the handle's stream, over the LAST rollout) writes float64 [T][B] arrays:
 *   q[src][which][t][b]   the value of twin `which` on the row (obs_seq[t][b], actions[t][b]), widened from float32, under the
 *                         online (src = 0) or the target (src = 1) image; for every installed twin.  A row's value depends on that
 *                         row and the image alone.
 *   q_min[src]            fmin over the installed twins (one twin installed: that twin)
 *   q_adv                 q_min[online] - values[t][b], one rounded subtraction (IQL's advantage, offline.py:523-526)
 *   td_target             r' + gamma * vnext, the r' and vnext of gs_rollout_evaluate's recurrence: the terminal value under
 *                         bootstrap_mask and 0 otherwise where the transition ended an episode, values[t + 1][b] where it did not;
 *                         nothing contracted (offline.py:504-505 with the bootstrap option)
 * values and terminal_values are the reward critic's: GS_E_STATE unless gs_rollout_evaluate has run on the last rollout, without a
 * rollout, and with no Q network installed; GS_E_INVALID as gs_rollout_evaluate.  gs_rollout_q_view: device pointers (NULL for a
 * twin that is not installed), valid until the next gs_rollout; consumer_stream as gs_rollout_onpolicy_view.
 * gs_rollout_q_download: host copies, any pointer may be NULL (a twin that is not installed is left unwritten).  Both are GS_E_STATE
 * unless gs_rollout_evaluate_q has run on the last rollout.
 *
 * The Q learner.  GS_LEARNER_Q + which is a learner like a critic's (create, stats, info, download, view, set_loss with
 * GS_LOSS_DEFAULT or GS_LOSS_EXPECTILE, federation); info.dims[0] = obs_dim + action_dim.  gs_learner_step reads the batch's
 * observations (float32, under the Q network's own observation normalisation, compared on the host as for every network) and
 * indices, and through the indices (clamped into the rollout) the rollout's float64 actions and td_target: the input row is the
 * batch row followed by (float)action, the regression target (float)td_target.  It needs gs_rollout_evaluate_q on the last rollout
 * (GS_E_STATE before any launch).  The forward pass, the head, the backward pass, the reduction and Adam are "the learner"'s; Adam
 * writes the ONLINE image.
 *
 * Signals.  gs_learner_set_signal(h, net, GS_SIGNAL_Q) makes the next steps of the policy read (float)q_adv through the indices in
 * place of the batch's advantages (which are then not required), and those of the reward critic (GS_LEARNER_VALUE) read
 * (float)q_min[target] in place of the batch's returns (offline.py:484-493); the heads are the same kernels on the gathered
 * values.  Such a step needs the batch's indices and gs_rollout_evaluate_q on the last rollout (GS_E_STATE).  GS_SIGNAL_Q on any
 * other network and an unknown signal are GS_E_INVALID; no live learner is GS_E_STATE.  Host state like the loss: Adam's state and
 * the generation stay; gs_learner_create and a *_set* entry reset it to GS_SIGNAL_BATCH.
 *
 * Target networks.  gs_q_target_update(h, tau) (asynchronous), over every installed twin and every float of the packed image:
 *   t = (tau32 * p) + (omt32 * t)     tau32 = (float)tau, omt32 = (float)(1 - tau) (the difference in float64, rounded once)
 * in float32, every operation rounded, none contracted; the padding stays 0; tau = 1 copies the online values, tau = 0 keeps the
 * target.  tau outside [0, 1] or not finite: GS_E_INVALID; no Q network: GS_E_STATE.  gs_q_target_download: the target's parameters,
 * float32, flat in torch order (P = the learner's param_count).  A federation (gs_fed_create accepts GS_LEARNER_Q + which) writes
 * master parameters and the online images; target images are left alone. */
enum { GS_LEARNER_Q = 5 /* + which */ };
enum { GS_SIGNAL_BATCH = 0, GS_SIGNAL_Q = 1 };
int gs_q_mlp_check(const gs_policy_mlp* p, const gs_policy_mlp_opts* o, int32_t obs_dim, int32_t action_dim);
int gs_q_mlp_set(gs_handle* h, int32_t which, const gs_policy_mlp* p, const gs_policy_mlp_opts* o);
typedef struct gs_q_eval_config {
  int32_t struct_size;            /* = sizeof(gs_q_eval_config) */
  int32_t bootstrap_mask;         /* as gs_gae_config */
  double gamma;
  double reward_shift, reward_scale;
} gs_q_eval_config;
int gs_rollout_evaluate_q(gs_handle* h, const gs_q_eval_config* cfg);
typedef struct gs_rollout_q {
  int32_t T, B, installed, rows_per_tile;   /* installed: bit `which` */
  const double* q[2][2];          /* [src][which], [T][B] each; NULL: twin not installed */
  const double* q_min[2];         /* [src] */
  const double* q_adv;
  const double* td_target;
} gs_rollout_q;
int gs_rollout_q_view(gs_handle* h, gs_rollout_q* out, void* consumer_stream);
typedef struct gs_rollout_q_host {
  double* q[2][2];
  double* q_min[2];
  double* q_adv;
  double* td_target;
} gs_rollout_q_host;
int gs_rollout_q_download(gs_handle* h, const gs_rollout_q_host* out);
int gs_learner_set_signal(gs_handle* h, int32_t net, int32_t signal);
int gs_learner_get_signal(gs_handle* h, int32_t net, int32_t* signal);
int gs_q_target_update(gs_handle* h, double tau);
int gs_q_target_download(gs_handle* h, int32_t which, float* params);

/* ---- the pathwise actor step: the policy's gradient through the twin Q networks ----
 * The actor update that SAC, TD3, DDPG + BC, MADDPG and CQL share (the reference's CQL._update_actor, algorithms/offline.py:230-244:
 * (alpha * log_prob - min(Q1, Q2)(s, pi(s))).mean() with pi(s) drawn by the reparameterisation trick, offline.py:114-136): the action
 * is sampled inside the step, the twins evaluate it, and dQ/da flows back into the policy.  Additive to ABI 2: no struct above
 * changes, GS_LOSS_* and GS_SIGNAL_* are as they were, and a handle that calls neither entry computes what it computed before.
 *
 * gs_learner_step_pathwise (asynchronous, on the handle's stream) steps the POLICY's learner alone, on the minibatch of n samples
 * gs_onpolicy_batch left in `batch`.  Every installed twin is used read-only (one twin installed: the minimum is that twin).  It
 * needs: a live learner for the policy AND for every installed twin (the twin's transposed images are what the backward pass
 * reads), at least one installed twin, gs_onpolicy_prepare on the last rollout with dtype GS_COMPUTE_F32, and obs_shift / obs_scale
 * bit-equal (compared on the host, per network) to the policy's and to every installed twin's observation normalisation:
 * GS_E_STATE otherwise.  It reads batch->observations, and batch->indices when bc_coef != 0 only; neither recorded
 * log-probabilities nor batch->advantages nor gs_rollout_evaluate_q.  GS_E_INVALID: a wrong struct_size, alpha or bc_coef NaN,
 * negative or infinite, stochastic outside {0, 1}, n outside 1 .. 2^24, a missing pointer.  Every check runs before any launch.
 *
 * Per sample i.  Layers in float32 on the matrix cores (gs_learner_step's kernels), heads in float64 on float32 values, head
 * gradients rounded once to float32, nothing contracted:
 *     ls_k = clamp(log_std_k, -20, 2);   std_k = exp(ls_k)
 *     eps_k = component k & 3 of the four normals (the recipe of the load noise: words (0, 1) and (2, 3) one Box-Muller pair each,
 *             cosine then sine) of Philox4x32-10 with counter (i, k >> 2, draw, 'PWNO' = 0x50574E4F) and key seed;
 *             0 when stochastic == 0 (the deterministic actor a = tanh(mean))
 *     x_k = mean_k + std_k * eps_k;   a_k = tanh(x_k)
 *     lp = sum_k (((-0.5 eps_k) eps_k - ls_k) - 0.5 log(2 pi)) - log((1 - a_k a_k) + 1e-6)      in action order from k = 0
 *   exp, tanh and log above are NOT a math library's: they are sums of rounded float64 +, -, *, / (frexp, ldexp and rint are exact),
 *   so that a host restates the heads to the bit whatever library it has (a library's own functions agree across machines to an
 *   ulp only).  With LN2_HI = 0x1.62e42feep-1, LN2_LO = 0x1.a39ef35793c76p-33, every sum by Horner's rule from the last term:
 *     exp(x):   k = rint(x * 1.4426950408889634);  r = (x - k LN2_HI) - k LN2_LO;  p = sum_{j=0..17} r^j / j!;  ldexp(p, k)
 *     tanh(x):  u = min(|x|, 40);  u < 0.5:  y = 2 u,  m = y * sum_{j=1..23} y^(j-1) / j!,  t = m / (m + 2);
 *               else  e = exp(-2 u),  t = (1 - e) / (1 + e);  copysign(t, x)
 *     log(v):   (m, e) = frexp(v);  m < 0.7071067811865476: m = 2 m, e = e - 1;  f = m - 1;  s = f / (2 + f);  z = s s;
 *               P = sum_{j=1..15} z^(j-1) / (2 j + 1);  t2 = 2 s;  e LN2_HI + (e LN2_LO + (t2 + t2 (z P)))
 *   (1 / j! and 1 / (2 j + 1) are the rounded float64 quotients; 0.5 log(2 pi) is 0.91893853320467274178.)  Each lies within 4 ulp
 *   of the correctly rounded value on the heads' ranges.  lp is gs_logp_term's expression (policy_head.h) with this log.
 *   The twins' input row is [obs_i | (float)a_k].  Twin w runs forward with saved activations and gives q_w (float32, widened); the
 *   head gradient 1.0f goes into its last layer's delta, the backward pass runs to the first layer's delta0, and
 *     dqda_w[i][k] = sum_j delta0[i][j] * W0[j][obs_dim + k]      W0: the twin's float32 master parameters; float32 products and sums,
 *                                                                 j ascending from 0 in ONE chain: the order depends on H0 alone
 *     w* = (q_0 <= q_1) ? 0 : 1 (one twin: that twin);   qmin = q_{w*}
 *     bc_i = sum_k (a_k - s_k)(a_k - s_k)      s: the stored float64 action, read through the clamped index; 0 when bc_coef == 0
 *     term_i = (alpha * lp - qmin) + bc_coef * bc_i;      L = (1/n) sum_i term_i
 *     G_k = ((((alpha * (2 a_k)) / ((1 - a_k a_k) + 1e-6) - dqda_{w*}[k]) + (2 bc_coef) (a_k - s_k)) * (1 - a_k a_k)) / n
 *     dL/dmean_k = G_k
 *     dL/dlog_std_k = (G_k * std_k) * eps_k - alpha / n   where -20 <= log_std_k <= 2, and 0 outside
 *   Then the policy's backward pass, gradient reduction, statistics and Adam are "the learner"'s, by the same kernels: Adam rewrites
 *   the installed policy image, and the policy learner's step count advances.  The twins' parameters, gradients, Adam state, step
 *   counts, online and target images are not written.  A row's action, log-probability, q and dqda depend on that row, the
 *   parameters, seed and draw alone.
 * gs_learner_stats on the policy afterwards: loss = L, surrogate = (1/n) sum qmin_i, entropy = -(1/n) sum lp_i, approx_kl,
 * clip_fraction and value_loss NaN, grad_norm as ever; reduced by ONE workgroup in the order of gs_episode_stats.
 * gs_learner_pathwise_view: device pointers of the last pathwise step's arrays (GS_E_STATE without one); q[w] and dq_da[w] are
 * NULL for a twin that was not installed.  Lifetime and consumer_stream as gs_learner_view; gs_learner_view on the policy is
 * GS_E_STATE after a pathwise step (its arrays belong to gs_learner_step). */
typedef struct gs_pathwise_config {
  int32_t struct_size;            /* = sizeof(gs_pathwise_config) */
  int32_t stochastic;             /* 0: eps = 0, the deterministic actor a = tanh(mean) */
  double alpha, bc_coef;          /* finite, >= 0 */
  uint64_t seed;
  uint32_t draw, reserved;
} gs_pathwise_config;
typedef struct gs_pathwise_view_out {
  int32_t n, action_dim, installed, pre_head_stride;   /* installed: bit `which` */
  const float* pre_head;          /* [n] rows of pre_head_stride floats, the first 2 A of a row: mean | log_std as the heads read them;
                                     the learners' shared scratch: valid until the next step of ANY learner of the handle */
  const double* actions;          /* [n][A] */
  const double* noise;            /* [n][A] */
  const double* log_probs;        /* [n] */
  const double* q[2];             /* [n] each */
  const double* q_min;            /* [n] */
  const double* bc_terms;         /* [n] */
  const double* loss_terms;       /* [n] term_i */
  const int32_t* which;           /* [n] w* */
  const float* dq_da[2];          /* [n][A] each */
} gs_pathwise_view_out;
int gs_learner_step_pathwise(gs_handle* h, const gs_onpolicy_batch_out* batch, int32_t n, const gs_pathwise_config* cfg, void* consumer_stream);
int gs_learner_pathwise_view(gs_handle* h, gs_pathwise_view_out* out, void* consumer_stream);

/* ---- policy-action TD targets: Q_target(s', pi(s')) - alpha log pi(a' | s') ----
 * The Bellman target of SAC, TD3 + BC, DDPG and the Bellman half of CQL (the reference's CQL._update_critic, algorithms/offline.py:
 * 173-178): the POLICY's action at the next state, valued by the target twins.  Additive to ABI 2: no struct above changes, and a
 * handle that calls none of these entries computes what it computed before.
 *
 * gs_rollout_evaluate_q_next (asynchronous, on the handle's stream, over the LAST rollout) needs a rollout, at least one installed
 * twin and an installed policy with GS_COMPUTE_F32 and GS_HEAD_GAUSSIAN_TANH (GS_E_STATE otherwise); it does not need
 * gs_rollout_evaluate.  GS_E_INVALID: a wrong struct_size, a bootstrap_mask, gamma, reward_shift or reward_scale gs_rollout_evaluate
 * refuses, alpha NaN, negative or infinite, stochastic outside {0, 1}.  Every check runs before any launch.  With i = t B + b the
 * index of transition (t, b), whose next state is the row obs_seq[t + 1][b]:
 *   next_pre_head[i][0 .. 2A)   float32, mean | log_std of the installed policy on that row: the float32 layers of the policy's
 *                               compute path (float64 normalisation rounded once, products and sums on the matrix cores), 64 rows a tile
 *   next_actions[i][A], next_log_probs[i]     the sampling head of "the pathwise actor step", operation for operation in float64
 *                               on those float32 values with ITS exp, tanh and log, nothing contracted; eps_k is component k & 3 of
 *                               Philox4x32-10 with counter (i, k >> 2, draw, 'QNXT' = 0x514E5854) and key seed, 0 when stochastic
 *                               == 0 (a = tanh(mean)); lp in ONE chain from k = 0
 *   next_noise[i][A]            eps as the head used it
 *   q_next[which][i]            the value of twin `which` under its TARGET image on (obs_seq[t + 1][b], next_actions[i]), as q[1]
 *                               of gs_rollout_evaluate_q is on the stored action
 *   q_next_min[i]               fmin over the installed twins (one twin: that twin)
 *   td_target[i]                r' + gamma * v;  r' = (rew - reward_shift) * reward_scale;  v = q_next_min[i] - alpha *
 *                               next_log_probs[i] where the transition did not end an episode, term_value[e] where it did and its
 *                               flag meets bootstrap_mask, 0 otherwise.  Every product and every sum rounded, in that order: alpha *
 *                               lp, the difference, gamma * v, the sum.  bootstrap_mask 0 is the reference's (1 - terminals).
 * Under a non-zero mask (and a terminal list) entry e of the terminal list, for the transition (t, b) of term_idx[e], gets
 * term_pre_head / term_actions / term_noise / term_log_probs / term_q[which] / term_q_min / term_value the same way on its terminal observation,
 * with the noise counter (t B + b, k >> 2, draw, 'QNTE' = 0x514E5445): the list's order does not enter.  Entries in list order, the
 * first terminal_count of them; under mask 0 they are not written.
 * A row's outputs depend on that row, the images, seed, draw and its transition's index alone.  The arrays are made on first use,
 * sized by the rollout's capacity, and go with the rollout's buffers; gs_policy_mlp_set* and gs_q_mlp_set make the evaluation stale,
 * a learner's step does not: the targets are those of the last evaluation (re-evaluate between epochs).
 * gs_rollout_q_next_view: device pointers (NULL for a twin that is not installed), valid until the next gs_rollout; consumer_stream
 * as gs_rollout_onpolicy_view.  gs_rollout_q_next_download: host copies, any pointer may be NULL; the terminal arrays take the
 * terminal count of the last rollout.  Both are GS_E_STATE unless gs_rollout_evaluate_q_next has run on the last rollout.
 *
 * gs_q_set_target_source(h, source): which array a step of GS_LEARNER_Q + which regresses on through the batch's indices:
 * GS_Q_TARGET_VALUE (the default) td_target of gs_rollout_evaluate_q, GS_Q_TARGET_POLICY td_target of gs_rollout_evaluate_q_next,
 * which must then be current on the last rollout (GS_E_STATE before any launch) while gs_rollout_evaluate_q need not be.  Host state
 * of the handle; an unknown value is GS_E_INVALID.  Signals (GS_SIGNAL_Q) read gs_rollout_evaluate_q's arrays whatever the source. */
enum { GS_Q_TARGET_VALUE = 0, GS_Q_TARGET_POLICY = 1 };
typedef struct gs_q_next_config {
  int32_t struct_size;            /* = sizeof(gs_q_next_config) */
  int32_t bootstrap_mask;         /* as gs_gae_config */
  int32_t stochastic;             /* 0: eps = 0, the deterministic actor a' = tanh(mean) */
  int32_t reserved;
  double gamma, alpha;            /* alpha: finite, >= 0 */
  double reward_shift, reward_scale;
  uint64_t seed;
  uint32_t draw, reserved2;
} gs_q_next_config;
int gs_rollout_evaluate_q_next(gs_handle* h, const gs_q_next_config* cfg);
typedef struct gs_rollout_q_next {
  int32_t T, B, installed, rows_per_tile;   /* installed: bit `which` */
  int32_t action_dim, terminal_capacity;    /* terminal arrays: terminal_capacity entries allocated, NULL under bootstrap_mask 0 */
  const float* next_pre_head;     /* [T][B][2 A] */
  const double* next_actions;     /* [T][B][A] */
  const double* next_noise;       /* [T][B][A] eps as the head used it */
  const double* next_log_probs;   /* [T][B] */
  const double* q_next[2];        /* [which], [T][B] each; NULL: twin not installed */
  const double* q_next_min;
  const double* td_target;
  const float* term_pre_head;     /* [terminal_capacity][2 A] */
  const double* term_actions;     /* [terminal_capacity][A] */
  const double* term_noise;
  const double* term_log_probs;   /* [terminal_capacity] */
  const double* term_q[2];
  const double* term_q_min;
  const double* term_value;
} gs_rollout_q_next;
int gs_rollout_q_next_view(gs_handle* h, gs_rollout_q_next* out, void* consumer_stream);
typedef struct gs_rollout_q_next_host {
  float* next_pre_head;
  double* next_actions;
  double* next_noise;
  double* next_log_probs;
  double* q_next[2];
  double* q_next_min;
  double* td_target;
  float* term_pre_head;           /* the first terminal_count entries are written */
  double* term_actions;
  double* term_noise;
  double* term_log_probs;
  double* term_q[2];
  double* term_q_min;
  double* term_value;
} gs_rollout_q_next_host;
int gs_rollout_q_next_download(gs_handle* h, const gs_rollout_q_next_host* out);
int gs_q_set_target_source(gs_handle* h, int32_t source);
int gs_q_get_target_source(gs_handle* h, int32_t* source);

/* ---- the conservative critic step: a twin's regression plus the logsumexp penalty ----
 * The critic update of CQL (the reference's CQL._update_critic with CQL._compute_cql_loss, algorithms/offline.py:166-228), per twin w
 * on n minibatch rows:
 *     L_w = mse(Q_w(s, a_data), y) + conservative_weight * (logsumexp_j q_j - mean_i Q_w(s_i, a_data_i))
 * where j runs over ALL 3 n values Q_w(s, a_data) | Q_w(s, a_uniform) | Q_w(s, a_policy): the logsumexp runs over the BATCH, as the
 * reference's logsumexp(dim=0) does (not per state, as the CQL paper's).  The twins share no parameter, so the reference's summed
 * loss separates into one step per twin.  Additive to ABI 2: no struct above changes, and a handle that never calls these entries
 * computes what it computed before.
 *
 * gs_learner_step_conservative (asynchronous, on the handle's stream) steps the learner of twin net = GS_LEARNER_Q + which alone, on
 * the minibatch of n samples gs_onpolicy_batch left in `batch`.  It needs (GS_E_STATE otherwise): everything gs_learner_step needs
 * for that Q learner under the current gs_q_set_target_source (gs_rollout_evaluate_q, or gs_rollout_evaluate_q_next under
 * GS_Q_TARGET_POLICY, on the last rollout); the Q learner's loss at GS_LOSS_DEFAULT; a live learner for the POLICY (GS_COMPUTE_F32,
 * GS_HEAD_GAUSSIAN_TANH), whose network is read and not written; obs_shift / obs_scale bit-equal to the policy's and to this twin's
 * normalisation; 1 <= action_dim <= 128.  GS_E_INVALID: a wrong struct_size, a net that is not GS_LEARNER_Q + {0, 1},
 * conservative_weight NaN, negative or infinite, stochastic outside {0, 1}, n outside 1 .. 2^24 / 3, a batch without observations
 * or indices.  Every check runs before any launch.
 *
 * Per step, nothing contracted.  The twin's input rows j in [0, 3 n): [0, n) the data block, [n, 2 n) the uniform block, [2 n, 3 n)
 * the policy block; all three carry the observation columns of batch row j mod n.  With i = j mod n:
 *   data action      the stored float64 action through the clamped index, rounded once (gs_learner_step's rule); y_i = (float)td[idx_i]
 *   uniform action   u_k = ((double)word + 0.5) * 2^-31 - 1.0, word = word k & 3 of Philox4x32-10 with counter (i, k >> 2, draw,
 *                    'CQLU' = 0x43514C55) and key seed: exact in float64, strictly inside (-1, 1); the column is (float)u_k
 *   policy action    the sampling head of "the pathwise actor step", operation for operation, on the policy learner's pre-head values
 *                    of row i, its noise under the tag 'CQLN' = 0x43514C4E in place of 'PWNO'; 0 noise when stochastic == 0
 * Q1 and Q2 stepped with the same seed and draw see the same candidate actions: neither step writes the policy.
 * One forward pass of the twin over the 3 n rows with saved activations gives q_j (float32, widened).  ONE workgroup of 1024 threads:
 *     m = max_j q_j;   d_j = q_j - m;   e_j = d_j < -700 ? 0 : exp(d_j)      exp and log: those of "the pathwise actor step"
 *     S = sum_j e_j      thread t adds j = t, t + 1024, ... ascending from 0.0, then the balanced tree over the 1024 threads
 *     lse = m + log(S);   qbar = (sum_{i < n} q_i) / n  in the same order;   penalty = lse - qbar
 * The head, per row, with inv_n = 1.0 / n, p_j = e_j / S and cw = conservative_weight:
 *     data rows:        dq = q_i - (double)y_i;  term_i = dq * dq;  g = (2.0 * dq) * inv_n + cw * (p_i - inv_n)
 *     candidate rows:   g = cw * p_j
 *     dL/dq_j = (float)g
 * Then the twin's backward pass, gradient reduction (ceil(3 n / 256) segments), statistics and Adam are "the learner"'s over the
 * 3 n rows, by the same kernels: Adam rewrites the ONLINE image of twin `which`, and its step count advances.  The other twin, the
 * policy and both target images are not written.  A row's q depends on that row and the parameters alone.
 * gs_learner_stats on that net afterwards: value_loss = (sum_i term_i) / n, surrogate = penalty, loss = value_loss + cw * penalty,
 * entropy, approx_kl and clip_fraction NaN, grad_norm as ever.
 * gs_learner_conservative_view: device pointers of the LAST conservative step's arrays, whichever twin took it (GS_E_STATE without
 * one).  Lifetime and consumer_stream as gs_learner_pathwise_view; pre_head lies in the learners' shared scratch.  gs_learner_view
 * on that Q net is GS_E_STATE after a conservative step (its arrays belong to gs_learner_step). */
typedef struct gs_conservative_config {
  int32_t struct_size;            /* = sizeof(gs_conservative_config) */
  int32_t stochastic;             /* policy candidates: 1 sampled, 0 tanh(mean) */
  double conservative_weight;     /* finite, >= 0 (the reference's default is 5.0) */
  uint64_t seed;
  uint32_t draw, reserved;
} gs_conservative_config;
typedef struct gs_conservative_view_out {
  int32_t net, n, action_dim, pre_head_stride;
  const float* pre_head;          /* [n] rows of pre_head_stride floats, the first 2 A of a row: the policy's mean | log_std; the
                                     learners' shared scratch: valid until the next step of ANY learner of the handle */
  const double* random_actions;   /* [n][A] u_k */
  const double* policy_actions;   /* [n][A] */
  const double* policy_noise;     /* [n][A] */
  const double* policy_log_probs; /* [n] */
  const float* targets;           /* [n] y_i */
  const double* q;                /* [3 n] */
  const double* weights;          /* [3 n] p_j */
  const double* loss_terms;       /* [n] term_i */
  const double* scalars;          /* [4] m, S, lse, qbar */
} gs_conservative_view_out;
int gs_learner_step_conservative(gs_handle* h, int32_t net, const gs_onpolicy_batch_out* batch, int32_t n, const gs_conservative_config* cfg,
                                 void* consumer_stream);
int gs_learner_conservative_view(gs_handle* h, gs_conservative_view_out* out, void* consumer_stream);

/* ---- per-minibatch targets: refresh the rollout's bootstrap signals over a row list ----
 * The reference recomputes every bootstrap quantity inside each update(batch), with the networks as they are at that moment
 * (algorithms/offline.py:173-178 for CQL, :482-540 for IQL); gs_rollout_evaluate_q and gs_rollout_evaluate_q_next write them once over
 * the whole rollout.  gs_learner_refresh re-evaluates the selected groups for the n transitions of a minibatch with the images as
 * they are NOW and writes the results into the same per-rollout arrays at those transitions' positions; every other position keeps
 * its bits.  The learner's steps read those arrays through the batch's indices, so no step changes.  Additive to ABI 2: no struct
 * above changes, and a handle that never calls this entry computes what it computed before.
 *
 * gs_learner_refresh (asynchronous, on the handle's stream) reads batch->indices alone: j_i = t B + b, clamped into the rollout as
 * gs_learner_step clamps it.  Groups (bits of `groups`; several may be set, they run in this order):
 *   GS_REFRESH_TD_POLICY   "policy-action TD targets" at j: the installed policy on the next state (noise counter (j, k >> 2, draw,
 *                          'QNXT'), key seed), the TARGET twins on its action; writes next_pre_head, next_actions, next_noise,
 *                          next_log_probs, q_next[which], q_next_min and td_target at j.  Where done[j] & bootstrap_mask and the
 *                          transition has a terminal entry e, also that entry's term_* arrays (tag 'QNTE', the entry's (t, b)),
 *                          term_value[e], and td_target[j] from it.  Rounding order: that section's.  Needs gs_rollout_evaluate_q_next
 *                          on the last rollout under the SAME bootstrap_mask, so that every row holds the result of some evaluation.
 *   GS_REFRESH_Q_TARGET    the TARGET twins on (s_j, a_j): q[target][which][j], q_min[target][j] of gs_rollout_evaluate_q.
 *   GS_REFRESH_TD_VALUE    the installed value network on the next state of j (on the terminal observation where done[j] &
 *                          bootstrap_mask and an entry exists; 0 for any other finished transition): td_target[j] of
 *                          gs_rollout_evaluate_q = r' + gamma * vnext.  The values stay in the refresh's scratch: values, advantages
 *                          and returns of gs_rollout_evaluate are NOT written.
 *   GS_REFRESH_Q_ADV       the value network on s_j and the ONLINE twins on (s_j, a_j): q[online][which][j], q_min[online][j], q_adv[j]
 *                          = q_min - V, one rounded subtraction.
 * The last three need gs_rollout_evaluate_q on the last rollout; the last two an installed value network; TD_POLICY a policy with
 * GS_COMPUTE_F32 and GS_HEAD_GAUSSIAN_TANH; every group an installed twin: GS_E_STATE otherwise.  GS_E_INVALID: a wrong struct_size,
 * groups 0 or an unknown bit, what gs_rollout_evaluate refuses of bootstrap_mask / gamma / reward_shift / reward_scale, alpha NaN,
 * negative or infinite, stochastic outside {0, 1}, n outside 1 .. 2^24, a batch without indices.  Every check runs before any launch:
 * a refused call leaves every array's bits as they were.
 * A refreshed row holds exactly the bits a full gs_rollout_evaluate_q_next / gs_rollout_evaluate_q under the same config and images
 * leaves there (a row's outputs depend on that row, the images, seed, draw and its transition's index alone).  An index may occur
 * more than once in a batch: the duplicates compute the same bits from the same inputs, so their colliding stores are benign.
 * The views and downloads of those two evaluations stay as they are and show the refreshed rows.  consumer_stream: as
 * gs_learner_step. */
enum { GS_REFRESH_TD_POLICY = 1, GS_REFRESH_Q_TARGET = 2, GS_REFRESH_TD_VALUE = 4, GS_REFRESH_Q_ADV = 8 };
typedef struct gs_refresh_config {
  int32_t struct_size;            /* = sizeof(gs_refresh_config) */
  int32_t groups;                 /* GS_REFRESH_* bits */
  int32_t bootstrap_mask;         /* as gs_gae_config */
  int32_t stochastic;             /* TD_POLICY: 0: eps = 0, a' = tanh(mean) */
  double gamma, alpha;            /* alpha: finite, >= 0 (TD_POLICY) */
  double reward_shift, reward_scale;
  uint64_t seed;
  uint32_t draw, reserved;
  uint64_t reserved2;
} gs_refresh_config;
int gs_learner_refresh(gs_handle* h, const gs_onpolicy_batch_out* batch, int32_t n, const gs_refresh_config* cfg, void* consumer_stream);

/* ---- the federation: clipped, noised federated averaging over the learners of K handles, in place ----
 * K handles of ONE process and ONE device, each with a live learner for the same network `net` (GS_LEARNER_*), form a federation.
 * A round measures the clients' updates against the global parameters, clips them, averages them, adds Gaussian noise and writes
 * the new global parameters into EVERY client's master parameters, forward image and transposed image -- on the device, no weight
 * on the host, Adam's moments and step counts kept.  Additive to ABI 2.
 *
 * gs_fed_create: 1 <= n_clients <= GS_FED_MAX_CLIENTS distinct handles on one device, else GS_E_INVALID.  Every client must hold a
 * live learner for `net` (GS_E_STATE).  All clients must agree in layer count, widths and activation, and their networks'
 * observation normalisation (the handles' host copies) must be bit-equal: GS_E_INVALID otherwise -- an average of weights behind
 * different normalisations is not an average of functions.  The global parameters g are float32 [P] in torch order (as the
 * learner's), owned by the federation and snapshotted from client 0's master parameters.  NO client is written by create.
 * gs_fed_set_global is the explicit broadcast: g (params != NULL: taken from the host first) goes, bit for bit, into every
 * client's master parameters and images; moments and step counts are left alone.
 *
 * Lifetime.  The federation keeps the handles, never their buffers, and remembers the generation of each client's learner (every
 * gs_learner_create advances it).  A client whose learner was dropped (its network installed again) or created again since
 * gs_fed_create, or that was gs_destroy'ed, makes every call below GS_E_STATE, the message naming the client; only gs_fed_destroy
 * still succeeds (it may run before or after the clients' gs_destroy).  Every check runs before anything is launched: a refused
 * call changes nothing.
 *
 * Streams.  The federation has a stream of its own.  A call that reads or writes the clients (set_global, measure, aggregate)
 * first makes that stream wait for an event recorded on every client's stream -- queued learner steps finish first -- and
 * (set_global, aggregate) afterwards makes every client's stream wait for the federation's event: the client's next
 * gs_learner_step, gs_rollout or network installation is ordered after the round without a host wait.  Only gs_fed_measure,
 * gs_fed_stats and gs_fed_download wait on the host (set_global with host parameters waits for its own previous upload only).
 *
 * Arithmetic: float64 on the float32 values, every product and sum rounded, nothing contracted.  The participants (indices into
 * the clients, each at most once, 1 <= n <= n_clients) are taken in the order of the list; p_k: participant k's master parameters.
 *     d_k[j] = (double)p_k[j] - (double)g[j]
 *     G_ik   = sum_j d_i[j] d_k[j]                       norm_k = sqrt(G_kk)
 *     c_k    = clip_norm > 0 ? min(1, clip_norm / (norm_k + 1e-6)) : 1              (the form of Adam's clip)
 *     u_k    = server_lr * (w_k / W),  W = w_0 + w_1 + ... in list order            (host, float64)
 *     a_k    = u_k * c_k                                                            (device)
 *     s[j]   = ((0 + a_0 d_0[j]) + a_1 d_1[j]) + ...                                (ascending k)
 *     g'[j]  = (float)( ((double)g[j] + s[j]) + noise_std * z[j] )                  (the noise term only when noise_std > 0)
 *   z[j] = component j & 3 of the four normals of one Philox4x32-10 call with counter (j >> 2, round, net, 'FEDN' = 0x4645444E)
 *   and key `seed`, by the recipe of the environment's load noise: every output word w is a uniform (w + 1/2) 2^-32, words (0, 1)
 *   and (2, 3) are one Box-Muller pair each -- sqrt(-2 log u_a) cos(2 pi u_b), then the sine.
 *   The order of a sum G_ik: a workgroup of 256 threads takes 1024 consecutive parameters, thread t the parameters base + t,
 *   base + 256 + t, base + 512 + t, base + 768 + t in that order; the 256 sums go through the butterfly of the learner's gradient
 *   norm (xor 32, 16, ..., 1 within a wavefront, then xor 2, 1 over the four wavefronts).  ONE workgroup of 1024 threads per
 *   entry then adds the workgroups' sums, thread t those of workgroups t, t + 1024, ..., and the same butterfly over 16 wavefronts
 *   (the order of gs_episode_stats).  No floating-point atomics: the bits of G are a function of the parameters alone, G is
 *   symmetric bit for bit, and gs_fed_aggregate -- which computes the diagonal only, with the same kernels -- finds the norms
 *   that gs_fed_measure reports as sqrt(G_kk), bit for bit.
 *   Consequences: clients all equal to g give g' == g bit for bit (a parameter -0 becomes +0).  ONE participant with weight 1,
 *   server_lr 1, no clip and no noise makes g' the participant's parameters bit for bit wherever p - g is exact in float64 (the
 *   exponents of p[j] and g[j] less than 29 apart) -- in general g + (p - g) is p to within 2^-52 of the larger of the two.
 *
 * gs_fed_aggregate (asynchronous) runs one round: one thread per parameter computes g'[j] and stores it into g and, for ALL
 * n_clients clients -- a client that sat the round out starts its next one from the global model -- into the master parameters,
 * the client's slot of the forward image and (layers >= 1) of the transposed image; padding is never written and stays zero.
 * reset_moments != 0: the same thread zeroes every client's m and v, and the clients' step counts become 0; otherwise Adam's
 * state is left as it is.  GS_E_INVALID: a wrong struct_size, n_participants < 1, a participant out of range or named twice,
 * a weight that is not finite or negative, weights that sum to 0, or a clip_norm, noise_std or server_lr that is not finite or
 * below 0.
 * gs_fed_measure: the Gram matrix [n][n] (row-major, host) of the listed participants' updates; changes nothing.
 * gs_fed_stats: the last round's figures (GS_E_STATE before the first round).  gs_fed_download: g, host float32 [param_count].
 * gs_fed_info: the shape.  gs_fed_destroy: waits for the federation's stream and frees what it owns; the clients stay as they are. */
typedef struct gs_fed gs_fed;
enum { GS_FED_MAX_CLIENTS = 32 };
typedef struct gs_fed_info_out {
  int32_t n_clients, net;
  int64_t param_count, rounds;     /* rounds: gs_fed_aggregate calls that ran */
  int32_t block_params;            /* parameters per workgroup of the reductions (1024) */
  int32_t reserved;
} gs_fed_info_out;
typedef struct gs_fed_round {
  int32_t struct_size;             /* = sizeof(gs_fed_round) */
  int32_t n_participants;
  const int32_t* participants;     /* [n] indices into the clients */
  const double* weights;           /* [n] the reference's num_samples */
  double clip_norm, noise_std, server_lr;      /* clip_norm 0: no clipping; noise_std 0: no noise */
  uint64_t seed;
  uint32_t round;
  int32_t reset_moments;
} gs_fed_round;
typedef struct gs_fed_stats_out {
  double norm[GS_FED_MAX_CLIENTS];             /* per participant, in list order: norm_k, c_k, a_k */
  double clip_scale[GS_FED_MAX_CLIENTS];
  double coefficient[GS_FED_MAX_CLIENTS];
  double noise_std;
  int64_t rounds;
  uint32_t round;
  int32_t n;
} gs_fed_stats_out;
int gs_fed_create(gs_handle* const* clients, int32_t n_clients, int32_t net, gs_fed** out);
int gs_fed_destroy(gs_fed* f);
int gs_fed_info(gs_fed* f, gs_fed_info_out* out);
int gs_fed_set_global(gs_fed* f, const float* params);
int gs_fed_measure(gs_fed* f, const int32_t* participants, int32_t n, double* gram);
int gs_fed_aggregate(gs_fed* f, const gs_fed_round* r);
int gs_fed_stats(gs_fed* f, gs_fed_stats_out* out);
int gs_fed_download(gs_fed* f, float* global_params);

/* ---- parameter anchors: FedProx's proximal term and elastic weight consolidation on a Fisher diagonal ----
 * Two terms on the PARAMETERS of a learner (net: GS_LEARNER_*, the learner's own ids), added to the reduced gradient of every step
 * -- gs_learner_step, gs_learner_step_pathwise and gs_learner_step_conservative alike -- before the statistics and Adam:
 *     PROX:  L += mu / 2 * sum_p (w_p - a_p)^2                 a: the PROX centre, float32 [P] in torch order
 *     EWC:   L += lambda / 2 * sum_p A_p (w_p - c_p)^2         A: the consolidated importance, c: the consolidated centre, float32 [P]
 * Both coefficients are 0 after gs_learner_create, and while both are 0 no launch, buffer or bit of a step differs from a learner
 * that never heard of anchors.  Nothing is allocated until an entry below is called.  Additive to ABI 2.
 *
 * The term (gs_k_train_anchor, queued right behind the gradient's reduction, only when a coefficient is non-zero).  Per parameter,
 * all float32, every operation rounded, nothing contracted, in this order (w: the master parameter, g: the reduced gradient):
 *     mu != 0:      g = g + mu * (w - a)
 *     lambda != 0:  g = g + lambda * (A * (w - c))
 * with mu = float32(prox_mu) and lambda = float32(ewc_lambda), the host's doubles rounded once.  The result replaces the gradient:
 * grad_norm, the norm clip, Adam and gs_learner_download's grads see the TOTAL gradient, as torch.nn.utils.clip_grad_norm_ behind
 * (loss + penalty).backward() does.  A difference of zero adds +0: the step right after gs_learner_anchor_here(NULL) has the
 * gradient of a step without the term, bit for bit.  The gradient norm's per-workgroup sums are recomputed on the new gradient in
 * the tree of the reduction (four per thread in order, a butterfly over 256 threads); three more per-workgroup float64 sums in the
 * same tree keep sum g_loss^2 (the gradient before the terms), sum d^2 with d = w - a, and sum A (d d) with d = w - c (d the
 * float32 difference the gradient used; the squares and products in float64, each rounded).
 *
 * gs_learner_anchor_here sets the PROX centre: params_host == NULL: a device copy of the learner's current master parameters
 * (queued behind its steps); otherwise P floats in torch order taken from the host.  It does not change prox_mu.
 * gs_learner_anchor_set / _get: the coefficients, read by the next step (a queued step keeps the ones it was queued with).  Both
 * must be finite and >= 0 (GS_E_INVALID; gs_learner_anchor_check holds these rules on the host alone, as gs_cost_config_check).
 * prox_mu > 0 without a PROX centre and ewc_lambda > 0 before the first gs_learner_fisher_commit are GS_E_STATE.
 *
 * The Fisher diagonal of a task.  gs_learner_fisher_begin zeroes the pending sum (float64 [P]) and the sample count.
 * gs_learner_fisher_accumulate has exactly the preconditions and argument rules of gs_learner_step for that net under its current
 * loss (GS_LOSS_*) and signal; without a begin since the last commit or clear it is GS_E_STATE.  It runs gs_learner_step's
 * gather (where the net has one), forward pass, head and backward-data pass, then
 *     pending[p] += sum_i (d l_i / d theta_p)^2        over the n samples, l_i the per-sample terms of L = (1/n) sum_i l_i
 * computed as the weight-gradient product on squared operands: per layer sum_i ((float)n delta_i)^2 (a_i)^2 on the float32 matrix
 * cores with the geometry, chains and join order of the step's weight gradient ((float)n delta undoes the 1/n the heads put into
 * delta; the bias: sum_i ((float)n delta_i)^2), one partial per segment of rows_per_segment rows, the partials added in ascending
 * segment order in float32, the result widened and added to pending.  This is the per-sample (empirical) Fisher diagonal on the
 * learner's OWN loss -- not the square of a whole batch's gradient, which equals it at n = 1 only.  It changes no master
 * parameter, image, m, v, step count, statistic or grads; the per-sample arrays of gs_learner_view become those of this pass (the
 * clip or cap flags the Fisher was taken under among them).  The pathwise and conservative steps couple the samples of a batch and are not offered.
 * gs_learner_fisher_commit ends the task with the CURRENT master parameters w as its optimum:
 *     F   = max((float)(pending / samples), (float)min_importance)                      min_importance finite and >= 0
 *     A'  = decay A + F                                                                 decay in (0, 1]: 1 sums the tasks, < 1 is online EWC
 *     c'  = ((decay A) c + F w) / A'                                                    (w where A' is 0)
 * per parameter in float64, each rounded once to float32; the first commit gives A = F, c = w.  Zero samples or no begin is
 * GS_E_STATE.  The pending sum and its count stay readable until the next begin.  Because sum_k F_k (p - p_k) = A (p - c) in
 * real arithmetic (decay 1), the GRADIENT is that of the sum over tasks of F_k / 2 (p - p_k)^2 for any number of tasks at the cost
 * of two arrays; the penalty VALUE differs from that sum by a constant that does not depend on p.
 *
 * gs_learner_anchor_clear: which = GS_ANCHOR_PROX, GS_ANCHOR_EWC or both; a cleared slot loses its arrays, its coefficient
 * becomes 0 (GS_ANCHOR_EWC also ends an open task and zeroes the task count).
 * gs_learner_anchor_stats (waits): of the last step taken with a non-zero coefficient (GS_E_STATE before one):
 *     penalty_prox = prox_mu / 2 * sum (w - a)^2,  penalty_ewc = ewc_lambda / 2 * sum A (w - c)^2   at the parameters BEFORE Adam,
 *     the workgroups' sums added on the host in ascending order; grad_norm_loss = the norm before the terms, the workgroups' sums
 *     added in the order of gs_learner_stats' grad_norm: by bits what gs_learner_stats would have reported without the terms;
 *     tasks = commits merged into the EWC slot, fisher_samples = the samples of the pending sum.
 * gs_learner_anchor_download: host copies, float32 [P] (prox, ewc_importance, ewc_centre) and float64 [P] (fisher_pending); any
 * pointer may be NULL; a slot that holds nothing is GS_E_STATE when asked for.
 * Lifetime: gs_learner_create and installing the network again drop everything here, as they drop the learner.  Every check runs
 * before anything is launched: a refused call changes nothing.  An unknown net or a wrong struct_size is GS_E_INVALID, a net
 * without a live learner GS_E_STATE. */
enum { GS_ANCHOR_PROX = 1, GS_ANCHOR_EWC = 2 };
typedef struct gs_learner_anchor_config {
  int32_t struct_size;             /* = sizeof(gs_learner_anchor_config) */
  int32_t reserved;
  double prox_mu, ewc_lambda;
} gs_learner_anchor_config;
typedef struct gs_fisher_config {
  int32_t struct_size;             /* = sizeof(gs_fisher_config) */
  int32_t reserved;
  double min_importance;           /* the reference's importance_threshold (1e-3 there) */
  double decay;                    /* (0, 1] */
} gs_fisher_config;
typedef struct gs_learner_anchor_stats_out {
  double penalty_prox, penalty_ewc, grad_norm_loss;
  double prox_mu, ewc_lambda;      /* the coefficients of that step */
  int64_t tasks, fisher_samples;
} gs_learner_anchor_stats_out;
int gs_learner_anchor_check(const gs_learner_anchor_config* cfg);
int gs_learner_anchor_here(gs_handle* h, int32_t net, const float* params_host);
int gs_learner_anchor_set(gs_handle* h, int32_t net, const gs_learner_anchor_config* cfg);
int gs_learner_anchor_get(gs_handle* h, int32_t net, gs_learner_anchor_config* out);
int gs_learner_fisher_begin(gs_handle* h, int32_t net);
int gs_learner_fisher_accumulate(gs_handle* h, int32_t net, const gs_onpolicy_batch_out* batch, int32_t n, void* consumer_stream);
int gs_learner_fisher_commit(gs_handle* h, int32_t net, const gs_fisher_config* cfg);
int gs_learner_anchor_clear(gs_handle* h, int32_t net, int32_t which);
int gs_learner_anchor_stats(gs_handle* h, int32_t net, gs_learner_anchor_stats_out* out);
int gs_learner_anchor_download(gs_handle* h, int32_t net, float* prox, float* ewc_importance, float* ewc_centre, double* fisher_pending);

/* ---- checkpoint / resume: [B][state_dim] float64 blob ------------
 * layout per instance: time, step, constraint_violations, total_losses, episode_reward,
 * frequency, irradiance, wind, temperature, cloud, seed_lo, seed_hi,
 * soc[n_bats], battery_power[n_bats], curtailment[n_gens], Vm[n], Va[n], flow[m], loading[m] */
int gs_get_state(gs_handle* h, double* state);
int gs_set_state(gs_handle* h, const double* state);

/* ---- multi-GPU: one optional exchange per step, RCCL all-gather of observations over
 * xGMI.  RCCL is dlopen'ed on first use. --------------------------- */
int gs_comm_unique_id(uint8_t id_out[128]);
int gs_comm_init(gs_handle* h, const uint8_t id[128], int32_t rank, int32_t world_size);
/* gathers this handle's device-resident obs [B][obs_dim] from all ranks into a device
 * buffer [world*B][obs_dim]; obs_full_host may be NULL (stay on device) */
int gs_allgather_obs(gs_handle* h, double* obs_full_host);
int gs_comm_destroy(gs_handle* h);
/* What the communicator reports about this member: asked of RCCL itself (ncclCommCount, ncclCommUserRank, ncclCommCuDevice,
 * ncclGetVersion; -1 where the library lacks the entry point), plus the HIP device's UUID -- so that the output of an N-rank
 * run shows N ranks on N distinct devices.  transport: 1 RCCL, 2 the in-process loopback (nranks / rank from the group). */
typedef struct gs_comm_info_t {
  int32_t transport, nranks, rank, device, comm_device, rccl_version, reserved0, reserved1;
  uint8_t device_uuid[16];
} gs_comm_info_t;
int gs_comm_info(gs_handle* h, gs_comm_info_t* out);
/* The in-process transport: `nshards` handles of ONE process (shard r built with first_instance = r * B; normally all on
 * one device) form the communicator, rank = position in `shards`.  A member's compact block reaches the others by
 * device-to-device copies on their exchange streams where RCCL would move it over xGMI; compaction, slot offsets,
 * expansion, constant columns, the double-buffered observation buffers and their events are the code the RCCL transport
 * runs.  With this transport gs_allgather_obs completes when the LAST member has called (a grouped call): earlier callers
 * return at once, their obs_full_host (if any) is filled by that last call.  What it is for: rehearsing and testing the
 * N > 1 exchange on a box with fewer GPUs than ranks (tests/test_gpu_loopback.py; bench.py flags such a run
 * "transport": "loopback"), and a single process that keeps several shards on one GPU. */
int gs_comm_init_loopback(gs_handle* const* shards, int32_t nshards);
/* The form SURVEY.md section 8(b) specified: one call gathers for every member (all members of one loopback communicator,
 * or the RCCL ranks one process drives, issued as one ncclGroup); obs_full_host: NULL or [nshards * B][obs_dim], filled
 * from shard 0's gathered block (every member's is the same). */
int gs_allgather_obs_shards(gs_handle* const* shards, int32_t nshards, double* obs_full_host);
/* The gathered block where it lies, [world * B][obs_dim] in rank order, for a learner on the GPU (valid until the member's
 * next gather completes).  consumer_stream (hipStream_t as void*): made to wait on the device for the gather; NULL: the
 * call returns when the gather has finished.  gs_allgather_obs_download is the host copy of the same block. */
typedef struct gs_gathered_obs {
  const double* observations;
  int64_t rows;                   /* world * B */
  int32_t obs_dim, rank, world, reserved;
} gs_gathered_obs;
int gs_allgather_obs_view(gs_handle* h, gs_gathered_obs* out, void* consumer_stream);
int gs_allgather_obs_download(gs_handle* h, double* obs_full_host);

/* ---- measurement: HIP-event timing of every kernel launched on the handle's stream ------ */
enum { GS_K_UNPACK = 0, GS_K_ENV_PRE = 1, GS_K_SOLVE = 2, GS_K_ENV_POST = 3, GS_K_PACK = 4, GS_K_COUNT = 5 };
/* on = 1: a HIP event pair around every launch (per-kernel totals; the events themselves cost a few us per launch);
 * on = 2: ONE event pair around everything launched until the next gs_timing_read -- call that right after the last
 * launch of the region; it returns the span as the time of the most-launched kernel, i.e. duration + gaps per launch */
int gs_timing_enable(gs_handle* h, int32_t on);
/* diagnostic build aid: the first call arms per-phase cycle counters inside the solver kernels
 * (block 0 / wave 0; phases: prologue, init, mismatch, bottom-up, flag, top-down, final mismatch,
 * epilogue), later calls return the sums accumulated since the previous call and clear them. */
int gs_debug_stamps(gs_handle* h, uint64_t* cycles_out, int32_t n);
/* The host-side schedule of the meshed Newton-Raphson step kernel (gs_k_step_nr_mesh2; csrc/mesh_schedule.h) for a topology,
 * built WITHOUT a device: the block elimination that replaces np.linalg.solve (power_flow.py:186-190) as per-(wavefront, row,
 * sub-group) items, pull lists and Ybus rows.  header[16]: ok, n_levels, n_rows, max_rows_per_wave, n_pivots, msg_units,
 * n_messages, n_accumulators, max_degree, unit_bytes, zero_off, dummy_off, body_off, region_bytes, item_bytes, n_adj.  unit_budget:
 * the message units the level assignment tries to stay below (0: levels as early as possible).  Call once
 * with the arrays NULL for the sizes (items: nw * ni * 8 records of item_bytes; rowinfo: nw * ni * 4; adj_y: 2 * n_adj), then
 * with buffers.  tests/test_mesh_schedule.py replays the tables in NumPy against a dense solve. */
int gs_mesh_schedule_dump(const gs_topology* topo, int32_t zero_z_mode, int32_t nw, int32_t ni, int32_t acc_cap, int32_t unit_budget, int32_t region_base,
                          int32_t slot_bytes, int32_t* header, char* why, int32_t why_cap, void* items, int32_t* rowinfo,
                          int32_t* adj_off, double* adj_y);
/* The same schedule as the kernel reads it: 16 words per item (GS_MESH_W_*, csrc/gs_internal.h), rowinfo with the neighbour count
 * of the packed form, the Ybus table it stages in LDS ((n_pairs + 1) off-diagonal entries, then the diagonal entry of every
 * voltage slot) and the neighbour lists.  counts[4]: n_pairs, doubles of ytab, entries of adj_ent, words per item; arrays may be
 * NULL (first call).  GS_E_TOPOLOGY if the feeder is not eligible. */
/* Test aid, host arithmetic only: the constant linear map of the meshed member's first Newton step from the flat start,
 * x = W [P_spec of the non-slack buses in bus order; 1] (power_flow.py:125-134 flat start, :243-287 exact Jacobian, :186-190 solve; Q_spec = 0),
 * W row-major [2 (n - 1)][n]: rows (d theta, d|V|) per non-slack bus, last column the constant term.  All-PQ networks only. */
int gs_flat_newton_map_dump(const gs_topology* topo, int32_t zero_z_mode, double* out);
int gs_mesh_schedule_dump_packed(const gs_topology* topo, int32_t zero_z_mode, int32_t nw, int32_t ni, int32_t acc_cap, int32_t unit_budget, int32_t region_base,
                                 int32_t slot_bytes, int32_t* counts, int32_t* packed, int32_t* rowinfo, double* ytab, int32_t* adj_ent);
/* Diagnostic: (start, end) of each of the first n_blocks workgroups of the last step launch, in ticks of the GPU's 100 MHz
 * real-time clock (second-generation step kernels; arm with gs_debug_stamps while GS_STAMP_BLOCK_TIMES is set). */
int gs_debug_block_times(gs_handle* h, uint64_t* out, int32_t n_blocks);
/* total_ms[GS_K_COUNT], launches[GS_K_COUNT] accumulated since the last call; resets them */
int gs_timing_read(gs_handle* h, double* total_ms, int64_t* launches);
/* test aid: overwrite one family of device rows with values[B][width] (width = n, m or 1), so that kernels
 * reading the device state (the post-step checks below) can be driven with fixture data */
enum { GS_ROWS_VM = 0, GS_ROWS_LINE_LOADING = 1, GS_ROWS_ENV_LINE_LOADING = 2, GS_ROWS_LINE_FLOW = 3, GS_ROWS_FREQUENCY = 4,
       GS_ROWS_CONVERGED = 5, GS_ROWS_ITERATIONS = 6, GS_ROWS_MAX_MISMATCH = 7,
       GS_ROWS_LOAD_POWER = 8 /* [n_loads] realised load powers of the last step (dynamics.py:54-75) */, GS_ROWS_COUNT = 9 };
int gs_debug_write_rows(gs_handle* h, int32_t which, const double* values);
/* test aid: the same families read back as values[B][width] (what the statistical tests of the stochastic load
 * model look at: the realised load powers are not part of the observation, grid_env.py:769-770) */
int gs_debug_read_rows(gs_handle* h, int32_t which, double* values);
/* test aid: the kernels' own square root, division and logarithm (csrc/fastmath.h) applied on the current device to host arrays of
 * n elements, out[i] = op(in_a[i] [, in_b[i]]); in_b may be NULL except for the division.  Element i is thread i of a launch of
 * 256-thread workgroups: elements 64 k .. 64 k + 63 share a wavefront. */
enum { GS_FASTMATH_SQRT = 0 /* gs_sqrt_fast(a) */, GS_FASTMATH_DIV = 1 /* gs_div_fast(a, b) */, GS_FASTMATH_LOG01 = 2 /* gs_log01(a) */,
       GS_FASTMATH_SQRT_CORE = 3 /* gs_sqrt_core(a): a in [2^-767, +inf) only */, GS_FASTMATH_COUNT = 4 };
int gs_debug_fastmath(int32_t op, int64_t n, const double* in_a, const double* in_b, double* out);

/* ======================================================================================
 * Post-step checks on the state a step / solve left on the device.
 * Replaces, batched and without a host round trip of voltages and loadings:
 *   SafetyChecker.check_constraints / is_safe / get_violation_severity   utils/safety.py:114-203
 *   SafetyMonitor.check_constraints                                      utils/safety.py:313-394
 *   AdvancedRobustPowerFlowSolver._assess_solution_quality               environments/robust_power_flow.py:615-657
 * A gs_checks object is bound to one gs_handle (it reads that handle's device state and runs on
 * its stream) and carries what the reference classes carry between calls: the previous voltages
 * and frequency (rate-of-change limits), the consecutive-violation counter and the sticky
 * emergency mode.  thermal_data is not modelled, so severity never reaches GS_SEVERITY_CRITICAL.
 * ====================================================================================== */
enum {  /* rows of gs_checks_view.ints, each [B]; C_ = SafetyChecker, M_ = SafetyMonitor */
  GS_CI_C_NLOW = 0, GS_CI_C_NHIGH, GS_CI_C_FLOW, GS_CI_C_FHIGH, GS_CI_C_NOVER, GS_CI_C_VRATE, GS_CI_C_FRATE, GS_CI_C_TOTAL,
  GS_CI_C_SEVERITY,   /* 0 safe, 1 low, 2 medium, 3 high, 4 critical (safety.py:188-203) */
  GS_CI_M_NHIGH, GS_CI_M_NLOW, GS_CI_M_NEMERG, GS_CI_M_FHIGH, GS_CI_M_FLOW, GS_CI_M_FEMERG, GS_CI_M_NOVER, GS_CI_M_TOTAL,
  GS_CI_M_ACTION,     /* emergency_action_required */
  GS_CI_M_CONSEC, GS_CI_M_EMODE, GS_CI_COUNT
};
enum { GS_CF_VRATE = 0, GS_CF_FRATE, GS_CF_QUALITY, GS_CF_COUNT };   /* rows of gs_checks_view.reals, each [B] */
enum {  /* bits of gs_checks_view.bus_mask[b][i] / line_mask[b][k] */
  GS_BM_C_LOW = 1, GS_BM_C_HIGH = 2, GS_BM_M_LOW = 4, GS_BM_M_HIGH = 8, GS_BM_M_EMERGENCY = 16,
  GS_LM_C_OVERLOAD = 1, GS_LM_M_OVERLOAD = 2
};

typedef struct gs_checks_config {
  int32_t struct_size;             /* = sizeof(gs_checks_config) */
  int32_t loading_source;          /* 0: |S|/rating of the load-flow solution (PowerFlowSolution.line_loadings);
                                      1: the environment's |P|/rating (Line.update_state, base.py:261-264) */
  double voltage_limits[2], frequency_limits[2], line_loading_limit;      /* SafetyChecker.__init__, safety.py:100-112 */
  double rate_voltage, rate_frequency, timestep;
  double mon_voltage_limits[2], mon_frequency_limits[2], mon_line_loading_limit;   /* SafetyMonitor.__init__, :296-311 */
  double mon_emergency_voltage[2], mon_emergency_frequency[2];
  double quality_tolerance;        /* the solver tolerance `_assess_solution_quality` compares max_mismatch with */
} gs_checks_config;

typedef struct gs_checks_view {    /* host buffers, any may be NULL */
  int32_t* ints;                   /* [GS_CI_COUNT][B] */
  double* reals;                   /* [GS_CF_COUNT][B] */
  uint8_t* bus_mask;               /* [B][n] */
  uint8_t* line_mask;              /* [B][m] */
} gs_checks_view;

typedef struct gs_checks gs_checks;

int gs_checks_create(gs_handle* h, const gs_checks_config* cfg, gs_checks** out);
void gs_checks_destroy(gs_checks* c);
/* frequency per instance for handles without an environment (solver-only); NULL = back to the handle's own */
int gs_checks_set_frequency(gs_checks* c, const double* frequency_hz);
/* one check_constraints call per instance on the handle's current device state (asynchronous) */
int gs_checks_run(gs_checks* c);
int gs_checks_download(gs_checks* c, const gs_checks_view* out);
/* forget previous state, counters and emergency mode of the masked instances (NULL = all): a freshly
 * constructed SafetyChecker() / SafetyMonitor() */
int gs_checks_reset(gs_checks* c, const uint8_t* mask);
/* HIP-event timing of gs_checks_run is off unless enabled (a per-step check over a long run records nothing) */
int gs_checks_timing_enable(gs_checks* c, int32_t on);
int gs_checks_timing_read(gs_checks* c, double* total_ms, int64_t* launches);
/* on != 0: every later gs_step / gs_step_device evaluates these checks inside its own kernel (the epilogue already holds
 * the voltages and loadings), exactly as one gs_checks_run after the step would; gs_checks_download then returns the
 * checks of the last step.  Do not call gs_checks_run as well (the stateful parts would advance twice).  One fused checks
 * object per handle; the environment's |P| / rating or the solution's |S| / rating as configured. */
int gs_checks_set_fused(gs_checks* c, int32_t on, int32_t want_masks);

/* ======================================================================================
 * Three-phase unbalanced radial load flow (BASELINE.json config 5).  NEW functionality: the
 * reference names UnbalancedPowerFlow (README.md:187-197, API_REFERENCE.md:420) but contains no
 * implementation, so there is no reference interface to cite beyond the solver plug point
 * (environments/power_flow.py:38-46) whose record layout the outputs follow, with a phase axis.
 * Mapping differs from the single-phase path: one workgroup per instance (networks of thousands
 * of nodes, batches of ~1000).  Feeders of up to ~9 700 phase conductors stay in that workgroup's
 * registers and LDS for the whole solve, the sweeps evaluated as prefix sums over depth-first
 * orders of the tree (csrc/gridstep3_resident.h); larger ones are swept level by level through HBM.
 * ====================================================================================== */
typedef struct gs3_topology {
  int32_t struct_size;            /* = sizeof(gs3_topology) */
  int32_t n;                      /* nodes; node `source` is the three-phase source (slack) */
  int32_t source;
  int32_t reserved;
  const int32_t* parent;          /* [n] upstream node of each node, -1 for the source */
  const uint8_t* phases;          /* [n] bit mask (1 = a, 2 = b, 4 = c) of the phases the node's upstream line carries;
                                     must be a subset of the parent's mask; the source has 7 */
  const double* z_re;             /* [n][3][3] series impedance of the upstream line, per unit (ignored for the source) */
  const double* z_im;             /* [n][3][3] */
  const double* v_source;         /* [3] source voltage magnitudes; angles are 0, -120, +120 degrees */
} gs3_topology;

typedef struct gs3_solution_view {
  double* v_re;                   /* [B][n][3] phase-to-neutral voltage, rectangular; absent phases = 0 */
  double* v_im;                   /* [B][n][3] */
  double* losses;                 /* [B] total real losses (sum over phases) */
  double* max_mismatch;           /* [B] */
  int32_t* iterations;            /* [B] */
  uint8_t* converged;             /* [B] */
} gs3_solution_view;

typedef struct gs3_handle gs3_handle;

int gs3_create(const gs3_topology* topo, double tolerance, int32_t max_iterations, int32_t batch, int32_t device,
               gs3_handle** out);
void gs3_destroy(gs3_handle* h);
const char* gs3_last_error(const gs3_handle* h);
/* P_spec / Q_spec [B][n][3]: net injection per node and phase (generation - load), per unit */
int gs3_solve(gs3_handle* h, const double* P_spec, const double* Q_spec, const gs3_solution_view* out);
/* device-resident variant for measurement */
int gs3_upload_injections(gs3_handle* h, const double* P_spec, const double* Q_spec);
int gs3_solve_device(gs3_handle* h);
int gs3_download_solution(gs3_handle* h, const gs3_solution_view* out);
int gs3_synchronize(gs3_handle* h);
/* average milliseconds of the solve kernel over the launches since the last call (HIP events) */
int gs3_timing_read(gs3_handle* h, double* total_ms, int64_t* launches);
int gs3_describe(const gs3_handle* h, char* buf, int32_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* GRIDSTEP_H */
