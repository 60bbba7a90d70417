"""MI355X-native batched AC power-flow env.step() -- drop-in for the hot path of
danieleschmidt/grid-fed-rl-gym (GridEnvironment.step / NewtonRaphsonSolver.solve).

Host side is plain Python + NumPy over a C-ABI shared library (libgridstep.so, ctypes);
all arithmetic on the path runs in hand-written HIP kernels for gfx950.  There is no CPU
fallback: importing the solver/environment classes works anywhere, but constructing them
without the built library or without a GPU raises.
"""
from .components import (Bus, Line, Load, PowerFlowSolution, BatchedPowerFlowSolution,
                         PowerFlowError, InvalidActionError)
from .feeders import (FeederSpec, flatten_feeder, flatten_network, to_objects, reference_env_network,
                      with_reference_env_renewables, simple_radial, ieee13_like, ieee123_like,
                      random_meshed, scalable_like, randomized_line_impedances, randomized_load_powers)

from .solver import (BatchedNewtonRaphsonSolver, NewtonRaphsonSolver, FastDecoupledSolver,
                     BatchedForwardBackwardSweepSolver, BatchedRobustPowerFlowSolver, DistributionPowerFlow, parallel_power_flow_batch,
                     injections_from_dicts)
from .env import BatchedGridEnvironment, VectorizedEnvironment, Box
from .rollout import (collect_random_data, collect_policy_data, collect_onpolicy_data, evaluate_rollout, gae_np, rollout_device, GridDataset,
                      DeviceGridDataset, ConstraintLimits, costs_np, rollout_costs_np, rollout_costs, evaluate_rollout_costs,
                      constraint_values, collect_constrained_data, episodes_np, rollout_episodes, EpisodeRecords, EpisodeMonitor,
                      evaluate_policy, permutation_np, onpolicy_batch_np, OnPolicyBatches, evaluate_rollout_q, q_rollout_np, td_target_np,
                      q_combine_np, polyak_np, evaluate_rollout_q_next, policy_rows_np, q_next_noise_np, td_policy_np,
                      refresh_targets, refresh_rows_np, load_rollout_data, transitions_to_rollout, rollout_to_transitions, concat_rollouts,
                      download_rollout, save_rollout, load_rollout, continue_rollout, rollout_window_np, ReplayWindow)
from .policy import MLPPolicy, MLPValue, MLPQ
from .learner import (DeviceLearner, ppo_grad_np, value_grad_np, awr_grad_np, expectile_grad_np, pathwise_grad_np, pathwise_noise_np, adam_np,
                      split_parameters, anchor_term_np, anchor_penalty_terms_np, fisher_np, fisher_importance_np, ewc_merge_np)
from .federated import FederatedLearners, fedavg_np, fed_noise_np, filter_outliers_np, gaussian_sigma
from .sharding import LoopbackShards, ShardedGridEnvironment, shard_range
from .multi_agent import AgentConfig, BatchedMultiAgentWrapper
from .feeders import feeder_from_dict, feeder_to_dict, network_dict_normalized
from .safety import BatchedSafetyChecker, BatchedSafetyMonitor, PostStepChecks, device_quality_score
from .unbalanced import UnbalancedPowerFlow, UnbalancedFeederSpec, UnbalancedSolution, unbalanced_from_single_phase, ieee8500_like

__all__ = [
    "BatchedNewtonRaphsonSolver", "NewtonRaphsonSolver", "FastDecoupledSolver",
    "BatchedForwardBackwardSweepSolver", "BatchedRobustPowerFlowSolver", "DistributionPowerFlow", "parallel_power_flow_batch",
    "injections_from_dicts", "BatchedGridEnvironment", "VectorizedEnvironment", "Box",
    "collect_random_data", "collect_policy_data", "rollout_device", "MLPPolicy", "MLPValue", "collect_onpolicy_data", "evaluate_rollout", "gae_np", "GridDataset", "DeviceGridDataset",
    "ConstraintLimits", "costs_np", "rollout_costs_np", "rollout_costs", "evaluate_rollout_costs", "constraint_values", "collect_constrained_data",
    "episodes_np", "rollout_episodes", "EpisodeRecords", "EpisodeMonitor", "evaluate_policy",
    "permutation_np", "onpolicy_batch_np", "OnPolicyBatches",
    "MLPQ", "evaluate_rollout_q", "q_rollout_np", "td_target_np", "q_combine_np", "polyak_np",
    "evaluate_rollout_q_next", "policy_rows_np", "q_next_noise_np", "td_policy_np",
    "refresh_targets", "refresh_rows_np",
    "load_rollout_data", "transitions_to_rollout", "rollout_to_transitions", "concat_rollouts", "download_rollout", "save_rollout", "load_rollout",
    "continue_rollout", "rollout_window_np", "ReplayWindow",
    "DeviceLearner", "ppo_grad_np", "value_grad_np", "awr_grad_np", "expectile_grad_np", "pathwise_grad_np", "pathwise_noise_np", "adam_np", "split_parameters",
    "anchor_term_np", "anchor_penalty_terms_np", "fisher_np", "fisher_importance_np", "ewc_merge_np",
    "FederatedLearners", "fedavg_np", "fed_noise_np", "filter_outliers_np", "gaussian_sigma",
    "ShardedGridEnvironment", "LoopbackShards", "shard_range",
    "AgentConfig", "BatchedMultiAgentWrapper", "feeder_from_dict", "feeder_to_dict", "network_dict_normalized",
    "BatchedSafetyChecker", "BatchedSafetyMonitor", "PostStepChecks", "device_quality_score",
    "UnbalancedPowerFlow", "UnbalancedFeederSpec", "UnbalancedSolution", "unbalanced_from_single_phase", "ieee8500_like",
    "Bus", "Line", "Load", "PowerFlowSolution", "BatchedPowerFlowSolution", "PowerFlowError",
    "InvalidActionError", "FeederSpec", "flatten_feeder", "flatten_network", "to_objects",
    "reference_env_network", "with_reference_env_renewables", "simple_radial", "ieee13_like",
    "ieee123_like", "random_meshed", "scalable_like", "randomized_line_impedances", "randomized_load_powers",
]
__version__ = "0.1.0"
