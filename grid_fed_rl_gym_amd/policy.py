"""MLP policies for closed-loop rollouts on the device (``gs_rollout`` with ``GS_POLICY_MLP``, include/gridstep.h).

The reference's actors are plain MLPs (algorithms/base.py:157-177 ``_build_mlp``: ``Linear`` + relu / tanh / elu, sizes
``[obs_dim] + [256, 256(, 256)] + [2 * action_dim]``) whose head is ``tanh(mean)`` or
``tanh(mean + exp(clamp(log_std, -20, 2)) * eps)`` (algorithms/offline.py:69-76, 114-136).  ``MLPPolicy`` holds such a network
as NumPy arrays, hands it to the device (``env.set_policy`` / ``rollout_device(policy=...)`` / ``collect_policy_data``) and
restates its forward pass in NumPy (``forward_np``) -- what the device kernel is tested against.  NumPy only: a torch module is
read through duck typing (``from_sequential``), torch itself is never imported here.

Two compute paths.  "float64" (the default) folds ``GridDataset``'s normalisation into the first layer and runs every layer in
float64.  "float32" is the precision of the reference's torch actors: the normalisation stays a stage of its own,
``z = (obs - mean) * (1 / std)`` in float64 on the raw observation and ONE rounding to float32 (a raw 1e5-watt column rounded to
float32 first loses 2.4e-3 W, which a folded weight multiplies and the layer sums over every such column); weights, biases,
products, sums and hidden activations are float32; the head is evaluated in float64 on the float32 pre-head values.

``MLPValue`` is a critic for ``env.set_value`` / ``evaluate_rollout``: the same layers with a scalar output, on the float32 path.
"""
from __future__ import annotations

from typing import Any, List, Optional, Sequence

import numpy as np

from . import _lib

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0       # algorithms/offline.py:73


class MLPPolicy:
    """``weights[l]`` [out, in] (torch's ``Linear.weight`` layout) and ``biases[l]`` [out] of 1 .. 4 linear layers,
    ``activation`` ("relu" | "tanh" | "elu") between them, ``head`` "tanh" (last width = action_dim) or "gaussian_tanh" (last
    width = 2 * action_dim: mean | log_std, as ``torch.chunk`` splits).  ``obs_mean`` / ``obs_std``: ``GridDataset``'s observation
    normalisation, folded into the first layer here (``W1' = W1 / std``, ``b1' = b1 - W1 (mean / std)``), so that the policy --
    and the device kernel -- take raw observations.  ``compute``: "float64" or "float32" (the module docstring); either way
    ``weights`` / ``biases`` are the folded float64 arrays, and ``weight0`` / ``bias0`` / ``obs_mean`` / ``obs_std`` keep the
    unfolded first layer and the normalisation (mean 0 and std 1 if none was given) for the float32 path."""

    def __init__(self, weights: Sequence[Any], biases: Sequence[Any], activation: str = "relu", head: str = "gaussian_tanh",
                 obs_mean: Optional[Any] = None, obs_std: Optional[Any] = None, compute: str = "float64") -> None:
        if compute not in _lib.COMPUTE:
            raise ValueError(f"compute must be one of {sorted(_lib.COMPUTE)}, got {compute!r}")
        self.compute = compute
        if activation not in _lib.ACTIVATION:
            raise ValueError(f"activation must be one of {sorted(_lib.ACTIVATION)}, got {activation!r}")
        if head not in _lib.HEAD:
            raise ValueError(f"head must be one of {sorted(_lib.HEAD)}, got {head!r}")
        if len(weights) != len(biases) or not 1 <= len(weights) <= _lib.GS_POLICY_MAX_LAYERS:
            raise ValueError(f"1 .. {_lib.GS_POLICY_MAX_LAYERS} layers with one bias each, got {len(weights)} weights and {len(biases)} biases")
        self.weights: List[np.ndarray] = [np.array(w, dtype=np.float64) for w in weights]
        self.biases: List[np.ndarray] = [np.array(b, dtype=np.float64) for b in biases]
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            if w.ndim != 2 or b.shape != (w.shape[0],):
                raise ValueError(f"layer {l}: weights must be [out, in] and biases [out], got {w.shape} and {b.shape}")
            if l and w.shape[1] != self.weights[l - 1].shape[0]:
                raise ValueError(f"layer {l} takes {w.shape[1]} inputs, layer {l - 1} gives {self.weights[l - 1].shape[0]}")
        self.activation, self.head = activation, head
        if (obs_mean is None) != (obs_std is None):
            raise ValueError("obs_mean and obs_std go together")
        self.weight0, self.bias0 = self.weights[0].copy(), self.biases[0].copy()
        self.obs_mean: Optional[np.ndarray] = None
        self.obs_std: Optional[np.ndarray] = None
        if obs_mean is not None:
            mean = np.asarray(obs_mean, dtype=np.float64).reshape(-1)
            std = np.asarray(obs_std, dtype=np.float64).reshape(-1)
            if mean.shape != (self.obs_dim,) or std.shape != (self.obs_dim,):
                raise ValueError(f"obs_mean / obs_std must have shape ({self.obs_dim},)")
            w1 = self.weights[0]
            self.biases[0] = self.biases[0] - w1 @ (mean / std)
            self.weights[0] = w1 / std[None, :]
            self.obs_mean, self.obs_std = mean.copy(), std.copy()

    @property
    def obs_dim(self) -> int:
        return int(self.weights[0].shape[1])

    @property
    def action_dim(self) -> int:
        out = int(self.weights[-1].shape[0])
        return out // 2 if self.head == "gaussian_tanh" else out

    @classmethod
    def from_sequential(cls, module: Any, head: str = "gaussian_tanh", obs_mean: Optional[Any] = None,
                        obs_std: Optional[Any] = None, compute: str = "float64") -> "MLPPolicy":
        """From a torch ``nn.Sequential`` of ``Linear`` and activation modules (what ``_build_mlp`` returns), by duck typing:
        a child with ``weight`` and ``bias`` is a linear layer (read through ``.detach().cpu().numpy()``), any other child
        names the activation by its class (ReLU / Tanh / ELU)."""
        names = {"ReLU": "relu", "Tanh": "tanh", "ELU": "elu"}
        weights, biases, acts = [], [], []
        for child in module:
            if hasattr(child, "weight") and hasattr(child, "bias"):
                weights.append(child.weight.detach().cpu().numpy().astype(np.float64))
                biases.append(child.bias.detach().cpu().numpy().astype(np.float64))
            else:
                kind = names.get(type(child).__name__)
                if kind is None:
                    raise ValueError(f"from_sequential: unsupported module {type(child).__name__}")
                if kind == "elu" and float(getattr(child, "alpha", 1.0)) != 1.0:
                    raise ValueError("from_sequential: ELU with alpha != 1")
                if len(acts) != len(weights) - 1:
                    raise ValueError("from_sequential: one activation behind every linear layer but the last")
                acts.append(kind)
        if len(acts) != len(weights) - 1 or len(set(acts)) > 1:
            raise ValueError("from_sequential: one and the same activation behind every linear layer but the last")
        return cls(weights, biases, activation=acts[0] if acts else "relu", head=head, obs_mean=obs_mean, obs_std=obs_std,
                   compute=compute)

    def to_struct(self, stochastic: bool = False):
        """(gs_policy_mlp, the arrays it points into): the folded layers for compute "float64", the unfolded ones for
        "float32" (``to_opts`` carries their normalisation)."""
        if stochastic and self.head != "gaussian_tanh":
            raise ValueError("a stochastic policy needs the Gaussian head")
        if self.compute == "float32":
            return _lib.policy_struct([self.weight0] + self.weights[1:], [self.bias0] + self.biases[1:], self.activation, self.head, stochastic)
        return _lib.policy_struct(self.weights, self.biases, self.activation, self.head, stochastic)

    def to_opts(self):
        """(gs_policy_mlp_opts or None, the arrays it points into): None for compute "float64" (plain gs_policy_mlp_set),
        GS_COMPUTE_F32 with obs_shift = mean and obs_scale = 1 / std for "float32"."""
        if self.compute != "float32":
            return None, None
        if self.obs_mean is None:
            return _lib.policy_opts("float32")
        return _lib.policy_opts("float32", self.obs_mean, 1.0 / self.obs_std)

    def _activate(self, x: np.ndarray) -> np.ndarray:
        zero = x.dtype.type(0)
        if self.activation == "relu":
            return np.maximum(x, zero)
        if self.activation == "tanh":
            return np.tanh(x)
        return np.where(x > zero, x, np.expm1(np.minimum(x, zero)))

    def normalise_f32(self, obs: Any) -> np.ndarray:
        """The float32 path's first stage: ``(obs - mean) * (1 / std)`` in float64, rounded to float32 once."""
        x = np.asarray(obs, dtype=np.float64)
        if self.obs_mean is not None:
            x = (x - self.obs_mean) * (1.0 / self.obs_std)
        return x.astype(np.float32)

    def pre_head_np(self, obs: Any, compute: Optional[str] = None, exact: bool = False) -> np.ndarray:
        """The last linear layer's output on raw observations ``obs`` [..., obs_dim].  ``compute`` (default: the policy's own)
        "float32": the device contract of GS_COMPUTE_F32 -- float32-rounded weights, biases and normalised observations,
        float32 products, sums and activations; with ``exact`` the same rounded operands evaluated in float64 throughout
        (what the float32 result is measured against)."""
        compute = self.compute if compute is None else compute
        if compute not in _lib.COMPUTE:
            raise ValueError(f"compute must be one of {sorted(_lib.COMPUTE)}, got {compute!r}")
        if compute == "float64":
            if exact:
                raise ValueError("exact goes with compute='float32'")
            x = np.asarray(obs, dtype=np.float64)
            layers = list(zip(self.weights, self.biases))
        else:
            work = np.float64 if exact else np.float32
            x = self.normalise_f32(obs).astype(work)
            layers = [(w.astype(np.float32).astype(work), b.astype(np.float32).astype(work))
                      for w, b in zip([self.weight0] + self.weights[1:], [self.bias0] + self.biases[1:])]
        for l, (w, b) in enumerate(layers):
            x = x @ w.T + b
            if l < len(layers) - 1:
                x = self._activate(x)
        return x

    def forward_np(self, obs: Any, eps: Optional[Any] = None, compute: Optional[str] = None, exact: bool = False) -> np.ndarray:
        """Actions [..., action_dim] on raw observations: ``tanh(out)`` (plain head), ``tanh(mean)`` (Gaussian head) or, with
        ``eps`` [..., action_dim], ``tanh(mean + exp(clamp(log_std, -20, 2)) * eps)``.  The head is float64 on every path;
        ``compute`` / ``exact``: as for ``pre_head_np``."""
        out = self.pre_head_np(obs, compute, exact).astype(np.float64)
        if self.head == "tanh":
            if eps is not None:
                raise ValueError("eps needs the Gaussian head")
            return np.tanh(out)
        a = self.action_dim
        mean, log_std = out[..., :a], out[..., a:]
        if eps is None:
            return np.tanh(mean)
        return np.tanh(mean + np.exp(np.clip(log_std, LOG_STD_MIN, LOG_STD_MAX)) * np.asarray(eps, dtype=np.float64))

    def log_prob_np(self, obs: Any, eps: Any, compute: Optional[str] = None, exact: bool = False) -> np.ndarray:
        """The log-probability [...] of the action ``forward_np(obs, eps)`` samples, as the device records it with the action
        (``log_probs`` of a stochastic rollout; include/gridstep.h): per action
        ``-0.5 eps^2 - log_std - 0.5 log(2 pi) - log((1 - a^2) + 1e-6)``, ``log_std`` clamped, summed in action order from
        action 0.  That is the reference's ``Normal(mean, std).log_prob(x)`` minus its tanh correction
        (algorithms/offline.py:114-136), with ``(x - mean)^2 / (2 std^2)`` written as ``eps^2 / 2``.  Gaussian head only."""
        if self.head != "gaussian_tanh":
            raise ValueError("log_prob_np needs the Gaussian head")
        out = self.pre_head_np(obs, compute, exact).astype(np.float64)
        a = self.action_dim
        eps = np.asarray(eps, dtype=np.float64)
        ls = np.clip(out[..., a:], LOG_STD_MIN, LOG_STD_MAX)
        act = np.tanh(out[..., :a] + np.exp(ls) * eps)
        terms = (((-0.5 * eps) * eps - ls) - HALF_LOG_2PI) - np.log((1.0 - act * act) + 1e-6)
        total = terms[..., 0].copy()
        for k in range(1, a):
            total += terms[..., k]
        return total


HALF_LOG_2PI = 0.9189385332046727      # 0.5 * log(2 pi)


class MLPValue:
    """A value network (critic) for ``env.set_value`` / ``evaluate_rollout``: the reference's ``_build_mlp`` with a scalar output
    (IQL's and AWR's value functions).  ``weights`` / ``biases`` as for ``MLPPolicy``, the last layer of width 1; ``obs_mean`` /
    ``obs_std``: the observation normalisation.  The device evaluates it at the precision of torch critics -- the float32 path of
    ``MLPPolicy``: normalisation in float64 rounded once, float32 layers -- and returns the scalar widened to float64."""

    def __init__(self, weights: Sequence[Any], biases: Sequence[Any], activation: str = "relu", obs_mean: Optional[Any] = None,
                 obs_std: Optional[Any] = None) -> None:
        self._net = MLPPolicy(weights, biases, activation=activation, head="tanh", obs_mean=obs_mean, obs_std=obs_std, compute="float32")
        if self._net.weights[-1].shape[0] != 1:
            raise ValueError(f"a value network's last layer has one output, got {self._net.weights[-1].shape[0]}")
        self.activation = activation

    @property
    def obs_dim(self) -> int:
        return self._net.obs_dim

    @property
    def obs_mean(self) -> Optional[np.ndarray]:
        return self._net.obs_mean

    @property
    def obs_std(self) -> Optional[np.ndarray]:
        return self._net.obs_std

    @property
    def weights(self) -> List[np.ndarray]:
        """The layers as given (the first one unfolded: the normalisation is a stage of its own)."""
        return [self._net.weight0] + self._net.weights[1:]

    @property
    def biases(self) -> List[np.ndarray]:
        return [self._net.bias0] + self._net.biases[1:]

    @classmethod
    def from_sequential(cls, module: Any, obs_mean: Optional[Any] = None, obs_std: Optional[Any] = None) -> "MLPValue":
        """From a torch ``nn.Sequential`` of ``Linear`` and activation modules, read as ``MLPPolicy.from_sequential`` reads it."""
        net = MLPPolicy.from_sequential(module, head="tanh", compute="float32")
        return cls([net.weight0] + net.weights[1:], [net.bias0] + net.biases[1:], activation=net.activation, obs_mean=obs_mean, obs_std=obs_std)

    def to_struct(self):
        """(gs_policy_mlp with head GS_HEAD_LINEAR, the arrays it points into)"""
        return _lib.policy_struct(self.weights, self.biases, self.activation, _lib.GS_HEAD_LINEAR, False)

    def to_opts(self):
        """(gs_policy_mlp_opts with GS_COMPUTE_F32 and the normalisation, the arrays it points into)"""
        return self._net.to_opts()

    def forward_np(self, obs: Any, exact: bool = False) -> np.ndarray:
        """Values [...] on raw observations [..., obs_dim], float64: the device contract (float32-rounded weights, biases and
        normalised observations, float32 products, sums and activations); with ``exact`` the same rounded operands evaluated
        in float64 throughout (what the float32 result is measured against)."""
        return self._net.pre_head_np(obs, "float32", exact).astype(np.float64)[..., 0]


class MLPQ:
    """A state-action critic Q(s, a) for ``env.set_q`` / ``evaluate_rollout_q``: the reference's ``TwinCritic`` tower (``_build_mlp``
    over ``cat(state, action)`` with a scalar output; algorithms/offline.py).  ``weights`` / ``biases`` as for ``MLPValue``, the first
    layer ``obs_dim + action_dim`` wide; ``obs_mean`` / ``obs_std`` [obs_dim] normalise the OBSERVATION columns only, the action
    columns enter as they are.  The device evaluates it on the float32 path: the observation normalised in float64 and rounded once,
    the stored float64 action rounded once, float32 layers; the scalar is returned widened to float64."""

    def __init__(self, weights: Sequence[Any], biases: Sequence[Any], obs_dim: int, activation: str = "relu", obs_mean: Optional[Any] = None,
                 obs_std: Optional[Any] = None) -> None:
        self._net = MLPPolicy(weights, biases, activation=activation, head="tanh", compute="float32")
        if self._net.weights[-1].shape[0] != 1:
            raise ValueError(f"a Q network's last layer has one output, got {self._net.weights[-1].shape[0]}")
        self.obs_dim = int(obs_dim)
        if not 0 < self.obs_dim < self._net.obs_dim:
            raise ValueError(f"a Q network takes obs_dim + action_dim = {self._net.obs_dim} inputs with 0 < obs_dim, got obs_dim = {obs_dim}")
        if (obs_mean is None) != (obs_std is None):
            raise ValueError("obs_mean and obs_std go together")
        self.obs_mean: Optional[np.ndarray] = None
        self.obs_std: Optional[np.ndarray] = None
        if obs_mean is not None:
            self.obs_mean = np.array(obs_mean, dtype=np.float64).reshape(-1)
            self.obs_std = np.array(obs_std, dtype=np.float64).reshape(-1)
            if self.obs_mean.shape != (self.obs_dim,) or self.obs_std.shape != (self.obs_dim,):
                raise ValueError(f"obs_mean / obs_std must have shape ({self.obs_dim},)")
        self.activation = activation

    @property
    def action_dim(self) -> int:
        return self._net.obs_dim - self.obs_dim

    @property
    def weights(self) -> List[np.ndarray]:
        return self._net.weights

    @property
    def biases(self) -> List[np.ndarray]:
        return self._net.biases

    @classmethod
    def from_sequential(cls, module: Any, obs_dim: Optional[int] = None, obs_mean: Optional[Any] = None, obs_std: Optional[Any] = None,
                        activation: Optional[str] = None) -> "MLPQ":
        """From a torch ``nn.Sequential`` of ``Linear`` and activation modules (a tower of the reference's CQL ``TwinCritic``), read as
        ``MLPPolicy.from_sequential`` reads it; or, with ``activation`` named, from a ``ModuleList`` of ``Linear`` layers alone (a
        tower of IQL's).  ``obs_dim``: by default the length of ``obs_mean``."""
        if obs_dim is None:
            if obs_mean is None:
                raise ValueError("MLPQ.from_sequential: name obs_dim (or give obs_mean / obs_std)")
            obs_dim = int(np.asarray(obs_mean).reshape(-1).shape[0])
        children = list(module)
        if activation is not None and all(hasattr(c, "weight") and hasattr(c, "bias") for c in children):
            ws = [c.weight.detach().cpu().numpy().astype(np.float64) for c in children]
            bs = [c.bias.detach().cpu().numpy().astype(np.float64) for c in children]
            return cls(ws, bs, obs_dim, activation=activation, obs_mean=obs_mean, obs_std=obs_std)
        net = MLPPolicy.from_sequential(module, head="tanh", compute="float32")
        if activation is not None and activation != net.activation and len(net.weights) > 1:
            raise ValueError(f"MLPQ.from_sequential: activation = {activation!r}, the module's is {net.activation!r}")
        return cls(net.weights, net.biases, obs_dim, activation=net.activation, obs_mean=obs_mean, obs_std=obs_std)

    @classmethod
    def twins(cls, module: Any, obs_dim: Optional[int] = None, obs_mean: Optional[Any] = None, obs_std: Optional[Any] = None,
              activation: Optional[str] = None) -> "tuple":
        """(Q1, Q2) from a ``TwinCritic``-shaped module: its towers ``module.q1`` and ``module.q2``, each read by ``from_sequential``
        (``activation``: by default the class of ``module.activation`` where the towers hold linear layers alone)."""
        if activation is None and hasattr(module, "activation") and not callable(getattr(module.activation, "lower", None)):
            activation = {"ReLU": "relu", "Tanh": "tanh", "ELU": "elu"}.get(type(module.activation).__name__)
        only_linear = all(hasattr(c, "weight") and hasattr(c, "bias") for c in module.q1)
        act = activation if only_linear else None
        return tuple(cls.from_sequential(tower, obs_dim, obs_mean, obs_std, act) for tower in (module.q1, module.q2))

    def to_struct(self):
        """(gs_policy_mlp with head GS_HEAD_LINEAR, the arrays it points into)"""
        return _lib.policy_struct(self.weights, self.biases, self.activation, _lib.GS_HEAD_LINEAR, False)

    def to_opts(self):
        """(gs_policy_mlp_opts with GS_COMPUTE_F32 and the observation columns' normalisation, the arrays it points into)"""
        if self.obs_mean is None:
            return _lib.policy_opts("float32")
        return _lib.policy_opts("float32", self.obs_mean, 1.0 / self.obs_std)

    def input_f32(self, obs: Any, actions: Any) -> np.ndarray:
        """The network's float32 input rows [..., obs_dim + action_dim]: ``(obs - mean) * (1 / std)`` in float64 rounded once, then the
        float64 actions rounded once."""
        x = np.asarray(obs, dtype=np.float64)
        if self.obs_mean is not None:
            x = (x - self.obs_mean) * (1.0 / self.obs_std)
        return np.concatenate([x.astype(np.float32), np.asarray(actions, dtype=np.float64).astype(np.float32)], axis=-1)

    def forward_np(self, obs: Any, actions: Any, exact: bool = False) -> np.ndarray:
        """Q values [...] on raw observations [..., obs_dim] and actions [..., action_dim], float64: the device contract (float32
        products, sums and activations on the float32-rounded operands); with ``exact`` the same rounded operands evaluated in float64
        throughout (what the float32 result is measured against)."""
        return self._net.pre_head_np(self.input_f32(obs, actions), "float32", exact).astype(np.float64)[..., 0]
