"""MLP policies for closed-loop rollouts on the device (``gs_rollout`` with ``GS_POLICY_MLP``, include/gridstep.h).

The reference's actors are plain MLPs (algorithms/base.py:157-177 ``_build_mlp``: ``Linear`` + relu / tanh / elu, sizes
``[obs_dim] + [256, 256(, 256)] + [2 * action_dim]``) whose head is ``tanh(mean)`` or
``tanh(mean + exp(clamp(log_std, -20, 2)) * eps)`` (algorithms/offline.py:69-76, 114-136).  ``MLPPolicy`` holds such a network
as NumPy arrays, hands it to the device (``env.set_policy`` / ``rollout_device(policy=...)`` / ``collect_policy_data``) and
restates its forward pass in NumPy (``forward_np``) -- what the device kernel is tested against.  NumPy only: a torch module is
read through duck typing (``from_sequential``), torch itself is never imported here.
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
    and the device kernel -- take raw observations."""

    def __init__(self, weights: Sequence[Any], biases: Sequence[Any], activation: str = "relu", head: str = "gaussian_tanh",
                 obs_mean: Optional[Any] = None, obs_std: Optional[Any] = None) -> None:
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
        if obs_mean is not None:
            mean = np.asarray(obs_mean, dtype=np.float64).reshape(-1)
            std = np.asarray(obs_std, dtype=np.float64).reshape(-1)
            if mean.shape != (self.obs_dim,) or std.shape != (self.obs_dim,):
                raise ValueError(f"obs_mean / obs_std must have shape ({self.obs_dim},)")
            w1 = self.weights[0]
            self.biases[0] = self.biases[0] - w1 @ (mean / std)
            self.weights[0] = w1 / std[None, :]

    @property
    def obs_dim(self) -> int:
        return int(self.weights[0].shape[1])

    @property
    def action_dim(self) -> int:
        out = int(self.weights[-1].shape[0])
        return out // 2 if self.head == "gaussian_tanh" else out

    @classmethod
    def from_sequential(cls, module: Any, head: str = "gaussian_tanh", obs_mean: Optional[Any] = None,
                        obs_std: Optional[Any] = None) -> "MLPPolicy":
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
        return cls(weights, biases, activation=acts[0] if acts else "relu", head=head, obs_mean=obs_mean, obs_std=obs_std)

    def to_struct(self, stochastic: bool = False):
        """(gs_policy_mlp, the arrays it points into)."""
        if stochastic and self.head != "gaussian_tanh":
            raise ValueError("a stochastic policy needs the Gaussian head")
        return _lib.policy_struct(self.weights, self.biases, self.activation, self.head, stochastic)

    def pre_head_np(self, obs: Any) -> np.ndarray:
        """The last linear layer's output on raw observations ``obs`` [..., obs_dim]."""
        x = np.asarray(obs, dtype=np.float64)
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            x = x @ w.T + b
            if l < len(self.weights) - 1:
                if self.activation == "relu":
                    x = np.maximum(x, 0.0)
                elif self.activation == "tanh":
                    x = np.tanh(x)
                else:
                    x = np.where(x > 0.0, x, np.expm1(np.minimum(x, 0.0)))
        return x

    def forward_np(self, obs: Any, eps: Optional[Any] = None) -> np.ndarray:
        """Actions [..., action_dim] on raw observations: ``tanh(out)`` (plain head), ``tanh(mean)`` (Gaussian head) or, with
        ``eps`` [..., action_dim], ``tanh(mean + exp(clamp(log_std, -20, 2)) * eps)``."""
        out = self.pre_head_np(obs)
        if self.head == "tanh":
            if eps is not None:
                raise ValueError("eps needs the Gaussian head")
            return np.tanh(out)
        a = self.action_dim
        mean, log_std = out[..., :a], out[..., a:]
        if eps is None:
            return np.tanh(mean)
        return np.tanh(mean + np.exp(np.clip(log_std, LOG_STD_MIN, LOG_STD_MAX)) * np.asarray(eps, dtype=np.float64))
