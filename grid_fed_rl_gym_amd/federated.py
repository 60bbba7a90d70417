"""Federated rounds over device learners (``gs_fed_*``, include/gridstep.h "the federation"): K
``DeviceLearner``s of one process and one device -- one utility each, with its own feeders (``load_powers=``, ``line_impedances=``)
and its own rollouts -- average their networks where they lie.  ``FederatedLearners.round`` measures the clients' updates against
the global parameters, clips them, averages them by weight, adds Gaussian noise and writes the result into every client's master
parameters and packed images: no weight crosses the host and Adam's moments and step counts survive the round.

``round(prox_mu=...)`` adds FedProx's proximal term to the clients' local steps.

What it restates of the reference: ``FedAvgAggregator.aggregate`` (federated/core.py: the mean weighted by ``num_samples``),
``FederatedOfflineRL._train_round`` (aggregate, hand the global model back to EVERY client), ``DifferentialPrivacy`` (privacy.py:
norm clipping and the Gaussian mechanism) and ``SecureAsyncAggregator._filter_byzantine_updates`` (async_coordinator.py:159-219).
Deviation: the outlier filter looks at the UPDATES p_k - g, not at the raw parameters -- networks that share a start all have a
cosine of ~1 on raw parameters, whatever their updates did.

``fedavg_np``, ``fed_noise_np`` and ``filter_outliers_np`` restate the arithmetic in NumPy -- what the kernels are tested against.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .components import PowerFlowError
from .rollout import _philox4x32

FED_NOISE_TAG = 0x4645444E      # 'FEDN'
_M32 = 0xFFFFFFFF


def fed_noise_words(seed: int, round: int, net: int, quads: int, tag: int = FED_NOISE_TAG) -> np.ndarray:
    """The Philox4x32-10 words [quads, 4] of the federation's noise: counter (q, round, net, tag), key ``seed``."""
    q = np.arange(int(quads), dtype=np.uint64)
    c1 = np.full(q.shape, int(round) & _M32, dtype=np.uint64)
    c2 = np.full(q.shape, int(net) & _M32, dtype=np.uint64)
    c3 = np.full(q.shape, int(tag) & _M32, dtype=np.uint64)
    return np.stack(_philox4x32(q, c1, c2, c3, int(seed) & _M32, (int(seed) >> 32) & _M32), axis=1)


def fed_noise_np(seed: int, round: int, net: int, P: int, tag: int = FED_NOISE_TAG) -> np.ndarray:
    """z [P] of a round: z[j] = component j & 3 of the four normals of quad j >> 2 -- every word w a uniform (w + 1/2) 2^-32, words
    (0, 1) and (2, 3) one Box-Muller pair each, cosine then sine (the recipe of the environment's load noise)."""
    P = int(P)
    w = fed_noise_words(seed, round, net, (P + 3) // 4, tag).astype(np.float64)
    u = (w + 0.5) * (1.0 / 4294967296.0)
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    ta, tb = 2.0 * math.pi * u[:, 1], 2.0 * math.pi * u[:, 3]
    return np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], axis=1).reshape(-1)[:P]


def fed_coefficients_np(weights, norms, clip_norm: float = 0.0, server_lr: float = 1.0):
    """(c_k, a_k) of a round: c_k = min(1, clip_norm / (norm_k + 1e-6)) (1 without a clip), a_k = (server_lr (w_k / W)) c_k with
    W the sum of the weights in list order."""
    w = [float(x) for x in weights]
    W = 0.0
    for x in w:
        W = W + x
    c = [min(1.0, float(clip_norm) / (float(nk) + 1e-6)) if clip_norm > 0.0 else 1.0 for nk in norms]
    a = [(float(server_lr) * (x / W)) * ck for x, ck in zip(w, c)]
    return np.array(c, dtype=np.float64), np.array(a, dtype=np.float64)


def fedavg_np(g, params, weights, norms=None, clip_norm: float = 0.0, noise_std: float = 0.0, server_lr: float = 1.0, seed: int = 0,
              round: int = 0, net: int = 0, z=None) -> np.ndarray:
    """The new global parameters (float32 [P]) as ``gs_fed_aggregate`` computes them, operation by operation: ``g`` [P] the global
    parameters, ``params`` the participants' parameters in list order, ``weights`` their ``num_samples``; ``norms``: the norms of
    the updates p_k - g (the DEVICE's figures, as ``adam_np`` takes the device's ``grad_norm``), needed when ``clip_norm`` > 0.
    ``z``: the noise in place of ``fed_noise_np(seed, round, net, P)``."""
    g32 = np.asarray(g, dtype=np.float32).reshape(-1)
    g64 = g32.astype(np.float64)
    ps = [np.asarray(p, dtype=np.float32).reshape(-1) for p in params]
    if not ps or any(p.shape != g32.shape for p in ps) or len(ps) != len(weights):
        raise ValueError("fedavg_np: one parameter vector of g's length and one weight per participant")
    if clip_norm > 0.0 and (norms is None or len(norms) != len(ps)):
        raise ValueError("fedavg_np: clip_norm > 0 needs the norm of every participant's update")
    _, a = fed_coefficients_np(weights, norms if norms is not None else [0.0] * len(ps), clip_norm, server_lr)
    s = np.zeros_like(g64)
    for ak, p in zip(a, ps):
        s = s + ak * (p.astype(np.float64) - g64)
    x = g64 + s
    if noise_std > 0.0:
        x = x + float(noise_std) * (fed_noise_np(seed, round, net, g32.size) if z is None else np.asarray(z, dtype=np.float64))
    return x.astype(np.float32)


def filter_outliers_np(gram, tolerance: int) -> List[int]:
    """The reference's outlier rule (``_filter_byzantine_updates``) on the Gram matrix [n, n] of the updates: positions to DROP.
    sim_ik = G_ik / (sqrt(G_ii) sqrt(G_kk) + 1e-8) with a zero diagonal; the row means over n; the threshold is their 25th
    percentile; the positions strictly below it, in index order, at most ``tolerance`` of them; none when n <= 2 tolerance."""
    G = np.asarray(gram, dtype=np.float64)
    n = G.shape[0]
    tolerance = int(tolerance)
    if G.shape != (n, n):
        raise ValueError(f"filter_outliers_np: the Gram matrix must be square, got {G.shape}")
    if tolerance <= 0 or n <= 2 * tolerance:
        return []
    nrm = np.sqrt(np.diag(G))
    sim = G / (nrm[:, None] * nrm[None, :] + 1e-8)
    np.fill_diagonal(sim, 0.0)
    avg = np.mean(sim, axis=1)
    threshold = np.percentile(avg, 25)
    return [int(i) for i in np.where(avg < threshold)[0][:tolerance]]


def gaussian_sigma(epsilon: float, delta: float, sensitivity: float) -> float:
    """The Gaussian mechanism's noise scale, sqrt(2 ln(1.25 / delta)) sensitivity / epsilon (the reference's privacy.py:85): with
    ``clip_norm`` C and n participants of equal weight the mean's sensitivity is C / n."""
    if not (epsilon > 0.0 and 0.0 < delta < 1.0 and sensitivity >= 0.0):
        raise ValueError("gaussian_sigma: epsilon > 0, 0 < delta < 1, sensitivity >= 0")
    return math.sqrt(2.0 * math.log(1.25 / delta)) * sensitivity / epsilon


class FederatedLearners:
    """A federation of ``learners`` (a list of ``DeviceLearner``, one per client, on distinct environments of one device): one
    ``gs_fed`` per network that they all train.  The global parameters start as client 0's; nothing is written to a client until
    ``set_global`` or ``round``.  A client whose network is installed again, whose learner is created again or whose environment
    is closed ends the federation: every call raises until a new one is built."""

    def __init__(self, learners: Sequence[Any]) -> None:
        learners = list(learners)
        if not 1 <= len(learners) <= _lib.GS_FED_MAX_CLIENTS:
            raise ValueError(f"FederatedLearners: {len(learners)} learners outside 1 .. {_lib.GS_FED_MAX_CLIENTS}")
        if len({id(l.env) for l in learners}) != len(learners):
            raise ValueError("FederatedLearners: two learners share an environment")
        nets = [n for n in learners[0].nets if all(n in l.nets for l in learners)]
        if not nets:
            raise ValueError("FederatedLearners: the learners have no network in common")
        self.learners, self.nets = learners, tuple(nets)
        self.K = len(learners)
        self._lib = _lib.load()
        self._feds: Dict[int, C.c_void_p] = {}
        self._rounds = 0
        handles = (C.c_void_p * self.K)(*[l.env.handle._h for l in learners])
        try:
            for n in self.nets:
                f = C.c_void_p()
                self._check(self._lib.gs_fed_create(handles, self.K, _lib.learner_net(n), C.byref(f)))
                self._feds[_lib.learner_net(n)] = f
        except Exception:
            self.close()
            raise

    def _check(self, rc: int) -> None:
        if rc != _lib.GS_OK:
            raise PowerFlowError(f"libgridstep error {rc}: {self._lib.gs_last_error(None).decode()}")

    def _fed(self, net):
        k = _lib.learner_net(net)
        if k not in self._feds:
            raise ValueError(f"FederatedLearners: {net!r} is not one of the federation's networks {self.nets}")
        return k, self._feds[k]

    def _participants(self, participants) -> List[int]:
        part = list(range(self.K)) if participants is None else [int(p) for p in participants]
        if not part:
            raise ValueError("FederatedLearners: no participant")
        if any(not 0 <= p < self.K for p in part):
            raise ValueError(f"FederatedLearners: a participant outside 0 .. {self.K - 1} in {part}")
        if len(set(part)) != len(part):
            raise ValueError(f"FederatedLearners: a participant is named twice in {part}")
        return part

    def info(self, net="policy") -> dict:
        _, f = self._fed(net)
        o = _lib.gs_fed_info_out()
        self._check(self._lib.gs_fed_info(f, C.byref(o)))
        return dict(n_clients=int(o.n_clients), net=int(o.net), param_count=int(o.param_count), rounds=int(o.rounds), block_params=int(o.block_params))

    def measure(self, net="policy", participants=None) -> np.ndarray:
        """The Gram matrix [n, n] of the participants' updates p_k - g (float64; waits for the clients' queued steps)."""
        _, f = self._fed(net)
        part = self._participants(participants)
        idx = (C.c_int32 * len(part))(*part)
        gram = np.empty((len(part), len(part)), dtype=np.float64)
        self._check(self._lib.gs_fed_measure(f, idx, len(part), gram.ctypes.data_as(C.POINTER(C.c_double))))
        return gram

    def global_parameters(self, net="policy") -> np.ndarray:
        """The global parameters, flat float32 in torch order (``learner.split_parameters`` gives (W, b) lists)."""
        _, f = self._fed(net)
        out = np.empty(self.info(net)["param_count"], dtype=np.float32)
        self._check(self._lib.gs_fed_download(f, out.ctypes.data))
        return out

    def set_global(self, net="policy", params=None) -> None:
        """The broadcast: the global parameters (``params``: flat float32 to take first) into every client, bit for bit; Adam's
        state is left alone."""
        _, f = self._fed(net)
        ptr = None
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float32).reshape(-1)
            if params.size != self.info(net)["param_count"]:
                raise ValueError(f"FederatedLearners.set_global: {params.size} values for {self.info(net)['param_count']} parameters")
            ptr = params.ctypes.data
        self._check(self._lib.gs_fed_set_global(f, ptr))

    def aggregate(self, net, participants, weights, clip_norm=0.0, noise_std=0.0, server_lr=1.0, seed=0, round=0, reset_moments=False,
                  struct_size=None, prox_mu=None) -> None:
        """``gs_fed_aggregate`` as it is (asynchronous): what ``round`` calls per network.  ``prox_mu``: see ``round``."""
        _, f = self._fed(net)
        prox_mu = self._prox_mu(prox_mu)
        part = [int(p) for p in participants]
        idx = (C.c_int32 * max(len(part), 1))(*part)
        w = (C.c_double * max(len(part), 1))(*[float(x) for x in weights])
        r = _lib.gs_fed_round(C.sizeof(_lib.gs_fed_round) if struct_size is None else int(struct_size), len(part), idx, w, float(clip_norm),
                              float(noise_std), float(server_lr), int(seed) & 0xFFFFFFFFFFFFFFFF, int(round) & _M32, int(bool(reset_moments)))
        self._check(self._lib.gs_fed_aggregate(f, C.byref(r)))
        if prox_mu is not None:
            # (the round has written the global model into every client, and every client's stream waits for it: the copy of a
            # client's own parameters IS the global model)
            for l in self.learners:
                l.anchor_here(net)
                l.set_anchor(net, prox_mu=prox_mu)

    @staticmethod
    def _prox_mu(prox_mu) -> Optional[float]:
        if prox_mu is None:
            return None
        prox_mu = float(prox_mu)
        if not math.isfinite(prox_mu) or prox_mu < 0.0:
            raise ValueError(f"FederatedLearners: prox_mu = {prox_mu} must be finite and >= 0")
        return prox_mu

    def stats(self, net="policy") -> dict:
        """The last round's ``participants``-ordered ``norms``, ``clip_scales`` (c_k) and ``coefficients`` (a_k), ``noise_std``,
        ``round`` and ``rounds`` (waits for the round)."""
        _, f = self._fed(net)
        o = _lib.gs_fed_stats_out()
        self._check(self._lib.gs_fed_stats(f, C.byref(o)))
        n = int(o.n)
        return dict(norms=np.array(o.norm[:n]), clip_scales=np.array(o.clip_scale[:n]), coefficients=np.array(o.coefficient[:n]),
                    noise_std=float(o.noise_std), round=int(o.round), rounds=int(o.rounds), n=n)

    def round(self, weights=None, participants=None, clip_norm=0.0, noise_std=0.0, server_lr=1.0, seed=0, reset_moments=False,
              byzantine_tolerance=0, prox_mu=None) -> Dict[str, dict]:
        """One federated round of every network.  ``weights``: one per participant (``num_samples``; equal by default);
        ``participants``: client indices (all by default); ``clip_norm`` / ``noise_std``: the clip of every update's norm and the
        Gaussian noise on the result (0: off); ``byzantine_tolerance`` > 0: ``measure`` and ``filter_outliers_np`` first, the
        dropped clients neither count nor weigh (they still receive the global model).  The round counter, which the noise is
        drawn on, advances by itself.  ``prox_mu`` (FedProx): with a value, once the global model is in the
        clients, every client's learner of that network takes its own parameters -- the global model -- as its PROX centre
        (``anchor_here``) and ``set_anchor(prox_mu=...)``: the local steps until the next round are pulled back by
        ``prox_mu (w - g)``; None leaves the clients' anchors alone.  Returns per network the ``stats`` with ``participants`` (who was averaged) and ``filtered``
        (client indices the filter dropped)."""
        part = self._participants(participants)
        w = [1.0] * len(part) if weights is None else [float(x) for x in weights]
        if len(w) != len(part):
            raise ValueError(f"FederatedLearners.round: {len(w)} weights for {len(part)} participants")
        if any(not math.isfinite(x) or x < 0.0 for x in w):
            raise ValueError("FederatedLearners.round: the weights must be finite and >= 0")
        for k, x in dict(clip_norm=clip_norm, noise_std=noise_std, server_lr=server_lr).items():
            if not math.isfinite(float(x)) or float(x) < 0.0:
                raise ValueError(f"FederatedLearners.round: {k} = {x} must be finite and >= 0")
        prox_mu = self._prox_mu(prox_mu)
        if int(byzantine_tolerance) < 0:
            raise ValueError("FederatedLearners.round: byzantine_tolerance must be >= 0")
        plans = {}
        for net in self.nets:
            keep, kw, dropped = part, w, []
            if byzantine_tolerance > 0:
                drop = set(filter_outliers_np(self.measure(net, part), byzantine_tolerance))
                dropped = [p for i, p in enumerate(part) if i in drop]
                keep = [p for i, p in enumerate(part) if i not in drop]
                kw = [x for i, x in enumerate(w) if i not in drop]
            if not sum(kw) > 0.0:
                raise ValueError("FederatedLearners.round: the weights sum to 0")
            plans[net] = (keep, kw, dropped)
        out = {}
        for net in self.nets:
            keep, kw, dropped = plans[net]
            self.aggregate(net, keep, kw, clip_norm, noise_std, server_lr, seed, self._rounds, reset_moments, prox_mu=prox_mu)
        for net in self.nets:
            keep, kw, dropped = plans[net]
            out[net] = dict(self.stats(net), participants=list(keep), filtered=dropped)
        self._rounds += 1
        return out

    @property
    def rounds(self) -> int:
        return self._rounds

    def close(self) -> None:
        for f in self._feds.values():
            if f:
                self._lib.gs_fed_destroy(f)
        self._feds = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
