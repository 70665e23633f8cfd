"""Linear probes of the policy's GRU state: what does h_t know about the quadrotor it flies, and how early in an episode?

The policy is one set of weights for any quadrotor because the GRU identifies the system in flight.  A probe regresses per-env
targets y (log mass, thrust-to-weight, motor lag, ...) on the state h_t ENTERING each recorded step, separately for every bucket of
episode age.  The data-sized part runs on the device in one pass over the recording (rq_trajectory_probe_moments, csrc/rq_probe.hip):
per bucket the second moments S = sum of z z^T with z = [1, h (16), y (M)].  Everything after that is 17 x 17 algebra per bucket
in float64, here: the fit solves the normal equations, and R^2 on ANOTHER recording needs only that recording's moments.

    y, names = probing.targets_from_params(params.numpy(), env.config, ["log_mass", "thrust_to_weight", "tau_rise"])
    y, mean, std = probing.standardise(y)
    probe = probing.HiddenProbe(policy, y, names, probing.log_age_edges(500, 10))
    W = probe.fit(probe.moments(traj_a))
    r2 = probe.r2(probe.moments(traj_b), W)          # [buckets, targets], held out

Targets that change during an episode - the wrench of a scheduled gust, the velocity of a moving setpoint - go with the recording,
not with the probe (rq_trajectory_probe_moments_timed): "does the state know what is pushing on the vehicle right now, and how many
steps after the onset?"

    Y = traj.wrench_targets(bank, ids, params, start_steps, device=True)       # [T, 6, ld] on the device, never on the host
    probe = probing.HiddenProbe(policy, None, probing.WRENCH_NAMES, edges)
    m = probe.moments(traj, targets=Y, device=True)

What the policy DOES with what it knows is read off the same recording as effective feedback gains (``feedback_gains``,
rq_trajectory_policy_gain_table): the local Jacobian da/dobs [4, 22] at every live step, summed per env and age bucket on the device.

    gains = probing.feedback_gains(traj, policy, edges=probing.log_age_edges(500, 10))
    g = gains.by_age()                                # [B, 4, 22]: how the control law settles over an episode's first steps
    kp = probing.GainTable.block(g, "position")       # [B, 4, 3]: the position gain

How the vehicles FLEW needs no policy at all (``flight_table``, rq_trajectory_flight_table): deviation from the setpoint, tilt, rates,
effort, saturation and reward per env and age bucket, with the age counted from ``start_steps`` - the row of a wrench schedule or a
moving setpoint, so a bucket of age is "time since the poke".

    table = probing.flight_table(traj, edges=probing.linear_age_edges(90, 250, 32), start_steps=start, tolerance=0.05)
    curves = table.by_group(wrench_ids, M)            # dict of [M, B]: a step response per scenario

Age follows the forward's episode rule: 0 at the first recorded step; a step is live when its done code is not 4; after a live
step with code 1 or 2 the age is 0 again, after any other live step one more; frozen steps neither count nor age.
"""

import numpy as np

from . import _lib

HIDDEN = _lib.POLICY_HIDDEN_DIM
DIM = 32                      # z = [1, h (16), y (M <= 15)], zero-padded
MAX_TARGETS, MAX_BUCKETS = 15, 32
MIN_SAMPLES = HIDDEN + 2      # a bucket with fewer samples than unknowns + 1 is not fitted
WRENCH_NAMES = ["fx", "fy", "fz", "tx", "ty", "tz"]          # the columns of ``Trajectory.wrench_targets``

# rq_param_field (include/raptor_quad.h)
_P_MASS, _P_JXX, _P_JZZ = 0, 1, 3
_P_C0, _P_C1, _P_C2, _P_TORQUE_CONST, _P_TAU_RISE, _P_TAU_FALL = 16, 17, 18, 19, 20, 21
_P_RPM_MAX, _P_HOVER_ACTION = 23, 25


def _thrust_to_weight(p, g):
    r = p[:, _P_RPM_MAX]
    return 4.0 * (p[:, _P_C0] + p[:, _P_C1] * r + p[:, _P_C2] * r * r) / (p[:, _P_MASS] * g)


TARGETS = {
    "log_mass": lambda p, g: np.log(p[:, _P_MASS]),
    "thrust_to_weight": _thrust_to_weight,            # four rotors at RPM_MAX over m g
    "log_jxx": lambda p, g: np.log(p[:, _P_JXX]),
    "log_jzz": lambda p, g: np.log(p[:, _P_JZZ]),
    "tau_rise": lambda p, g: p[:, _P_TAU_RISE],
    "tau_fall": lambda p, g: p[:, _P_TAU_FALL],
    "torque_const": lambda p, g: p[:, _P_TORQUE_CONST],
    "hover_action": lambda p, g: p[:, _P_HOVER_ACTION],
}


def targets_from_params(params, config, names):
    """``params`` [N, 26] (``VectorParameters.numpy()``), ``config`` the env's configuration (its ``gravity`` is read; a float is
    taken as g) -> (y [N, M] float32, names).  Supported names: the keys of ``TARGETS``."""
    p = np.asarray(params, np.float64)
    if p.ndim != 2 or p.shape[1] != _lib.PARAM_DIM:
        raise ValueError(f"params must be [N, {_lib.PARAM_DIM}]")
    names = list(names)
    unknown = [n for n in names if n not in TARGETS]
    if unknown:
        raise ValueError(f"unknown target(s) {unknown}; supported: {sorted(TARGETS)}")
    if not 1 <= len(names) <= MAX_TARGETS:
        raise ValueError(f"1 .. {MAX_TARGETS} targets, not {len(names)}")
    g = float(getattr(config, "gravity", config))
    y = np.stack([TARGETS[n](p, g) for n in names], axis=1)
    return y.astype(np.float32), names


def standardise(y):
    """-> (y standardised to zero mean and unit variance over envs, mean [M], std [M]).  The probe's R^2 is SST - SSE over SST from
    fp32 moments: a target far from zero mean would lose both to cancellation.  A constant target keeps std 1."""
    y = np.asarray(y, np.float64)
    mean = y.mean(axis=0)
    std = y.std(axis=0)
    std = np.where(std > 0, std, 1.0)
    return ((y - mean) / std).astype(np.float32), mean, std


def log_age_edges(limit, n):
    """n buckets of episode age up to ``limit`` (exclusive), doubling: 0, 1, 2, 4, 8, ..., limit -> uint32 [n + 1]."""
    n, limit = int(n), int(limit)
    if not 1 <= n <= MAX_BUCKETS:
        raise ValueError(f"1 .. {MAX_BUCKETS} buckets, not {n}")
    edges = [0] + [1 << k for k in range(n - 1)] + [limit]
    if any(b <= a for a, b in zip(edges, edges[1:])) or limit >= 1 << 32:
        raise ValueError(f"{n} doubling buckets do not fit below {limit}")
    return np.asarray(edges, np.uint32)


def episode_steps(done, start_steps=None):
    """The episode step count every env of a recording had at every step: ``done`` [T, N] codes, ``start_steps`` [N] the counts
    when the recording began (``env.episode_steps()`` right before the rollout; None: 0) -> k [T, N] int64, -1 on a frozen step
    (code 4).  k stays across a frozen step, is 0 after a step with code 1 or 2 and one more after any other - the row a wrench
    schedule or a moving setpoint was read at (clamped to the table)."""
    done = np.asarray(done)
    if done.ndim != 2:
        raise ValueError("done must be [T, N]")
    T, N = done.shape
    k = np.zeros(N, np.int64) if start_steps is None else np.asarray(start_steps).astype(np.int64).copy()
    if k.shape != (N,):
        raise ValueError(f"start_steps must be [{N}]")
    out = np.full((T, N), -1, np.int64)
    for t in range(T):
        live = done[t] != 4
        out[t, live] = k[live]
        k = np.where((done[t] == 1) | (done[t] == 2), 0, np.where(live, k + 1, k))
    return out


def table_targets(table, k, ids=None):
    """Per-step targets gathered from any row table along ``k`` (``episode_steps``): ``table`` [rows, C], or [M, rows, C] with
    ``ids`` [N] naming every env's table -> float32 [T, N, C], row min(k, rows - 1), zeros where k is -1 (frozen).  A reference's
    velocity columns, for instance, ask "does the state know where the path goes?"."""
    tab = np.asarray(table, np.float32)
    k = np.asarray(k, np.int64)
    if k.ndim != 2:
        raise ValueError("k must be [T, N]")
    if tab.ndim == 2:
        if ids is not None:
            raise ValueError("ids belong to a bank of tables [M, rows, C]")
        tab, ids = tab[None], np.zeros(k.shape[1], np.int64)
    elif tab.ndim == 3:
        ids = np.zeros(k.shape[1], np.int64) if ids is None else np.asarray(ids).astype(np.int64)
        if ids.shape != (k.shape[1],) or (ids < 0).any() or (ids >= tab.shape[0]).any():
            raise ValueError(f"ids must be [{k.shape[1]}] table numbers below {tab.shape[0]}")
    else:
        raise ValueError("table must be [rows, C] or [M, rows, C]")
    out = tab[ids[None, :], np.clip(k, 0, tab.shape[1] - 1)]
    out[k < 0] = 0.0
    return out


class ProbeMoments:
    """Per age bucket the sums of z z^T, ``S`` [B, 32, 32] float64, and the samples, ``counts`` [B].  Moments of several
    recordings (or of several devices' shares of one) add with ``+``."""

    def __init__(self, S, counts):
        self.S = np.asarray(S, np.float64)
        self.counts = np.asarray(counts, np.uint64)
        if self.S.ndim != 3 or self.S.shape[1:] != (DIM, DIM) or self.counts.shape != (self.S.shape[0],):
            raise ValueError("S must be [B, 32, 32] and counts [B]")

    def __add__(self, other):
        if self.S.shape != other.S.shape:
            raise ValueError("moments of different bucket counts do not add")
        return ProbeMoments(self.S + other.S, self.counts + other.counts)

    def __radd__(self, other):          # sum([...]) starts from 0
        return self if isinstance(other, int) and other == 0 else NotImplemented


class HiddenProbe:
    """``targets`` [N, M] float32 (finite; one row per env, constant over time), ``names`` [M], ``age_edges`` [B + 1] strictly
    ascending (``log_age_edges``).  ``policy``: the fp32 policy without Standardize / SampleAndSquash stages, at the native rate.
    ``targets=None``: the probe fixes only M = ``len(names)`` and every ``moments`` call brings the targets of its recording, one
    value per step (``moments(traj, targets=Y)``)."""

    def __init__(self, policy, targets=None, names=(), age_edges=(0, 1)):
        if targets is None:
            if not 1 <= len(names) <= MAX_TARGETS:
                raise ValueError(f"1 .. {MAX_TARGETS} names, not {len(names)}")
            y = None
        else:
            y = np.asarray(targets, np.float32)
            if y.ndim != 2 or not 1 <= y.shape[1] <= MAX_TARGETS:
                raise ValueError(f"targets must be [N, 1 .. {MAX_TARGETS}]")
            if len(names) != y.shape[1]:
                raise ValueError("one name per target")
            if not np.isfinite(y).all():
                raise ValueError("targets must be finite")
        e = np.asarray(age_edges, np.int64)
        if e.ndim != 1 or not 2 <= e.size <= MAX_BUCKETS + 1 or (np.diff(e) <= 0).any() or e[0] < 0 or e[-1] >= 1 << 32:
            raise ValueError(f"age_edges must be 2 .. {MAX_BUCKETS + 1} strictly ascending uint32 values")
        self.policy, self.names = policy, list(names)
        self.age_edges = e.astype(np.uint32)
        self.n_targets, self.n_buckets = len(self.names), e.size - 1
        self._y = None if y is None else np.ascontiguousarray(y.T)           # [M, N]: what the engine reads
        self._y_dev = None

    # ---- the device's part ----
    def _moments_timed(self, traj, targets, device):
        """``moments(traj, targets=Y)``: everything wrong with Y raises ValueError before any library call"""
        B, M = self.n_buckets, self.n_targets
        T, N = len(traj), int(traj._env.N_ENVIRONMENTS)
        edges = self.age_edges.ctypes.data
        if not device:
            y = np.asarray(targets)
            if y.dtype != np.float32:
                raise ValueError(f"targets must be float32, not {y.dtype}")
            if y.shape != (T, N, M):
                raise ValueError(f"targets must be [T, N, M] = [{T}, {N}, {M}], not {list(y.shape)}")
            if not np.isfinite(y).all():
                raise ValueError("targets must be finite")
            y = np.ascontiguousarray(y.transpose(0, 2, 1))          # the engine's [T, M, N], once
            pol = self.policy._handle(traj._env._device)
            h = traj._require("trajectory")
            traj._learner_forwards = getattr(traj, "_learner_forwards", 0) + 1
            S, counts = np.empty((B, DIM, DIM), np.float64), np.empty(B, np.uint64)
            _lib.call("rq_trajectory_probe_moments_timed", h, pol, _lib.fptr(y), N, M, edges, B, S.ctypes.data, counts.ctypes.data, 0)
            return ProbeMoments(S, counts)
        import torch
        if not isinstance(targets, torch.Tensor):
            raise ValueError("device=True takes a torch tensor [T, M, ld >= N] on the trajectory's device")
        dev = traj.tensors()["done"].device
        if targets.dtype != torch.float32:
            raise ValueError(f"targets must be float32, not {targets.dtype}")
        if targets.dim() != 3 or tuple(targets.shape[:2]) != (T, M) or targets.shape[2] < N:
            raise ValueError(f"targets must be [T, M, ld >= N] = [{T}, {M}, >= {N}], not {list(targets.shape)}")
        if targets.device != dev or not targets.is_contiguous():
            raise ValueError(f"targets must be a contiguous tensor on {dev}")
        pol = self.policy._handle(traj._env._device)
        h = traj._require("trajectory")
        traj._learner_forwards = getattr(traj, "_learner_forwards", 0) + 1
        S = torch.empty((B, DIM, DIM), dtype=torch.float64, device=dev)
        counts = torch.empty(B, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the engine runs on its own stream
        _lib.call("rq_trajectory_probe_moments_timed", h, pol, targets.data_ptr(), int(targets.shape[2]), M, edges, B, S.data_ptr(),
                  counts.data_ptr(), 1)
        return ProbeMoments(S.cpu().numpy(), counts.cpu().numpy().astype(np.uint64))

    def moments(self, traj, targets=None, device=False):
        """The moments of ``traj`` under this probe's policy -> ProbeMoments (host, float64).  ``device=True`` (torch): targets,
        moments and counts stay in device memory for the call - the targets are uploaded once per probe - and only the
        B x 8 KB result crosses.
        ``targets=Y``: the targets of THIS recording, one value per step - NumPy float32 [T, N, M], finite, or with ``device=True`` a
        torch tensor [T, M, ld >= N] on the trajectory's device (what ``traj.wrench_targets(..., device=True)`` returns)."""
        if targets is not None:
            return self._moments_timed(traj, targets, device)
        if self._y is None:
            raise ValueError("this probe holds no targets: pass the recording's, moments(traj, targets=Y)")
        N = self._y.shape[1]
        pol = self.policy._handle(traj._env._device)
        h = traj._require("trajectory")
        traj._learner_forwards = getattr(traj, "_learner_forwards", 0) + 1      # the saved state may be this call's now
        B, M = self.n_buckets, self.n_targets
        edges = self.age_edges.ctypes.data
        if not device:
            S, counts = np.empty((B, DIM, DIM), np.float64), np.empty(B, np.uint64)
            _lib.call("rq_trajectory_probe_moments", h, pol, _lib.fptr(self._y), N, M, edges, B, S.ctypes.data, counts.ctypes.data, 0)
            return ProbeMoments(S, counts)
        import torch
        dev = traj.tensors()["done"].device
        if self._y_dev is None or self._y_dev.device != dev:
            self._y_dev = torch.from_numpy(self._y).to(dev)
        S = torch.empty((B, DIM, DIM), dtype=torch.float64, device=dev)
        counts = torch.empty(B, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()              # the engine runs on its own stream
        _lib.call("rq_trajectory_probe_moments", h, pol, self._y_dev.data_ptr(), N, M, edges, B, S.data_ptr(), counts.data_ptr(), 1)
        return ProbeMoments(S.cpu().numpy(), counts.cpu().numpy().astype(np.uint64))

    # ---- the host's part: float64 algebra on [B, 32, 32] ----
    def _blocks(self, moments):
        K, M = 1 + HIDDEN, self.n_targets
        S = moments.S
        if S.shape[0] != self.n_buckets:
            raise ValueError(f"moments of {S.shape[0]} buckets, the probe has {self.n_buckets}")
        return S[:, :K, :K], S[:, :K, K:K + M], S[:, K:K + M, K:K + M]

    def fit(self, moments, ridge=1e-6):
        """-> W [B, 17, M]: per bucket the least-squares read-out y ~ W[0] + h . W[1:], from the normal equations G W = C in
        float64.  ``ridge`` is relative: ridge x the mean second moment of the hidden features is added to their diagonal, the
        intercept is not penalised.  A bucket with fewer than 18 samples gives NaN rows."""
        G, Cm, _ = self._blocks(moments)
        K = 1 + HIDDEN
        W = np.full((self.n_buckets, K, self.n_targets), np.nan)
        for b in range(self.n_buckets):
            if int(moments.counts[b]) < MIN_SAMPLES:
                continue
            A = G[b].copy()
            lam = float(ridge) * np.trace(A[1:, 1:]) / HIDDEN
            A[np.arange(1, K), np.arange(1, K)] += lam
            try:
                W[b] = np.linalg.solve(A, Cm[b])
            except np.linalg.LinAlgError:
                W[b] = np.linalg.lstsq(A, Cm[b], rcond=None)[0]
        return W

    def r2(self, moments, W):
        """-> R^2 [B, M] of the read-out ``W`` on the data behind ``moments`` - the recording it was fitted on, or a held-out
        one - from the moments alone: SSE = sum yy - 2 tr(W^T C) + tr(W^T G W) per target, SST = sum yy - (sum y)^2 / n."""
        G, Cm, Y = self._blocks(moments)
        out = np.full((self.n_buckets, self.n_targets), np.nan)
        for b in range(self.n_buckets):
            n = float(moments.counts[b])
            if n < MIN_SAMPLES or not np.isfinite(W[b]).all():
                continue
            yy = np.diag(Y[b])
            sse = yy - 2.0 * np.einsum("km,km->m", W[b], Cm[b]) + np.einsum("km,kl,lm->m", W[b], G[b], W[b])
            sst = yy - Cm[b][0] ** 2 / n
            with np.errstate(divide="ignore", invalid="ignore"):
                out[b] = np.where(sst > 0, 1.0 - sse / sst, np.nan)
        return out


# ---------------------------------------------------------------------------- the effective feedback gains ---
# the 22 columns of a gain G = da/dobs, by block of the observation
OBSERVATION_BLOCKS = {"position": (0, 3), "orientation": (3, 12), "linear_velocity": (12, 15), "angular_velocity": (15, 18),
                      "last_action": (18, 22)}
_W0 = (0, 16 * 22)            # layer_0's weights in the flat checkpoint, [16, 22] row-major


class GainTable:
    """What ``feedback_gains`` returns: ``sum`` [B, 4, 16, N] float32 - per age bucket and env the sum over its live steps of
    A = da/dp0, the Jacobian of the four actions with respect to layer_0's 16 pre-activations -, ``count`` [B, N] - the number of
    those steps -, ``edges`` [B + 1] (uint32, NumPy) and ``W0``, layer_0's weights: [16, 22], or [P, 16, 22] together with
    ``policy_ids`` [N] for a bank.  The gain is G = da/dobs = A W0 [4, 22]; W0 is constant over a recording, so the sums hold A and
    every method multiplies by W0 once, after its reduction over envs (under a bank each policy's part by its own W0, then the
    parts are added).  The arrays are NumPy or torch tensors, as the call made them; every method works in float64 on whatever they
    are and returns the same kind.  A mean over nothing is NaN."""

    def __init__(self, sum, count, edges, W0, policy_ids=None):
        self.sum, self.count = sum, count
        self.edges = np.asarray(edges, np.uint32)
        self.W0 = np.asarray(W0, np.float64)
        if len(sum.shape) != 4 or tuple(sum.shape[1:3]) != (4, HIDDEN) or tuple(count.shape) != (sum.shape[0], sum.shape[3]) \
                or self.edges.shape != (sum.shape[0] + 1,):
            raise ValueError("sum must be [B, 4, 16, N], count [B, N] and edges [B + 1]")
        N = int(sum.shape[3])
        if policy_ids is None:
            if self.W0.shape != (HIDDEN, 22):
                raise ValueError("W0 must be [16, 22] (or [P, 16, 22] with policy_ids)")
            self.W0, self.policy_ids = self.W0[None], np.zeros(N, np.int64)
            self._bank = False
        else:
            self.policy_ids = np.asarray(policy_ids).astype(np.int64)
            if self.W0.ndim != 3 or self.W0.shape[1:] != (HIDDEN, 22) or self.policy_ids.shape != (N,) or \
                    (N and (self.policy_ids.min() < 0 or self.policy_ids.max() >= self.W0.shape[0])):
                raise ValueError(f"W0 must be [P, 16, 22] and policy_ids [{N}] integers below P")
            self._bank = True

    # ---- float64 views, [B, 4, 16, N] and [B, N], and W0 of the same kind ----
    def _torch(self):
        return hasattr(self.sum, "data_ptr")

    def _f64(self):
        if self._torch():
            import torch
            return self.sum.to(torch.float64), self.count.to(torch.float64), torch.as_tensor(self.W0, device=self.sum.device)
        return np.asarray(self.sum, np.float64), np.asarray(self.count, np.float64), self.W0

    def _index(self, ids):
        if self._torch():
            import torch
            return torch.as_tensor(np.asarray(ids, np.int64), device=self.sum.device)
        return np.asarray(ids, np.int64)

    def _grouped(self, s, c, ids, G):
        """s [B, 4, 16, N], c [B, N], ids [N] below G -> (gs [G, P, B, 4, 16], gc [G, B]): the sums of A by group and policy"""
        P, B, N = self.W0.shape[0], int(s.shape[0]), int(s.shape[3])
        key = np.asarray(ids, np.int64) * P + self.policy_ids
        if self._torch():
            import torch
            gs = torch.zeros((G * P, B, 4, HIDDEN), dtype=torch.float64, device=s.device).index_add(0, self._index(key), s.permute(3, 0, 1, 2))
            gc = torch.zeros((G, B), dtype=torch.float64, device=s.device).index_add(0, self._index(ids), c.T)
        else:
            gs, gc = np.zeros((G * P, B, 4, HIDDEN)), np.zeros((G, B))
            np.add.at(gs, key, s.transpose(3, 0, 1, 2))
            np.add.at(gc, np.asarray(ids, np.int64), c.T)
        return gs.reshape(G, P, B, 4, HIDDEN), gc

    def _gains(self, gs, gc, W0):
        """gs [G, P, B, 4, 16] sums of A, gc [G, B] -> [G, B, 4, 22]: each policy's part times its own W0, added, over the count"""
        if self._torch():
            import torch
            g = torch.einsum("gpbik,pkf->gbif", gs, W0)
            n = gc[:, :, None, None]
            return torch.where(n > 0, g / torch.clamp(n, min=1.0), torch.full_like(g, float("nan")))
        g = np.einsum("gpbik,pkf->gbif", gs, W0)
        n = gc[:, :, None, None]
        return np.where(n > 0, g / np.maximum(n, 1.0), np.nan)

    def by_age(self):
        """-> [B, 4, 22]: the mean gain of all envs by age bucket - how the control law settles over an episode's first steps"""
        return self.by_group(np.zeros(int(self.sum.shape[3]), np.int64), 1)[0]

    def by_group(self, ids, n_groups):
        """``ids`` [N] integers below ``n_groups`` - the policy, scenario or parameter bin of every env -> [G, B, 4, 22]: the mean
        gain of each group's envs by age bucket.  A group may mix the policies of a bank."""
        s, c, W0 = self._f64()
        G, N = int(n_groups), int(s.shape[3])
        g = np.asarray(ids.cpu() if hasattr(ids, "data_ptr") else ids)
        if g.shape != (N,) or not np.issubdtype(g.dtype, np.integer) or (N and (g.min() < 0 or g.max() >= G)):
            raise ValueError(f"ids must be [{N}] integers below {G}")
        return self._gains(*self._grouped(s, c, g, G), W0)

    def per_env(self, bucket=None):
        """-> [4, 22, N]: every env's mean gain at the ages of ``bucket``; None: over all buckets"""
        s, c, W0 = self._f64()
        if bucket is None:
            s, c = s.sum(0), c.sum(0)
        else:
            s, c = s[int(bucket)], c[int(bucket)]
        if self._torch():
            import torch
            g = torch.einsum("ike,ekf->ife", s, W0[self._index(self.policy_ids)])
            return torch.where(c > 0, g / torch.clamp(c, min=1.0), torch.full_like(g, float("nan")))
        g = np.einsum("ike,ekf->ife", s, W0[self.policy_ids])
        return np.where(c > 0, g / np.maximum(c, 1.0), np.nan)

    @staticmethod
    def block(g, name, axis=None):
        """The columns of the observation block ``name`` (``OBSERVATION_BLOCKS``) of a gain array ``g``.  ``axis``: where its 22
        columns lie; None: the last axis if that has 22 entries (``by_age``, ``by_group``), else the one before it (``per_env``)."""
        if name not in OBSERVATION_BLOCKS:
            raise ValueError(f"unknown block {name!r}; the blocks: {sorted(OBSERVATION_BLOCKS)}")
        if axis is None:
            axis = -1 if g.shape[-1] == 22 else -2
        if g.shape[axis] != 22:
            raise ValueError("the axis holds no 22 observation columns")
        a, z = OBSERVATION_BLOCKS[name]
        index = [slice(None)] * len(g.shape)
        index[axis] = slice(a, z)
        return g[tuple(index)]


def feedback_gains(traj, policy, edges=None, start="initial", policy_ids=None):
    """The policy's effective feedback gains on the recording, per env and bucket of episode age -> ``GainTable``.  One pass on
    the device (rq_trajectory_policy_gain_table) that stores nothing of the recording's Jacobians.

    At every live step, at the recorded observation x and the state h entering the step, the gain is the local Jacobian
    G = da/dx [4, 22] of the action: its columns are the position gain (0..2), the attitude gain (3..11, R row-major), the damping
    gain (12..14, linear velocity), the rate gain (15..17, angular velocity) and the action feedback (18..21)
    (``OBSERVATION_BLOCKS``).  G is the INSTANTANEOUS gain at fixed h: the path of x_t into later actions through the recurrence is
    not part of it.  ReLU'(0) = 0, as in the learner's backward.

    ``policy``: a ``Raptor`` (fp32, no Standardize / SampleAndSquash stage, native rate), or a ``PolicyBank`` together with
    ``policy_ids`` - one id per env, constant on every aligned block of 64.  ``edges`` and the ages as for
    ``training.imitation_error`` (None: one bucket for every age); ``start`` as for ``Distiller``.

    The table's arrays are device tensors when torch is present, NumPy otherwise; the call orders itself against torch's current
    stream.  The trajectory's saved state is not touched: a pending ``trajectory_actions`` backward stays valid."""
    from .training import START, Distiller, _age_edges, _device_ptr
    if start not in START:
        raise ValueError('start must be "initial" or "current"')
    e = _age_edges(edges)
    N = int(traj._env.N_ENVIRONMENTS)
    bank = hasattr(policy, "n_policies")
    if bank and policy_ids is None:
        raise ValueError("a PolicyBank needs policy_ids: one id per env, constant on every aligned block of 64")
    if not bank and policy_ids is not None:
        raise ValueError("policy_ids belong to a PolicyBank")
    ids = None
    if bank:
        from .policy_bank import check_policy_ids
        ids = check_policy_ids(policy_ids, policy.n_policies, N)
    head = (policy._h, ids.ctypes.data) if bank else (policy._handle(traj._env._device),)
    name = "rq_trajectory_policies_gain_table" if bank else "rq_trajectory_policy_gain_table"
    dev = Distiller._torch_device(traj)
    B = e.size - 1
    if dev is None:
        total, count = np.empty((B, 4, HIDDEN, N), np.float32), np.empty((B, N), np.uint32)
        _lib.call(name, traj._require("trajectory"), *head, e.ctypes.data, B, START[start], _lib.fptr(total), count.ctypes.data, N, 0)
    else:
        import torch
        total = torch.empty((B, 4, HIDDEN, N), dtype=torch.float32, device=dev)
        count = torch.empty((B, N), dtype=torch.int32, device=dev)          # the engine's uint32; a recording has fewer than 2^31 steps
        torch.cuda.current_stream(dev).synchronize()          # the engine runs on its own stream
        _lib.call(name, traj._require("trajectory"), *head, e.ctypes.data, B, START[start], _device_ptr(total), _device_ptr(count), N, 1)
    w = np.asarray(policy.weights, np.float64)                # after any device-side update: fetched when first read
    W0 = w[..., _W0[0]:_W0[1]].reshape(w.shape[:-1] + (HIDDEN, 22))
    return GainTable(total, count, e, W0, ids if bank else None)


# ---------------------------------------------------------------------------- the flight table ---
# the columns of ``FlightTable.sum`` and ``FlightTable.peak``, in the order of the header's enums (RQ_FLIGHT_*, RQ_FLIGHT_PEAK_*)
FLIGHT_SUMS = ["pos2", "vel2", "omega2", "tilt", "act2", "dact2", "saturated", "outside", "reward"]
FLIGHT_PEAKS = ["pos2", "tilt", "omega2"]


def linear_age_edges(lo, hi, n):
    """n equal buckets of episode age over [lo, hi) -> uint32 [n + 1]; the width is (hi - lo) // n, at least 1, and the last edge
    is lo + n * width <= hi.  Around the onset of a poke: ``linear_age_edges(onset - 10, onset + 150, 32)``."""
    lo, hi, n = int(lo), int(hi), int(n)
    if not 1 <= n <= MAX_BUCKETS:
        raise ValueError(f"1 .. {MAX_BUCKETS} buckets, not {n}")
    if lo < 0 or hi >= 1 << 32 or hi <= lo:
        raise ValueError(f"[{lo}, {hi}) is no range of uint32 ages")
    width = (hi - lo) // n
    if width == 0:
        raise ValueError(f"{n} buckets over [{lo}, {hi}) would have width 0")
    return np.asarray([lo + k * width for k in range(n + 1)], np.uint32)


class FlightTable:
    """What ``flight_table`` returns: ``sum`` [B, 9, N] float32 (columns ``FLIGHT_SUMS``) - per age bucket and env the sums over its
    live steps of the squared deviation from the setpoint, the squared linear and angular velocity, the tilt 1 - R22, the squared
    action, the squared change of action, the number of saturated commands, the steps outside the tolerance and the reward -,
    ``peak`` [B, 3, N] float32 (columns ``FLIGHT_PEAKS``) - the largest squared deviation, tilt and squared rate -, ``count``
    [B, N] - the number of those steps - and ``edges`` [B + 1] (uint32, NumPy).  The arrays are NumPy or torch tensors, as the call
    made them; every method works in float64 on whatever they are and returns the same kind.  A mean over nothing is NaN."""

    CURVES = ["rms_position", "mean_tilt", "rms_rate", "effort", "command_change", "share_saturated", "share_outside", "mean_reward"]

    def __init__(self, sum, peak, count, edges):
        self.sum, self.peak, self.count = sum, peak, count
        self.edges = np.asarray(edges, np.uint32)
        if len(sum.shape) != 3 or sum.shape[1] != len(FLIGHT_SUMS) or tuple(peak.shape) != (sum.shape[0], len(FLIGHT_PEAKS), sum.shape[2]) \
                or tuple(count.shape) != (sum.shape[0], sum.shape[2]) or self.edges.shape != (sum.shape[0] + 1,):
            raise ValueError("sum must be [B, 9, N], peak [B, 3, N], count [B, N] and edges [B + 1]")

    def _torch(self):
        return hasattr(self.sum, "data_ptr")

    def _f64(self):
        if self._torch():
            import torch
            return self.sum.to(torch.float64), self.count.to(torch.float64)
        return np.asarray(self.sum, np.float64), np.asarray(self.count, np.float64)

    @staticmethod
    def _over(s, c):
        """s / c where c > 0, NaN elsewhere"""
        if hasattr(s, "data_ptr"):
            import torch
            return torch.where(c > 0, s / torch.clamp(c, min=1.0), torch.full_like(s, float("nan")))
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(c > 0, s / np.maximum(c, 1.0), np.nan)

    @staticmethod
    def _column(name):
        if name not in FLIGHT_SUMS:
            raise ValueError(f"unknown column {name!r}; the columns: {FLIGHT_SUMS}")
        return FLIGHT_SUMS.index(name)

    def mean(self, name):
        """-> [B, N]: the mean of column ``name`` (``FLIGHT_SUMS``) over the steps of env i at the ages of bucket b"""
        s, c = self._f64()
        return self._over(s[:, self._column(name)], c)

    def rms_position(self):
        """-> [B, N]: the root-mean-square distance from the setpoint"""
        return self.mean("pos2") ** 0.5

    @classmethod
    def _curves(cls, s, c):
        """s [..., 9] sums and c [...] counts in float64 -> the dict of curves [...]"""
        m = {name: cls._over(s[..., k], c) for k, name in enumerate(FLIGHT_SUMS)}
        return {"rms_position": m["pos2"] ** 0.5, "mean_tilt": m["tilt"], "rms_rate": m["omega2"] ** 0.5, "effort": m["act2"],
                "command_change": m["dact2"], "share_saturated": m["saturated"] / 4.0, "share_outside": m["outside"],
                "mean_reward": m["reward"]}

    def by_age(self):
        """-> a dict of [B] curves over all envs (``CURVES``): the step response of the fleet"""
        s, c = self._f64()
        return self._curves(s.sum(2), c.sum(1))

    def _ids(self, ids, n_groups):
        G, N = int(n_groups), int(self.sum.shape[2])
        g = np.asarray(ids.cpu() if hasattr(ids, "data_ptr") else ids)
        if g.shape != (N,) or g.dtype == bool or not np.issubdtype(g.dtype, np.integer) or (N and (g.min() < 0 or g.max() >= G)):
            raise ValueError(f"ids must be [{N}] integers below {G}")
        return g.astype(np.int64), G

    def by_group(self, ids, n_groups):
        """``ids`` [N] integers below ``n_groups`` - the wrench scenario, reference, teacher or policy of every env -> the dict of
        ``by_age`` with [G, B] curves, each over its group's envs; a group without a counted step gives NaN."""
        g, G = self._ids(ids, n_groups)
        s, c = self._f64()
        B = int(s.shape[0])
        if self._torch():
            import torch
            at = torch.as_tensor(g, device=s.device)
            gs = torch.zeros((G, B, len(FLIGHT_SUMS)), dtype=torch.float64, device=s.device).index_add(0, at, s.permute(2, 0, 1))
            gc = torch.zeros((G, B), dtype=torch.float64, device=s.device).index_add(0, at, c.T)
        else:
            gs, gc = np.zeros((G, B, len(FLIGHT_SUMS))), np.zeros((G, B))
            np.add.at(gs, g, s.transpose(2, 0, 1))
            np.add.at(gc, g, c.T)
        return self._curves(gs, gc)

    def peak_by_group(self, ids, n_groups):
        """-> [G, B, 3] (columns ``FLIGHT_PEAKS``): the maximum over a group's envs of the peaks; NaN where the group counted nothing"""
        g, G = self._ids(ids, n_groups)
        _, c = self._f64()
        B = int(self.peak.shape[0])
        if self._torch():
            import torch
            p = self.peak.to(torch.float64)
            at = torch.as_tensor(g, device=p.device)
            out = torch.zeros((G, B, len(FLIGHT_PEAKS)), dtype=torch.float64, device=p.device)
            src = p.permute(2, 0, 1)
            out = out.scatter_reduce(0, at[:, None, None].expand_as(src), src, "amax", include_self=True)
            gc = torch.zeros((G, B), dtype=torch.float64, device=p.device).index_add(0, at, c.T)
            return torch.where((gc > 0)[:, :, None], out, torch.full_like(out, float("nan")))
        p = np.asarray(self.peak, np.float64)
        out, gc = np.zeros((G, B, len(FLIGHT_PEAKS))), np.zeros((G, B))
        np.maximum.at(out, g, p.transpose(2, 0, 1))
        np.add.at(gc, g, c.T)
        return np.where((gc > 0)[:, :, None], out, np.nan)

    def per_env(self):
        """-> the dict of ``by_age`` with [N] curves: every env over all buckets - with ``edges=None`` over the whole recording"""
        s, c = self._f64()
        return self._curves(s.sum(0).T, c.sum(0))

    @staticmethod
    def recovery(curve, onset_bucket, level):
        """A host helper: the first bucket at or after ``onset_bucket`` from which ``curve`` [B] stays <= ``level`` to its end, or
        -1 (a NaN is not below the level)."""
        y = np.asarray(curve.cpu() if hasattr(curve, "data_ptr") else curve, np.float64)
        if y.ndim != 1 or not 0 <= int(onset_bucket) < y.size:
            raise ValueError("curve must be [B] and onset_bucket one of its buckets")
        with np.errstate(invalid="ignore"):
            ok = y <= float(level)
        for b in range(int(onset_bucket), y.size):
            if ok[b:].all():
                return b
        return -1


def flight_table(traj, edges=None, start_steps=None, tolerance=0.05, device=None):
    """The flight of every env of the recording, per bucket of episode age -> ``FlightTable``.  One pass on the device
    (rq_trajectory_flight_table) that reads the recording alone - no policy - and stores nothing of it.

    ``edges``: [B + 1] strictly ascending episode ages, B <= 32 (``linear_age_edges``, ``log_age_edges``); None: one bucket for
    every age.  ``start_steps`` [N]: what ``env.episode_steps()`` returned right before the rollout that recorded step 0 (None: 0) -
    the age is the row index of a wrench schedule or a moving setpoint, so a bucket of age is "time since the poke".
    ``tolerance``: the distance from the setpoint beyond which a step counts as ``outside``.

    ``device``: True - torch tensors on the trajectory's device; False - NumPy; None - tensors when torch is present.  The call
    orders itself against torch's current stream as ``training.imitation_error`` does."""
    from .training import Distiller, _age_edges, _device_ptr
    e = _age_edges(edges)
    N = int(traj._env.N_ENVIRONMENTS)
    tol = float(tolerance)
    if not np.isfinite(tol) or tol < 0:
        raise ValueError("tolerance must be finite and not negative")
    k = None
    if start_steps is not None:
        k = np.asarray(start_steps)
        if k.shape != (N,) or k.dtype == bool or not np.issubdtype(k.dtype, np.integer) or (k < 0).any() or (k >= 1 << 32).any():
            raise ValueError(f"start_steps must be {N} non-negative integers (env.episode_steps())")
        k = np.ascontiguousarray(k.astype(np.uint32))
    dev = None if device is False else Distiller._torch_device(traj)
    if device and dev is None:
        raise ValueError("device=True needs torch")
    B, ka = e.size - 1, None if k is None else k.ctypes.data
    if dev is None:
        total, peak = np.empty((B, len(FLIGHT_SUMS), N), np.float32), np.empty((B, len(FLIGHT_PEAKS), N), np.float32)
        count = np.empty((B, N), np.uint32)
        _lib.call("rq_trajectory_flight_table", traj._require("trajectory"), ka, tol, e.ctypes.data, B, _lib.fptr(total), _lib.fptr(peak),
                  count.ctypes.data, N, 0)
        return FlightTable(total, peak, count, e)
    import torch
    total = torch.empty((B, len(FLIGHT_SUMS), N), dtype=torch.float32, device=dev)
    peak = torch.empty((B, len(FLIGHT_PEAKS), N), dtype=torch.float32, device=dev)
    count = torch.empty((B, N), dtype=torch.int32, device=dev)          # the engine's uint32; a recording has fewer than 2^31 steps
    torch.cuda.current_stream(dev).synchronize()          # the engine runs on its own stream
    _lib.call("rq_trajectory_flight_table", traj._require("trajectory"), ka, tol, e.ctypes.data, B, _device_ptr(total), _device_ptr(peak),
              _device_ptr(count), N, 1)
    return FlightTable(total, peak, count, e)
