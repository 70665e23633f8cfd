"""The teacher bank (rq_teacher.hip) against a float64 reference with a per-element error bound (tests/teacher_reference.py),
at every launch shape and input edge the oracle comparisons of test_gpu_teachers.py leave out: all 108 register-stationary
kernels, step slicing (T >= 128), column chunking of the dense-stack kernel, row independence under inf / NaN inputs, and
magnitudes from 2^-10 to past the f16 range.  Run with -s to see the slack (largest |label - ref| / bound) of every case."""
import numpy as np
import pytest

import teacher_reference as R
from gpu_common import World

pytestmark = pytest.mark.gpu

ACT = R.ACT_CODE
FAMILY = [(64, 64), (64, 32), (32, 64), (32, 32), (32, 16), (16, 32), (16, 16), (64, 16), (16, 64)]
_TRAJ = {}


def _trajectory(device, oracle, n, T, seed=61):
    """a recorded trajectory of n envs x T steps (shared within the module); callers overwrite its observations"""
    key = (n, T, seed)
    if key not in _TRAJ:
        w = World(device, oracle, n, seed=seed, episode_step_limit=50)
        tr = w.vector.Trajectory(w.env, T)
        w.vector.rollout(device, w.env, w.params, w.state, w.policy, w.rng, T, "fused", True, trajectory=tr)
        _TRAJ[key] = (w, tr)
    return _TRAJ[key][1]


def _write_obs(device, tr, obs, pad=0.0):
    """obs [T, n, 22] into the trajectory's device block [T, 22, ld]; the padding envs n..ld get `pad`"""
    import torch
    device.synchronize()
    t = tr.tensors()["obs"]
    n = obs.shape[1]
    t[:, :, :n] = torch.from_numpy(np.ascontiguousarray(obs.transpose(0, 2, 1))).to(t.device)
    t[:, :, n:] = pad
    torch.cuda.synchronize()


def _weights(rng, n_teachers, in_dim, widths, scale=(1.0, 1.0, 1.0, 1.0)):
    """He-scaled teachers; scale[l] multiplies layer l (the last entry: all later layers)"""
    dims = [in_dim] + list(widths) + [4]
    out = []
    for _ in range(n_teachers):
        parts = []
        for i in range(len(dims) - 1):
            s = scale[min(i, len(scale) - 1)]
            parts.append(rng.standard_normal(dims[i + 1] * dims[i]) * s / np.sqrt(dims[i]))
            parts.append(rng.standard_normal(dims[i + 1]) * 0.1 * s)
        out.append(np.concatenate(parts))
    return np.asarray(out, np.float32)


def _ragged_ids(rng, n, n_teachers):
    """teacher 0 flies one env, teacher 1 seventeen (a full tile + one env), the last nobody; the rest random"""
    ids = rng.integers(2, n_teachers - 1, n).astype(np.uint32)
    ids[5] = 0
    ids[40:57] = 1
    return ids


def _bank(device, W, in_dim, widths, act, out_act):
    from raptor_amd.teachers import TeacherBank
    return TeacherBank.from_layers(device, W, in_dim, widths, act, out_act)


def _oracle(oracle, W, in_dim, widths, act, out_act, obs, ids):
    if len(widths) == 2 and all(h in (16, 32, 64) for h in widths):
        return oracle.teacher_relabel(W, in_dim, widths[0], widths[1], ACT[act], ACT[out_act], obs, ids, 8)
    return oracle.mlp_relabel(W, in_dim, widths, ACT[act], ACT[out_act], obs, ids, 8)


# ---------------------------------------------------------------------------- 1. all 108 register-stationary kernels ---
@pytest.mark.parametrize("h1,h2", FAMILY)
def test_every_register_stationary_kernel_meets_the_float64_bound(device, oracle, h1, h2):
    rng = np.random.default_rng(h1 * 100 + h2)
    n, T, n_teachers, in_dim = 600, 4, 12, 22
    tr = _trajectory(device, oracle, n, T)
    obs = (rng.standard_normal((T, n, 22)) * 1.5).astype(np.float32)
    _write_obs(device, tr, obs)
    ids = _ragged_ids(rng, n, n_teachers)
    for act in ("relu", "tanh"):
        for out_act in ("identity", "tanh"):
            W = _weights(rng, n_teachers, in_dim, [h1, h2])
            bank = _bank(device, W, in_dim, [h1, h2], act, out_act)
            ref_o = _oracle(oracle, W, in_dim, [h1, h2], act, out_act, obs, ids)
            for prec in ("fp32", "bf16", "f16x2"):
                bank.set_precision(prec)
                got = tr.relabel_teachers(bank, ids)
                ref, e = R.relabel_bound(W, in_dim, [h1, h2], act, out_act, obs, ids, prec)
                R.assert_within(got, ref, e, f"{h1}/{h2} {act}/{out_act} {prec}")
                if prec != "bf16":
                    assert np.abs(got - ref_o).max() < 1e-5, (prec, np.abs(got - ref_o).max())
                else:
                    assert np.abs(got - ref_o).max() < 5e-2


# ---------------------------------------------------------------------------- 2. step slicing ---
@pytest.mark.parametrize("T", [127, 128, 129, 200, 321])
def test_step_slices_meet_the_float64_bound(device, oracle, T):
    """launch_hh slices the steps across waves from T = 128 on (t_begin > 0, prefetch clamped to the slice)"""
    rng = np.random.default_rng(T)
    n, n_teachers, in_dim, widths = 333, 9, 21, [32, 64]
    tr = _trajectory(device, oracle, n, T)
    obs = rng.standard_normal((T, n, 22)).astype(np.float32)
    _write_obs(device, tr, obs, pad=np.nan)
    ids = _ragged_ids(rng, n, n_teachers)
    W = _weights(rng, n_teachers, in_dim, widths)
    bank = _bank(device, W, in_dim, widths, "relu", "tanh")
    for prec in ("fp32", "bf16", "f16x2"):
        bank.set_precision(prec)
        got = tr.relabel_teachers(bank, ids)
        ref, e = R.relabel_bound(W, in_dim, widths, "relu", "tanh", obs, ids, prec)
        R.assert_within(got, ref, e, f"T={T} {prec}")


def test_step_slicing_is_invisible_in_the_bits(device, oracle):
    """A T = 200 run (three slices of 67 steps) against 64-step runs (one slice) of the same observations: the first
    slice's first 64 steps and the second slice's (t_begin = 67) first 64 steps carry the same bits."""
    rng = np.random.default_rng(200)
    n, n_teachers, in_dim, widths = 320, 7, 22, [64, 32]
    long, short = _trajectory(device, oracle, n, 200, seed=62), _trajectory(device, oracle, n, 64, seed=63)
    obs = rng.standard_normal((200, n, 22)).astype(np.float32)
    ids = _ragged_ids(rng, n, n_teachers)
    W = _weights(rng, n_teachers, in_dim, widths)
    bank = _bank(device, W, in_dim, widths, "tanh", "identity")
    _write_obs(device, long, obs)
    sliced = {p: None for p in ("fp32", "bf16", "f16x2")}
    for prec in sliced:
        bank.set_precision(prec)
        sliced[prec] = long.relabel_teachers(bank, ids)
    for start in (0, 67):
        _write_obs(device, short, obs[start:start + 64])
        for prec in sliced:
            bank.set_precision(prec)
            assert np.array_equal(short.relabel_teachers(bank, ids), sliced[prec][start:start + 64]), (start, prec)


def test_a_tile_count_just_above_a_fraction_of_the_chip(device, oracle):
    """4 097 tiles = 16 384 / 4 + 1: four slices of 81 steps (the last 78) at T = 321; a sample of teachers checked"""
    from raptor_amd.teachers import balanced_teacher_assignment
    rng = np.random.default_rng(4097)
    n, T, n_teachers, in_dim, widths = 4097 * 16, 321, 241, 22, [16, 32]
    tr = _trajectory(device, oracle, n, T)
    ids = balanced_teacher_assignment(n, n_teachers)      # 17 whole tiles per teacher
    W = _weights(rng, n_teachers, in_dim, widths)
    bank = _bank(device, W, in_dim, widths, "relu", "identity")
    sel = np.nonzero(np.isin(ids, [0, 77, 160, 240]))[0]
    device.synchronize()
    import torch
    obs = tr.tensors()["obs"][:, :, torch.from_numpy(sel)].permute(0, 2, 1).cpu().numpy()     # the recorded observations
    for prec in ("fp32", "bf16", "f16x2"):
        bank.set_precision(prec)
        got = tr.relabel_teachers(bank, ids)[:, sel]
        ref, e = R.relabel_bound(W, in_dim, widths, "relu", "identity", obs, ids[sel], prec)
        R.assert_within(got, ref, e, f"4097 tiles T=321 {prec}")
    del _TRAJ[(n, T, 61)]                                 # 1.9 GB of observations


# ---------------------------------------------------------------------------- 3. chunks of the dense-stack kernel ---
LAYERS_CASES = [(64, [48], "relu", "identity"), (64, [64, 48, 32], "tanh", "tanh"), (64, [48, 64], "relu", "tanh"),
                (64, [16], "tanh", "identity"), (128, [128, 128, 128], "relu", "identity"), (128, [48, 80], "tanh", "tanh"),
                (128, [96], "relu", "tanh"), (128, [112, 16, 64], "tanh", "identity")]


@pytest.mark.parametrize("hp,widths,act,out_act", LAYERS_CASES)
def test_dense_stack_chunks_meet_the_float64_bound(device, oracle, hp, widths, act, out_act):
    """Teachers of 1, 0, kStride - 1, kStride, kStride + 1 and ~5 000 envs (kStride = 32 x waves = 128 / 256 columns): at
    ~16 000 columns per teacher the launcher splits every teacher into three chunks of columns rounded to 16."""
    rng = np.random.default_rng(hp + sum(widths))
    ks = 128 if hp == 64 else 256
    sizes = [1, 0, ks - 1, ks, ks + 1]
    n, T, in_dim = 6000, 16, 19
    sizes.append(n - sum(sizes))
    ids = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    rng.shuffle(ids)
    tr = _trajectory(device, oracle, n, T)
    obs = rng.standard_normal((T, n, 22)).astype(np.float32)
    _write_obs(device, tr, obs, pad=np.nan)
    W = _weights(rng, len(sizes), in_dim, widths)
    bank = _bank(device, W, in_dim, widths, act, out_act)
    assert bank.n_teachers * 8192 <= n * T          # chunks > 1
    got = tr.relabel_teachers(bank, ids)
    ref, e = R.relabel_bound(W, in_dim, widths, act, out_act, obs, ids, "fp32")
    R.assert_within(got, ref, e, f"layers HP={hp} {widths} {act}/{out_act}")
    assert np.abs(got - _oracle(oracle, W, in_dim, widths, act, out_act, obs, ids)).max() < 1e-5
    assert np.array_equal(got, tr.relabel_teachers(bank, ids))


# ---------------------------------------------------------------------------- 4. row independence ---
ROW_KERNELS = [([32, 64], "fp32"), ([32, 64], "bf16"), ([32, 64], "f16x2"), ([48], "fp32"), ([128, 80], "fp32")]


@pytest.mark.parametrize("in_dim", [1, 4, 5, 21, 22])
def test_rows_do_not_see_each_others_infinities(device, oracle, in_dim):
    """One (env, step) feature set to +-inf, NaN or 1e30 changes no other label's bits; NaN in the features >= in_dim
    and in the padding envs n..ld changes nothing; overwrite=True leaves the action columns >= n alone."""
    import torch
    rng = np.random.default_rng(in_dim)
    n, T, n_teachers = 200, 3, 5
    tr = _trajectory(device, oracle, n, T, seed=64)
    obs = rng.standard_normal((T, n, 22)).astype(np.float32)
    ids = _ragged_ids(rng, n, n_teachers)
    t0, e0 = 1, 41
    for widths, prec in ROW_KERNELS:
        W = _weights(rng, n_teachers, in_dim, widths)
        bank = _bank(device, W, in_dim, widths, "relu", "identity")
        bank.set_precision(prec)
        _write_obs(device, tr, obs)
        base = tr.relabel_teachers(bank, ids)
        others = np.ones(base.shape, bool)
        others[t0, e0] = False
        for v in (np.inf, -np.inf, np.nan, 1e30):
            o = obs.copy()
            o[t0, e0, in_dim - 1] = v
            _write_obs(device, tr, o)
            got = tr.relabel_teachers(bank, ids)
            assert np.array_equal(got[others], base[others]), (widths, prec, v)
        o = obs.copy()
        o[:, :, in_dim:] = np.nan
        _write_obs(device, tr, o, pad=np.nan)
        assert np.array_equal(tr.relabel_teachers(bank, ids), base), (widths, prec)
        device.synchronize()
        act = tr.tensors()["act"]
        act[:, :, n:] = -7.25
        torch.cuda.synchronize()
        tr.relabel_teachers(bank, ids, overwrite=True, fetch=False)
        device.synchronize()
        assert bool((act[:, :, n:] == -7.25).all()), (widths, prec)
        assert np.array_equal(act[:, :, :n].permute(0, 2, 1).cpu().numpy(), base)


# ---------------------------------------------------------------------------- 5. magnitudes ---
@pytest.mark.parametrize("scale", [2.0 ** -10, 2.0 ** 10])
@pytest.mark.parametrize("widths,act,out_act", [([64, 64], "relu", "identity"), ([16, 32], "tanh", "tanh"), ([96, 48], "relu", "identity")])
def test_scaled_inputs_and_weights_meet_the_bound(device, oracle, scale, widths, act, out_act):
    """2^-10: observations and layer-1 weights both scaled (pre-activations ~2^-20; the f16x2 lo pieces subnormal, its
    absolute floor).  2^10: the observations only (ReLU activations in the thousands, inside the f16 range).  Every bound
    is finite and below the label's own size (median e / |ref| < 1), so the comparison can tell a label from zero."""
    rng = np.random.default_rng(int(np.log2(scale)) + 40 + sum(widths))
    n, T, n_teachers, in_dim = 500, 3, 6, 22
    tr = _trajectory(device, oracle, n, T, seed=65)
    obs = (rng.standard_normal((T, n, 22)) * scale).astype(np.float32)
    _write_obs(device, tr, obs)
    ids = _ragged_ids(rng, n, n_teachers)
    W = _weights(rng, n_teachers, in_dim, widths, scale=(scale if scale < 1 else 1.0, 1.0))
    bank = _bank(device, W, in_dim, widths, act, out_act)
    for prec in (("fp32", "bf16", "f16x2") if widths[0] <= 64 else ("fp32",)):
        bank.set_precision(prec)
        got = tr.relabel_teachers(bank, ids)
        ref, e = R.relabel_bound(W, in_dim, widths, act, out_act, obs, ids, prec)
        R.assert_within(got, ref, e, f"x{scale:g} {widths} {act}/{out_act} {prec}")
        assert np.median(e / np.abs(ref)) < 1.0, (prec, np.median(e / np.abs(ref)))


def test_split_f16_teacher_saturates_out_of_range_inputs(device, oracle):
    """f16x2: observations up to 1e30, and ReLU activations past 65 504 (W1 scaled up), give finite labels wherever fp32
    does (a plain split turns them into hi = inf, lo = -inf and the labels into NaN); inputs just inside the f16 range
    (6e4, with ReLU activations up to ~3.8e4, also inside it) meet the bound."""
    rng = np.random.default_rng(65504)
    n, T, n_teachers, in_dim, widths = 300, 3, 4, 22, [64, 32]
    tr = _trajectory(device, oracle, n, T, seed=66)
    ids = _ragged_ids(rng, n, n_teachers)
    obs = rng.standard_normal((T, n, 22)).astype(np.float32)
    obs[:, ::3, 5] = 1e30
    obs[:, 1::3, 0] = -7e4
    for act in ("relu", "tanh"):
        W = _weights(rng, n_teachers, in_dim, widths)
        bank = _bank(device, W, in_dim, widths, act, "identity")
        _write_obs(device, tr, obs)
        ref32 = tr.relabel_teachers(bank, ids)
        bank.set_precision("f16x2")
        got = tr.relabel_teachers(bank, ids)
        fin = np.isfinite(ref32)
        assert fin.all() and np.isfinite(got).all(), (act, int((~np.isfinite(got)).sum()))
    # ReLU activations past 65 504: W1 scaled by 300 (still inside the f16 range) on observations of a few hundred
    W = _weights(rng, n_teachers, in_dim, widths, scale=(300.0, 1.0))
    bank = _bank(device, W, in_dim, widths, "relu", "identity")
    big = (rng.standard_normal((T, n, 22)) * 300).astype(np.float32)
    _write_obs(device, tr, big)
    ref32 = tr.relabel_teachers(bank, ids)
    ref, e = R.relabel_bound(W, in_dim, widths, "relu", "identity", big, ids, "fp32")
    R.assert_within(ref32, ref, e, "fp32, ReLU activations past 65 504")
    assert np.isinf(R.relabel_bound(W, in_dim, widths, "relu", "identity", big, ids, "f16x2")[1]).any()   # past the range
    bank.set_precision("f16x2")
    got = tr.relabel_teachers(bank, ids)
    assert np.isfinite(ref32).all() and np.isfinite(got).all(), int((~np.isfinite(got)).sum())
    # just inside the range: inputs up to 6e4, W1 scaled by 2^-2 so that the ReLU activations reach past 2^15 in layer 1
    # and 2^14 in layer 2 yet stay below 65 504 - a saturation below the f16 maximum (at 2^13 or 2^14, say) breaks the bound
    inside = (rng.uniform(-1, 1, (T, n, 22)) * 6e4).astype(np.float32)
    W = _weights(rng, n_teachers, in_dim, widths, scale=(2.0 ** -2, 1.0))
    bank = _bank(device, W, in_dim, widths, "relu", "identity")
    _write_obs(device, tr, inside)
    bank.set_precision("f16x2")
    got = tr.relabel_teachers(bank, ids)
    ref, e = R.relabel_bound(W, in_dim, widths, "relu", "identity", inside, ids, "f16x2")
    peaks = np.max([R.hidden_peak(R.unpack(W[k], in_dim, widths), "relu", inside[:, ids == k, :in_dim].reshape(-1, in_dim))
                    for k in np.unique(ids)], axis=0)
    R.assert_within(got, ref, e, f"f16x2 inputs up to 6e4, ReLU activations up to {peaks.tolist()}")
    assert peaks[0] > 2.0 ** 15 and peaks[1] > 2.0 ** 14 and (peaks < 65504.0).all(), peaks


def test_weights_outside_the_f16_range_are_refused_for_f16x2(device, oracle):
    """A weight of 3e4 under tanh (pre-scaled to -8.7e4) or of 7e4 under ReLU has no f16x2 image: set_precision says so;
    fp32 and bf16 still label the bank, and a weight of 6e4 under ReLU is held and meets the bound."""
    rng = np.random.default_rng(7)
    n, T, n_teachers, in_dim, widths = 64, 2, 2, 22, [16, 16]
    tr = _trajectory(device, oracle, n, T, seed=67)
    obs = rng.standard_normal((T, n, 22)).astype(np.float32) * 1e-3
    _write_obs(device, tr, obs)
    ids = (np.arange(n) % n_teachers).astype(np.uint32)
    for act, v, fits in (("tanh", 3e4, False), ("relu", 7e4, False), ("relu", 6e4, True)):
        W = _weights(rng, n_teachers, in_dim, widths)
        W[1, 3] = v                                     # W1[0, 3] of teacher 1
        bank = _bank(device, W, in_dim, widths, act, "identity")
        if not fits:
            with pytest.raises(Exception, match="teacher 1 has a weight outside the f16 range"):
                bank.set_precision("f16x2")
            assert bank.precision == "fp32"
            for prec in ("fp32", "bf16"):
                bank.set_precision(prec)
                assert np.isfinite(tr.relabel_teachers(bank, ids)).all()
            continue
        bank.set_precision("f16x2")
        got = tr.relabel_teachers(bank, ids)
        ref, e = R.relabel_bound(W, in_dim, widths, act, "identity", obs, ids, "f16x2")
        R.assert_within(got, ref, e, f"f16x2 weight {v:g}")
