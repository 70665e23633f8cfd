"""A teacher bank on a moving setpoint (rq_rollout_teachers_track, rq_rollout_teachers_track_refs; TeacherBank.fly / closed_loop):
one reference or one per env, fused and chained.  Every comparison is on the bits (tests/rollout_common.py) - fused against
chained, both against the host loop, the reference bank against single references, the hover table against the untracked rollout -
except where the oracle's re-sampled sin / cos enter (the project's 1e-4 bar for those, as in test_gpu_teacher_rollout.py).

Shapes: episode_step_limit 7 and tables of 7 rows, launches of 12 + 8 steps (the row index restarts at episode ends and crosses a
launch), a third of the envs pushed outside termination_position first so that they fly out of phase with the rest.  One test needs a
window WITHOUT episode ends (the host loop, 12 steps): it alone flies a limit and tables of 13."""
import numpy as np
import pytest

import raptor_amd.l2f as l2f
from raptor_amd import _lib, tracking
from gpu_common import World
from rollout_common import assert_same, assert_same_recording, bits, push, random_table, snapshot

pytestmark = pytest.mark.gpu

LIMIT = 7
CHUNKS = (12, 8)
M = 3
KW = dict(episode_step_limit=LIMIT, termination_position=0.6)
NOISE = dict(noise_position=0.01, noise_linear_velocity=0.02)
TRACK_KEYS = ("track_sq", "track_steps")


@pytest.fixture(scope="module")
def tables():
    t = np.stack([random_table(LIMIT, 31 + r) for r in range(M)])
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def refbank(device, tables):
    return l2f.ReferenceBank(device, tables)


@pytest.fixture(scope="module")
def refs(device, tables):
    return [l2f.Reference(device, np.array(tables[r])) for r in range(M)]


def _weights(rng, n_teachers, in_dim, widths, scale=1.0):
    from raptor_amd.teachers import layers_parameter_count
    W = np.empty((n_teachers, layers_parameter_count(in_dim, widths)), np.float32)
    for t in range(n_teachers):
        parts, prev = [], in_dim
        for h in list(widths) + [4]:
            parts += [rng.standard_normal(h * prev) * scale / np.sqrt(prev), rng.standard_normal(h) * 0.1]
            prev = h
        W[t] = np.concatenate(parts).astype(np.float32)
    return W


def _bank(device, W, in_dim, widths, act="relu", out_act="tanh", precision="fp32"):
    from raptor_amd.teachers import TeacherBank
    return TeacherBank.from_layers(device, W, in_dim, widths, act, out_act, precision)


def _ids(kind, n, K, rng):
    """the assignments of test_gpu_teacher_rollout.py: one teacher; random and ragged with an empty and a one-env teacher; balanced"""
    if kind == "balanced":
        from raptor_amd.teachers import balanced_teacher_assignment
        return balanced_teacher_assignment(n, K)
    if kind == "single":
        return np.full(n, K - 1, np.uint32)
    ids = rng.integers(0, K - 2, n).astype(np.uint32)
    ids[n // 2] = K - 1
    return ids


def _rids(n):
    """different ids inside every 16-env tile"""
    return (np.arange(n) % M).astype(np.uint32)


def _launch(w, bank, ids, steps, mode, autoreset, tr=None, ref=None, rids=None):
    bank.fly(w.vector, w.device, w.env, w.params, w.state, w.rng, steps, ids, mode, autoreset, trajectory=tr, reference=ref,
             reference_ids=rids)


def _fly(device, oracle, n, bank, ids, mode, autoreset, ref=None, rids=None, chunks=CHUNKS, seed=5, pushed=True, extra=0, **cfg):
    """a fresh world, pushed, flown in `chunks` launches -> the world and its recording (room for `extra` more steps)"""
    w = World(device, oracle, n, seed=seed, **{**KW, **cfg})
    tr = w.vector.Trajectory(w.env, sum(chunks) + extra)
    if pushed:
        push(w, 1)
    for c in chunks:
        _launch(w, bank, ids, c, mode, autoreset, tr, ref, rids)
    return w, tr


# a * b + c in float32 with ONE rounding, as __fmaf_rn gives it: the product is exact in float64, the sum is made error-free
# (TwoSum) and rounded to odd there, so that the final rounding to float32 is the rounding of the exact value
def _fma32(a, b, c):
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    raw = s.view(np.int64)
    nudge = np.where((err > 0) == (s > 0), 1, -1)
    odd = np.where((err != 0) & (raw & 1 == 0), raw + nudge, raw).view(np.float64)
    return odd.astype(np.float32)


def _accumulate(total, p, row):
    """track_accumulate (rq_device_math.hpp): d = p - r per axis, e = fma(dz, dz, fma(dy, dy, dx dx)), total + e, all float32"""
    d = (p.astype(np.float32) - row[:, :3].astype(np.float32)).astype(np.float32)
    e = _fma32(d[:, 2], d[:, 2], _fma32(d[:, 1], d[:, 1], _fma32(d[:, 0], d[:, 0], np.zeros(len(d), np.float32))))
    return _fma32(e, np.ones(len(d), np.float32), total)


def test_the_host_side_fma_rounds_once():
    """the yardstick of the tracking sums checked by itself: a product kept exact, and a float32 tie that only the tail below
    float64's last bit breaks (rounding twice would land on the even neighbour)"""
    a = np.float32([1.0 + 2.0 ** -12])
    assert _fma32(a, a, np.float32([-1.0]))[0] == np.float32(2.0 ** -11 + 2.0 ** -24)
    assert (a * a - np.float32(1.0))[0] == np.float32(2.0 ** -11)
    assert _fma32(a, a, np.float32([2.0 ** -60]))[0] == np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert _fma32(a, a, np.float32([-2.0 ** -60]))[0] == np.float32(1.0 + 2.0 ** -11)
    assert _fma32(a, a, np.float32([0.0]))[0] == np.float32(1.0 + 2.0 ** -11)          # the tie itself: to even


# ------------------------------------------------------------------ 1. fused equals chained -----
_ARCHS = [((16, 16), "relu", "identity"), ((32, 64), "tanh", "tanh"), ((64, 64), "relu", "tanh")]


@pytest.mark.parametrize("arch", _ARCHS)
@pytest.mark.parametrize("n,kind", [(1, "single"), (15, "random"), (16, "balanced"), (17, "random"), (200, "random")])
def test_fused_equals_chained(device, oracle, refs, refbank, arch, n, kind):
    widths, act, out_act = arch
    rng = np.random.default_rng(n * 7 + widths[0])
    K = 9
    bank = _bank(device, _weights(rng, K, 22, widths), 22, list(widths), act, out_act)
    ids = _ids(kind, n, K, rng)
    for ref, rids in ((refs[1], None), (refbank, _rids(n))):
        what = f"n={n} {kind} {'bank' if rids is not None else 'single'}"
        for noise in (True, False):
            cfg = NOISE if noise else {}
            wf, tf = _fly(device, oracle, n, bank, ids, "fused", True, ref, rids, seed=n, **cfg)
            wc, tc = _fly(device, oracle, n, bank, ids, "chained", True, ref, rids, seed=n, **cfg)
            sf = snapshot(wf)
            assert_same(sf, snapshot(wc), what=f"{what} noise={noise}")
            assert_same_recording(tf.numpy(), tc.numpy(), what)
            assert (tf.numpy()["done"] != 0).any() and sf["fin_counts"].min() >= 2          # episode ends were crossed
            assert np.array_equal(sf["track_steps"], np.full(n, sum(CHUNKS), np.uint32)) and (sf["track_sq"] > 0).all()
        # a freezing rollout: an env flies its one episode and sits still - a frozen env adds nothing to the sums
        wf, tf = _fly(device, oracle, n, bank, ids, "fused", False, ref, rids, seed=n + 1, extra=5)
        wc, tc = _fly(device, oracle, n, bank, ids, "chained", False, ref, rids, seed=n + 1, extra=5)
        sf = snapshot(wf)
        assert_same(sf, snapshot(wc), what=f"{what} freezing")
        assert_same_recording(tf.numpy(), tc.numpy(), what)
        assert sf["frozen"].all() and np.array_equal(sf["track_steps"], sf["fin_lengths"]) and sf["track_steps"].max() <= LIMIT
        # ... and a thawing one
        for w, tr, mode in ((wf, tf, "fused"), (wc, tc, "chained")):
            _launch(w, bank, ids, 5, mode, True, tr, ref, rids)
        st = snapshot(wf)
        assert_same(st, snapshot(wc), what=f"{what} thaw")
        assert_same_recording(tf.numpy(), tc.numpy(), what)
        assert not st["frozen"].any() and np.array_equal(st["track_steps"], sf["track_steps"] + 5)


# ------------------------------------------------------------------ 2. the host loop -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
@pytest.mark.parametrize("banked", [False, True])
def test_rollout_equals_the_host_loop(device, oracle, mode, banked):
    """observe -> subtract the row of the env's episode step count on the host -> bank.evaluate -> vector.step -> assign, 12 steps in
    a window without episode ends (limit and tables of 13 rows: the one test off the file's limit of 7), noise on; the tracking sum
    recomputed on the host in float32 in track_accumulate's order."""
    n, T, K, rows = 100, 12, 5, 13
    rng = np.random.default_rng(2)
    bank = _bank(device, _weights(rng, K, 22, [32, 16], scale=0.2), 22, [32, 16], "tanh", "identity")     # gentle: nobody terminates
    ids = (np.arange(n) % K).astype(np.uint32)
    tabs = np.stack([random_table(rows, 41 + r) for r in range(M)])
    rids = _rids(n) if banked else np.zeros(n, np.uint32)
    ref = l2f.ReferenceBank(device, tabs) if banked else l2f.Reference(device, tabs[0])
    cfg = dict(episode_step_limit=rows, termination_position=1.0, **NOISE)
    w, tr = _fly(device, oracle, n, bank, ids, mode, False, ref, rids if banked else None, chunks=(T,), seed=3, pushed=False, **cfg)
    rec = tr.numpy()
    assert (rec["done"] == 0).all()
    u = World(device, oracle, n, seed=3, **cfg)
    obs = np.zeros((n, u.env.OBSERVATION_DIM), np.float32)
    sq = np.zeros(n, np.float32)
    for t in range(T):
        u.vector.observe(device, u.env, u.params, u.state, obs, u.rng)
        k = u.env.episode_steps()
        assert (k == t).all()
        row = tabs[rids, np.minimum(k, rows - 1)]
        o = obs[:, :22].copy()
        o[:, 0:3] -= row[:, 0:3]
        o[:, 12:15] -= row[:, 3:6]
        sq = _accumulate(sq, u.state.numpy()[:, 0:3], row)
        a = bank.evaluate(o, ids)
        assert np.array_equal(bits(o), bits(rec["obs"][t])), t
        assert np.array_equal(bits(a), bits(rec["act"][t])), t
        u.vector.step(device, u.env, u.params, u.state, a, u.next_state, u.rng)
        u.state.assign(u.next_state)
        assert np.array_equal(bits(u.env.rewards()), bits(rec["rew"][t])), t
        assert np.array_equal(u.env.done_codes(), rec["done"][t]), t
    sw = snapshot(w)
    assert_same(sw, snapshot(u), skip=TRACK_KEYS, what=mode)
    assert np.array_equal(bits(sw["track_sq"]), bits(sq))
    assert np.array_equal(sw["track_steps"], np.full(n, T, np.uint32))


# ------------------------------------------------------------------ 3. the teacher saw the shifted observation -----
@pytest.mark.parametrize("kind", ["fp32", "bf16", "stack"])
def test_relabelling_a_tracked_recording_returns_its_actions(device, oracle, refbank, kind):
    rng = np.random.default_rng(11)
    n, K = 70, 6
    widths = [32, 48, 32] if kind == "stack" else [64, 32]
    in_dim = 19 if kind == "fp32" else 22
    bank = _bank(device, _weights(rng, K, in_dim, widths), in_dim, widths, "tanh", "identity", "fp32" if kind == "stack" else kind)
    ids = rng.integers(0, K, n).astype(np.uint32)
    rids = _rids(n)
    w, tr = _fly(device, oracle, n, bank, ids, "fused" if kind == "fp32" else "chained", True, refbank, rids, seed=21, **NOISE)
    rec = tr.numpy()
    live = rec["done"] != 4
    assert live.all() and (rec["done"] != 0).any()
    lab = tr.relabel_teachers(bank, ids)
    assert np.array_equal(bits(lab[live]), bits(rec["act"][live]))
    # and what it saw is not what an untracked teacher sees
    w0, tr0 = _fly(device, oracle, n, bank, ids, "chained", True, seed=21, **NOISE)
    assert not np.array_equal(tr0.numpy()["obs"][0, :, 0:3], rec["obs"][0, :, 0:3])


# ------------------------------------------------------------------ 4. reference bank equals single references -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_reference_bank_equals_single_references(device, oracle, refs, refbank, mode):
    rng = np.random.default_rng(4)
    n, K = 50, 4
    bank = _bank(device, _weights(rng, K, 22, [16, 32]), 22, [16, 32])
    ids = rng.integers(0, K, n).astype(np.uint32)
    rids = _rids(n)
    for autoreset in (True, False):
        w, tr = _fly(device, oracle, n, bank, ids, mode, autoreset, refbank, rids, **NOISE)
        snap, rec = snapshot(w), tr.numpy()
        seen = []
        for r in range(M):
            b, tb = _fly(device, oracle, n, bank, ids, mode, autoreset, refs[r], **NOISE)
            sel = rids == r
            assert_same(snap, snapshot(b), rows=sel, what=f"{mode} autoreset={autoreset} reference {r}")
            rb = tb.numpy()
            assert_same_recording({k: v[:, sel] for k, v in rec.items()}, {k: v[:, sel] for k, v in rb.items()}, f"reference {r}")
            seen.append(rb["obs"][0, :, 0:3])
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


# ------------------------------------------------------------------ 5. the hover table equals the untracked rollout -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_hover_table_equals_untracked(device, oracle, mode):
    rng = np.random.default_rng(5)
    n, K = 40, 3
    bank = _bank(device, _weights(rng, K, 22, [32, 32]), 22, [32, 32])
    ids = rng.integers(0, K, n).astype(np.uint32)
    hold = l2f.Reference(device, tracking.hold(LIMIT))
    w, tr = _fly(device, oracle, n, bank, ids, mode, True, hold)
    u = World(device, oracle, n, seed=5, **KW)
    ut = u.vector.Trajectory(u.env, sum(CHUNKS))
    push(u, 1)
    for c in CHUNKS:
        _lib.call("rq_rollout_teachers", device._h, u.env._h, u.params._h, u.state._h, bank._h, ids.ctypes.data, u.rng._h, c,
                  l2f.ROLLOUT_FUSED if mode == "fused" else l2f.ROLLOUT_CHAINED, l2f.ROLLOUT_AUTORESET, ut._require("trajectory"))
    sw, rec = snapshot(w), tr.numpy()
    assert_same(sw, snapshot(u), skip=TRACK_KEYS, what=mode)
    assert_same_recording(rec, ut.numpy(), mode, frozen_too=True)
    sq = np.zeros(n, np.float32)
    for t in range(sum(CHUNKS)):                 # noise off: the recorded position columns are the true position
        sq = _accumulate(sq, rec["obs"][t][:, 0:3], np.zeros((n, 6), np.float32))
    assert np.array_equal(bits(sw["track_sq"]), bits(sq)) and (sq > 0).all()
    assert np.array_equal(sw["track_steps"], np.full(n, sum(CHUNKS), np.uint32))


# ------------------------------------------------------------------ 6. constant-action teachers against the oracle -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_constant_action_teachers_against_the_oracle(device, oracle, tables, refbank, mode):
    """Teachers with zero weights and output bias c_k act c_k exactly, whatever they see: the recorded observation is the oracle's
    with the row of the oracle's own episode step count subtracted, rewards and done codes are the oracle's on the ABSOLUTE state -
    bit for bit until an env's first re-sample, within 1e-4 after it (the oracle's sin / cos in sample_initial_state)."""
    from raptor_amd.teachers import TeacherBank, parameter_count
    n, K = 100, 5
    rng = np.random.default_rng(1)
    c = rng.uniform(-0.3, 0.3, (K, 4)).astype(np.float32)
    W = np.zeros((K, parameter_count(22, 16, 16)), np.float32)
    W[:, -4:] = c
    bank = TeacherBank(device, W, 22, 16, 16, "relu", "identity")
    ids = (np.arange(n) % K).astype(np.uint32)
    rids = _rids(n)
    w, tr = _fly(device, oracle, n, bank, ids, mode, True, refbank, rids)
    rec = tr.numpy()
    v = World(device, oracle, n, seed=5, **KW)
    push(v, 1)
    O, st, P = oracle, v.st, v.P
    S = v.state.numpy().copy()                     # start from the GPU's initial state (sin / cos ulps), pushed
    reset = np.zeros(n, bool)
    for t in range(sum(CHUNKS)):
        row = tables[rids, np.minimum(st.steps, LIMIT - 1)]
        o = O.observe(v.cfg, v.seed, t, 0, P, S)[:, :22].astype(np.float32)
        o[:, 0:3] -= row[:, 0:3]
        o[:, 12:15] -= row[:, 3:6]
        assert np.array_equal(bits(o[~reset]), bits(rec["obs"][t][~reset])), t
        assert np.abs(o[reset] - rec["obs"][t][reset]).max(initial=0.0) < 1e-4, t
        assert np.array_equal(rec["act"][t], c[ids])
        S, r, term = O.step(v.cfg, P, S, c[ids])
        O.stats_update(v.cfg, r, term, st)
        ended = term.astype(bool) | (st.steps == 0)
        assert np.array_equal(bits(r[~reset]), bits(rec["rew"][t][~reset])), t
        assert np.abs(r[reset] - rec["rew"][t][reset]).max(initial=0.0) < 1e-4, t
        codes = np.where(term != 0, 1, np.where(ended, 2, 0)).astype(np.uint8)
        assert np.array_equal(codes, rec["done"][t]), t
        if ended.any():
            fresh = O.sample_initial_state(v.cfg, v.seed, st.episode, 0, P)      # increments every counter: undo the others
            st.episode[~ended] -= 1
            S[ended] = fresh[ended]
            reset |= ended
    assert (rec["done"][0] == 1).any() and (rec["done"] == 2).any() and reset.all()
    assert np.array_equal(st.episode, w.env.episode_index())
    assert np.array_equal(st.fin_counts, w.env.finished_counts())
    assert np.abs(S - w.state.numpy()).max() < 1e-4


# ------------------------------------------------------------------ 7. a neighbour's table leaves a row alone -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_a_neighbours_table_leaves_a_row_alone(device, oracle, tables, refbank, mode):
    """A reference bank refuses a non-finite entry, so table 2's poisoned row holds the largest finite float instead of a NaN: the
    envs on tables 0 and 1 - lane neighbours of those on table 2 in every tile - are bit-identical to a run whose table 2 is
    ordinary, and the envs on table 2 record that row in what their teacher saw."""
    rng = np.random.default_rng(7)
    n, K = 40, 4
    bank = _bank(device, _weights(rng, K, 22, [32, 32]), 22, [32, 32])
    ids = rng.integers(0, K, n).astype(np.uint32)
    rids = _rids(n)
    big = np.finfo(np.float32).max
    poisoned = np.array(tables)
    poisoned[2, 3, :] = big
    wa, ta = _fly(device, oracle, n, bank, ids, mode, True, refbank, rids)
    wb, tb = _fly(device, oracle, n, bank, ids, mode, True, l2f.ReferenceBank(device, poisoned), rids)
    keep = rids != 2
    assert_same(snapshot(wa), snapshot(wb), rows=keep, what=mode)
    ra, rb = ta.numpy(), tb.numpy()
    assert_same_recording({k: v[:, keep] for k, v in ra.items()}, {k: v[:, keep] for k, v in rb.items()}, mode, frozen_too=True)
    # envs on table 2 that reached row 3 in their first episode saw it: position and velocity entries near -FLT_MAX, nothing else
    at_row_3 = rb["obs"][3][~keep]
    hit = at_row_3[:, 0] < -1e38
    assert hit.sum() >= (~keep).sum() // 2
    assert (at_row_3[hit][:, [0, 1, 2, 12, 13, 14]] < -1e38).all() and (np.abs(at_row_3[hit][:, 3:12]) <= 1.0).all()
    assert not (np.abs(rb["obs"][:, keep]) > 1e30).any()


# ------------------------------------------------------------------ 8. refusals -----
def test_refusals_leave_everything_untouched(device, oracle, tables, refs, refbank):
    rng = np.random.default_rng(8)
    n, K = 20, 3
    W = _weights(rng, K, 22, [16, 16])
    bank = _bank(device, W, 22, [16, 16])
    bf = _bank(device, W, 22, [16, 16], precision="bf16")
    ids = (np.arange(n) % K).astype(np.uint32)
    rids = _rids(n)
    w = World(device, oracle, n, seed=4, **KW)
    tr = w.vector.Trajectory(w.env, 30)
    push(w, 1)
    _launch(w, bank, ids, 3, "fused", True, tr, refbank, rids)
    before, rec, epoch = snapshot(w), tr.numpy(), w.rng.epoch
    short = l2f.Reference(device, random_table(LIMIT - 1))
    short_bank = l2f.ReferenceBank(device, np.array(tables[:, :LIMIT - 1]))
    dev2 = l2f.Device(0)
    far_ref = l2f.Reference(dev2, np.array(tables[0]))
    far_bank = l2f.ReferenceBank(dev2, tables)
    bad_rids = rids.copy()
    bad_rids[13] = M
    bad_ids = ids.copy()
    bad_ids[4] = K

    def raw(name, *tail, bank_=bank, ids_=ids, steps=2, mode=l2f.ROLLOUT_FUSED, flags=l2f.ROLLOUT_AUTORESET):
        _lib.call(name, device._h, w.env._h, w.params._h, w.state._h, bank_._h, ids_.ctypes.data, w.rng._h, steps, mode, flags,
                  tr._require("trajectory"), *tail)
    one, many = "rq_rollout_teachers_track", "rq_rollout_teachers_track_refs"
    for mode in (l2f.ROLLOUT_FUSED, l2f.ROLLOUT_CHAINED):
        for words, call in (
                ("fewer rows than episode_step_limit", lambda: raw(one, short._h, mode=mode)),
                ("fewer rows than episode_step_limit", lambda: raw(many, short_bank._h, rids.ctypes.data, mode=mode)),
                ("another device", lambda: raw(one, far_ref._h, mode=mode)),
                ("another device", lambda: raw(many, far_bank._h, rids.ctypes.data, mode=mode)),
                (f"env 13 names reference {M} of a bank of {M}", lambda: raw(many, refbank._h, bad_rids.ctypes.data, mode=mode)),
                ("teacher id out of range", lambda: raw(one, refs[0]._h, ids_=bad_ids, mode=mode)),
                ("teacher id out of range", lambda: raw(many, refbank._h, rids.ctypes.data, ids_=bad_ids, mode=mode)),
                ("unknown flags", lambda: raw(one, refs[0]._h, flags=8, mode=mode)),
                ("too small", lambda: raw(one, refs[0]._h, steps=28, mode=mode)),
                ("too small", lambda: raw(many, refbank._h, rids.ctypes.data, steps=28, mode=mode)),
                ("null reference", lambda: raw(one, None, mode=mode)),
                ("null reference", lambda: raw(many, None, rids.ctypes.data, mode=mode)),
                ("null reference_id", lambda: raw(many, refbank._h, None, mode=mode))):
            with pytest.raises(Exception, match=words):
                call()
    with pytest.raises(Exception, match="unknown mode"):
        raw(one, refs[0]._h, mode=7)
    with pytest.raises(Exception, match="chained"):
        raw(one, refs[0]._h, bank_=bf)
    with pytest.raises(Exception, match="chained"):
        raw(many, refbank._h, rids.ctypes.data, bank_=bf)

    def fly(bank_=bank, ids_=ids, steps=2, mode="fused", **kw):
        _launch(w, bank_, ids_, steps, mode, True, tr, **kw)
    for words, call in (("fewer rows than episode_step_limit", lambda: fly(ref=short)),
                        ("fewer rows than episode_step_limit", lambda: fly(ref=short_bank, rids=rids, mode="chained")),
                        ("another device", lambda: fly(ref=far_ref)),
                        ("another device", lambda: fly(ref=far_bank, rids=rids)),
                        (f"env 13 names reference {M}", lambda: fly(ref=refbank, rids=bad_rids)),
                        ("teacher id out of range", lambda: fly(ids_=bad_ids, ref=refs[0])),
                        ("chained", lambda: fly(bank_=bf, ref=refs[0])),
                        ("chained", lambda: fly(bank_=bf, ref=refbank, rids=rids)),
                        ("too small", lambda: fly(steps=28, ref=refbank, rids=rids))):
        with pytest.raises(Exception, match=words):
            call()
    with pytest.raises(Exception):
        fly(mode="warp", ref=refs[0])
    assert_same(before, snapshot(w), what="after refusals")
    assert w.rng.epoch == epoch and len(tr) == 3
    now = tr.numpy()
    assert all(np.array_equal(bits(now[k]), bits(rec[k])) for k in rec)
    # the next tracked rollout equals one on a world that never saw the refusals
    _launch(w, bank, ids, 4, "fused", True, tr, refbank, rids)
    u = World(device, oracle, n, seed=4, **KW)
    ut = u.vector.Trajectory(u.env, 30)
    push(u, 1)
    _launch(u, bank, ids, 3, "fused", True, ut, refbank, rids)
    _launch(u, bank, ids, 4, "fused", True, ut, refbank, rids)
    assert_same(snapshot(w), snapshot(u), what="after the refusals")
    assert_same_recording(tr.numpy(), ut.numpy(), frozen_too=True)
    # a bf16 bank flies chained
    _launch(w, bf, ids, 2, "chained", True, tr, refbank, rids)
    assert w.rng.epoch == epoch + 6


# ------------------------------------------------------------------ 9. closed_loop -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_closed_loop_tables(device, oracle, refs, refbank, mode):
    from raptor_amd.policy_bank import policy_tracking_table
    from raptor_amd.teachers import teacher_episode_table
    rng = np.random.default_rng(9)
    n, K = 60, 5
    bank = _bank(device, _weights(rng, K, 22, [16, 16]), 22, [16, 16])
    ids = rng.integers(0, K - 1, n).astype(np.uint32)               # teacher K - 1 flies nothing
    rids = tracking.spread_reference_ids(n, M, ids)
    w = World(device, oracle, n, seed=6, **KW)
    push(w, 1)
    _launch(w, bank, ids, 5, mode, True, None, refs[0])              # statistics that closed_loop must start afresh
    args = (w.vector, device, w.env, w.params, w.state, w.rng, 20, ids)
    t1 = bank.closed_loop(*args, mode=mode, reference=refs[2])
    sq, cnt = w.env.tracking_error()
    assert np.array_equal(cnt, np.full(n, 20, np.uint32))
    plain = teacher_episode_table(w.env, ids, K)
    assert set(t1) == set(plain) | {"tracking_rmse"}
    for k in plain:
        assert np.array_equal(t1[k], plain[k], equal_nan=True), k
    assert t1["tracking_rmse"].shape == (K,)
    assert np.array_equal(t1["tracking_rmse"], policy_tracking_table(sq, cnt, ids, K), equal_nan=True)
    assert np.isnan(t1["tracking_rmse"][K - 1]) and (t1["tracking_rmse"][:K - 1] > 0).all() and t1["episodes"].sum() >= 2 * n
    t2 = bank.closed_loop(*args, mode=mode, reference=refbank, reference_ids=rids)
    sq, cnt = w.env.tracking_error()
    assert np.array_equal(cnt, np.full(n, 20, np.uint32))
    assert t2["tracking_rmse"].shape == (K, M)
    assert np.array_equal(t2["tracking_rmse"], tracking.reference_tracking_table(sq, cnt, rids, M, ids, K), equal_nan=True)
    assert np.isnan(t2["tracking_rmse"][K - 1]).all() and np.isfinite(t2["tracking_rmse"][:K - 1]).all()
    for k in plain:
        assert np.array_equal(t2[k], teacher_episode_table(w.env, ids, K)[k], equal_nan=True), k
    assert "tracking_rmse" not in bank.closed_loop(*args, mode=mode)
