"""tests/rollout_common.py by itself, on small hand-made dicts: six GPU suites see through its comparisons, so what they let pass and
what they refuse is pinned here.  NumPy only, no GPU."""
import numpy as np
import pytest

from rollout_common import assert_same, assert_same_recording, bank_weights, ids_of, join


def _snap():
    return dict(state=np.arange(12, dtype=np.float32).reshape(4, 3), steps=np.arange(4, dtype=np.uint32))


def _nan(payload):
    return np.array([0x7FC00000 | payload], np.uint32).view(np.float32)[0]


def test_assert_same_passes_on_equal_bits_and_names_what_and_key():
    a, b = _snap(), _snap()
    a["state"][1, 1] = b["state"][1, 1] = np.nan
    assert_same(a, b, what="equal")
    b["steps"][2] += 1
    with pytest.raises(AssertionError, match="the flight: steps"):
        assert_same(a, b, what="the flight")


def test_assert_same_tells_the_zeros_apart():
    a, b = _snap(), _snap()
    a["state"][0, 0], b["state"][0, 0] = 0.0, -0.0
    assert np.array_equal(a["state"], b["state"])               # a comparison by value would let it pass
    with pytest.raises(AssertionError, match="state"):
        assert_same(a, b)


def test_assert_same_tells_nan_payloads_apart():
    a, b = _snap(), _snap()
    a["state"][2, 1], b["state"][2, 1] = _nan(1), _nan(2)
    assert np.array_equal(a["state"], b["state"], equal_nan=True)
    with pytest.raises(AssertionError, match="state"):
        assert_same(a, b)


def test_assert_same_wants_the_same_keys():
    a, b = _snap(), _snap()
    del b["steps"]
    for x, y in ((a, b), (b, a)):
        with pytest.raises(AssertionError, match="keys"):
            assert_same(x, y)
    with pytest.raises(AssertionError, match="keys"):
        assert_same(a, b, skip=("steps",))                      # a skipped key is still a key both must hold


def test_assert_same_wants_the_same_shapes():
    a, b = _snap(), _snap()
    b["state"] = b["state"].reshape(3, 4)                       # the same bytes
    with pytest.raises(AssertionError, match="state"):
        assert_same(a, b)
    b["state"] = a["state"][:3]
    with pytest.raises(AssertionError, match="state"):
        assert_same(a, b, rows=slice(0, 3))                     # equal on the rows, but not the same shape
    b["state"] = a["state"].view(np.int32)                      # the same bits under another type
    with pytest.raises(AssertionError, match="state"):
        assert_same(a, b)


def test_assert_same_rows_and_skip():
    a, b = _snap(), _snap()
    b["state"][3, 0] += 1
    rows = np.array([True, True, True, False])
    assert_same(a, b, rows=rows)                                # the only difference lies outside the rows
    assert_same(a, b, rows=slice(0, 3))
    assert_same(a, b, skip=("state",))                          # ... or under a skipped key
    for r in (slice(None), np.array([False, False, False, True]), slice(2, 4)):
        with pytest.raises(AssertionError, match="state"):
            assert_same(a, b, rows=r)
    with pytest.raises(AssertionError, match="state"):
        assert_same(a, b, skip=("steps",))


def _recording(T=3, n=4):
    g = np.random.default_rng(0)
    rec = dict(obs=g.standard_normal((T, n, 22)).astype(np.float32), act=g.standard_normal((T, n, 4)).astype(np.float32),
               rew=g.standard_normal((T, n)).astype(np.float32), done=np.zeros((T, n), np.uint8))
    rec["done"][1, 2] = 2
    rec["done"][2, 1] = 4
    return rec


def _copy(rec):
    return {k: v.copy() for k, v in rec.items()}


@pytest.mark.parametrize("key", ["obs", "act", "rew"])
def test_recording_ignores_frozen_entries_unless_told_not_to(key):
    a = _recording()
    b = _copy(a)
    assert_same_recording(a, b, "equal")
    assert_same_recording(a, b, "equal", frozen_too=True)
    b[key][2, 1] = -b[key][2, 1]                                # where done == 4
    assert_same_recording(a, b, "frozen entry")
    with pytest.raises(AssertionError, match=f"every entry: {key}"):
        assert_same_recording(a, b, "every entry", frozen_too=True)
    c = _copy(a)
    c[key][1, 2] = -c[key][1, 2]                                # where a transition was taken
    for frozen_too in (False, True):
        with pytest.raises(AssertionError, match=key):
            assert_same_recording(a, c, frozen_too=frozen_too)


def test_recording_is_compared_on_the_bits():
    a = _recording()
    a["rew"][0, 0] = 0.0
    b = _copy(a)
    b["rew"][0, 0] = -0.0
    with pytest.raises(AssertionError, match="rew"):
        assert_same_recording(a, b)


@pytest.mark.parametrize("frozen_too", [False, True])
def test_recording_never_ignores_a_done_code(frozen_too):
    a = _recording()
    for at, code in (((0, 0), 1), ((2, 1), 0), ((1, 2), 4), ((0, 3), 4)):      # a live entry, the frozen one thawed, live ones frozen
        b = _copy(a)
        b["done"][at] = code
        for x, y in ((a, b), (b, a)):
            with pytest.raises(AssertionError, match="done codes"):
                assert_same_recording(x, y, frozen_too=frozen_too)


def test_join_concatenates_snapshots_by_env_and_recordings_by_column():
    def piece(n, base):
        snap = dict(state=np.full((n, 3), base, np.float32), epoch=np.full(n, 7, np.uint32))
        rec = dict(obs=np.full((2, n, 22), base, np.float32), done=np.full((2, n), base, np.uint8))
        return snap, rec

    snap, rec = join([piece(3, 1), piece(2, 5)])
    assert snap.keys() == {"state", "epoch"} and rec.keys() == {"obs", "done"}
    assert snap["state"].shape == (5, 3) and snap["state"][:, 0].tolist() == [1, 1, 1, 5, 5]
    assert snap["epoch"].tolist() == [7] * 5                    # epoch is one entry per env like everything else
    assert rec["obs"].shape == (2, 5, 22) and rec["obs"][1, :, 0].tolist() == [1, 1, 1, 5, 5]
    assert rec["done"].shape == (2, 5) and rec["done"][0].tolist() == [1, 1, 1, 5, 5]
    snap, rec = join([(piece(3, 1)[0], None), (piece(2, 5)[0], None)])
    assert rec is None and snap["state"].shape == (5, 3)


def test_ids_of_and_bank_weights_are_what_they_were():
    """the values written out from the definitions the suites held before they shared these"""
    ids = ids_of([2, 0, 2, 1], 200)
    assert ids.dtype == np.uint32 and ids.shape == (200,) and ids.flags.c_contiguous
    assert ids[[0, 63, 64, 127, 128, 191, 192, 199]].tolist() == [2, 2, 0, 0, 2, 2, 1, 1]
    assert np.array_equal(ids, np.array([2] * 64 + [0] * 64 + [2] * 64 + [1] * 8, np.uint32))
    w = np.arange(2084, dtype=np.float32) / np.float32(2084) - np.float32(0.5)
    W = bank_weights(w, 3)
    assert W.shape == (3, 2084) and W.dtype == np.float32
    want = [[0xBF0ED10F, 0x3D0EDA03, 0x3EE070AB], [0xBF0A1D2C, 0x3C401A6C, 0x3F0DB524], [0xBEEFFB38, 0x3D566B12, 0x3EFF28BE]]
    assert W[:, [0, 1000, 2083]].view(np.uint32).tolist() == want
    # policy k is one draw of default_rng(100 + k), whatever the bank's size
    assert np.array_equal(bank_weights(w, 1)[0].view(np.uint32), W[0].view(np.uint32))
