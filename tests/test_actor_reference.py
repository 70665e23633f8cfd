"""The float64 bound model of the student actor (tests/actor_reference.py) proved on the CPU: the C oracle and the NumPy
emulations of the three operand images lie inside their bounds on every weights x inputs pair, a reference built from
subtly wrong weights lies outside them (the bound is a test, not a formality), and the f16x2 packer refuses what it
cannot hold."""
import ctypes as C

import numpy as np
import pytest

import actor_reference as AR

N = 256
GRID = [(wf, xf) for wf in AR.WEIGHT_FAMILIES for xf in AR.INPUT_FAMILIES]


def _worst(got_act, got_hid, ref):
    act, hid, ba, bh = ref
    return float(max(AR.ratio(got_act, act, ba).max(), AR.ratio(got_hid, hid, bh).max()))


@pytest.mark.parametrize("wf", AR.WEIGHT_FAMILIES)
def test_the_oracle_lies_inside_the_oracle_bound(oracle, wf):
    w = AR.weights(wf)
    for xf in AR.INPUT_FAMILIES:
        x, h = AR.inputs(xf, N)
        hid = h.copy()
        act = oracle.actor_batch_step(w, x, hid)              # reads 22 of the row's columns; hid updated in place
        ref = AR.step_bound(w, x, h, "oracle")
        assert np.isfinite(ref[2]).all() and np.isfinite(ref[3]).all(), (wf, xf)
        worst = _worst(act, hid, ref)
        print(f"[actor bound] oracle {wf} {xf}: max err / bound {worst:.3f}")
        assert worst <= 1.0, (wf, xf, worst)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "f16x2"])
@pytest.mark.parametrize("wf", AR.WEIGHT_FAMILIES)
def test_the_emulations_lie_inside_their_bounds(precision, wf):
    w = AR.weights(wf)
    for xf in AR.INPUT_FAMILIES:
        x, h = AR.inputs(xf, N)
        act, hid = AR.emulate_step(w, x, h, precision)
        ref = AR.step_bound(w, x, h, precision)
        assert np.isfinite(ref[2]).all() and np.isfinite(ref[3]).all(), (wf, xf)
        worst = _worst(act, hid, ref)
        print(f"[actor bound] {precision} emulation {wf} {xf}: max err / bound {worst:.3f}")
        assert worst <= 1.0, (precision, wf, xf, worst)


def test_the_initial_hidden_state_is_the_default_state():
    w = AR.weights("fresh")
    x, _ = AR.inputs("normal", 8)
    h0 = np.tile(w[2000:2016], (8, 1))
    for a, b in zip(AR.step_bound(w, x, None, "fp32"), AR.step_bound(w, x, h0, "fp32")):
        assert np.array_equal(a, b)
    for a, b in zip(AR.emulate_step(w, x, None, "f16x2"), AR.emulate_step(w, x, h0, "f16x2")):
        assert np.array_equal(a, b)


def _outside(w, w_ref, precision, xf="normal", h_from_weights=False, **fault):
    """the emulation of ``w`` against the reference of ``w_ref``: the largest err / bound (the state of a swapped h0 shows
    only from the reset state, which both sides take from their own weights)"""
    x, h = AR.inputs(xf, N)
    if h_from_weights:
        h = None
    act, hid = AR.emulate_step(w, x, h, precision, **fault)
    return _worst(act, hid, AR.step_bound(w_ref, x, h, precision))


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
@pytest.mark.parametrize("kind", AR.ALTERATIONS)
def test_a_reference_of_altered_weights_lies_outside_the_bound(precision, kind):
    """The bound is not vacuous: one swapped pair in any of the nine blocks, exchanged n biases, exchanged r / z rows or a
    halved n pre-scale puts at least one element outside the fp32 and f16x2 bounds."""
    for wf in ("fresh", "perturbed"):
        w = AR.weights(wf)
        worst = _outside(w, AR.altered(w, kind), precision, h_from_weights=kind == "swap_h0")
        print(f"[actor bound] {precision} {wf} {kind}: max err / bound {worst:.3g}")
        assert worst > 1.0, (precision, wf, kind, worst)


@pytest.mark.parametrize("wf", ["fresh", "perturbed", "sat8"])
def test_the_f16x2_emulation_without_its_lo_hi_product_lies_outside(wf):
    """(not on ``tiny``: a weight of 2^-12 has a lo piece below 2^-23, under the 2^-25 floor the split itself is allowed per
    operand - the product is legitimately invisible there)"""
    w = AR.weights(wf)
    assert _outside(w, w, "f16x2") <= 1.0
    worst = _outside(w, w, "f16x2", drop_lo_hi=True)
    print(f"[actor bound] f16x2 {wf} without lo(W) hi(x): max err / bound {worst:.3g}")
    assert worst > 1.0, (wf, worst)


@pytest.mark.parametrize("wf", ["fresh", "sat8"])
@pytest.mark.parametrize("kind", AR.STRUCTURAL)
def test_the_bf16_bound_is_tight_enough_to_see_a_structural_fault(wf, kind):
    w = AR.weights(wf)
    worst = _outside(w, AR.altered(w, kind), "bf16")
    print(f"[actor bound] bf16 {wf} {kind}: max err / bound {worst:.3g}")
    assert worst > 1.0, (wf, kind, worst)


def test_the_moved_bf16_model_lies_inside_the_bf16_bound():
    """tests/test_gpu_actor.py's model of the bf16 kernel (un-scaled gates, fp32 matmuls) is one more implementation of
    the same operand roundings."""
    w = AR.weights("shipped")
    x, h = AR.inputs("normal", N)
    act, hid = AR._actor_bf16_model(w, x, h)
    assert _worst(act, hid, AR.step_bound(w, x, h, "bf16")) <= 1.0


# ------------------------------------------------------------------------------ the f16x2 packer's range ---
def _pack(w, precision):
    from raptor_amd import _lib
    need = C.c_size_t()
    _lib.call("rq_policy_pack_image", w.ctypes.data, w.size, precision, None, 0, C.byref(need))
    img = np.zeros(need.value, np.float32)
    _lib.call("rq_policy_pack_image", w.ctypes.data, w.size, precision, img.ctypes.data, img.size, C.byref(need))
    return img.reshape(-1, 64)


def _f16_pieces(img, base):
    """4 dwords x 64 lanes of the f16x2 image -> [lane, 8] float16 (element e = 2 * dword + half)"""
    d = img.view(np.uint32)[base:base + 4]
    lo16 = (d & 0xFFFF).astype(np.uint16).view(np.float16)
    hi16 = (d >> 16).astype(np.uint16).view(np.float16)
    return np.stack([lo16, hi16], axis=-1).transpose(1, 0, 2).reshape(64, 8)


# (block, index inside the block, weight index, the pre-scale its image carries)
_RANGE_CASES = [("W0", 5 * 22 + 3, 5 * 22 + 3, 1.0), ("b0", 7, 352 + 7, 1.0), ("Wi", 2 * 16 + 9, 368 + 2 * 16 + 9, float(-AR.K_SIG)),
                ("Wh", 20 * 16 + 1, 1136 + 20 * 16 + 1, float(-AR.K_SIG)), ("Wi", 40 * 16 + 4, 368 + 40 * 16 + 4, float(-AR.K_TANH)),
                ("Wh", 33 * 16 + 15, 1136 + 33 * 16 + 15, float(-AR.K_TANH)), ("W2", 2 * 16 + 6, 2016 + 2 * 16 + 6, 1.0)]


@pytest.mark.parametrize("block,_i,index,k", _RANGE_CASES)
def test_f16x2_weights_out_of_range_are_refused_by_the_packer(block, _i, index, k):
    """hi = f16(v), lo = f16(v - hi): a pre-scaled weight of magnitude >= 65 520 splits into hi = inf and lo = -inf, a NaN on
    the matrix pipe (what ``split_f16`` shows; before this refusal the image held exactly those two infinities).  The
    packer now returns an error that names the weight; the largest weight that still rounds to 65 504 is packed, finite,
    and reconstructs; the fp32 and bf16 images take either."""
    from raptor_amd import _lib
    hi, lo = AR.split_f16(np.array([65520.0, -7.0e4], np.float32))
    assert np.isinf(hi).all() and np.isinf(lo).all() and (np.sign(hi) == -np.sign(lo)).all()
    w = AR.weights("fresh")
    for sign in (1.0, -1.0):
        bad = w.copy()
        bad[index] = np.float32(sign * 65520.0 / k * (1 + 2.0 ** -20))
        assert abs(float(np.float32(k) * bad[index])) >= 65520.0
        with pytest.raises(_lib.RaptorQuadError, match=rf"weight {index} ") as e:
            _pack(bad, _lib.POLICY_F16X2_MFMA)
        assert e.value.status == -1
        assert np.isfinite(_pack(bad, _lib.POLICY_FP32)).all()
        _pack(bad, _lib.POLICY_BF16_MFMA)
        ok = w.copy()
        ok[index] = np.float32(sign * 65519.0 / k * (1 - 2.0 ** -20))
        img = _pack(ok, _lib.POLICY_F16X2_MFMA)
        pieces = np.concatenate([_f16_pieces(img, base) for base in range(0, 72, 4)]).astype(np.float64)
        assert np.isfinite(pieces).all() and np.abs(pieces).max() == 65504.0
    # a non-finite weight is the caller's (every precision carries it as it is), not a range error
    nan = w.copy()
    nan[index] = np.nan
    _pack(nan, _lib.POLICY_F16X2_MFMA)
