"""The float64 teacher reference and its error bound (tests/teacher_reference.py), on the CPU: the bound holds for the C
oracle and for NumPy emulations of the bf16 and split-f16 kernels, and it rejects each of a set of injected faults on the
same data - so that the GPU tests that lean on it (test_gpu_teacher_edges.py) can fail."""
import numpy as np
import pytest

import teacher_reference as R

ACT = R.ACT_CODE


def _teacher(rng, in_dim, widths, scale=1.0):
    dims = [in_dim] + list(widths) + [4]
    parts = []
    for i in range(len(dims) - 1):
        parts.append(rng.standard_normal(dims[i + 1] * dims[i]) / np.sqrt(dims[i]))
        parts.append(rng.standard_normal(dims[i + 1]) * 0.1)
    return (np.concatenate(parts) * scale).astype(np.float32)


def _inputs(rng, n, in_dim, scale=1.0):
    return (rng.standard_normal((n, in_dim)) * scale).astype(np.float32)


def _oracle(oracle, block, in_dim, widths, act, out_act, x):
    """the C oracle on one teacher: x [N, in_dim] -> [N, 4]"""
    obs = np.zeros((1, x.shape[0], 22), np.float32)
    obs[0, :, :in_dim] = x
    ids = np.zeros(x.shape[0], np.uint32)
    if len(widths) == 2 and all(h in (16, 32, 64) for h in widths):
        return oracle.teacher_relabel(block[None], in_dim, widths[0], widths[1], ACT[act], ACT[out_act], obs, ids)[0]
    return oracle.mlp_relabel(block[None], in_dim, widths, ACT[act], ACT[out_act], obs, ids)[0]


CASES = [(22, [64, 64], "relu", "identity"), (22, [64, 64], "tanh", "tanh"), (5, [16, 32], "relu", "tanh"),
         (13, [32, 16], "tanh", "identity"), (22, [128, 48, 112], "tanh", "tanh"), (9, [96], "relu", "identity")]


@pytest.mark.parametrize("in_dim,widths,act,out_act", CASES)
@pytest.mark.parametrize("scale", [2.0 ** -10, 1.0, 2.0 ** 10])
def test_bound_holds_for_the_oracle(oracle, in_dim, widths, act, out_act, scale):
    rng = np.random.default_rng(in_dim * 31 + sum(widths))
    block = _teacher(rng, in_dim, widths)
    x = _inputs(rng, 4000, in_dim, scale)
    ref, e = R.forward_bound(R.unpack(block, in_dim, widths), act, out_act, x, "oracle")
    R.assert_within(_oracle(oracle, block, in_dim, widths, act, out_act, x), ref, e, f"oracle {in_dim}-{widths} x{scale:g}")


@pytest.mark.parametrize("in_dim,widths,act,out_act", [c for c in CASES if len(c[1]) == 2])
@pytest.mark.parametrize("precision", ["bf16", "f16x2"])
@pytest.mark.parametrize("scale", [2.0 ** -10, 1.0, 2.0 ** 10])
def test_bound_holds_for_emulated_16_bit_kernels(in_dim, widths, act, out_act, precision, scale):
    """Operands handled exactly as the packer and the kernel do (pre-scale, layer 1's bias slot, RNE roundings, the
    f16 split with its subnormal lo pieces at 2^-10); inputs and weights both scaled."""
    rng = np.random.default_rng(in_dim * 17 + sum(widths))
    block = _teacher(rng, in_dim, widths, scale=scale if scale < 1 else 1.0)
    x = _inputs(rng, 4000, in_dim, scale)
    layers = R.unpack(block, in_dim, widths)
    ref, e = R.forward_bound(layers, act, out_act, x, precision)
    got = R.emulate(layers, act, out_act, x, precision)
    R.assert_within(got, ref, e, f"{precision} emulation {in_dim}-{widths} {act}/{out_act} x{scale:g}")


# ---------------------------------------------------------------------------- faults ---
# One relu teacher on O(1) data; every fault must put at least one label outside twice the bound.
IN, WIDTHS = 5, [16, 16]


@pytest.fixture(scope="module")
def fault_case():
    rng = np.random.default_rng(2024)
    block = _teacher(rng, IN, WIDTHS)
    x = _inputs(rng, 2000, IN)
    return block, x


def _rejected(got, ref, e):
    return not R.within(got, ref, e).all()


def test_the_unfaulted_case_passes(oracle, fault_case):
    block, x = fault_case
    layers = R.unpack(block, IN, WIDTHS)
    for prec, got in (("oracle", _oracle(oracle, block, IN, WIDTHS, "relu", "identity", x)),
                      ("f16x2", R.emulate(layers, "relu", "identity", x, "f16x2")),
                      ("bf16", R.emulate(layers, "relu", "identity", x, "bf16"))):
        ref, e = R.forward_bound(layers, "relu", "identity", x, prec)
        R.assert_within(got, ref, e, f"unfaulted {prec}")


def test_rejects_f16x2_without_a_cross_product(fault_case):
    block, x = fault_case
    layers = R.unpack(block, IN, WIDTHS)
    ref, e = R.forward_bound(layers, "relu", "identity", x, "f16x2")
    assert _rejected(R.emulate(layers, "relu", "identity", x, "f16x2", drop_hi_lo=True), ref, e)


def _faulted_data(block, x, fault):
    """a correct evaluation of wrong data is the same as a faulty evaluation of the right data"""
    b, xx = block.copy(), x.copy()
    layers = R.unpack(b, IN, WIDTHS)
    if fault == "bias1 dropped":
        b[IN * WIDTHS[0]:IN * WIDTHS[0] + WIDTHS[0]] = 0.0
    elif fault == "last feature ignored":
        xx[:, IN - 1] = 0.0
    elif fault == "one W2 weight +1e-3":
        # the W2 weight on the largest path to an output: |W3[o, i]| |W2[i, k]| mean |h1_k|
        h1 = np.maximum(x.astype(np.float64) @ layers[0][0].T.astype(np.float64) + layers[0][1], 0.0)
        path = np.abs(layers[2][0]).max(axis=0)[:, None] * np.abs(layers[1][0]) * np.abs(h1).mean(axis=0)[None, :]
        i, k = np.unravel_index(np.argmax(path), path.shape)
        off = IN * WIDTHS[0] + WIDTHS[0] + i * WIDTHS[0] + k
        b[off] = np.float32(b[off] * (1 + 1e-3))
    return b, xx


@pytest.mark.parametrize("fault", ["bias1 dropped", "last feature ignored", "one W2 weight +1e-3"])
@pytest.mark.parametrize("precision", ["oracle", "f16x2"])
def test_rejects_wrong_data(oracle, fault_case, fault, precision):
    block, x = fault_case
    ref, e = R.forward_bound(R.unpack(block, IN, WIDTHS), "relu", "identity", x, precision)
    fb, fx = _faulted_data(block, x, fault)
    if precision == "oracle":
        got = _oracle(oracle, fb, IN, WIDTHS, "relu", "identity", fx)
    else:
        got = R.emulate(R.unpack(fb, IN, WIDTHS), "relu", "identity", fx, "f16x2")
    assert _rejected(got, ref, e), fault


def test_rejects_the_unsaturated_split(fault_case):
    """An input of 7e4 splits into hi = inf, lo = -inf: hi w + lo w is NaN - rejected; the saturating split stays finite."""
    block, x = fault_case
    layers = R.unpack(block, IN, WIDTHS)
    x = x.copy()
    x[7, 2] = 7e4
    ref, e = R.forward_bound(layers, "relu", "identity", x, "f16x2")
    bad = R.emulate(layers, "relu", "identity", x, "f16x2", saturate=False)
    assert np.isnan(bad[7]).any() and _rejected(bad, ref, e)
    good = R.emulate(layers, "relu", "identity", x, "f16x2")
    assert np.isfinite(good).all()
    rows = np.arange(len(x)) != 7
    R.assert_within(good[rows], ref[rows], e[rows], "saturating split, other rows")
    assert np.isinf(e[7]).all()                     # an operand past 65 504 leaves the model: no claim on that row


def test_split_matches_the_packers_rounding():
    """the emulation's f16 split is the packer's: hi + lo within 2^-22 |v| + 2^-25 of v, exact residual, inf at 65 520"""
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.standard_normal(10000) * s for s in (1e-6, 1e-3, 1.0, 1e3)]).astype(np.float32)
    hi, lo = R.split_f16(v)
    assert (np.abs(v - hi - lo) <= 2.0 ** -22 * np.abs(v) + 2.0 ** -25).all()
    hi, lo = R.split_f16(np.array([65519.0, 65520.0], np.float32))
    assert hi[0] == 65504.0 and np.isinf(hi[1])
    assert R.to_bf16(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)).tolist() == [1.0, 1.0 + 2.0 ** -6]
