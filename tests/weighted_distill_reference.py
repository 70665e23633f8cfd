"""Float64 restatement of the weighted distillation loss (rq_trajectory_policy_loss_grad_weighted and its siblings,
csrc/rq_grad_backward.inc under RQ_GRAD_WEIGHTED, the *_reduce_weighted kernels of csrc/rq_grad.hpp / rq_grad_bank.hpp) and the bound
the GPU tests hold the fp32 loss to.  The gradient's bound is policy_grad_reference.bound with the seed's roundings added
(tests/test_gpu_weighted_distill.py, C_SEED_W)."""
import numpy as np

U = 2.0 ** -24


def counting(live, weight):
    """live bool [...], weight broadcastable against it -> (counts bool [...], w float64 [...] with 0 where the entry does not
    count).  An entry counts when it is live and its weight is > 0: a weight that is 0, negative or NaN drops it."""
    w = np.broadcast_to(np.asarray(weight, np.float64), live.shape)
    with np.errstate(invalid="ignore"):
        counts = live & (w > 0)
    return counts, np.where(counts, w, 0.0)


def weighted_mse(act, target, live, weight):
    """act, target [...] float64-able, live bool of the same shape, weight broadcastable against them -> (loss, dL/dact, terms, W4):
    sum over the counting entries of w (act - target)^2, divided by W4 = the sum of their w.  What does not count is selected away
    before any arithmetic - act, target and weight alike - so NaN there goes nowhere.  W4 = 0: loss 0, a zero gradient."""
    counts, w = counting(live, weight)
    a = np.where(counts, np.asarray(act, np.float64), 0.0)
    y = np.where(counts, np.asarray(target, np.float64), 0.0)
    e = a - y
    terms = w * e * e
    W4 = w.sum()
    if W4 == 0:
        return 0.0, np.zeros_like(a), terms, 0.0
    return terms.sum() / W4, 2.0 * w * e / W4, terms, W4


def loss_bound(terms, W4, n_counting):
    """|fp32 loss - float64 loss| <= (N + 4 + (N + 1) 2^-28) u sum|terms| / W4, N = the counting terms.  First order, counted from the
    kernels as distill_reference.loss_bound counts the unweighted ones:
      * a term is fl(fl(w fl(a - y)) fl(a - y)) (rq_grad_backward.inc: err = a - y, daB = wt * err, sse += daB * err): the subtract's
        rounding enters twice, the product w e once, the product with e once - 4 roundings, one more than the unweighted term's 3;
      * the fp32 sum - lane, then the wave's 64 lanes, then the waves in order - adds at most N - 1 roundings on any path whatever
        its order (adding an exact 0, a dropped entry's, rounds nothing);
      * the normaliser: W4 is a float64 sum of N positive weights, at most N - 1 roundings of 2^-53 relative each, 1 / W4 and the
        product sse x (1 / W4) one each: (N + 1) 2^-53 = (N + 1) 2^-29 u; this restatement's own float64 sums (of the terms and of
        W4) are allowed as much again, hence 2^-28;
      * the product is rounded to fp32 once.
    (N - 1) + 4 + 1 = N + 4 roundings of u, plus the float64 fraction."""
    n = int(n_counting)
    return (n + 4 + (n + 1) * 2.0 ** -28) * U * np.abs(terms).sum() / (W4 if W4 > 0 else 1.0) + 2.0 ** -120
