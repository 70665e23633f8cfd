"""Float64 restatements for the distillation update (rq_trajectory_policy_loss_grad / rq_trajectory_distill, csrc/rq_grad.hpp):
the masked mean squared error and its seed dL/da, Adam as torch.optim.Adam states it (weight decay decoupled, as AdamW), the bounds
the GPU tests hold the fp32 kernels to, and a gather table applied in NumPy."""
import numpy as np

U = 2.0 ** -24


def masked_mse(act, target, live):
    """act, target [...] float64-able, live bool of the same shape -> (loss, dL/dact, terms): the mean over the live entries of
    (act - target)^2; what is not live is selected away before any arithmetic, so NaN there goes nowhere."""
    a = np.where(live, np.asarray(act, np.float64), 0.0)
    y = np.where(live, np.asarray(target, np.float64), 0.0)
    M = int(live.sum())
    terms = (a - y) ** 2
    if M == 0:
        return 0.0, np.zeros_like(a), terms
    return terms.sum() / M, 2.0 * (a - y) / M, terms


def loss_bound(terms, M):
    """|fp32 loss - float64 loss| <= (N + 4) u sum|terms| / M, N = the live terms.  First order, as policy_grad_reference.bound:
    a term is fl(fl(a - y)^2) - the subtract's rounding counts twice under the square, the square's once - the fp32 sum adds at
    most N - 1 roundings on any path whatever its order (adding an exact 0 rounds nothing), and the division rounds once."""
    return (M + 4) * U * np.abs(terms).sum() / max(M, 1) + 2.0 ** -120


class Adam:
    """torch.optim.Adam (amsgrad off, maximize off) on one float64 vector; weight_decay is decoupled (torch.optim.AdamW)."""

    def __init__(self, w, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.w = np.array(w, np.float64)
        self.m = np.zeros_like(self.w)
        self.v = np.zeros_like(self.w)
        self.t = 0
        self.lr, self.b1, self.b2, self.eps, self.wd = lr, betas[0], betas[1], eps, weight_decay

    def step(self, g):
        g = np.asarray(g, np.float64)
        self.t += 1
        self.m = self.b1 * self.m + (1.0 - self.b1) * g
        self.v = self.b2 * self.v + (1.0 - self.b2) * g * g
        mhat = self.m / (1.0 - self.b1 ** self.t)
        vhat = self.v / (1.0 - self.b2 ** self.t)
        self.w = self.w * (1.0 - self.lr * self.wd) - self.lr * mhat / (np.sqrt(vhat) + self.eps)
        return self.w


def apply_gather(table, w):
    """table: structured array (a, b: uint16, k: float32), w [2084] float32 -> the image, in fp32 as the device forms it:
    0 (a == 0xFFFF), k * w[a], or k * (w[a] + w[b]) - a multiply of a sum, each operation rounded once."""
    w = np.asarray(w, np.float32)
    a, b, k = table["a"].astype(np.int64), table["b"].astype(np.int64), table["k"].astype(np.float32)
    none = 0xFFFF
    x = w[np.where(a == none, 0, a)]
    x = np.where(b == none, x, (x + w[np.where(b == none, 0, b)]).astype(np.float32)).astype(np.float32)
    return np.where(a == none, np.float32(0.0), (k * x).astype(np.float32)).astype(np.float32)
