"""raptor_amd.training.BankDistiller without a GPU: the refusals Python makes itself - before the library is touched, so a stub bank
and a stub trajectory do - and the header's declarations of the calls it binds."""
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT

N, P = 300, 3                                   # five blocks, the last ragged


class _Untouchable:
    """stands where a library handle would: any use of it is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached for ({name}) before the arguments were checked")


def _stubs(n=N, p=P):
    bank = types.SimpleNamespace(n_policies=p, _h=_Untouchable())
    env = types.SimpleNamespace(N_ENVIRONMENTS=n, _device=_Untouchable())

    class Traj:
        _env = env

        def __len__(self):
            raise AssertionError("the trajectory was asked for its length before the arguments were checked")

        def _require(self, what):
            raise AssertionError("the trajectory's handle was taken before the arguments were checked")

    return bank, Traj()


def _ids(block_ids=(2, 0, 2, 1, 0), n=N):
    return np.repeat(np.asarray(block_ids, np.uint32), 64)[:n]


@pytest.mark.parametrize("kw", [dict(lr=[1e-3, 2e-3]), dict(lr=np.ones(4)), dict(betas=([0.9, 0.8], 0.999)), dict(betas=(0.9, np.ones(5))),
                                dict(eps=[1e-8] * 2), dict(weight_decay=np.zeros(7)), dict(lr=np.ones((3, 1))), dict(lr=[])])
def test_a_hyper_parameter_is_a_scalar_or_one_value_per_policy(kw):
    from raptor_amd.training import BankDistiller
    bank, _ = _stubs()
    with pytest.raises(ValueError, match="scalar or hold one value per policy"):
        BankDistiller(bank, **kw)


def test_scalars_and_sequences_become_one_config_per_policy():
    from raptor_amd.training import BankDistiller
    bank, _ = _stubs()
    d = BankDistiller(bank, lr=[2e-3, 0.0, 5e-4], betas=(0.8, [0.99, 0.999, 0.9]), eps=[1e-7], weight_decay=0.01)
    assert [c.lr for c in d._cfg] == [2e-3, 0.0, 5e-4]
    assert [c.beta1 for c in d._cfg] == [0.8] * 3 and [c.beta2 for c in d._cfg] == [0.99, 0.999, 0.9]
    assert [c.eps for c in d._cfg] == [1e-7] * 3 and [c.weight_decay for c in d._cfg] == [0.01] * 3
    d.set_lr(0.5)                               # no optimizer yet: remembered for its creation, nothing called
    assert [c.lr for c in d._cfg] == [0.5] * 3
    d.set_lr([1.0, 2.0, 3.0])
    assert [c.lr for c in d._cfg] == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="one value per policy"):
        d.set_lr([1.0, 2.0])


def test_step_and_loss_and_grad_refuse_before_the_library_is_touched():
    from raptor_amd.training import BankDistiller
    bank, traj = _stubs()
    d = BankDistiller(bank)
    good = _ids()
    with pytest.raises(ValueError, match="updates must be at least 1"):
        d.step(traj, good, updates=0)
    with pytest.raises(ValueError, match="updates must be at least 1"):
        d.step(traj, good, updates=-3)
    for call in (d.step, d.loss_and_grad):
        with pytest.raises(ValueError, match='"initial" or "current"'):
            call(traj, good, start="middle")
        split = good.copy()
        split[100] = 1
        with pytest.raises(ValueError, match="differ inside a 64-env block"):
            call(traj, split)
        too_big = good.copy()
        too_big[64:128] = P
        with pytest.raises(ValueError, match="out of range"):
            call(traj, too_big)
        with pytest.raises(ValueError, match="out of range"):
            call(traj, good.astype(np.int64) - 1)
        with pytest.raises(ValueError, match="one id per env"):
            call(traj, good[:-1])
        with pytest.raises(ValueError, match="one id per env"):
            call(traj, np.concatenate([good, good[-1:]]))
        with pytest.raises(ValueError, match="integers"):
            call(traj, good + 0.5)
    assert d._h is None                         # no optimizer was created on the way


def test_the_optimizer_state_calls_refuse_before_the_library_is_touched():
    from raptor_amd.training import BankDistiller, Distiller
    bank, _ = _stubs()
    d, b = Distiller(_Untouchable()), BankDistiller(bank)
    m, powers = np.zeros(2084, np.float32), np.ones(2)
    for bad in (dict(m=m[:-1], v=m, step=0, beta_powers=powers), dict(m=m.astype(np.float64), v=m, step=0, beta_powers=powers),
                dict(m=m, v=m, step=0, beta_powers=np.ones(3))):
        with pytest.raises(ValueError, match="float32|beta_powers"):
            d.set_state(**bad)
    with pytest.raises(ValueError, match="2084 values"):
        d.apply(m[:-1])
    M, steps, pw = np.zeros((P, 2084), np.float32), np.zeros(P, np.uint32), np.ones((P, 2))
    for bad in (dict(m=M[:2], v=M, step=steps, beta_powers=pw), dict(m=M, v=M, step=steps[:2], beta_powers=pw),
                dict(m=M, v=M, step=steps, beta_powers=pw[:, :1])):
        with pytest.raises(ValueError, match="float32|beta_powers|one count per policy"):
            b.set_state(**bad)
    assert d._h is None and b._h is None        # no optimizer was created on the way


def test_the_header_declares_every_bank_learner_call_bound():
    from raptor_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "raptor_quad.h")).read()
    new = ["rq_policy_bank_get_weights", "rq_trajectory_policies_loss_grad", "rq_bank_optimizer_create", "rq_bank_optimizer_destroy",
           "rq_bank_optimizer_set_lr", "rq_trajectory_policies_distill",
           "rq_optimizer_get_state", "rq_optimizer_set_state", "rq_optimizer_apply", "rq_bank_optimizer_get_state",
           "rq_bank_optimizer_set_state"]
    for name in new:
        assert name in _lib._SIGNATURES, name
        m = re.search(r"RQ_API int %s\(([^;]*)\);" % name, hdr, re.S)
        assert m, f"{name} is bound by raptor_amd/_lib.py but not declared in include/raptor_quad.h"
        assert len(m.group(1).split(",")) == len(_lib._SIGNATURES[name]), name
    src = open(os.path.join(ROOT, "raptor_amd", "training.py")).read() + open(os.path.join(ROOT, "raptor_amd", "policy_bank.py")).read()
    for name in set(re.findall(r'_lib\.call\("(rq_\w+)"', src)):
        assert re.search(r"RQ_API int %s\(" % name, hdr), name
