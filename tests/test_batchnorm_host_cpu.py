"""`adaptpoint_amd.batchnorm.mode` / `args` on CPU modules: which kernel arguments a BatchNorm module turns into.

The table below is written out from the two spellings the fused layers carried before the module existed -- the
set-abstraction one (`_sa_rule`) and the per-point one (`_pw_rule`), restated here -- and the test also shows that the two
agree on every case: they differed in how they asked (`track_running_stats` alone or with `running_mean is not None`;
`num_batches_tracked` gated on `bn.training` or on `training and nbt is not None`), not in what they answered.
Needs neither a GPU nor the library.
"""
import pytest
import torch
from torch import nn

from adaptpoint_amd import batchnorm, pointwise

FIELDS = ("gamma", "beta", "running_mean", "running_var", "num_batches_tracked")


def _sa_rule(bn):
    """The set-abstraction layers' spelling -> (training, fields that are None)."""
    training = bn.training or not bn.track_running_stats
    track = bn.track_running_stats
    present = dict(gamma=bn.weight is not None, beta=bn.bias is not None,
                   running_mean=track and bn.running_mean is not None, running_var=track and bn.running_var is not None,
                   num_batches_tracked=bool(track and bn.training) and bn.num_batches_tracked is not None)
    return training, {k for k in FIELDS if not present[k]}


def _pw_rule(bn, gamma, beta):
    """The per-point layers' spelling (gamma, beta: what the autograd node received) -> (training, None fields)."""
    training = bn.training or not bn.track_running_stats
    track = bn.track_running_stats and bn.running_mean is not None
    present = dict(gamma=gamma is not None, beta=beta is not None, running_mean=track, running_var=track,
                   num_batches_tracked=bool(track and training and bn.num_batches_tracked is not None))
    return training, {k for k in FIELDS if not present[k]}


def _bn(train, **kw):
    return nn.BatchNorm1d(4, **kw).train(train)


# name: (module, (training, track), fields that are None)
CASES = {
    "train": (_bn(True), (True, True), set()),
    "eval": (_bn(False), (False, True), {"num_batches_tracked"}),
    "no-stats-train": (_bn(True, track_running_stats=False), (True, False),
                       {"running_mean", "running_var", "num_batches_tracked"}),
    "no-stats-eval": (_bn(False, track_running_stats=False), (True, False),
                      {"running_mean", "running_var", "num_batches_tracked"}),
    "no-affine-train": (_bn(True, affine=False), (True, True), {"gamma", "beta"}),
    "no-affine-eval": (_bn(False, affine=False), (False, True), {"gamma", "beta", "num_batches_tracked"}),
}


@pytest.mark.parametrize("name", CASES)
def test_mode_and_args_of_a_module(name):
    bn, (training, track), none = CASES[name]
    assert batchnorm.mode(bn) == (training, track)
    a = batchnorm.args(bn)
    assert {k for k in FIELDS if getattr(a, k) is None} == none
    assert (a.eps, a.momentum, a.training) == (1e-5, 0.1, int(training))
    assert all(type(v) is t for v, t in zip(a[5:], (float, float, int)))
    tensors = dict(gamma=bn.weight, beta=bn.bias, running_mean=bn.running_mean, running_var=bn.running_var,
                   num_batches_tracked=bn.num_batches_tracked)
    assert all(getattr(a, k) == tensors[k].data_ptr() for k in FIELDS if k not in none)
    assert a == tuple(a) and a._fields == FIELDS + ("eps", "momentum", "training")       # (it splats in this order)
    # both earlier spellings say the same
    assert _sa_rule(bn) == (training, none) and _pw_rule(bn, bn.weight, bn.bias) == (training, none)


@pytest.mark.parametrize("train", [True, False])
def test_momentum_none_is_refused_unless_the_caller_names_a_stand_in(train):
    bn = _bn(train, momentum=None)
    assert batchnorm.mode(bn) == (train, True)
    with pytest.raises(RuntimeError, match="momentum=None"):
        batchnorm.args(bn)
    a = batchnorm.args(bn, no_momentum=0.0)                  # the per-point layers' eval-mode rule
    assert a.momentum == 0.0 and a.training == int(train)
    assert (a.num_batches_tracked is None) == (not train)
    assert batchnorm.args(_bn(train), no_momentum=0.0).momentum == 0.1      # a numeric momentum is never replaced


def test_no_norm_is_an_eval_mode_identity_with_buffers_only():
    bn = pointwise._NoNorm(4, torch.device("cpu"))
    assert batchnorm.mode(bn) == (False, True)
    a = batchnorm.args(bn, no_momentum=0.0)
    assert {k for k in FIELDS if getattr(a, k) is None} == {"gamma", "beta", "num_batches_tracked"}
    assert (a.running_mean, a.running_var) == (bn.running_mean.data_ptr(), bn.running_var.data_ptr())
    assert (a.eps, a.momentum, a.training) == (0.0, 0.0, 0)
    bias = torch.zeros(4)                                     # (conv_bias_act hands the convolution's bias in as beta)
    assert _pw_rule(bn, None, bias) == (False, {"gamma", "num_batches_tracked"})
    assert _pw_rule(bn, None, None) == (False, {"gamma", "beta", "num_batches_tracked"})


def test_ptr_tolerates_none():
    t = torch.zeros(3)
    assert batchnorm.ptr(None) is None and batchnorm.ptr(t) == t.data_ptr()
    from adaptpoint_amd import fused
    assert fused._ptr is batchnorm.ptr
