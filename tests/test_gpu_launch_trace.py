"""The launch sequence of every fused layer that carries a BatchNorm, as a literal: which C entries a forward + backward
pass calls, in which order, and which of their optional buffers are absent (None).

Every launch of the package goes through `fused._call` (or a module's own import of it); the test wraps them all, as
scripts/profile_gan_calls.py does, and records (entry, positions of the arguments after the device that are None).  The
lists below are the contract of the host code between a `torch.nn.BatchNorm*` module and the kernels: a change there
that adds, drops or reorders a launch, or hands a kernel a different set of optional buffers, fails here -- at the
smallest shapes the route predicates accept, in training and in eval mode.  The BatchNorm buffers are checked with it:
a training-mode pass bumps num_batches_tracked once and moves the running statistics, an eval-mode pass leaves all three
bit-equal.  (The residual EdgeConv case has C = H = 64: the residual is the block's input, so the widths must match.)
"""
import contextlib
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

T, E = "train", "eval"


@contextlib.contextmanager
def recording():
    import adaptpoint_amd   # noqa: F401
    from adaptpoint_amd import fused
    orig, trace = fused._call, []

    def rec(name, dev, *a, **kw):
        trace.append((name, tuple(i for i, v in enumerate(a) if v is None)))
        return orig(name, dev, *a, **kw)
    mods = [m for n, m in list(sys.modules.items())
            if n.startswith("adaptpoint_amd.") and getattr(m, "_call", None) is orig]
    for m in mods:
        m._call = rec
    try:
        yield trace
    finally:
        for m in mods:
            m._call = orig


def _rand(dev, *shape, seed=0):
    return torch.randn(*shape, device=dev, generator=torch.Generator(dev).manual_seed(seed))


def _bn(cls, c, dev, training, seed):
    bn = cls(c).to(dev).train(training)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(c, device=dev, generator=torch.Generator(dev).manual_seed(seed)))
        bn.bias.copy_(_rand(dev, c, seed=seed + 1) * 0.2)
        bn.running_mean.copy_(_rand(dev, c, seed=seed + 2) * 0.1)
        bn.running_var.copy_(0.5 + torch.rand(c, device=dev, generator=torch.Generator(dev).manual_seed(seed + 3)))
    return bn


def _conv(cls, cin, cout, dev, seed):
    torch.manual_seed(seed)
    return cls(cin, cout, 1, bias=False).to(dev)


def _cloud(dev, B, N, seed):
    return torch.rand(B, N, 3, device=dev, generator=torch.Generator(dev).manual_seed(seed)).contiguous()


# Every case: (dev, training) -> (run, outputs-of-interest BatchNorms); `run` does one forward + backward pass and returns
# the tensors a digest of the pass would cover (scripts compare them between two versions of the package).
def case_conv_bn_act(dev, training):
    from adaptpoint_amd import pointwise
    conv, bn = _conv(torch.nn.Conv1d, 3, 5, dev, 1), _bn(torch.nn.BatchNorm1d, 5, dev, training, 2)
    x = _rand(dev, 2, 3, 130, seed=3).requires_grad_(True)

    def run():
        out = pointwise.conv_bn_act(x, conv, bn)
        out.backward(_rand(dev, *out.shape, seed=4))
        return out, x.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad
    return run, [bn]


def case_conv_bias_act(dev, training):
    from adaptpoint_amd import pointwise
    w, b = _rand(dev, 5, 3, 1, seed=1).requires_grad_(True), _rand(dev, 5, seed=2).requires_grad_(True)
    x = _rand(dev, 2, 3, 130, seed=3).requires_grad_(True)

    def run():
        out = pointwise.conv_bias_act(x, w, b)
        out.backward(_rand(dev, *out.shape, seed=4))
        return out, x.grad, w.grad, b.grad
    return run, []


def _case_propagate(dev, training, skip):
    from adaptpoint_amd import propagation
    B, C1, C2, O, n, m = 2, 3, 4, 5, 130, 7
    conv = _conv(torch.nn.Conv1d, (C1 if skip else 0) + C2, O, dev, 1)
    bn = _bn(torch.nn.BatchNorm1d, O, dev, training, 2)
    f1 = _rand(dev, B, C1, n, seed=3).requires_grad_(True) if skip else None
    f2 = _rand(dev, B, C2, m, seed=4).requires_grad_(True)
    nearest = torch.randint(0, m, (B, n, 3), device=dev, generator=torch.Generator(dev).manual_seed(5)).int()
    weights = torch.rand(B, n, 3, device=dev, generator=torch.Generator(dev).manual_seed(6))
    weights = (weights / weights.sum(-1, keepdim=True)).contiguous()
    assert propagation.supported(f1, f2, conv, bn)

    def run():
        out = propagation.propagate(f1, f2, nearest, weights, conv, bn)
        out.backward(_rand(dev, *out.shape, seed=7))
        return (out, f2.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad) + ((f1.grad,) if skip else ())
    return run, [bn]


def case_propagate_skip(dev, training):
    return _case_propagate(dev, training, True)


def case_propagate_coarse_only(dev, training):
    return _case_propagate(dev, training, False)


def case_affine_group_bn_act(dev, training):
    from adaptpoint_amd import affine_group as AG
    B, N, S, K, C, O = 1, 8, 1, 1, 16, 32                     # the smallest case of tests/test_gpu_affine_group.py
    i32 = dict(dtype=torch.int32, device=dev)
    graph = AG.group_index(torch.tensor([[4]], **i32), torch.zeros(B, S, 3, device=dev), torch.tensor([[[3]]], **i32), N)
    bn = _bn(torch.nn.BatchNorm1d, O, dev, training, 2)
    x = _rand(dev, B, N, C, seed=3).requires_grad_(True)
    w = _rand(dev, O, 2 * C, 1, seed=4).requires_grad_(True)
    alpha = (1.0 + 0.1 * _rand(dev, C, seed=5)).requires_grad_(True)
    beta = (0.1 * _rand(dev, C, seed=6)).requires_grad_(True)

    def run():
        out = AG.affine_group_bn_act(x, graph, alpha, beta, w, bn)
        out.backward(_rand(dev, *out.shape, seed=7))
        return out, x.grad, w.grad, alpha.grad, beta.grad, bn.weight.grad, bn.bias.grad
    return run, [bn]


def case_local_aggregation(dev, training):
    from adaptpoint_amd import fused_wide, local_aggr
    from adaptpoint_amd.layers import ball_query
    B, C, H, N = 2, 4, 64, 65
    p = _cloud(dev, B, N, 1)
    index = fused_wide.neighbour_index(ball_query(0.4, 32, p, p), p, N)
    conv, bn = _conv(torch.nn.Conv2d, C + 3, H, dev, 2), _bn(torch.nn.BatchNorm2d, H, dev, training, 3)
    f = _rand(dev, B, C, N, seed=4).requires_grad_(True)
    assert local_aggr.covers(B, N, 32, C, conv.weight.shape[:2])

    def run():
        out = local_aggr.aggregate(p, f, index, 0.4, conv, bn)
        out.backward(_rand(dev, *out.shape, seed=5))
        return out, f.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad
    return run, [bn]


def _case_edge_conv(dev, training, C, slope, residual):
    from adaptpoint_amd import edge_conv as EC
    B, H, N, K = 2, 64, 65, 3
    idx = torch.randint(0, N, (B, N, K), device=dev, generator=torch.Generator(dev).manual_seed(1)).int()
    graph = EC.edge_index(idx)
    conv, bn = _conv(torch.nn.Conv2d, 2 * C, H, dev, 2), _bn(torch.nn.BatchNorm2d, H, dev, training, 3)
    x = _rand(dev, B, C, N, seed=4).requires_grad_(True)
    assert EC.covers(B, N, K, C, H)

    def run():
        out = EC.edge_conv(x, graph, conv, bn, slope, residual=x if residual else None)
        out.backward(_rand(dev, *out.shape, seed=5))
        return out, x.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad
    return run, [bn]


def case_edge_conv_leaky(dev, training):
    return _case_edge_conv(dev, training, 3, 0.2, False)


def case_edge_conv_relu_residual(dev, training):
    return _case_edge_conv(dev, training, 64, 0.0, True)


def case_randla_encode_pool(dev, training):
    import randla_reference as R
    from adaptpoint_amd.randla import (AttentivePooling, LocalSpatialEncoding, encode_pool, encoding_moments,
                                       fused_layer_reason)
    t = R.tensors(R.layer_inputs(*R.CASES[0], seed=1), dev, torch.float32)     # the smallest case of tests/test_gpu_randla.py
    C, K = t['w'].shape[0], t['idx'].shape[2]
    lse, pool = LocalSpatialEncoding(C, K, dev).to(dev), AttentivePooling(2 * C, C).to(dev)
    bn = lse.mlp.batch_norm
    with torch.no_grad():
        lse.mlp.conv.weight.copy_(t['w'].view(C, 10, 1, 1))
        lse.mlp.conv.bias.copy_(t['b'])
        for dst, src in ((bn.weight, 'gamma'), (bn.bias, 'beta'), (bn.running_mean, 'rm'), (bn.running_var, 'rv')):
            dst.copy_(t[src])
        pool.score_fn[0].weight.copy_(t['A'])
    lse.train(training)
    pool.train(training)
    assert fused_layer_reason(lse, pool, t['coords'], t['idx']) is None
    f = t['f'].clone().requires_grad_()
    mom = encoding_moments(t['coords'], t['idx'], t['dist'], False) if training else None

    def run():
        out = encode_pool(lse, pool, t['coords'], f.unsqueeze(3), t['idx'], t['dist'], mom, False)
        (out.squeeze(3) * t['g']).sum().backward()
        return (out, f.grad, lse.mlp.conv.weight.grad, lse.mlp.conv.bias.grad, bn.weight.grad, bn.bias.grad,
                pool.score_fn[0].weight.grad)
    return run, [bn]


def case_wide_grouped_mlp_max(dev, training):
    from adaptpoint_amd import fused_wide
    from adaptpoint_amd.layers import ball_query
    B, C, H, N, M = 2, 4, 32, 65, 33                          # H = 32: the narrowest width of fused_wide.WIDTHS
    p = _cloud(dev, B, N, 1)
    new_p = p[:, :M].contiguous()
    idx = ball_query(0.4, 32, p, new_p)
    index = fused_wide.neighbour_index(idx, new_p, N)
    conv1, conv2 = _conv(torch.nn.Conv2d, C + 3, H, dev, 2), _conv(torch.nn.Conv2d, H, 2 * H, dev, 3)
    bn1, bn2 = _bn(torch.nn.BatchNorm2d, H, dev, training, 4), _bn(torch.nn.BatchNorm2d, 2 * H, dev, training, 8)
    f = _rand(dev, B, C, N, seed=5).requires_grad_(True)
    assert fused_wide.supported(p, f, idx, conv1, conv2, (bn1, bn2))

    def run():
        out = fused_wide.grouped_mlp_max(p, new_p, f, idx, 0.4, conv1, bn1, conv2, bn2, index=index)
        out.backward(_rand(dev, *out.shape, seed=6))
        return (out, f.grad, conv1.weight.grad, conv2.weight.grad, bn1.weight.grad, bn1.bias.grad, bn2.weight.grad,
                bn2.bias.grad)
    return run, [bn1, bn2]


CASES = {f.__name__[5:]: f for f in (case_conv_bn_act, case_conv_bias_act, case_propagate_skip, case_propagate_coarse_only,
                                     case_affine_group_bn_act, case_local_aggregation, case_edge_conv_leaky,
                                     case_edge_conv_relu_residual, case_randla_encode_pool, case_wide_grouped_mlp_max)}


def trace_of(name, mode, dev):
    """-> (trace, [(bn, its three buffers before the pass)], the pass's tensors)."""
    run, bns = CASES[name](dev, mode == T)
    before = [(bn, [b.clone() for b in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]) for bn in bns]
    with recording() as trace:
        tensors = run()
    torch.cuda.synchronize()
    return trace, before, tensors


def _all_present(*names):
    return [(n, ()) for n in names]


_PW_BACKWARD = _all_present("apn_pw_bn_act_grad", "apn_pw_conv_grad_input", "apn_pw_conv_grad_weight")
_NO_NORM = [("apn_pw_conv_forward", (8,)), ("apn_pw_bn_act", (4, 6, 14))] + _PW_BACKWARD        # no rows, gamma, counter
_FP_BACKWARD = [("apn_pw_bn_act_grad", ()), ("apn_three_interpolate_grad", ())]
_AG_BACKWARD = ([("apn_pw_bn_act_grad", ()), ("apn_pw_transpose", ()), ("apn_ag_combine_bwd", ()), ("apn_ag_fold", ()),
                 ("apn_ag_sigma_bwd", ()), ("apn_pw_contract", (16,)), ("apn_pw_contract", ())]
                + _all_present("apn_ag_fold", "apn_ag_fold", "apn_ag_fold"))
_AG_FORWARD = [("apn_ag_moments", ()), ("apn_ag_fold", ()), ("apn_pw_contract", (16,))]
_FOLD_OF_SUMS = ("apn_sa_bn_fold", (0, 14, 16))                 # no rows, no sign rider
_FOLD_EVAL = ("apn_sa_bn_fold", (0, 2, 11, 14, 16))             # ... nor sums, nor the counter
_EC_DENSE = [("apn_pw_contract", (16,)), ("apn_pw_contract", ())]
_LA_DENSE = [("apn_pw_contract", (16,)), ("apn_pw_contract", ()), ("apn_pw_contract", ())]
_WIDE_TAIL = [("apn_sa_wide_colsum", ()), ("apn_sa_wide_bwd_fin", (2,)),
              ("apn_sa_wide_point_grads", (20, 21, 22, 23, 25, 26)), ("apn_sa_wide_colsum_f32", ())]


def _edge_conv(training, residual):
    out = ("apn_ec_out_res", () if residual else (6,))
    if training:
        return ([("apn_pw_contract", (16,)), ("apn_ec_pool_fwd", ()), ("apn_la_stats_fold", ()), _FOLD_OF_SUMS, out,
                 ("apn_ec_bwd_prep_act", ()), ("apn_sa_wide_consts2", (2,)), ("apn_ec_pool_bwd", ())] + _EC_DENSE)
    return ([("apn_pw_contract", (16,)), ("apn_ec_pool_fwd", (10, 11)), _FOLD_EVAL, out,
             ("apn_ec_bwd_prep_act", ()), ("apn_sa_wide_consts2", (2,)), ("apn_ec_pool_bwd", (10,))] + _EC_DENSE)


EXPECTED = {
    ("conv_bn_act", T): _all_present("apn_pw_conv_forward", "apn_pw_bn_act") + _PW_BACKWARD,
    ("conv_bn_act", E): [("apn_pw_conv_forward", (8,)), ("apn_pw_bn_act", (4, 14))] + _PW_BACKWARD,
    ("conv_bias_act", T): _NO_NORM,
    ("conv_bias_act", E): _NO_NORM,
    ("propagate_skip", T): ([("apn_pw_contract2", ()), ("apn_fp_blend_stats", (11, 12, 13, 14, 17, 18)),
                             ("apn_pw_bn_act", ())] + _FP_BACKWARD + _all_present("apn_pw_contract2", "apn_pw_contract2")),
    ("propagate_skip", E): ([("apn_pw_contract2", ()), ("apn_fp_blend_stats", (9,))] + _FP_BACKWARD
                            + _all_present("apn_pw_contract2", "apn_pw_contract2")),
    ("propagate_coarse_only", T): ([("apn_pw_contract", (16,)), ("apn_fp_blend_stats", (4, 11, 12, 13, 14, 17, 18)),
                                    ("apn_pw_bn_act", ())] + _FP_BACKWARD + [("apn_pw_contract", (16,)), ("apn_pw_contract", ())]),
    ("propagate_coarse_only", E): ([("apn_pw_contract", (16,)), ("apn_fp_blend_stats", (4, 9))] + _FP_BACKWARD
                                   + [("apn_pw_contract", (16,)), ("apn_pw_contract", ())]),
    ("affine_group_bn_act", T): (_AG_FORWARD + [("apn_ag_combine_fwd", (13, 14, 15, 16, 19, 20)), ("apn_pw_bn_act", ())]
                                 + _AG_BACKWARD),
    ("affine_group_bn_act", E): _AG_FORWARD + [("apn_ag_combine_fwd", (11,))] + _AG_BACKWARD,
    ("local_aggregation", T): ([("apn_pw_contract", (16,)), ("apn_la_pool_fwd", ()), ("apn_la_stats_fold", ()), _FOLD_OF_SUMS,
                                ("apn_sa_wide_out", (6, 7, 8)), ("apn_sa_wide_bwd_prep", (10,)),
                                ("apn_sa_wide_consts2", (2,)), ("apn_la_pool_bwd", (19,))] + _LA_DENSE),
    ("local_aggregation", E): ([("apn_pw_contract", (16,)), ("apn_la_pool_fwd", (13, 14)), _FOLD_EVAL,
                                ("apn_sa_wide_out", (6, 7, 8)), ("apn_sa_wide_bwd_prep", (10,)),
                                ("apn_sa_wide_consts2", (2,)), ("apn_la_pool_bwd", (13, 19))] + _LA_DENSE),
    ("edge_conv_leaky", T): _edge_conv(True, False),
    ("edge_conv_leaky", E): _edge_conv(False, False),
    ("edge_conv_relu_residual", T): _edge_conv(True, True),
    ("edge_conv_relu_residual", E): _edge_conv(False, True),
    ("randla_encode_pool", T): _all_present("apn_rl_fold", "apn_rl_forward", "apn_rl_backward", "apn_rl_finalize"),
    ("randla_encode_pool", E): [("apn_rl_fold", (1, 12)), ("apn_rl_forward", ()), ("apn_rl_backward", ()),
                                ("apn_rl_finalize", (3,))],
    ("wide_grouped_mlp_max", T): ([("apn_sa_wide_fwd_prep", (15, 16)), ("apn_sa_bn_fold", (2,)), ("apn_sa_wide_fwd_main", ()),
                                   ("apn_sa_bn_fold", (2, 14, 16)), ("apn_sa_wide_out", (6, 7, 8)),
                                   ("apn_sa_wide_bwd_prep", (9, 10)), ("apn_sa_wide_bwd_mid", (2,)),
                                   ("apn_sa_wide_bwd_main", ())] + _WIDE_TAIL),
    ("wide_grouped_mlp_max", E): ([("apn_sa_wide_fwd_prep", (15, 16, 17, 18)), ("apn_sa_bn_fold", (0, 2, 11)),
                                   ("apn_sa_wide_fwd_main", ()), _FOLD_EVAL, ("apn_sa_wide_out", (6, 7, 8)),
                                   ("apn_sa_wide_bwd_prep", (9, 10)), ("apn_sa_wide_bwd_mid", (2,)),
                                   ("apn_sa_wide_bwd_main", (11,))] + _WIDE_TAIL),
}


@pytest.mark.parametrize("mode", [T, E])
@pytest.mark.parametrize("name", CASES)
def test_launches_and_buffers(dev, name, mode):
    trace, before, _ = trace_of(name, mode, dev)
    assert trace == EXPECTED[name, mode]
    for bn, (rm, rv, nbt) in before:
        if mode == T:
            assert int(nbt) == 0 and int(bn.num_batches_tracked) == 1
            assert not torch.equal(bn.running_mean, rm) and not torch.equal(bn.running_var, rv)
        else:
            assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv)
            assert torch.equal(bn.num_batches_tracked, nbt)
