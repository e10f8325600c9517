"""GPU suite of the fused RandLA-Net layer (csrc/randla.hip, adaptpoint_amd/randla.py): the raw apn_rl_* entries on exact
cases, compared bit for bit, then the Python layer against the float64 statement of the reference's FULL layer
(tests/randla_reference.py: concatenation and the 2C x 2C score layer) at every case of randla_reference.CASES.

The bar: the fused forward, and each gradient relative to its own norm, lie within 8 x the composed float32 PyTorch
form's own distance to float64 on the same inputs on the same GPU -- eight is the margin tests/test_gpu_emd.py grants a
kernel that reorders sums; this one also centres and folds the BatchNorm and derives variances from moments.  Where the
composed form is exact (a distance of zero) so must the kernels be.  The dead blocks of the score weight and the bias in
front of the training-mode BatchNorm are exact zeros.  MEASURED holds the distances seen on an MI355X (documentation: the test asserts the bar, not them)."""
import functools

import numpy as np
import pytest
import torch

import randla_reference as R

pytestmark = pytest.mark.gpu

MARGIN = 8.0
PROJECTION = 1e-3

# Measured on an MI355X, relative L2 distance to float64, "fused / composed" per tensor (training mode, seed 1; the
# bar is fused <= 8 x composed; f: the fused gradient is the exact pass-through).  Worst ratio: 1.7 (beta at (1,37,3,8)).
MEASURED = {
    (1, 1, 1, 8): dict(out="0 / 0", w="0 / 0", gamma="0 / 0", beta="0 / 0", A="0 / 0", f="0 / 0"),
    (1, 37, 3, 8): dict(out="4.6e-8 / 6.1e-8", w="1.1e-7 / 1.8e-7", gamma="4.3e-8 / 7.7e-8", beta="1.2e-7 / 7.1e-8",
                        A="3.7e-7 / 7.7e-7", f="1e-16 / 6.1e-8"),
    (3, 130, 16, 8): dict(out="4.0e-8 / 7.7e-8", w="1.4e-7 / 8.4e-7", gamma="9.9e-8 / 1.3e-7", beta="8.6e-8 / 9.6e-8",
                          A="5.2e-7 / 2.0e-6", f="2e-16 / 8.8e-8"),
    (1, 37, 16, 32): dict(out="3.6e-8 / 7.6e-8", w="1.4e-7 / 3.3e-7", gamma="1.1e-7 / 1.1e-7", beta="1.5e-7 / 1.2e-7",
                          A="2.1e-7 / 1.3e-6", f="2e-16 / 8.9e-8"),
    (3, 130, 5, 32): dict(out="4.6e-8 / 6.5e-8", w="1.3e-7 / 4.7e-7", gamma="9.0e-8 / 9.7e-8", beta="9.3e-8 / 7.5e-8",
                          A="7.3e-7 / 1.7e-6", f="1e-16 / 6.6e-8"),
    (1, 130, 16, 64): dict(out="4.0e-8 / 7.9e-8", w="1.4e-7 / 4.9e-7", gamma="1.1e-7 / 1.2e-7", beta="1.1e-7 / 1.0e-7",
                           A="3.6e-7 / 1.7e-6", f="2e-16 / 8.8e-8"),
    (1, 37, 32, 64): dict(out="3.5e-8 / 1.0e-7", w="1.3e-7 / 5.1e-7", gamma="9.3e-8 / 1.2e-7", beta="1.3e-7 / 9.4e-8",
                          A="1.8e-7 / 1.3e-6", f="2e-16 / 1.1e-7"),
    (1, 130, 16, 128): dict(out="3.8e-8 / 7.8e-8", w="1.3e-7 / 5.6e-7", gamma="1.1e-7 / 1.1e-7", beta="1.3e-7 / 1.1e-7",
                            A="3.6e-7 / 1.8e-6", f="2e-16 / 8.7e-8"),
    (3, 37, 1, 128): dict(out="3.9e-8 / 5.2e-8", w="1.3e-7 / 2.8e-7", gamma="1.1e-7 / 1.1e-7", beta="8.7e-8 / 6.2e-8",
                          A="0 / 0", f="0 / 0"),
    (2, 130, 16, 16): dict(out="4.2e-8 / 8.2e-8", w="1.5e-7 / 8.1e-7", gamma="1.9e-7 / 2.1e-7", beta="1.5e-7 / 1.4e-7",
                           A="5.0e-7 / 2.5e-6", f="2e-16 / 8.9e-8"),
    "eval (3, 130, 5, 32)": dict(out="3.2e-8 / 5.9e-8", w="9.6e-8 / 3.2e-7", gamma="8.7e-8 / 6.6e-8",
                                 beta="7.0e-8 / 8.7e-8", A="1.1e-6 / 5.2e-6", f="1e-16 / 6.4e-8", b="6.9e-8 / 1.0e-7"),
    "euclidean (1, 130, 16, 64)": dict(out="4.1e-8 / 7.8e-8", w="1.3e-7 / 4.8e-7", gamma="1.3e-7 / 1.5e-7",
                                       beta="1.5e-7 / 1.0e-7", A="4.0e-7 / 1.7e-6", f="2e-16 / 8.8e-8"),
}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _call(name, *args):
    from adaptpoint_amd.fused import _call as call
    call(name, _dev(), *args)


def _raw_forward(coords, idx, dist, wf, A_hh, root=False):
    B, N, K = idx.shape
    C = A_hh.shape[0]
    at = A_hh.t().contiguous()
    pooled = torch.empty(B, C, N, device=coords.device)
    _call("apn_rl_forward", B, N, K, C, coords.data_ptr(), idx.data_ptr(), dist.data_ptr(), int(root), wf.data_ptr(),
          at.data_ptr(), pooled.data_ptr())
    return pooled


def _integer_wf(C, seed, dev):
    """Integer W' (C,10), b' (C) and mu (10): every h = relu(W' (e - mu) + b') on a lattice cloud is an integer below
    2^24, exact in float32 whatever the order."""
    rng = np.random.default_rng(seed)
    W, b, mu = rng.integers(-2, 3, size=(C, 10)), rng.integers(-3, 4, size=C), rng.integers(-2, 3, size=10)
    wf = torch.from_numpy(np.concatenate([W.ravel(), b, mu]).astype(np.float32)).to(dev)
    return wf, W.astype(np.float64), b.astype(np.float64), mu.astype(np.float64)


@pytest.mark.parametrize("case", [(1, 1, 1, 8), (3, 37, 1, 128), (2, 37, 1, 32)])
def test_one_neighbour_pools_to_its_hidden_value_bit_for_bit(case):
    B, N, K, C = case
    dev = _dev()
    t = R.tensors(R.layer_inputs(B, N, K, C, seed=11, integer=True), dev, torch.float32)
    wf, W, b, mu = _integer_wf(C, 100 + C, dev)
    pooled = _raw_forward(t['coords'], t['idx'], t['dist'], wf, t['A'][:C, :C].contiguous())
    e = R.encoding(t['coords'].double(), t['idx'], t['dist'].double()).cpu().numpy()          # (B,10,N,1)
    h = np.maximum(np.einsum('ci,bink->bcnk', W, e - mu.reshape(1, 10, 1, 1)) + b.reshape(1, C, 1, 1), 0.0)[..., 0]
    assert np.abs(h).max() < 2 ** 24 and h.any()
    assert np.array_equal(pooled.cpu().numpy(), h.astype(np.float32))


@pytest.mark.parametrize("C", [8, 16, 32, 64, 128])
def test_sixteen_copies_of_one_neighbour_pool_to_that_neighbour_bit_for_bit(C):
    """Equal logits give scores of exactly 1/16 and sixteen equal addends of h/16 sum exactly: the K = 16 result is the
    K = 1 result for that neighbour, whatever A_hh is."""
    B, N = 2, 37
    dev = _dev()
    t = R.tensors(R.layer_inputs(B, N, 16, C, seed=13), dev, torch.float32)
    wf = torch.cat([t['w'].reshape(-1), t['b'], t['rm'].new_tensor(np.linspace(-0.3, 0.3, 10))]).contiguous()
    pick = t['idx'][:, :, 5:6].contiguous()                      # some neighbour of every row, not itself
    dpick = t['dist'][:, :, 5:6].contiguous()
    A = t['A'][:C, :C].contiguous()
    one = _raw_forward(t['coords'], pick, dpick, wf, A)
    many = _raw_forward(t['coords'], pick.expand(B, N, 16).contiguous(), dpick.expand(B, N, 16).contiguous(), wf, A)
    assert one.abs().sum() > 0 and torch.equal(one, many)
    assert torch.equal(many, _raw_forward(t['coords'], pick.expand(B, N, 16).contiguous(),
                                          dpick.expand(B, N, 16).contiguous(), wf, (3.0 * A).contiguous()))


@pytest.mark.parametrize("case", [(3, 130, 16, 8), (1, 37, 3, 32)])
def test_training_statistics_on_a_lattice_equal_the_float64_statement(case):
    """Integer coordinates and integer weights: the 65 moments are sums of integers (exact in float64 in any order) and
    the batch mean / biased variance equal the direct float64 statistics after rounding to float32."""
    B, N, K, C = case
    dev = _dev()
    from adaptpoint_amd import _lib
    from adaptpoint_amd.randla import encoding_moments
    t = R.tensors(R.layer_inputs(B, N, K, C, seed=17, integer=True), dev, torch.float32)
    mom = encoding_moments(t['coords'], t['idx'], t['dist'], False)
    e = R.encoding(t['coords'].double(), t['idx'], t['dist'].double())
    flat = e.permute(1, 0, 2, 3).reshape(10, -1)
    second = flat @ flat.t()
    expect = torch.cat([flat.sum(1)] + [second[i, i:] for i in range(10)])
    assert torch.equal(mom, expect)
    wf = torch.empty(11 * C + 10, device=dev)
    stat = torch.empty(3 * C, dtype=torch.float64, device=dev)
    rm, rv = t['rm'].clone(), t['rv'].clone()
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    count = float(B * N * K)
    _call("apn_rl_fold", C, mom.data_ptr(), count, t['w'].data_ptr(), t['b'].data_ptr(), t['gamma'].data_ptr(),
          t['beta'].data_ptr(), R.EPS, R.MOMENTUM, 1, rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), wf.data_ptr(),
          stat.data_ptr())
    _, mean, var = R.hidden(e, t['w'].double(), t['b'].double(), t['gamma'].double(), t['beta'].double())
    assert torch.equal(stat[:C].float(), mean.float()) and torch.equal(stat[C:2 * C].float(), var.float())
    assert int(nbt) == 1 and _lib.load().apn_rl_moment_rows(B, N, K) >= 1
    # the running buffers as nn.BatchNorm2d leaves them (unbiased variance), to float32 rounding
    bn = torch.nn.BatchNorm2d(C, eps=R.EPS, momentum=R.MOMENTUM).to(dev)
    with torch.no_grad():
        bn.running_mean.copy_(t['rm'])
        bn.running_var.copy_(t['rv'])
        pre = torch.einsum('ci,bink->bcnk', t['w'], e.float()) + t['b'].view(1, -1, 1, 1)
        bn(pre)
    assert int(bn.num_batches_tracked) == 1
    _assert_buffers(rm, rv, bn, pre)


def _assert_buffers(running_mean, running_var, bn, pre):
    """Equal to nn.BatchNorm2d's to float32 rounding: its statistics are float32 sums over a few thousand values -- 16
    ulps of the activations' scale for the mean, of the variance for the variance."""
    ulp = 2.0 ** -23
    torch.testing.assert_close(running_mean, bn.running_mean, rtol=0, atol=16 * ulp * pre.abs().max().item())
    torch.testing.assert_close(running_var, bn.running_var, rtol=16 * ulp, atol=0)


def _modules(C, K, t, training):
    from adaptpoint_amd.randla import AttentivePooling, LocalSpatialEncoding
    dev = t['w'].device
    lse, pool = LocalSpatialEncoding(C, K, dev).to(dev), AttentivePooling(2 * C, C).to(dev)
    with torch.no_grad():
        lse.mlp.conv.weight.copy_(t['w'].view(C, 10, 1, 1))
        lse.mlp.conv.bias.copy_(t['b'])
        bn = lse.mlp.batch_norm
        bn.weight.copy_(t['gamma'])
        bn.bias.copy_(t['beta'])
        bn.running_mean.copy_(t['rm'])
        bn.running_var.copy_(t['rv'])
        pool.score_fn[0].weight.copy_(t['A'])
    lse.train(training)
    pool.train(training)
    return lse, pool


def _fused(inputs, training=True, root=False):
    """The Python layer on the kernels -> (out (B,2C,N), {name: gradient of sum(out * g)}, lse)."""
    from adaptpoint_amd.randla import encode_pool, encoding_moments, fused_layer_reason
    dev = _dev()
    t = R.tensors(inputs, dev, torch.float32)
    C, K = t['w'].shape[0], t['idx'].shape[2]
    lse, pool = _modules(C, K, t, training)
    assert fused_layer_reason(lse, pool, t['coords'], t['idx']) is None
    f = t['f'].clone().requires_grad_()
    mom = encoding_moments(t['coords'], t['idx'], t['dist'], root) if training else None
    out = encode_pool(lse, pool, t['coords'], f.unsqueeze(3), t['idx'], t['dist'], mom, root).squeeze(3)
    (out * t['g']).sum().backward()
    bn = lse.mlp.batch_norm
    grads = dict(w=lse.mlp.conv.weight.grad.view(C, 10), b=lse.mlp.conv.bias.grad, gamma=bn.weight.grad,
                 beta=bn.bias.grad, A=pool.score_fn[0].weight.grad, f=f.grad)
    return out.detach(), grads, lse


@functools.lru_cache(maxsize=None)
def _references(case, training=True, root=False):
    """(float64, composed float32) statements of the full layer on the GPU: (out, grads, mean, var) each."""
    inputs = R.layer_inputs(*case, seed=1)
    dev = _dev()
    return (R.layer_with_gradients(R.full_layer, inputs, dev, torch.float64, training, root),
            R.layer_with_gradients(R.full_layer, inputs, dev, torch.float32, training, root))


def _compare(case, training=True, root=False):
    C = case[3]
    (o64, g64, _, _), (o32, g32, _, _) = _references(case, training, root)
    out, grads, _ = _fused(R.layer_inputs(*case, seed=1), training, root)
    rows = {'out': (R.rel(out, o64), R.rel(o32, o64))}
    for k in ('w', 'gamma', 'beta', 'A', 'f') + (() if training else ('b',)):
        rows[k] = (R.rel(grads[k], g64[k]), R.rel(g32[k], g64[k]))
        if g64[k].numel() >= 8192:
            assert R.projection(grads[k], g64[k]) <= PROJECTION, (case, k)
    print(case, "train" if training else "eval", "root" if root else "", {k: "%.1e / %.1e" % v for k, v in rows.items()})
    # the dead blocks, and the bias in front of a training-mode BatchNorm: exact zeros
    A = grads['A']
    assert not A[:C, C:].any() and not A[C:, :C].any() and not A[C:, C:].any()
    if training:
        assert not grads['b'].any()
    bad = {k: v for k, v in rows.items() if not v[0] <= MARGIN * v[1]}
    assert not bad, (case, bad)


@pytest.mark.parametrize("case", R.CASES)
def test_layer_against_float64_within_eight_times_the_composed_distance(case):
    _compare(case)


def test_eval_mode_runs_on_the_running_buffers():
    _compare((3, 130, 5, 32), training=False)


def test_euclidean_distance_takes_the_root_in_the_kernel():
    _compare((1, 130, 16, 64), root=True)


@pytest.mark.parametrize("case", [(3, 130, 16, 8), (1, 130, 16, 128), (3, 130, 5, 32)])
def test_two_runs_give_the_same_bits(case):
    inputs = R.layer_inputs(*case, seed=2)
    o1, g1, _ = _fused(inputs)
    o2, g2, _ = _fused(inputs)
    assert torch.equal(o1, o2) and all(torch.equal(g1[k], g2[k]) for k in g1)


def test_running_buffers_after_a_step_equal_batchnorms():
    case = (3, 130, 16, 8)
    inputs = R.layer_inputs(*case, seed=1)
    _, _, lse = _fused(inputs)
    t = R.tensors(inputs, _dev(), torch.float32)
    bn = torch.nn.BatchNorm2d(case[3], eps=R.EPS, momentum=R.MOMENTUM).to(_dev())
    with torch.no_grad():
        bn.running_mean.copy_(t['rm'])
        bn.running_var.copy_(t['rv'])
        e = R.encoding(t['coords'], t['idx'], t['dist'])
        pre = torch.einsum('ci,bink->bcnk', t['w'], e) + t['b'].view(1, -1, 1, 1)
        bn(pre)
    mine = lse.mlp.batch_norm
    assert int(mine.num_batches_tracked) == int(bn.num_batches_tracked) == 1
    _assert_buffers(mine.running_mean, mine.running_var, bn, pre)


def test_out_of_range_indices_are_clamped():
    B, N, K, C = 1, 37, 3, 8
    dev = _dev()
    t = R.tensors(R.layer_inputs(B, N, K, C, seed=19), dev, torch.float32)
    wf = torch.cat([t['w'].reshape(-1), t['b'], torch.zeros(10, device=dev)]).contiguous()
    A = t['A'][:C, :C].contiguous()
    wild = t['idx'].clone()
    wild[0, 0, 0], wild[0, 1, 1] = -5, N + 1000
    tame = wild.clamp(0, N - 1)
    assert torch.equal(_raw_forward(t['coords'], wild, t['dist'], wf, A), _raw_forward(t['coords'], tame, t['dist'], wf, A))
