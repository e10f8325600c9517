"""GPU: PointWOLF and RSMix (adaptpoint_amd.online_aug, csrc/online_aug.hip) against the reference's outputs recorded in
tests/golden/online_aug_golden.npz, against the CPU restatements of tests/online_aug_reference.py with hand-built draws,
and inside the training steps that use them (gan.ClassifierStep, gan.GanStep)."""
import copy

import numpy as np
import pytest
import torch

import online_aug_reference as R

pytestmark = pytest.mark.gpu
B = 8


@pytest.fixture(scope="module")
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "online_aug_golden.npz"))


def _pw_xyz(golden, dev):
    return torch.from_numpy(np.ascontiguousarray(R.golden_points(int(golden["pw_points_seed"]))[:, :, :3])).to(dev)


# ------------------------------------------------------------------------------------------------------------ PointWOLF
def test_pointwolf_matches_reference_golden(dev, golden):
    from adaptpoint_amd.online_aug import PointWOLF
    xyz = _pw_xyz(golden, dev)
    torch.manual_seed(int(golden["pw_seed"]))
    x0, out = PointWOLF()(xyz)
    assert x0 is xyz or torch.equal(x0, xyz)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - golden["pw_out"]).max())
    # the bar: a small factor over the float64 restatement's own distance to the reference (float32 rounding there)
    bar = 8 * float(golden["pw_restatement_dist"])
    print(f"PointWOLF vs reference: {err:.3e} (restatement {float(golden['pw_restatement_dist']):.3e}, bar {bar:.3e})")
    assert err < bar


def test_pointwolf_anchors_are_the_fps_wrapper_picks(dev, golden):
    from adaptpoint_amd import ops
    from adaptpoint_amd.online_aug import PointWOLF
    xyz = _pw_xyz(golden, dev)
    idx, anchors = PointWOLF().anchors(xyz)
    ref = torch.empty(B, 4, dtype=torch.int32, device=dev)
    ops.furthest_point_sampling_wrapper(B, xyz.shape[1], 4, xyz, torch.full((B, xyz.shape[1]), 1e10, device=dev), ref)
    assert torch.equal(idx, ref) and np.array_equal(idx.cpu().numpy(), golden["pw_fidx"])
    assert torch.equal(anchors, torch.gather(xyz, 1, ref.long().unsqueeze(-1).expand(-1, -1, 3)))


def test_pointwolf_kernel_against_restatement_with_given_draws(dev, golden):
    """Hand-packed draws (every switch pattern, extreme angles) through the params kernel + deformation."""
    from adaptpoint_amd.online_aug import PointWOLF
    xyz = _pw_xyz(golden, dev)[:, :1024].contiguous()
    pw = PointWOLF(w_num_anchor=6, w_sigma=0.3)
    g = torch.Generator().manual_seed(5)
    M = 6
    keep = (torch.arange(B * M * 3) % 2).float()[torch.randperm(B * M * 3, generator=g)]
    code = (torch.arange(B * M) % 7 + 1).float()
    deg = torch.rand(B * M * 3, generator=g) * 20 - 10
    scale = 1 + 2 * torch.rand(B * M * 3, generator=g)
    trl = torch.rand(B * M * 3, generator=g) * 0.5 - 0.25
    kcode = (torch.arange(B) % 7 + 1).float()
    draws = torch.cat([keep, code, deg, scale, trl, kcode])
    _, out = pw(xyz, draws=draws)
    idx, _ = pw.anchors(xyz)
    ref = R.pointwolf_f64(xyz.cpu().numpy(), idx.cpu().numpy(), draws.numpy(), sigma=0.3).numpy()
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f"PointWOLF (hand-built draws) vs float64 restatement: {err:.3e}")
    assert err < 2e-6


def test_pointwolf_device_draws_capture_and_replay(dev, golden):
    from adaptpoint_amd import graphs
    from adaptpoint_amd.online_aug import PointWOLF
    xyz = _pw_xyz(golden, dev)
    pw = PointWOLF()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        pw(xyz, device_draws=True)                                   # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    g = graphs.new_graph()
    with torch.cuda.graph(g):
        _, out = pw(xyz, device_draws=True)
    state = torch.cuda.get_rng_state(dev)
    g.replay()
    replayed = out.clone()
    torch.cuda.set_rng_state(state, dev)
    _, eager = pw(xyz, device_draws=True)
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager)
    g.replay()
    assert not torch.equal(out, replayed)                            # a replay draws afresh
    assert torch.isfinite(out).all() and float(out.norm(dim=-1).max()) < 1.0


# ---------------------------------------------------------------------------------------------------------------- RSMix
def _check_rsmix(dev, points, label, seed, n_sample, knn, draws=None):
    from adaptpoint_amd.online_aug import rsmix
    np.random.seed(seed)
    mixed, lam, la, lb = rsmix(torch.from_numpy(points).to(dev), torch.from_numpy(label).to(dev), 1.0, n_sample, knn,
                               draws=draws)
    tail = np.random.rand()
    np.random.seed(seed)
    out, lam_r, la_r, lb_r, counts = R.rsmix_np(points, label, 1.0, n_sample, knn, draws=draws)
    assert tail == np.random.rand(), "the device path consumed numpy's stream differently"
    assert np.array_equal(mixed.cpu().numpy(), out)
    assert np.array_equal(lam.cpu().numpy(), lam_r)
    assert np.array_equal(la.cpu().numpy(), la_r) and np.array_equal(lb.cpu().numpy(), lb_r)
    return mixed, counts


@pytest.mark.parametrize("case", range(4))
def test_rsmix_matches_reference_golden(dev, golden, case):
    from adaptpoint_amd.online_aug import rsmix
    points = R.golden_points(int(golden["rs_points_seed"]))
    erased = np.unpackbits(golden[f"rs{case}_erased"], axis=1)[:, :points.shape[1]].astype(bool)
    ref = R.rsmix_reconstruct(points, erased, golden[f"rs{case}_appended"], erased.sum(1))
    np.random.seed(int(golden[f"rs{case}_seed"]))
    mixed, lam, la, lb = rsmix(torch.from_numpy(points).to(dev), torch.from_numpy(golden["rs_label"]).to(dev),
                               beta=1.0, n_sample=512, knn=bool(golden[f"rs{case}_knn"]))
    assert np.array_equal(lam.cpu().numpy(), golden[f"rs{case}_lam"])
    assert np.array_equal(la.cpu().numpy(), golden[f"rs{case}_label_a"])
    assert np.array_equal(lb.cpu().numpy(), golden[f"rs{case}_label_b"])
    assert np.array_equal(mixed.cpu().numpy(), ref)


def _cloud(Bn, N, C, seed):
    pts = R.golden_points(seed, B=Bn, N=N)
    if C > 4:
        extra = np.random.RandomState(seed).standard_normal((Bn, N, C - 4)).astype(np.float32)
        pts = np.concatenate([pts, extra], -1)
    return np.ascontiguousarray(pts[:, :, :C])


def _self_distance(points, c):
    """d(q, q) per point of cloud c: the expanded form's rounding makes it a little positive, zero or negative."""
    x = points[c, :, :3]
    return np.array([R.rsmix_distance(x[i:i + 1], x[i].astype(np.float64))[0] for i in range(x.shape[0])])


@pytest.mark.parametrize("C", [3, 6])
def test_rsmix_kernels_set_sizes(dev, C):
    """Ball mode with a fixed radius over ragged sets: |E| = |A| (partner = itself, same query), |E| > |A| and |E| < |A|
    among the other clouds, and the n_sample cap (a radius covering the cloud)."""
    points = _cloud(6, 1000, C, 11)
    label = np.arange(6)
    perm = np.array([0, 2, 1, 4, 5, 3])
    i1 = np.array([5, 17, 230, 999, 0, 640])
    i2 = np.array([5, 400, 3, 77, 512, 901])
    _, counts = _check_rsmix(dev, points, label, 1, 128, False, draws=(0.25, perm, i1, i2))
    e, a = counts[:6], counts[6:]
    assert e[0] == a[0] and (e > a).any() and (e < a).any(), counts
    _, counts = _check_rsmix(dev, points, label, 2, 128, False, draws=(3.0, perm, i1, i2))
    assert (counts == 128).all()
    _, counts = _check_rsmix(dev, points, label, 3, 300, True, draws=(0.4, perm, i1, i2))
    assert (counts == 121).all()


def test_rsmix_kernels_empty_sets(dev):
    """A radius of 0: a query whose self-distance rounds above 0 selects nothing.  An empty add set (dup rows of the
    cloud itself, lambda 0) and an empty erase set (the cloud unchanged)."""
    points = _cloud(4, 700, 4, 12)
    pos = [np.nonzero(_self_distance(points, c) > 0)[0] for c in range(4)]
    zero = [np.nonzero(_self_distance(points, c) <= 0)[0] for c in range(4)]
    perm = np.array([1, 0, 3, 2])
    # cloud 0: E non-empty, A (cloud 1) empty; cloud 1: E empty; clouds 2, 3: both non-empty
    i1 = np.array([zero[0][0], pos[1][0], zero[2][0], zero[3][0]])
    i2 = np.array([pos[1][1], zero[0][1], zero[3][1], zero[2][1]])
    mixed, counts = _check_rsmix(dev, points, np.arange(4), 4, 64, False, draws=(0.0, perm, i1, i2))
    assert counts[0] > 0 and counts[4] == 0 and counts[1] == 0
    assert np.array_equal(mixed[1].cpu().numpy(), points[1])


def test_rsmix_kernels_ties_at_the_threshold(dev):
    """knn with duplicated points: every copy at the k-th distance is a member (up to n_sample)."""
    points = _cloud(3, 1200, 4, 13)
    points[:, 300:420] = points[:, 10:11]                               # 120 copies of point 10
    perm = np.array([1, 2, 0])
    i1 = np.array([10, 10, 305])
    i2 = np.array([10, 400, 11])
    _, counts = _check_rsmix(dev, points, np.arange(3), 5, 256, True, draws=(0.1, perm, i1, i2))
    assert (counts[:3] >= 121).all(), counts                             # k = 26 falls among the copies


def test_rsmix_two_runs_bit_identical(dev):
    from adaptpoint_amd.online_aug import rsmix
    p = torch.from_numpy(_cloud(16, 4096, 4, 14)).to(dev)
    lab = torch.arange(16, device=dev)
    outs = []
    for _ in range(2):
        np.random.seed(9)
        outs.append(rsmix(p, lab, 1.0, 1024, True))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))


def test_rsmix_limits(dev):
    from adaptpoint_amd.online_aug import rsmix
    lab = torch.zeros(2, dtype=torch.long, device=dev)
    with pytest.raises(ValueError, match="8192"):
        rsmix(torch.zeros(2, 8193, 3, device=dev), lab, n_sample=512)
    with pytest.raises(ValueError, match="n_sample"):
        rsmix(torch.zeros(2, 512, 3, device=dev), lab, n_sample=512)
    with pytest.raises(ValueError, match="C >= 3"):
        rsmix(torch.zeros(2, 512, 2, device=dev), lab, n_sample=64)


# ------------------------------------------------------------------------------------------------------ training steps
def _classifier(dev):
    from adaptpoint_amd.pointnext import PointNextSClassifier, fill_parameters_by_name
    m = fill_parameters_by_name(PointNextSClassifier(fused=True))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m.to(dev)


def test_classifier_step_rsmix_matches_composed_iteration(dev):
    """train_one_epoch_rsmix's iteration: gate draw, RSMix, resample, the reference's per-sample loss loop."""
    from adaptpoint_amd.gan import ClassifierStep, resample
    points = _cloud(8, 2048, 4, 15)
    target = np.arange(8) % 15
    m1 = _classifier(dev)
    m2 = copy.deepcopy(m1)
    cfg = dict(beta=1.0, nsample=512, knn=True, rsmix_prob=0.5)
    seed = next(s for s in range(100) if np.random.RandomState(s).rand() < 0.5)
    np.random.seed(seed)
    step = ClassifierStep(m1, optimizer=torch.optim.SGD(m1.parameters(), lr=0.1), rsmix=cfg)
    _, loss = step(torch.from_numpy(points).to(dev), torch.from_numpy(target).to(dev))
    # composed: the same statements, RSMix from the numpy restatement
    np.random.seed(seed)
    assert np.random.rand(1) < cfg['rsmix_prob']
    mixed, lam, ta, tb, _ = R.rsmix_np(points, target, 1.0, 512, True)
    pos, x = resample(torch.from_numpy(mixed).to(dev), 1024, 4)
    m2.train()
    logits = m2({'pos': pos, 'x': x})
    lam_t = torch.from_numpy(lam).to(dev)
    ref = 0
    for i in range(8):
        ref = ref + (m2.criterion(logits[i:i + 1], torch.tensor([ta[i]], device=dev)) * (1 - lam_t[i])
                     + m2.criterion(logits[i:i + 1], torch.tensor([tb[i]], device=dev)) * lam_t[i])
    ref = ref / 8
    ref.backward()
    torch.nn.utils.clip_grad_norm_(m2.parameters(), 10.0, norm_type=2)
    torch.optim.SGD(m2.parameters(), lr=0.1).step()
    print(f"rsmix step: loss {loss.item():.6f} composed {ref.item():.6f}")
    assert abs(loss.item() - ref.item()) < 1e-6
    for (n, a), b in zip(m1.named_parameters(), m2.parameters()):
        assert (a - b).abs().max().item() < 1e-5, n


def test_classifier_step_pointwolf_matches_composed_iteration(dev, golden):
    """train_one_epoch_pointwolf's iteration: PointWOLF in place on points[:, :, :3], resample, loss.  The composed
    iteration applies PointWOLF with the draws the restatement checks (the CPU generator's, replayed), so both halves
    see the same cloud bit for bit; the deformation itself is held to the restatement by the tests above."""
    from adaptpoint_amd.gan import ClassifierStep, resample
    from adaptpoint_amd.online_aug import PointWOLF
    points = torch.from_numpy(_cloud(8, 2048, 4, 16)).to(dev)
    target = torch.arange(8, device=dev) % 15
    m1 = _classifier(dev)
    m2 = copy.deepcopy(m1)
    pw = PointWOLF()
    torch.manual_seed(3)
    np.random.seed(3)
    p1 = points.clone()
    _, loss = ClassifierStep(m1, optimizer=torch.optim.SGD(m1.parameters(), lr=0.1), pointwolf=pw)(p1, target)
    torch.manual_seed(3)
    np.random.seed(3)
    draws = pw.draw_params(8)
    p2 = points.clone()
    _, p2[:, :, :3] = pw(p2[:, :, :3].contiguous(), draws=draws)
    assert torch.equal(p1, p2), "the step applies PointWOLF to the caller's points in place"
    idx, _ = pw.anchors(points[:, :, :3].contiguous())
    f64 = R.pointwolf_f64(points[:, :, :3].cpu().numpy(), idx.cpu().numpy(), draws.numpy()).numpy()
    assert np.abs(p2[:, :, :3].cpu().numpy() - f64).max() < 2e-6
    pos, x = resample(p2, 1024, 4)
    m2.train()
    _, ref = m2.get_logits_loss({'pos': pos, 'x': x}, target)
    ref.backward()
    torch.nn.utils.clip_grad_norm_(m2.parameters(), 10.0, norm_type=2)
    torch.optim.SGD(m2.parameters(), lr=0.1).step()
    assert abs(loss.item() - ref.item()) < 1e-6
    for (n, a), b in zip(m1.named_parameters(), m2.parameters()):
        assert (a - b).abs().max().item() < 1e-5, n


def test_gan_step_pointwolf_then_generator_draws(dev, golden):
    """GanStep(pointwolf=...) returns PointWOLF's cloud, and the generator's CPU draws come after PointWOLF's."""
    from adaptpoint_amd.augmentor import AdaptPointAugmentor
    from adaptpoint_amd.discriminator import PointDiscriminator1
    from adaptpoint_amd.gan import GanStep
    from adaptpoint_amd.online_aug import PointWOLF
    from adaptpoint_amd.pointnext import PointNextSClassifier, SmoothCrossEntropy, fill_parameters_by_name
    G = fill_parameters_by_name(AdaptPointAugmentor(fused=True)).to(dev)
    D = fill_parameters_by_name(PointDiscriminator1(num_classes=15, fused=True))
    for mod in D.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    D = D.to(dev)
    C = _classifier(dev)
    nets = [copy.deepcopy(n) for n in (G, D, C)]
    points = torch.from_numpy(_cloud(4, 1024, 4, 17)).to(dev)
    label = torch.tensor([1, 5, 9, 14], device=dev)
    pw = PointWOLF()
    torch.manual_seed(21)
    res = GanStep(G, D, C, SmoothCrossEntropy(0.3), pointwolf=pw)(points, label)
    torch.manual_seed(21)
    draws = pw.draw_params(4)
    res2 = GanStep(*nets, SmoothCrossEntropy(0.3))(points, label)
    _, expect = pw(points[:, :, :3].contiguous(), draws=draws)
    assert torch.equal(res["pointwolf"], expect)
    assert "pointwolf" not in res2
    for k in ("g_loss_raw", "g_loss", "d_loss", "gen"):
        assert torch.equal(res[k], res2[k]), k
