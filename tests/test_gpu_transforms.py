"""GPU: the ScanObjectNN dataset transforms (adaptpoint_amd.transforms, csrc/cloud_transform.hip) against the reference's
outputs recorded in tests/golden/transforms_golden.npz and the restatements of tests/transforms_reference.py, inside a
captured training step, and ClassifierStep(wolfmix=...)."""
import copy
import os

import numpy as np
import pytest
import torch

import transforms_reference as R

pytestmark = pytest.mark.gpu
B = 8
DT = {'train': ['PointsToTensor', 'PointCloudScaling', 'PointCloudCenterAndNormalize', 'PointCloudRotation'],
      'vote': ['PointCloudRotation'],
      'val': ['PointsToTensor', 'PointCloudCenterAndNormalize'],
      'kwargs': {'scale': [0.9, 1.1], 'angle': [0.0, 1.0, 0.0], 'gravity_dim': 1}}
CHAIN_OF = {'train': 'train', 'val': 'val', 'c': 'val', 'vote': 'vote'}
ULP1 = float(np.spacing(np.float32(1)))          # 1 ulp at the unit sphere's scale


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transforms_golden.npz"))


def _kw(names, gravity_dim=1):
    cn = 'PointCloudCenterAndNormalize' in names
    return dict(scale='PointCloudScaling' in names, heights_scaled=cn, center=cn, normalize=cn,
                rotate='PointCloudRotation' in names, gravity_dim=gravity_dim)


def _ulp_distance(a, b):
    return np.abs(R._ordered(np.asarray(a, np.float32)) - R._ordered(np.asarray(b, np.float32)))


# -------------------------------------------------------------------------------------------------------- host draws
@pytest.mark.parametrize("case", ["train", "val", "c", "vote"])
def test_host_draws_match_reference_golden(dev, golden, case):
    from adaptpoint_amd.transforms import build_transforms_from_cfg
    n = int(golden[f"{case}_n"])
    raw_np = R.golden_clouds(int(golden[f"{case}_cloud_seed"]), B, n)
    raw = torch.from_numpy(raw_np).to(dev)
    tf = build_transforms_from_cfg(CHAIN_OF[case], DT, num_points=n)
    assert tf.shuffle == (case == 'train')
    np.random.seed(int(golden[f"{case}_np_seed"]))
    torch.manual_seed(int(golden[f"{case}_torch_seed"]))
    out, perm, params = tf(raw, record=True)
    out, perm, params = out.cpu().numpy(), perm.cpu().numpy(), params.cpu().numpy()
    gperm = golden["train_perm"].astype(np.int64) if case == 'train' else np.tile(np.arange(n), (B, 1))
    assert np.array_equal(perm, gperm), "permutation"
    assert np.array_equal(out[:, :, 3], golden[f"{case}_heights"]), "heights"
    gp = golden[f"{case}_params"]
    assert np.array_equal(params[:, :3], gp[:, :3]) and _ulp_distance(params[:, 3:], gp[:, 3:]).max() <= 1
    # pos with the reference's own draws: at least as close to float64 as the reference's float32 output
    kw = _kw(DT[CHAIN_OF[case]])
    draws = (torch.from_numpy(gperm.astype(np.int32)) if case == 'train' else None, torch.from_numpy(gp))
    pos = tf(raw, draws=draws).cpu().numpy()
    f64 = R.restate(raw_np, gperm if case == 'train' else None, gp, n, dtype=np.float64, **kw)
    dist = np.abs(pos[:, :, :3].astype(np.float64) - f64[:, :, :3]).max()
    bar = float(golden[f"{case}_dist32"]) + ULP1
    print(f"{case}: device {dist:.3e}, reference float32 {float(golden[f'{case}_dist32']):.3e}")
    assert dist <= bar
    assert np.array_equal(pos[:, :, 3], golden[f"{case}_heights"])
    # and the kernel's arithmetic is the float32 restatement's, bit for bit
    f32 = R.restate(raw_np, gperm if case == 'train' else None, gp, n, dtype=np.float32, **kw)
    assert np.array_equal(pos, f32)


# ------------------------------------------------------------------------------------------------------ device draws
def test_device_draws_properties_and_restatement(dev):
    from adaptpoint_amd.transforms import build_transforms_from_cfg, N_CLOUD_UNIFORMS
    n = 2048
    raw_np = R.golden_clouds(501, B, n)
    raw = torch.from_numpy(raw_np).to(dev)
    tf = build_transforms_from_cfg('train', DT)
    torch.manual_seed(21)
    state = torch.cuda.get_rng_state(dev)
    out, perm, params = tf(raw, device_draws=True, record=True)
    torch.cuda.set_rng_state(state, dev)
    u = torch.rand(B * N_CLOUD_UNIFORMS + B * n, device=dev).cpu().numpy()
    out, perm, params = out.cpu().numpy(), perm.cpu().numpy(), params.cpu().numpy()
    for b in range(B):
        assert np.array_equal(np.sort(perm[b]), np.arange(n)), "a permutation"
    s = params[:, :3]
    assert np.all((s >= np.float32(0.9)) & (s <= np.float32(1.1)))
    Rm = params[:, 3:].reshape(B, 3, 3).astype(np.float64)
    assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
    assert np.abs(np.linalg.det(Rm) - 1).max() < 1e-6
    pos = out[:, :, :3].astype(np.float64)
    assert np.abs(pos.mean(1)).max() < 1e-6
    assert np.abs(np.sqrt((pos ** 2).sum(-1)).max(1) - 1).max() < 1e-6
    assert np.all(out[:, :, 3].min(1) == 0)
    # the restatement fed the same uniforms
    u_cloud = u[:B * N_CLOUD_UNIFORMS].reshape(B, N_CLOUD_UNIFORMS)
    u_point = u[B * N_CLOUD_UNIFORMS:].reshape(B, n)
    rperm, rparams = R.device_params(u_cloud, u_point, scale=[0.9, 1.1], angle=[0.0, 1.0, 0.0])
    assert np.array_equal(perm, rperm)
    assert np.array_equal(params[:, :3], rparams[:, :3]) and _ulp_distance(params[:, 3:], rparams[:, 3:]).max() <= 1
    f32 = R.restate(raw_np, rperm, params, n, dtype=np.float32, **_kw(DT['train']))
    assert np.array_equal(out, f32)


def test_device_draws_mirror_and_isotropic_scale(dev):
    from adaptpoint_amd.transforms import CloudTransform, N_CLOUD_UNIFORMS
    n = 256
    raw_np = R.golden_clouds(502, B, n)
    raw = torch.from_numpy(raw_np).to(dev)
    for kw in (dict(scale=[0.5, 2.0], mirror=[0.5, -1, 0.5]), dict(scale=[0.5, 2.0], anisotropic=False),
               dict(scale=[0.5, 2.0], scale_xyz=[True, False, True])):
        tf = CloudTransform(['PointsToTensor', 'PointCloudScaling'], 'val', **kw)
        torch.manual_seed(5)
        state = torch.cuda.get_rng_state(dev)
        out, _, params = tf(raw, device_draws=True, record=True)
        torch.cuda.set_rng_state(state, dev)
        u = torch.rand(B * N_CLOUD_UNIFORMS + B * n, device=dev).cpu().numpy()
        _, rparams = R.device_params(u[:B * N_CLOUD_UNIFORMS].reshape(B, -1), u[B * N_CLOUD_UNIFORMS:].reshape(B, n),
                                     scale=kw['scale'], anisotropic=kw.get('anisotropic', True),
                                     scale_xyz=kw.get('scale_xyz', (True, True, True)), mirror=kw.get('mirror'))
        assert np.array_equal(params.cpu().numpy()[:, :3], rparams[:, :3]), kw
        f32 = R.restate(raw_np, None, params.cpu().numpy(), n, dtype=np.float32, **_kw(tf.names))
        assert np.array_equal(out.cpu().numpy(), f32), kw
    assert np.any(params.cpu().numpy()[:, 1] == 1)


# ------------------------------------------------------------------------------------------------- rows and limits
def test_rows_gather_nan_rows_raw_untouched_and_repeatable(dev):
    from adaptpoint_amd.transforms import build_transforms_from_cfg
    S, n_raw, n = 6, 2048, 1024
    raw_np = R.golden_clouds(503, S, n_raw)
    raw = torch.from_numpy(raw_np).to(dev)
    before = raw.clone()
    rows = torch.tensor([3, 0, 99, 5, -1, 2], device=dev)
    tf = build_transforms_from_cfg('train', DT, num_points=n)
    np.random.seed(4)
    torch.manual_seed(4)
    out, perm, params = tf(raw, rows, record=True)
    np.random.seed(4)
    torch.manual_seed(4)
    again = tf(raw, rows)
    torch.cuda.synchronize()
    assert torch.equal(raw.view(torch.int32), before.view(torch.int32)), "raw is never written"
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "two runs bit-identical"
    out = out.cpu().numpy()
    bad = [2, 4]
    assert np.isnan(out[bad]).all()
    good = [0, 1, 3, 5]
    assert not np.isnan(out[good]).any()
    f32 = R.restate(raw_np, perm.cpu().numpy()[good], params.cpu().numpy()[good], n, rows=[3, 0, 5, 2],
                    dtype=np.float32, **_kw(DT['train']))
    assert np.array_equal(out[good], f32)
    # device draws: also bit-identical from the same generator state
    torch.manual_seed(8)
    d1 = tf(raw, rows[:2], device_draws=True)
    torch.manual_seed(8)
    d2 = tf(raw, rows[:2], device_draws=True)
    assert torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    assert torch.equal(raw.view(torch.int32), before.view(torch.int32))


def test_limits_raise(dev):
    from adaptpoint_amd.transforms import CloudTransform
    tf = CloudTransform(DT['val'], 'val', gravity_dim=1)
    with pytest.raises(ValueError, match="8192"):
        tf(torch.zeros(2, 8193, 3, device=dev))
    with pytest.raises(ValueError, match="num_points"):
        CloudTransform(DT['val'], 'val', num_points=2048)(torch.zeros(2, 1024, 3, device=dev))
    with pytest.raises(ValueError, match="raw"):
        tf(torch.zeros(2, 1024, 4, device=dev))
    with pytest.raises(ValueError, match="raw"):
        tf(torch.zeros(2, 1024, 3))
    with pytest.raises(ValueError, match="rows"):
        tf(torch.zeros(2, 1024, 3, device=dev), torch.zeros(2, dtype=torch.float32, device=dev))
    big = CloudTransform(DT['val'], 'val', gravity_dim=1)(torch.rand(2, 8192, 3, device=dev))
    assert big.shape == (2, 8192, 4) and torch.isfinite(big).all()


# ------------------------------------------------------------------------------------------------ capture + step
def _classifier(dev):
    from adaptpoint_amd.pointnext import PointNextSClassifier, fill_parameters_by_name
    m = fill_parameters_by_name(PointNextSClassifier(fused=True))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m.to(dev)


def _snapshot(m, o):
    return (copy.deepcopy(m.state_dict()),
            {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.state[p].items()}
             for g in o.param_groups for p in g['params'] if p in o.state})


def _restore(m, o, snap):
    """In place: the captured graph keeps pointing at the same tensors."""
    with torch.no_grad():
        own = m.state_dict()
        for k, v in snap[0].items():
            own[k].copy_(v)
        for g in o.param_groups:
            for p in g['params']:
                if p in o.state:
                    for k, v in snap[1][id(p)].items():
                        if torch.is_tensor(v):
                            o.state[p][k].copy_(v)
        o.zero_grad(set_to_none=False)


def test_device_draw_transform_and_classifier_step_in_one_graph(dev, monkeypatch):
    from adaptpoint_amd import fused, graphs
    from adaptpoint_amd.gan import ClassifierStep
    from adaptpoint_amd.transforms import build_transforms_from_cfg
    monkeypatch.setattr(fused, "DETERMINISTIC", True)
    raw = torch.from_numpy(R.golden_clouds(504, 8, 2048)).to(dev)
    rows = torch.tensor([5, 1, 6, 2], device=dev)
    target = torch.tensor([3, 7, 1, 12], device=dev)
    choice = torch.from_numpy(np.random.RandomState(3).choice(1200, 1024, False).astype(np.int32)).to(dev)
    tf = build_transforms_from_cfg('train', DT)
    C = _classifier(dev)
    opt = torch.optim.AdamW(C.parameters(), lr=2e-3, weight_decay=0.05, capturable=True, fused=True)
    step = ClassifierStep(C, optimizer=opt)

    def run():
        x = tf(raw, rows, device_draws=True)
        _, loss = step(x, target, choice=choice)
        return x, loss

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    snap = _snapshot(C, opt)
    state = torch.cuda.get_rng_state(dev)
    x_e, loss_e = run()
    x_e, loss_e = x_e.clone(), loss_e.clone()
    w_e = copy.deepcopy(C.state_dict())
    _restore(C, opt, snap)
    graph, (x_c, loss_c), census = graphs.capture(run, leaves=list(C.parameters()),
                                                  what="the transform + classifier step graph")
    print("transform + classifier step graph:", census)
    _restore(C, opt, snap)
    torch.cuda.set_rng_state(state, dev)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x_c.view(torch.int32), x_e.view(torch.int32)), "replayed transform"
    assert torch.equal(loss_c, loss_e)
    now = C.state_dict()
    assert all(torch.equal(now[k], w_e[k]) for k in now)
    graph.replay()                                   # a replay draws afresh
    torch.cuda.synchronize()
    assert not torch.equal(x_c, x_e)


def test_classifier_step_wolfmix_matches_composed_iteration(dev, monkeypatch):
    """train_one_epoch_wolfmix's iteration: PointWOLF in place on points[:, :, :3], the RSMix gate and mix, resample,
    the lambda-weighted loss -- against the same calls composed by hand."""
    from adaptpoint_amd import online_aug
    from adaptpoint_amd.gan import ClassifierStep, resample
    from adaptpoint_amd.online_aug import PointWOLF, mixed_loss
    rs = np.random.RandomState(17)
    pts = rs.randn(8, 2048, 3).astype(np.float32) * 0.4
    points = torch.from_numpy(np.concatenate([pts, pts[:, :, 1:2] - pts[:, :, 1:2].min(1, keepdims=True)], -1)).to(dev)
    target = torch.arange(8, device=dev) % 15
    m1 = _classifier(dev)
    m2 = copy.deepcopy(m1)
    pw = PointWOLF()
    cfg = dict(beta=1.0, nsample=512, knn=True, rsmix_prob=0.5)
    seed = next(s for s in range(100) if np.random.RandomState(s).rand() < 0.5)
    seen = []
    real_rsmix = online_aug.rsmix

    def spy(*a, **k):
        res = real_rsmix(*a, **k)
        seen.append(res)
        return res
    monkeypatch.setattr(online_aug, "rsmix", spy)
    with pytest.raises(ValueError, match="two different trainers"):
        ClassifierStep(m1, pointwolf=pw, rsmix=cfg)
    with pytest.raises(ValueError, match="wolfmix"):
        ClassifierStep(m1, pointwolf=pw, wolfmix=dict(pointwolf=pw, rsmix=cfg))
    torch.manual_seed(3)
    np.random.seed(seed)
    p1 = points.clone()
    step = ClassifierStep(m1, optimizer=torch.optim.SGD(m1.parameters(), lr=0.1),
                          wolfmix=dict(pointwolf=pw, rsmix=cfg))
    _, loss = step(p1, target)
    assert len(seen) == 1
    mixed1, lam1, ta1, tb1 = seen[0]
    # composed
    torch.manual_seed(3)
    np.random.seed(seed)
    p2 = points.clone()
    _, p2[:, :, :3] = pw(p2[:, :, :3])
    assert torch.equal(p1, p2), "PointWOLF in place on the caller's points"
    assert np.random.rand(1) < cfg['rsmix_prob']
    mixed2, lam2, ta2, tb2 = real_rsmix(p2, target, beta=1.0, n_sample=512, knn=True)
    assert torch.equal(mixed1, mixed2) and torch.equal(lam1, lam2)
    assert torch.equal(ta1, ta2) and torch.equal(tb1, tb2)
    pos, x = resample(mixed2, 1024, 4)
    m2.train()
    logits = m2({'pos': pos, 'x': x})
    ref = mixed_loss(m2.criterion, logits, ta2, tb2, lam2)
    ref.backward()
    torch.nn.utils.clip_grad_norm_(m2.parameters(), 10.0, norm_type=2)
    torch.optim.SGD(m2.parameters(), lr=0.1).step()
    print(f"wolfmix step: loss {loss.item():.6f} composed {ref.item():.6f}")
    assert abs(loss.item() - ref.item()) < 1e-6
    for (name, a), b in zip(m1.named_parameters(), m2.parameters()):
        assert (a - b).abs().max().item() < 1e-5, name
