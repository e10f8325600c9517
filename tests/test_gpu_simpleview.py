"""SimpleView on the GPU (adaptpoint_amd/simpleview.py over csrc/depth_views.hip).  The rasteriser is BIT-EQUAL to the
float32 numpy statement of tests/simpleview_reference.py (itself bit-equal to the reference: tests/test_simpleview_cpu.py)
on the exact lattice, at every splat size and at the tails of its loops; against the torch composition on the GPU and
float64,

    || fused - f64 || <= 4 || composed - f64 || + 2e-6 || f64 ||       images, dpoints; logits, loss, every gradient

with no call falling back; forward + backward capture without a memset node and replay the same bits; the narrow
`SimpleViewClassifier` through `ClassifierStep`, `Evaluator` and `feedback_loss`."""
import gc

import numpy as np
import pytest
import torch

import simpleview_reference as R

pytestmark = pytest.mark.gpu
RES = R.NARROW_RES


def _fallbacks():
    from adaptpoint_amd import simpleview as SV
    return dict(SV.COMPOSED_CALLS)


def _p2d(dev, q, H, W, sx, sy):
    from adaptpoint_amd import simpleview as SV
    img, sw = SV.points2depth(torch.from_numpy(q).to(dev), H, W, sx, sy, with_weight=True)
    return img.cpu().numpy(), sw.cpu().numpy()


def _views(dev, p, H, W):
    from adaptpoint_amd import simpleview as SV
    rot, trans = R.view_matrices()
    img, sw = SV.depth_views(torch.from_numpy(p).to(dev), torch.from_numpy(rot).to(dev), torch.from_numpy(trans).to(dev),
                             H, W, with_weight=True)
    return img.cpu().numpy(), sw.cpu().numpy()


def _bit_equal(got, want, what):
    for g, w, name in zip(got, want, ("img", "sw")):
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, name, int((g != w).sum()))


def _within(fused_err, composed_err, norm, what):
    print(f"{what}: fused {fused_err:.3e} composed {composed_err:.3e} norm {norm:.3e}")
    assert fused_err <= 4 * composed_err + 2e-6 * norm, (what, fused_err, composed_err, norm)


@pytest.fixture(scope="module")
def gold():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simpleview_golden.npz"))


def test_exact_lattice_is_bit_equal(dev, gold):
    before = _fallbacks()
    q = R.lattice(B=3, N=48, H=8, W=8)
    assert (q[..., 2] < 0).any()
    got = _p2d(dev, q, 8, 8, 1, 1)
    _bit_equal(got, R.points2depth(q, 8, 8, 1, 1), "lattice")
    assert np.array_equal(got[0], gold["a/lattice_img"]) and np.array_equal(got[1] + (got[1] == 0), gold["a/lattice_sw1"])
    assert _fallbacks() == before


@pytest.mark.parametrize("sx,sy", [(1, 1), (2, 4), (4, 4)])
def test_every_splat_size_is_bit_equal(dev, gold, sx, sy):
    before = _fallbacks()
    q = R.camera_points(3, 50, 3)
    got = _p2d(dev, q, 12, 20, sx, sy)
    _bit_equal(got, R.points2depth(q, 12, 20, sx, sy), (sx, sy))
    if (sx, sy) == (2, 4):
        assert R.RANDOM_SHAPES[3] == (12, 20, 2, 4, 50) and np.array_equal(got[0], gold["a/img3"])
    assert (got[0] != 0).any() and _fallbacks() == before


@pytest.mark.parametrize("n", [1, 63, 65])
def test_point_count_tails_are_bit_equal(dev, n):
    before = _fallbacks()
    q = R.camera_points(2, n, 10 + n)
    q[:, 0, 2] = np.abs(q[:, 0, 2])
    _bit_equal(_p2d(dev, q, 16, 16, 1, 1), R.points2depth(q, 16, 16, 1, 1), n)
    _bit_equal(_p2d(dev, q, 16, 16, 2, 2), R.points2depth(q, 16, 16, 2, 2), (n, 2))
    assert _fallbacks() == before


def test_image_count_and_large_image_tails_are_bit_equal(dev):
    before = _fallbacks()
    rot, trans = R.view_matrices()
    p = R.clouds(5, 33, 4, 16, 16)                                           # B * V = 30 images
    _bit_equal(_views(dev, p, 16, 16), R.depth_views(p, rot, trans, 16, 16), "B = 5, V = 6")
    p = R.clouds(4, 64, 1, 128, 128)
    got = _views(dev, p, 128, 128)
    _bit_equal(got, R.depth_views(p, rot, trans, 128, 128), "128 x 128")
    assert (got[0] != 0).sum() > 4 * 6 * 20 and _fallbacks() == before


def test_one_pixel_holding_every_point_is_bit_equal(dev):
    """A run of 200 keys walked by one thread: the sums in ascending point order."""
    before = _fallbacks()
    z = np.random.default_rng(9).uniform(0.3, 2.5, size=(1, 200))
    q = np.stack([0.1 * z, 0.2 * z, z], -1).astype(np.float32)
    want = R.points2depth(q, 16, 16, 1, 1)
    assert (want[1] != 0).sum() == 1
    _bit_equal(_p2d(dev, q, 16, 16, 1, 1), want, "one pixel")
    flipped = np.ascontiguousarray(q[:, ::-1])
    _bit_equal(_p2d(dev, flipped, 16, 16, 1, 1), R.points2depth(flipped, 16, 16, 1, 1), "one pixel, reversed")
    assert _fallbacks() == before


@pytest.fixture(scope="module")
def six(dev):
    """The fixture's clouds under the six views: kernel, composition on the GPU, float32 and float64 statements."""
    from adaptpoint_amd import simpleview as SV
    rot, trans = R.view_matrices()
    p = R.clouds(R.NARROW_B, R.NARROW_N, 0, RES, RES)
    before = _fallbacks()
    fused = _views(dev, p, RES, RES)
    fell_back = _fallbacks() != before
    t = [torch.from_numpy(a).to(dev) for a in (p, rot, trans)]
    composed = SV.depth_views(*t, RES, RES, fused=False).cpu().numpy()
    return dict(p=p, rot=rot, trans=trans, t=t, fused=fused, composed=composed, fell_back=fell_back,
                st32=R.depth_views(p, rot, trans, RES, RES), st64=R.depth_views(p, rot, trans, RES, RES, dtype=np.float64))


def test_six_views_bit_equal_and_against_the_composition(six, gold):
    assert not six['fell_back']
    _bit_equal(six['fused'], six['st32'], "six views")
    assert np.array_equal(six['fused'][0], gold["b/img"])
    ref = six['st64'][0]
    assert np.array_equal(six['fused'][0] != 0, six['composed'] != 0) and np.array_equal(ref != 0, six['composed'] != 0)
    _within(np.linalg.norm(six['fused'][0] - ref), np.linalg.norm(six['composed'] - ref), np.linalg.norm(ref), "six views")


def _backward_case(dev, p, rot, trans, H, W, sx, sy, seed):
    """dpoints of sum(g * img): kernel (twice), composition on the GPU, float64 autograd of the composition (CPU)."""
    from adaptpoint_amd import simpleview as SV
    V = 1 if rot is None else rot.shape[0]
    g = np.random.default_rng(seed).normal(size=(p.shape[0] * V, H, W)).astype(np.float32)

    def run(device, dtype, fused):
        x = torch.from_numpy(p).to(device=device, dtype=dtype).requires_grad_(True)
        gg = torch.from_numpy(g).to(device=device, dtype=dtype)
        if rot is None:
            img = SV.points2depth(x, H, W, sx, sy, fused=fused)
        else:
            img = SV.depth_views(x, torch.from_numpy(rot).to(device=device, dtype=dtype),
                                 torch.from_numpy(trans).to(device=device, dtype=dtype), H, W, sx, sy, fused=fused)
        (img * gg).sum().backward()
        return x.grad.detach().cpu()
    before = _fallbacks()
    a, b = run(dev, torch.float32, None), run(dev, torch.float32, None)
    assert _fallbacks() == before
    return a, b, run(dev, torch.float32, False), run("cpu", torch.float64, False), g


def test_host_matrices_beside_device_points_never_reach_the_kernel(dev):
    """`PCViews().rot_mat` lives on the host: with device points the call is counted and torch raises its own error."""
    from adaptpoint_amd import simpleview as SV
    views = SV.PCViews()
    before = _fallbacks()
    with pytest.raises(RuntimeError):
        SV.depth_views(torch.zeros(2, 8, 3, device=dev), views.rot_mat, views.translation, 8, 8)
    why = "rot / trans on another device than the points"
    assert _fallbacks().get(why, 0) == before.get(why, 0) + 1
    SV.COMPOSED_CALLS.clear()
    SV.COMPOSED_CALLS.update(before)


def test_backward_six_views(dev, six):
    a, b, comp, ref, g = _backward_case(dev, six['p'], six['rot'], six['trans'], RES, RES, 1, 1, 31)
    assert torch.equal(a, b) and torch.isfinite(a).all() and bool(a.any())
    assert R.rel(ref, R.depth_views_grad(six['p'], six['rot'], six['trans'], g, RES, RES)) < 1e-10
    _within(float((a.double() - ref).norm()), float((comp.double() - ref).norm()), float(ref.norm()), "dpoints, six views")


def test_backward_camera_frame_4x4(dev):
    H, W, sx, sy, N = R.RANDOM_SHAPES[R.GRAD_SHAPE]
    q = R.camera_points(R.RANDOM_B, N, R.GRAD_SHAPE)
    a, b, comp, ref, g = _backward_case(dev, q, None, None, H, W, sx, sy, 77)
    assert torch.equal(a, b) and (sx, sy) == (4, 4)
    assert not a[..., :2].any() and bool(a[..., 2].any())                      # x and y of the camera frame: exactly zero
    assert np.array_equal(a[..., :2].numpy().view(np.uint32), np.zeros((R.RANDOM_B, N, 2), np.uint32))
    assert R.rel(ref, R.points2depth_grad(q, g, H, W, sx, sy)) < 1e-10
    _within(float((a.double() - ref).norm()), float((comp.double() - ref).norm()), float(ref.norm()), "dpoints, 4 x 4")


def test_forward_and_backward_capture_without_a_memset_and_replay_the_same_bits(dev, six):
    from adaptpoint_amd import graphs
    from adaptpoint_amd import simpleview as SV
    before = _fallbacks()
    p, rot, trans = (t.clone() for t in six['t'])
    p.requires_grad_(True)
    g = torch.from_numpy(np.random.default_rng(5).normal(size=(R.NARROW_B * 6, RES, RES)).astype(np.float32)).to(dev)

    def run():
        img, sw = SV.depth_views(p, rot, trans, RES, RES, with_weight=True)
        (dp,) = torch.autograd.grad(img, [p], grad_outputs=g)
        return [img.detach(), sw, dp]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up: allocator pools, the kernel's LDS attribute
        eager = [t.clone() for t in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(run, leaves=[p], what="depth_views forward + backward")
    print("depth_views graph:", census)
    assert census.get("memset", 0) == 0 and census.get("kernel", 0) >= 2 and _fallbacks() == before
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in captured)
        assert all(torch.equal(a, b) for a, b in zip(eager, captured))


# ------------------------------------------------------------------ the model
def _model(dev, fused):
    from adaptpoint_amd.simpleview import SimpleViewClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return R.no_dropout(fill_parameters_by_name(SimpleViewClassifier(fused=fused, **R.narrow()))).to(dev)


@pytest.fixture(scope="module")
def step(dev):
    """One training step of the fused and of the composed model on the same inputs, and the module run in float64."""
    pos, gt = R.classifier_inputs(0)
    before = _fallbacks()
    res = dict(pos=pos.to(dev), gt=gt.to(dev))
    res['fused'] = R.train_step(_model(dev, True).train(), res['pos'], res['gt'])
    res['fell_back'] = _fallbacks() != before
    res['composed'] = R.train_step(_model(dev, False).train(), res['pos'], res['gt'])
    res['ref'] = R.run64(_model("cpu", False).train(), pos, gt)
    return res


def test_classifier_against_float64(step):
    ref, fused, comp = step['ref'], step['fused'], step['composed']
    assert not step['fell_back']
    for name in ('logits', 'loss', 'dpos'):
        f, c = (float((r[name].double().cpu() - ref[name]).norm()) for r in (fused, comp))
        _within(f, c, float(ref[name].norm()), name)
    assert sorted(ref['grads']) == sorted(fused['grads'])
    for n, g64 in ref['grads'].items():
        f, c = (float((r['grads'][n].double().cpu() - g64).norm()) for r in (fused, comp))
        _within(f, c, float(g64.norm()), n)


def test_eval_logits_against_float64(dev, step):
    before = _fallbacks()
    with torch.no_grad():
        a = _model(dev, True).eval()({'pos': step['pos']})
        b = _model(dev, False).eval()({'pos': step['pos']})
    ref = R.run64(_model("cpu", False), step['pos'].cpu(), training=False)['logits']
    assert _fallbacks() == before
    _within(float((a.double().cpu() - ref).norm()), float((b.double().cpu() - ref).norm()), float(ref.norm()), "eval logits")


def test_two_training_steps_bit_identical_is_recorded_not_promised(dev, step):
    """The image layers' backward is MIOpen's: whole-step reproducibility is printed, not asserted.  The rasteriser's
    own outputs are (test_backward_*)."""
    before = _fallbacks()
    again = R.train_step(_model(dev, True).train(), step['pos'], step['gt'])
    assert _fallbacks() == before
    differ = [n for n, g in again['grads'].items() if not torch.equal(g, step['fused']['grads'][n])]
    print("two whole training steps bit-identical:", torch.equal(again['logits'], step['fused']['logits']) and not differ
          and torch.equal(again['dpos'], step['fused']['dpos']), "; gradients that differ:", differ[:4])
    assert torch.isfinite(again['loss'])


def test_plugs_into_the_classifier_step_the_evaluator_and_the_feedback_loss(dev, step):
    from adaptpoint_amd import evaluate as E
    from adaptpoint_amd.gan import ClassifierStep, feedback_loss
    from adaptpoint_amd.synthetic import unit_sphere_cloud
    from adaptpoint_amd.transforms import CloudTransform
    before = _fallbacks()
    pos, gt = step['pos'], step['gt']
    height = pos[:, :, 1:2] - pos[:, :, 1:2].min(1, keepdim=True)[0]
    points = torch.cat([pos, height], -1).contiguous()                   # (B, N, 4): N <= npoints, nothing is resampled
    m = _model(dev, True)
    weights = {n: q.detach().clone() for n, q in m.named_parameters()}
    logits, loss = ClassifierStep(m)(points, gt)
    assert torch.isfinite(logits).all() and torch.isfinite(loss) and logits.shape == (R.NARROW_B, 15)
    assert all(torch.isfinite(q).all() for q in m.parameters())
    assert any(not torch.equal(q, weights[n]) for n, q in m.named_parameters())       # the optimizer stepped
    _within(float((logits.double().cpu() - step['ref']['logits']).norm()),
            float((step['composed']['logits'].double().cpu() - step['ref']['logits']).norm()),
            float(step['ref']['logits'].norm()), "ClassifierStep logits")

    S = 8
    cloud = torch.from_numpy(unit_sphere_cloud(S, R.NARROW_N, 77)).to(dev)
    labels = torch.randint(0, 15, (S,), generator=torch.Generator().manual_seed(77)).to(dev)
    ev = E.Evaluator(m, CloudTransform(['PointsToTensor', 'PointCloudCenterAndNormalize'], 'val', gravity_dim=1),
                     batch_size=S, num_points=R.NARROW_N, capture=False, keep_pred=True)
    macc, oa, accs, cm = ev.validate(cloud, labels)
    assert np.isfinite(macc) and np.isfinite(oa) and int(cm.value.sum()) == S

    x = points[:, :, :4].transpose(1, 2).contiguous()
    fake_pos = (pos * 1.05).detach().requires_grad_(True)
    fake = {'pos': fake_pos, 'x': torch.cat([fake_pos, height], -1).transpose(1, 2).contiguous()}
    fb, _, _ = feedback_loss(m, m.criterion, {'pos': pos, 'x': x}, fake, gt, 3.0, frozen=True)
    fb.backward()
    assert torch.isfinite(fb) and torch.isfinite(fake_pos.grad).all() and bool(fake_pos.grad.any())
    assert all(q.grad is None or not q.grad.any() for q in m.parameters())             # frozen: the inputs alone
    assert _fallbacks() == before
