"""CPU suite: SimpleView (adaptpoint_amd/simpleview.py) against the REFERENCE's `points2depth`, `PCViews` and `MVModel`
captured in tests/golden/simpleview_golden.npz (tests/golden/make_golden_simpleview.py): the numpy statements the GPU tests
compare the kernel with, the torch composition, the mirror model in training and eval mode, the input generator's margin,
the fallback reasons on CPU tensors, and a reference-named state_dict."""
import os

import numpy as np
import pytest
import torch

import simpleview_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5          # relative L2 per gradient tensor and buffer, as tests/test_pointvit_cpu.py holds them; activations: rtol 1e-5


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "simpleview_golden.npz"))


def _narrow(fused=False, **over):
    from adaptpoint_amd.simpleview import SimpleViewClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return R.no_dropout(fill_parameters_by_name(SimpleViewClassifier(fused=fused, **R.narrow(**over))))


def _cases():
    yield "lattice", R.lattice(), (8, 8, 1, 1), "a/lattice_img", "a/lattice_sw1"
    for k, (H, W, sx, sy, N) in enumerate(R.RANDOM_SHAPES):
        yield f"shape {k}", R.camera_points(R.RANDOM_B, N, k), (H, W, sx, sy), f"a/img{k}", f"a/sw1_{k}"


def test_float32_statement_is_bit_equal_to_the_reference(gold):
    for name, q, (H, W, sx, sy), k_img, k_sw in _cases():
        img, sw = R.points2depth(q, H, W, sx, sy)
        assert np.array_equal(img, gold[k_img]), name
        assert np.array_equal(sw + (sw == 0), gold[k_sw]), name
    assert (R.lattice()[..., 2] < 0).any() and (gold["a/lattice_img"] == 0).any()
    rot, trans = R.view_matrices()
    p = R.clouds(R.NARROW_B, R.NARROW_N, 0, R.NARROW_RES, R.NARROW_RES)
    assert np.array_equal(R.depth_views(p, rot, trans, R.NARROW_RES, R.NARROW_RES)[0], gold["b/img"])


def test_lattice_holds_its_edge_cases():
    q = R.lattice()
    valid, pixel, z, _ = R._splats(q, 8, 8, 1, 1, np.float32)
    assert (pixel[:, :3, 0, 0] == 3 * 8 + 5).all() and valid[:, :3].all()         # three depths on one pixel
    assert not valid[:, 4].any() and not valid[:, 5].any() and not valid[z < 0].any()
    img, sw = R.points2depth(q, 8, 8, 1, 1)
    # exact sums: every weight is 1/4, 1/2, 1 or 2 and every product z w is 1, so sv counts the splats of a pixel
    assert np.array_equal(sw * 4, np.round(sw * 4)) and sw[0].reshape(-1)[3 * 8 + 5] >= 2.75
    count = np.zeros((len(q), 64))
    for b in range(len(q)):
        np.add.at(count[b], pixel[b][valid[b]], 1)
    assert np.array_equal(img, count.reshape(img.shape).astype(np.float32) / (sw + (sw == 0))) and count.max() >= 3
    # the library's composition on the same lattice: the same bits
    from adaptpoint_amd import simpleview as SV
    c_img, c_sw = SV.composed_points2depth(torch.from_numpy(q), 8, 8, 1, 1, with_weight=True)
    assert np.array_equal(c_img.numpy(), img) and np.array_equal(c_sw.numpy(), sw)


def test_float64_statement_is_as_close_as_the_fixture_says(gold):
    for k, (H, W, sx, sy, N) in enumerate(R.RANDOM_SHAPES):
        img64 = R.points2depth(R.camera_points(R.RANDOM_B, N, k), H, W, sx, sy, np.float64)[0]
        err = R.rel(gold[f"a/img{k}"], img64)
        assert err <= 2.0 * float(gold["a/err64"][k]) + 1e-6, (k, err)
    rot, trans = R.view_matrices()
    p = R.clouds(R.NARROW_B, R.NARROW_N, 0, R.NARROW_RES, R.NARROW_RES)
    err = R.rel(gold["b/img"], R.depth_views(p, rot, trans, R.NARROW_RES, R.NARROW_RES, dtype=np.float64)[0])
    assert err <= 2.0 * float(gold["b/err64"]) + 1e-6


def test_composition_is_bit_equal_to_the_statement_on_cpu(gold):
    from adaptpoint_amd import simpleview as SV
    before = dict(SV.COMPOSED_CALLS)
    for name, q, (H, W, sx, sy), k_img, _ in _cases():
        img, sw = SV.composed_points2depth(torch.from_numpy(q), H, W, sx, sy, with_weight=True)
        st_img, st_sw = R.points2depth(q, H, W, sx, sy)
        assert np.array_equal(img.numpy(), st_img) and np.array_equal(sw.numpy(), st_sw), name
        assert np.array_equal(img.numpy(), gold[k_img]), name
        # the public operator on a CPU tensor: the same bits, counted
        assert torch.equal(SV.points2depth(torch.from_numpy(q), H, W, sx, sy), img)
    assert SV.COMPOSED_CALLS.get("cpu tensor", 0) == before.get("cpu tensor", 0) + 1 + len(R.RANDOM_SHAPES)
    assert torch.equal(SV.points2depth(torch.from_numpy(q), H, W, sx, sy, fused=False), img)       # not counted
    assert SV.COMPOSED_CALLS.get("cpu tensor", 0) == before.get("cpu tensor", 0) + 1 + len(R.RANDOM_SHAPES)
    views = SV.PCViews(resolution=R.NARROW_RES)
    p = R.clouds(R.NARROW_B, R.NARROW_N, 0, R.NARROW_RES, R.NARROW_RES)
    assert np.array_equal(views.get_img(torch.from_numpy(p)).numpy(), gold["b/img"])
    assert not SV.supported(torch.from_numpy(p), views.rot_mat, views.translation, 32, 32)
    SV.COMPOSED_CALLS.clear()
    SV.COMPOSED_CALLS.update(before)


def test_composition_gradient_is_the_analytic_statement(gold):
    from adaptpoint_amd import simpleview as SV
    H, W, sx, sy, N = R.RANDOM_SHAPES[R.GRAD_SHAPE]
    q = R.camera_points(R.RANDOM_B, N, R.GRAD_SHAPE)
    g = np.random.default_rng(77).normal(size=(R.RANDOM_B, H, W)).astype(np.float32)
    x = torch.from_numpy(q).requires_grad_(True)
    (SV.composed_points2depth(x, H, W, sx, sy) * torch.from_numpy(g)).sum().backward()
    assert not x.grad[..., :2].any() and x.grad[..., 2].any()                    # exactly zero in x and y
    assert np.array_equal(x.grad.numpy(), gold["a/grad"])
    want = R.points2depth_grad(q, g, H, W, sx, sy)
    assert not want[..., :2].any()
    # float32 rounding: the gradient is a sum of at most sx * sy terms a w (1 - z w + img w), each a handful of roundings
    assert R.rel(x.grad, want) < 16 * sx * sy * 2.0 ** -24
    x64 = torch.from_numpy(q).double().requires_grad_(True)
    (SV.composed_points2depth(x64, H, W, sx, sy) * torch.from_numpy(g).double()).sum().backward()
    assert R.rel(x64.grad, want) < 1e-12
    # six views: the chain through R_v[:, 2]
    rot, trans = R.view_matrices()
    p = R.clouds(2, 16, 3, 16, 16)
    gv = np.random.default_rng(78).normal(size=(12, 16, 16))
    p64 = torch.from_numpy(p).double().requires_grad_(True)
    (SV.composed_depth_views(p64, torch.from_numpy(rot).double(), torch.from_numpy(trans).double(), 16, 16)
     * torch.from_numpy(gv)).sum().backward()
    assert R.rel(p64.grad, R.depth_views_grad(p, rot, trans, gv, 16, 16)) < 1e-12


def test_state_dict_names_and_shapes_are_the_references(gold):
    from adaptpoint_amd.simpleview import MVModel
    m = MVModel()
    got = [(n, ",".join(str(s) for s in t.shape)) for n, t in m.state_dict().items()]
    assert got == list(zip(gold["e/names"].tolist(), gold["e/shapes"].tolist()))
    sd = {n: torch.full([int(s) for s in sh.split(",")] if sh else [], 0.5) for n, sh in got}
    assert not any(m.load_state_dict(sd, strict=True))
    assert float(m.img_model[6][1].conv2.weight.detach()[0, 0, 0, 0]) == 0.5
    assert m.img_model[0].weight.shape == (16, 1, 3, 3) and m.final_fc.model[3].in_features == 6 * 128
    assert m.num_views == 6 and m.resolution == 128 and m.num_classes == 15
    fresh = MVModel(channels=4)
    assert all(not b.bn2.weight.any() for b in fresh.modules() if hasattr(b, "bn2"))     # zero_init_residual


def _check_training(m, gold):
    pos, gt = R.classifier_inputs(0)
    got = R.train_step(m, pos, gt)
    np.testing.assert_allclose(got['logits'].numpy(), gold["c/logits"], rtol=1e-5)
    np.testing.assert_allclose(got['loss'].item(), gold["c/loss"], rtol=1e-5)
    names = [k[len("c/grad/"):] for k in gold.files if k.startswith("c/grad/")]
    assert sorted(names) == sorted(got['grads'])
    errs = {"dpos": R.rel(got['dpos'], gold["c/dpos"])}
    for n in names:
        g = got['grads'][n].reshape(-1)[torch.from_numpy(R.sample_index(n, got['grads'][n].numel()))]
        errs["grad/" + n] = R.rel(g, gold["c/grad/" + n])
    buffers = dict(m.named_buffers())
    for k in gold.files:
        if k.startswith("c/buf/"):
            n = k[len("c/buf/"):]
            if n.endswith("num_batches_tracked"):
                assert int(buffers[n]) == int(gold[k]) == 1, n
            else:
                errs["buf/" + n] = R.rel(buffers[n], gold[k])
    print("worst of %d relative errors: %.1e" % (len(errs), max(errs.values())))
    assert max(errs.values()) < BAR, {k: v for k, v in errs.items() if v >= BAR}


def test_composed_mirror_matches_the_reference_in_training_mode(gold):
    """Logits, loss, every parameter's gradient, dpos and the BatchNorm buffers after the step."""
    _check_training(_narrow().train(), gold)


def test_composed_mirror_matches_the_reference_in_eval_mode(gold):
    pos, _ = R.classifier_inputs(0)
    m = _narrow().eval()
    with torch.no_grad():
        logits = m({'pos': pos})
        assert torch.equal(m.encoder.forward_cls_feat(pos), logits) and torch.equal(m.encoder(pos), logits)
        assert m.encoder.get_img(pos).shape == (R.NARROW_B * 6, 1, R.NARROW_RES, R.NARROW_RES)
    np.testing.assert_allclose(logits.numpy(), gold["d/logits"], rtol=1e-5)


def test_fused_model_on_cpu_tensors_falls_back_counted_and_equals_the_composed():
    from adaptpoint_amd import simpleview as SV
    pos, _ = R.classifier_inputs(0)
    before = dict(SV.COMPOSED_CALLS)
    with torch.no_grad():
        a = _narrow(fused=None).eval()({'pos': pos})
        assert SV.COMPOSED_CALLS.get("cpu tensor", 0) == before.get("cpu tensor", 0) + 1
        b = _narrow(fused=False).eval()({'pos': pos})
        assert SV.COMPOSED_CALLS.get("cpu tensor", 0) == before.get("cpu tensor", 0) + 1
    assert torch.equal(a, b)
    SV.COMPOSED_CALLS.clear()
    SV.COMPOSED_CALLS.update(before)


def test_clouds_keep_every_pixel_decision_away_from_an_integer():
    for (B, N, seed, res) in ((R.NARROW_B, R.NARROW_N, 0, R.NARROW_RES), (4, 64, 1, 128), (2, 200, 2, 32)):
        p = R.clouds(B, N, seed, res, res)
        assert p.shape == (B, N, 3) and p.dtype == np.float32
        assert R.decision_margin(p, res, res).min() >= R.MARGIN
        assert np.linalg.norm(p, axis=-1).max() <= 1.0 + 1e-6
        assert np.array_equal(p, R.clouds(B, N, seed, res, res))
        # with that margin the float32 and float64 statements take the same pixels
        rot, trans = R.view_matrices()
        a = R.depth_views(p, rot, trans, res, res)[1]
        b = R.depth_views(p, rot, trans, res, res, dtype=np.float64)[1]
        assert np.array_equal(a != 0, b != 0)


def test_interface_refusals_and_the_view_table():
    from adaptpoint_amd import simpleview as SV
    with pytest.raises(NotImplementedError):
        SV.MVModel(use_img_transform=True)
    with pytest.raises(NotImplementedError):
        SV.MVModel(backbone='resnet50')
    with pytest.raises(ValueError):
        SV.composed_points2depth(torch.zeros(1, 2, 3), 8, 8, 3, 1)
    views = SV.PCViews()
    assert views.num_views == 6 and views.rot_mat.shape == (6, 3, 3) and views.translation.shape == (6, 1, 3)
    assert not views.rot_mat.is_cuda and SV.TRANS == -1.4
    eye = torch.eye(3).expand(6, 3, 3)
    assert torch.allclose(views.rot_mat @ views.rot_mat.transpose(1, 2), eye, atol=1e-6)
    one = SV.euler2mat(torch.tensor([0.3, -0.2, 0.5]))
    assert one.shape == (3, 3) and torch.allclose(one, SV.euler2mat(torch.tensor([[0.3, -0.2, 0.5]]))[0], atol=1e-7)
    # non-finite coordinates contribute nothing and index nothing
    q = torch.tensor([[[float('nan'), 0.0, 1.0], [0.0, float('inf'), 1.0], [0.1, 0.1, 1.0]]])
    img = SV.composed_points2depth(q, 8, 8, 1, 1)
    assert torch.isfinite(img).all() and int((img != 0).sum()) == 1


def test_every_tensor_handed_to_the_kernel_is_checked_before_a_pointer_is_taken():
    """`rot` and `trans` on another device than the points, of another dtype or of the wrong shape never reach the kernel:
    a counted reason (device, dtype) or a ValueError (shape), decided from metadata alone -- `meta` tensors stand in for
    another device here, nothing is launched."""
    from adaptpoint_amd import simpleview as SV
    views = SV.PCViews()
    p = torch.zeros(2, 8, 3)
    far = lambda t, dt=None: torch.empty(t.shape, dtype=dt or t.dtype, device="meta")
    why = SV._why_composed
    # the natural mistake: PCViews' host matrices beside points of another device
    assert why(far(p), views.rot_mat, views.translation, 32, 32, 1, 1) == "rot / trans on another device than the points"
    assert why(far(p), far(views.rot_mat), views.translation, 32, 32, 1, 1) == "rot / trans on another device than the points"
    assert why(p, far(views.rot_mat), far(views.translation), 32, 32, 1, 1) == "rot / trans on another device than the points"
    assert not SV.supported(far(p), views.rot_mat, views.translation, 32, 32)
    # all on one device: the remaining reasons, in order
    assert why(p, views.rot_mat, views.translation, 32, 32, 1, 1) == "cpu tensor"
    import unittest.mock as mock
    with mock.patch.object(torch.Tensor, "is_cuda", property(lambda self: True)):            # metadata only
        q, rot, trans = far(p), far(views.rot_mat), far(views.translation)
        assert why(q, rot, trans, 32, 32, 1, 1) is None and why(q, None, None, 32, 32, 4, 4) is None
        assert why(q, rot, far(views.translation, torch.float64), 32, 32, 1, 1) == "rot torch.float32 / trans torch.float64"
        assert why(q, far(views.rot_mat, torch.float64), trans, 32, 32, 1, 1) == "rot torch.float64 / trans torch.float32"
        assert why(far(p, torch.float64), rot, trans, 32, 32, 1, 1) == "dtype torch.float64"
        assert why(q, rot, trans, 32, 32, 3, 1) == "splat 3x1"
        assert "bounds" in why(q, rot, trans, 512, 512, 1, 1) and "bounds" in why(far(torch.zeros(1, 8192, 3)), None, None, 8, 8, 4, 4)
        assert "grid" in why(torch.empty(SV.MAX_IMAGES // 6 + 1, 1, 3, device="meta"), rot, trans, 8, 8, 1, 1)
    for bad_rot, bad_trans in ((views.rot_mat[:, :2], views.translation), (views.rot_mat.reshape(6, 9), views.translation),
                               (views.rot_mat, views.translation[:5]), (views.rot_mat, views.translation.reshape(3, 6)),
                               (views.rot_mat, None), (None, views.translation)):
        for fused in (None, False):
            with pytest.raises(ValueError):
                SV.depth_views(p, bad_rot, bad_trans, 8, 8, fused=fused)
    # the public call counts the reason and hands the mismatch to the composition (on real devices torch then raises its
    # own device error: tests/test_gpu_simpleview.py)
    reason = "rot / trans on another device than the points"
    n = SV.COMPOSED_CALLS.get(reason, 0)
    SV.depth_views(p, far(views.rot_mat), far(views.translation), 8, 8)
    assert SV.COMPOSED_CALLS.pop(reason) == n + 1
    if n:
        SV.COMPOSED_CALLS[reason] = n
