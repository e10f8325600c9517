"""CPU: the online augmenters' host side (adaptpoint_amd.online_aug) and the restatements of
tests/online_aug_reference.py against tests/golden/online_aug_golden.npz (tests/golden/make_golden_online_aug.py), and --
where the reference's source tree is present -- against the reference's own PointWOLF_classversion and rsmix."""
import os
import sys

import numpy as np
import pytest
import torch

import online_aug_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "online_aug_golden.npz")
B = 8


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _reference_tree():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden as MG
    return MG.REF


def test_pointwolf_host_draws_are_the_reference_draws(golden):
    """The same torch calls on the CPU default generator in the same order: bit for bit the reference's draws."""
    from adaptpoint_amd.online_aug import PointWOLF
    torch.manual_seed(int(golden["pw_seed"]))
    d = PointWOLF().draw_params(B).numpy()
    assert d.dtype == np.float32 and np.array_equal(d, golden["pw_draws"])
    # and they leave the generator where the reference's call leaves it
    torch.manual_seed(int(golden["pw_seed"]))
    PointWOLF().draw_params(B)
    after = torch.rand(4)
    torch.manual_seed(int(golden["pw_seed"]))
    torch.bernoulli(torch.Tensor(B, 4, 3).uniform_(0, 1)), torch.randint(1, 8, (B, 4))
    for rng in ((-10, 10), (1., 3), (-0.25, 0.25)):
        torch.FloatTensor(B, 4, 3).uniform_(*rng)
    torch.randint(1, 8, (B, 1))
    assert torch.equal(after, torch.rand(4))


def test_pointwolf_restatement_near_golden(golden):
    xyz = np.ascontiguousarray(R.golden_points(int(golden["pw_points_seed"]))[:, :, :3])
    d = np.abs(R.pointwolf_f64(xyz, golden["pw_fidx"], golden["pw_draws"]).numpy() - golden["pw_out"]).max()
    assert d == pytest.approx(float(golden["pw_restatement_dist"]), rel=1e-6) and d < 1e-6


@pytest.mark.parametrize("case", range(4))
def test_rsmix_restatement_equals_golden(golden, case):
    points = R.golden_points(int(golden["rs_points_seed"]))
    np.random.seed(int(golden[f"rs{case}_seed"]))
    out, lam, la, lb, counts = R.rsmix_np(points, golden["rs_label"], 1.0, 512, bool(golden[f"rs{case}_knn"]))
    erased = np.unpackbits(golden[f"rs{case}_erased"], axis=1)[:, :points.shape[1]].astype(bool)
    ref = R.rsmix_reconstruct(points, erased, golden[f"rs{case}_appended"], erased.sum(1))
    assert np.array_equal(out, ref) and np.array_equal(lam, golden[f"rs{case}_lam"])
    assert np.array_equal(lb, golden[f"rs{case}_label_b"]) and np.array_equal(counts, golden[f"rs{case}_counts"])


def test_rsmix_host_draws_follow_the_reference_stream(golden):
    """The package's count-dependent draws (rsmix_picks) consume numpy's stream exactly as the reference's per-cloud
    loop does, whatever the counts."""
    from adaptpoint_amd.online_aug import rsmix_draws, rsmix_picks
    for seed in range(5):
        np.random.seed(seed)
        cut, perm, i1, i2 = rsmix_draws(B, 2048, 1.0)
        counts = np.random.RandomState(seed).randint(0, 40, 2 * B)
        counts[:2] = 0                                    # an empty erase set, an empty add set
        rsmix_picks(counts, B, 2048, 64)
        tail = np.random.rand(3)
        np.random.seed(seed)
        assert np.random.beta(1.0, 1.0) == cut
        assert np.array_equal(np.random.choice(B, B, replace=False), perm)
        np.random.randint(0, 2048, (B, 1)), np.random.randint(0, 2048, (B, 1))
        for c in range(B):
            ne, na = counts[c], counts[B + c]
            if ne == 0:
                continue
            if na == 0:
                np.random.randint(0, 2048 - ne, size=ne)
            elif ne > na:
                np.random.randint(0, na, size=ne - na)
            elif ne < na:
                np.random.choice(np.arange(na) * 3, size=ne, replace=False)
        assert np.array_equal(tail, np.random.rand(3))


@pytest.mark.skipif(not os.path.isdir(_reference_tree()), reason="the reference's source tree is not present")
def test_restatements_equal_the_reference_on_cpu(golden):
    # the reference is imported in memory behind stub modules: leave the interpreter as it was for the tests after this
    saved_modules, saved_path = dict(sys.modules), list(sys.path)
    saved_tb = getattr(torch.utils, "tensorboard", None)
    try:
        _compare_with_reference(golden)
    finally:
        for k in [k for k in sys.modules if k not in saved_modules]:
            del sys.modules[k]
        sys.modules.update(saved_modules)
        sys.path[:] = saved_path
        if saved_tb is None:
            torch.utils.__dict__.pop("tensorboard", None)
        else:
            torch.utils.tensorboard = saved_tb


def _compare_with_reference(golden):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_online_aug as MO
    ref_pw, ref_rs = MO.import_online_aug()
    from oracle import oracle as O
    xyz = np.ascontiguousarray(R.golden_points(int(golden["pw_points_seed"]) + 1)[:, :, :3])
    out, draws = MO.record_pointwolf(ref_pw, xyz, 7)
    assert np.abs(R.pointwolf_f64(xyz, O.furthest_point_sampling(xyz, 4), draws).numpy() - out).max() < 1e-6
    points = R.golden_points(int(golden["rs_points_seed"]) + 1, B=6, N=1500)
    label = np.arange(6).reshape(6, 1)
    for knn in (False, True):
        for seed in (3, 4):
            np.random.seed(seed)
            ref = ref_rs.rsmix(points.copy(), label.copy(), beta=1.0, n_sample=256, KNN=knn)
            np.random.seed(seed)
            got = R.rsmix_np(points, label, 1.0, 256, knn)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1].astype(np.float32))
            assert np.array_equal(got[3], np.asarray(ref[3]).reshape(-1))
