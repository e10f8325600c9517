"""CPU: adaptpoint_amd.transforms' chain parsing and host draws against the reference's own draws
(tests/golden/transforms_golden.npz, tests/golden/make_golden_transforms.py), and the golden's compact form."""
import os

import numpy as np
import pytest
import torch

import transforms_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
DT = {'train': ['PointsToTensor', 'PointCloudScaling', 'PointCloudCenterAndNormalize', 'PointCloudRotation'],
      'vote': ['PointCloudRotation'],
      'val': ['PointsToTensor', 'PointCloudCenterAndNormalize'],
      'kwargs': {'scale': [0.9, 1.1], 'angle': [0.0, 1.0, 0.0], 'gravity_dim': 1}}
CHAIN_OF = {'train': 'train', 'val': 'val', 'c': 'val', 'vote': 'vote'}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "transforms_golden.npz"))


def _ulp_distance(a, b):
    return np.abs(R._ordered(np.asarray(a, np.float32)) - R._ordered(np.asarray(b, np.float32)))


@pytest.mark.parametrize("case", ["train", "val", "c", "vote"])
def test_draw_params_equal_the_reference_draws(golden, case):
    from adaptpoint_amd.transforms import build_transforms_from_cfg
    split = 'train' if case == 'train' else 'val'
    tf = build_transforms_from_cfg(CHAIN_OF[case], DT)
    tf.split, tf.shuffle = split, split == 'train'
    n = int(golden[f"{case}_n"])
    np.random.seed(int(golden[f"{case}_np_seed"]))
    torch.manual_seed(int(golden[f"{case}_torch_seed"]))
    perm, params = tf.draw_params(8, n)
    want = golden[f"{case}_params"]
    if case == 'train':
        assert np.array_equal(perm.numpy(), golden["train_perm"].astype(np.int64))
    else:
        assert perm is None
    assert np.array_equal(params[:, :3].numpy(), want[:, :3]), "scale"
    assert _ulp_distance(params[:, 3:].numpy(), want[:, 3:]).max() <= 1, "R within 1 float32 ulp of expm's"
    # the draws leave numpy's stream where the reference's leave it
    st = np.random.get_state()
    np.random.seed(int(golden[f"{case}_np_seed"]))
    for _ in range(8):
        if case == 'train':
            np.random.shuffle(np.zeros((n, 3), np.float32))
        if tf.rotation:
            for _ in range(3):
                np.random.uniform(-1, 1)
            np.random.shuffle([0, 1, 2])
    assert np.array_equal(st[1], np.random.get_state()[1]) and st[2] == np.random.get_state()[2]


def test_arange_shuffle_is_the_row_shuffle():
    """np.random.shuffle of arange(n) gives the permutation that shuffling the (n,3) rows applies, and leaves numpy's
    state where the row shuffle leaves it (what draw_params relies on)."""
    rows = np.random.RandomState(0).randn(2048, 3).astype(np.float32)
    for seed in (0, 1, 12345):
        np.random.seed(seed)
        order = np.arange(2048)
        np.random.shuffle(order)
        after = np.random.get_state()
        np.random.seed(seed)
        shuffled = rows.copy()
        np.random.shuffle(shuffled)
        assert np.array_equal(shuffled, rows[order])
        st = np.random.get_state()
        assert np.array_equal(after[1], st[1]) and after[2] == st[2]


def test_closed_form_axis_rotation_is_expm():
    """PointCloudRotation.M is scipy's expm of the skew matrix; the closed form equals its power series."""
    from adaptpoint_amd.transforms import axis_rotation
    for axis in range(3):
        for theta in (0.0, 0.3, -2.5, np.pi):
            e = np.zeros(3)
            e[axis] = 1
            K = np.cross(np.eye(3), e * theta)
            term, series = np.eye(3), np.eye(3)
            for k in range(1, 40):
                term = term @ K / k
                series = series + term
            assert np.abs(axis_rotation(axis, theta) - series).max() < 1e-14


def test_chain_parsing():
    from adaptpoint_amd.transforms import CloudTransform, build_transforms_from_cfg, PERMUTE, SCALE, HEIGHTS_SCALED, \
        CENTER, NORMALIZE, ROTATE, UNIFORM, ANISOTROPIC
    tr = build_transforms_from_cfg('train', DT, num_points=1024)
    assert tr.flags() == PERMUTE | SCALE | ANISOTROPIC | HEIGHTS_SCALED | CENTER | NORMALIZE | ROTATE
    assert tr.flags(device_draws=True) & UNIFORM and tr.num_points == 1024 and tr.heights_dim() == 1
    va = build_transforms_from_cfg('val', DT)
    assert va.flags() == HEIGHTS_SCALED | CENTER | NORMALIZE and not va.shuffle
    vo = build_transforms_from_cfg('vote', DT, dataset_gravity_dim=2)
    assert vo.flags() == ROTATE and vo.heights_dim() == 2          # no CenterAndNormalize: the dataset's axis
    assert build_transforms_from_cfg('test', DT) is None
    assert build_transforms_from_cfg('train', {'train': []}) is None
    # CenterAndNormalize's own default axis is 2, as in the reference, when the cfg gives none
    assert CloudTransform(['PointCloudCenterAndNormalize'], 'val').heights_dim() == 2
    assert CloudTransform(['PointCloudCenterAndNormalize'], 'val', centering=False).flags() == HEIGHTS_SCALED | NORMALIZE


@pytest.mark.parametrize("names, what", [
    (['PointsToTensor', 'PointCloudJitter'], 'PointCloudJitter'),
    (['PointCloudTranslation'], 'PointCloudTranslation'),
    (['PointCloudRotation', 'PointCloudScaling'], 'PointCloudScaling'),
    (['PointsToTensor', 'PointsToTensor'], 'PointsToTensor'),
])
def test_chain_rejections(names, what):
    from adaptpoint_amd.transforms import CloudTransform
    with pytest.raises(NotImplementedError, match=what):
        CloudTransform(names, 'train')


def test_append_xyz_is_rejected():
    from adaptpoint_amd.transforms import CloudTransform
    with pytest.raises(NotImplementedError, match="append_xyz"):
        CloudTransform(['PointsToTensor', 'PointCloudCenterAndNormalize'], 'val', append_xyz=True)


def test_packed_draw_layout():
    """(perm (B,n) int32 | None, params (B,12) float32 = scale (3) | R row-major (9)); a chain without a transform
    leaves its part at the identity."""
    from adaptpoint_amd.transforms import CloudTransform
    tf = CloudTransform(DT['train'], 'train', **DT['kwargs'])
    np.random.seed(1)
    torch.manual_seed(1)
    perm, params = tf.draw_params(3, 100)
    assert perm.dtype == torch.int32 and perm.shape == (3, 100) and params.dtype == torch.float32
    assert params.shape == (3, 12)
    for b in range(3):
        assert sorted(perm[b].tolist()) == list(range(100))
        s = params[b, :3].numpy()
        assert np.all((s >= 0.9) & (s <= 1.1)) and len(set(s.tolist())) == 3
        Rm = params[b, 3:].reshape(3, 3).numpy().astype(np.float64)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-6
        assert Rm[1, 1] == 1.0 and Rm[0, 1] == 0 and Rm[1, 0] == 0       # angle [0, 1, 0]: about y only
    iso = CloudTransform(['PointCloudScaling'], 'val', scale=[0.5, 2.0], anisotropic=False)
    _, p = iso.draw_params(2, 10)
    p = p.numpy()
    assert np.all(p[:, 0] == p[:, 1]) and np.all(p[:, 1] == p[:, 2])
    assert np.array_equal(p[:, 3:], np.tile(np.eye(3, dtype=np.float32).reshape(-1), (2, 1)))
    rot = CloudTransform(['PointCloudRotation'], 'val', angle=[0, 1, 0])
    _, p = rot.draw_params(2, 10)
    assert np.all(p[:, :3].numpy() == 1)


def test_golden_compact_form_round_trips(golden):
    """The golden holds the reference's pos as ulp offsets from the float64 restatement: rebuilt, its distance to the
    restatement is the recorded one, and its heights are the float32 restatement's."""
    for case in ("train", "val", "c", "vote"):
        n = int(golden[f"{case}_n"])
        raw = R.golden_clouds(int(golden[f"{case}_cloud_seed"]), 8, n)
        perm = golden["train_perm"].astype(np.int64) if case == "train" else None
        names = DT[CHAIN_OF[case]]
        cn = 'PointCloudCenterAndNormalize' in names
        kw = dict(scale='PointCloudScaling' in names, heights_scaled=cn, center=cn, normalize=cn,
                  rotate='PointCloudRotation' in names, gravity_dim=1)
        f64 = R.restate(raw, perm, golden[f"{case}_params"], n, dtype=np.float64, **kw)
        f32 = R.restate(raw, perm, golden[f"{case}_params"], n, dtype=np.float32, **kw)
        pos = R.from_ulp_offsets(golden[f"{case}_pos_ulps"].astype(np.int64), f64[:, :, :3])
        assert np.abs(pos.astype(np.float64) - f64[:, :, :3]).max() == float(golden[f"{case}_dist32"])
        assert np.array_equal(golden[f"{case}_heights"], f32[:, :, 3])
        # the kernel's float32 arithmetic is at least as close to float64 as the reference's
        assert np.abs(f32[:, :, :3].astype(np.float64) - f64[:, :, :3]).max() <= float(golden[f"{case}_dist32"]) + \
            np.spacing(np.float32(1))
