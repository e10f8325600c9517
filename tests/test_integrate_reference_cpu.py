"""CPU test: the zero-edit opt-in `adaptpoint_amd.integrate.patch_openpoints()` against what the reference's own classes
compute, recorded in tests/golden/integrate_reference_golden.npz (G19, `python tests/golden/make_golden.py integrate`:
the reference's SetAbstraction / PointsetGrouper / Anchor_selfattention / ConvBNReLU1D run by their own forwards over
the oracle operators -- initial state_dicts, outputs, gradients, state_dicts after the pass).  Here stand-in classes with
the reference's constructor-time layout (the golden's state_dict keys are asserted) take those initial weights and are
patched as the reference's classes are.  After the patch they keep their parameters and state_dict keys, their forwards
dispatch into adaptpoint_amd (on CPU tensors the package's host-side mirrors over the oracle stand in for the fused
kernels), and the results equal the reference's recorded ones."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "integrate_reference_golden.npz")


def furthest_point_sample(xyz, npoint):
    from adaptpoint_amd.layers import furthest_point_sample as fps
    return fps(xyz, npoint)


def _stand_in_reference_modules():
    """Two modules named like the reference's, holding classes with the reference's constructor-time attributes.  The
    forwards a patched tree can still reach (SetAbstraction configurations outside the fused path, ConvBNReLU1D on CPU
    tensors) compute what the reference's do; the other two are replaced by the patch whole."""
    from adaptpoint_amd.layers import BallGrouper
    pn = types.ModuleType("openpoints.models.backbone.pointnext")
    gen = types.ModuleType("openpoints.models_adaptpoint.generator_component4_15")

    class QueryAndGroup(nn.Module):
        def __init__(self, radius, nsample, normalize_dp=False):
            super().__init__()
            self.radius, self.nsample, self.normalize_dp = radius, nsample, normalize_dp
            self.normalize_by_std, self.normalize_by_allstd, self.normalize_by_allstd2 = False, False, False
            self.relative_xyz, self.return_only_idx = True, False

    class SetAbstraction(nn.Module):
        def __init__(self, cin, cout, layers=1, stride=1, radius=0.15, nsample=32, normalize_dp=False,
                     feature_type='dp_fj', use_res=False, is_head=False):
            super().__init__()
            self.stride, self.is_head, self.all_aggr = stride, is_head, not is_head and stride == 1
            self.use_res = use_res and not self.all_aggr and not is_head
            self.feature_type = feature_type
            mid = cout // 2 if stride > 1 else cout
            chans = [cin if is_head else 3 + cin] + [mid] * (layers - 1) + [cout]
            if self.use_res:
                self.skipconv = nn.Sequential(nn.Conv1d(cin, cout, 1))
                self.act = nn.ReLU(inplace=True)
            convs = []
            for i in range(len(chans) - 1):
                if is_head:
                    convs.append(nn.Sequential(nn.Conv1d(chans[i], chans[i + 1], 1)))
                    continue
                blk = [nn.Conv2d(chans[i], chans[i + 1], 1, bias=False), nn.BatchNorm2d(chans[i + 1])]
                if not (i == len(chans) - 2 and self.use_res):
                    blk.append(nn.ReLU(inplace=True))
                convs.append(nn.Sequential(*blk))
            self.convs = nn.Sequential(*convs)
            if not is_head:
                self.grouper = QueryAndGroup(radius, nsample, normalize_dp)
                self.sample_fn = furthest_point_sample

        def forward(self, pf):
            p, f = pf
            if self.is_head:
                return p, self.convs(f)
            idx = self.sample_fn(p, p.shape[1] // self.stride).long()
            new_p = torch.gather(p, 1, idx.unsqueeze(-1).expand(-1, -1, 3))
            fi = torch.gather(f, -1, idx.unsqueeze(1).expand(-1, f.shape[1], -1))
            dp, fj = BallGrouper(self.grouper.radius, self.grouper.nsample, self.grouper.normalize_dp)(new_p, p, f)
            if self.feature_type == 'dp_df':
                fj = fj - fi.unsqueeze(-1)
            out = self.convs(torch.cat([dp, fj], 1)).max(-1)[0]
            if self.use_res:
                out = self.act(out + self.skipconv(fi))
            return new_p, out

    class ConvBNReLU1D(nn.Module):
        def __init__(self, cin, cout, bias=False):
            super().__init__()
            self.act = nn.ReLU(inplace=True)
            self.net = nn.Sequential(nn.Conv1d(cin, cout, 1, bias=bias), nn.BatchNorm1d(cout), self.act)

        def forward(self, x):
            return self.net(x)

    class PointsetGrouper(nn.Module):
        def __init__(self, channel, reduce, kneighbors, radi):
            super().__init__()
            self.reduce, self.kneighbors, self.radi, self.normalize = reduce, kneighbors, radi, "anchor"
            self.affine_alpha = nn.Parameter(torch.ones([1, 1, 1, channel]))
            self.affine_beta = nn.Parameter(torch.zeros([1, 1, 1, channel]))

        def forward(self, xyz, points):
            raise AssertionError("the patch replaces this forward")

    class Anchor_selfattention(nn.Module):
        def __init__(self, dim, head_num):
            super().__init__()
            self.dim, self.head_num, self.head_dim = dim, head_num, dim // head_num
            self.to_qkv = nn.Linear(dim, dim * 3, bias=False)
            self.pos_embedding = nn.Sequential(nn.Conv1d(3, dim, 1), nn.BatchNorm1d(dim))
            self.res = nn.Sequential(nn.Conv1d(dim, dim, 1), nn.BatchNorm1d(dim))

        def forward(self, x, xyz=None):
            raise AssertionError("the patch replaces this forward")
    pn.SetAbstraction = SetAbstraction
    gen.ConvBNReLU1D, gen.PointsetGrouper, gen.Anchor_selfattention = ConvBNReLU1D, PointsetGrouper, Anchor_selfattention
    return pn, gen


@pytest.fixture
def golden_g19():
    return np.load(GOLDEN)


def _state_from(golden, k, stage):
    prefix = f"{k}_{stage}."
    return {n[len(prefix):]: torch.from_numpy(golden[n]) for n in golden.files if n.startswith(prefix)}


def test_patched_reference_classes_dispatch_to_this_package_and_agree(golden_g19, cpu_mirrors, monkeypatch):
    import golden_inputs as GI
    from adaptpoint_amd import integrate
    gd = golden_g19
    pn, gen = _stand_in_reference_modules()
    monkeypatch.setitem(sys.modules, integrate.TARGET_MODULES[0], pn)
    monkeypatch.setitem(sys.modules, integrate.TARGET_MODULES[1], gen)
    mods = {"sa": pn.SetAbstraction(32, 64, layers=2, stride=2, radius=0.15, nsample=32, normalize_dp=True, use_res=True),
            "head": pn.SetAbstraction(4, 32, layers=1, stride=1, is_head=True),
            "odd": pn.SetAbstraction(32, 64, layers=2, stride=2, radius=0.15, nsample=16, normalize_dp=True,
                                     feature_type='dp_df', use_res=True),
            "grp": gen.PointsetGrouper(channel=16, reduce=2, kneighbors=24, radi=0.2),
            "att": gen.Anchor_selfattention(32, 2),
            "cbr": gen.ConvBNReLU1D(16, 32, bias=False)}
    for k, m in mods.items():
        m.train()
        assert list(m.state_dict().keys()) == list(gd[f"{k}_keys"]), k          # the reference's layout
        m.load_state_dict(_state_from(gd, k, "init"))                            # the reference's initial weights
    keys = {k: list(m.state_dict().keys()) for k, m in mods.items()}
    params = {k: [id(q) for q in m.parameters()] for k, m in mods.items()}

    p = torch.from_numpy(GI.unit_sphere_cloud(2, 256, seed=3))
    f = torch.from_numpy(GI.seeded_normal((2, 32, 256), seed=4)).requires_grad_(True)
    x4 = torch.from_numpy(GI.seeded_normal((2, 4, 256), seed=5))
    pts = torch.from_numpy(GI.seeded_normal((2, 256, 16), seed=6)).requires_grad_(True)
    xa = torch.from_numpy(GI.seeded_normal((2, 64, 32), seed=7))
    xc = torch.from_numpy(GI.seeded_normal((2, 16, 256), seed=8))

    def run_all():
        sa, head, odd, grp, att, cbr = (mods[k] for k in ("sa", "head", "odd", "grp", "att", "cbr"))
        out = {}
        f1 = f.detach().clone().requires_grad_(True)
        new_p, o = sa([p, f1])
        (o * o).sum().backward()
        out["sa"] = [new_p, o.detach(), f1.grad] + [q.grad.clone() for q in sa.parameters()]
        sa.zero_grad()
        out["head"] = [head([p, x4])[1].detach()]
        out["odd"] = [odd([p, f.detach()])[1].detach()]
        pt1 = pts.detach().clone().requires_grad_(True)
        nx, g = grp(p, pt1)
        g.square().sum().backward()
        out["grp"] = [nx, g.detach(), pt1.grad, grp.affine_alpha.grad.clone()]
        grp.zero_grad()
        out["att"] = [att(xa, p[:, :64]).detach()]
        out["cbr"] = [cbr(xc).detach()]
        return out

    want = {k: [torch.from_numpy(gd[f"{k}_out{i}"]) for i in range(int(gd[f"{k}_nout"]))] for k in mods}
    integrate.COUNTS.clear()
    patched = integrate.patch_openpoints()
    try:
        assert set(patched) == set(integrate.TARGET_MODULES)
        assert pn.SetAbstraction.forward is integrate._sa_forward
        got = run_all()
        for k, m in mods.items():
            assert list(m.state_dict().keys()) == keys[k], k          # nothing added, renamed or re-registered
            assert [id(q) for q in m.parameters()] == params[k], k
        counts = dict(integrate.COUNTS)
    finally:
        integrate.unpatch_openpoints()
    assert pn.SetAbstraction.forward is not integrate._sa_forward and "fused" not in gen.PointsetGrouper.__dict__
    # dispatch: the covered configurations went into adaptpoint_amd, the uncovered one to the class's own forward, counted
    assert counts.get("SetAbstraction.fused") == 2, counts                                  # the block and the stem
    assert counts.get("SetAbstraction.reference: feature_type 'dp_df'") == 1, counts
    assert counts.get("PointsetGrouper.composed") == 1 and counts.get("Anchor_selfattention.composed") == 1, counts
    assert counts.get("ConvBNReLU1D.reference: CPU tensor") == 1, counts
    for k in want:
        assert len(got[k]) == len(want[k]), k
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            scale = float(b.abs().max()) + 1e-12
            assert float((a - b).abs().max()) <= 2e-5 * scale, (k, i, float((a - b).abs().max()), scale)
    for k, m in mods.items():                                                               # running statistics advanced alike
        after = _state_from(gd, k, "after")
        for name, v in m.state_dict().items():
            np.testing.assert_allclose(v.double().numpy(), after[name].double().numpy(), rtol=1e-5, atol=1e-6, err_msg=f"{k}.{name}")


def test_environment_switch_patches_lazily(monkeypatch):
    """APN_PATCH_OPENPOINTS=1: the drop-in module installs a post-import hook; unset, nothing is touched."""
    from adaptpoint_amd import integrate
    monkeypatch.delenv("APN_PATCH_OPENPOINTS", raising=False)
    assert not integrate.requested_by_environment()
    monkeypatch.setenv("APN_PATCH_OPENPOINTS", "1")
    assert integrate.requested_by_environment()
    try:
        integrate.patch_openpoints(lazy=True)
        assert any(isinstance(f, integrate._PostImport) for f in sys.meta_path)
    finally:
        integrate.unpatch_openpoints()
    assert not any(isinstance(f, integrate._PostImport) for f in sys.meta_path)
