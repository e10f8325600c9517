"""CPU suite: InvResMLP, LocalAggregation and the general PointNeXt encoder (adaptpoint_amd/pointnext.py) against the
REFERENCE's modules captured in tests/golden/invres_golden.npz (tests/golden/make_golden_invres.py), the float64
restatement the GPU tests compare against (tests/invres_reference.py) against the same fixture, and the argument
checks of the new C entries."""
import os

import numpy as np
import pytest
import torch

import invres_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5          # relative L2 per tensor: the reference itself sits 6e-7 from float64 on these inputs (a/err64)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "invres_golden.npz"))


def _block(flip=False, fused=False):
    from adaptpoint_amd.pointnext import InvResMLP, fill_parameters_by_name
    c = R.BLOCK
    blk = fill_parameters_by_name(InvResMLP(c['C'], expansion=c['expansion'], fused=fused,
                                            group_args=dict(NAME='ballquery', normalize_dp=True, radius=c['radius'],
                                                            nsample=c['nsample'])))
    return R.flip_every_third_gamma(blk) if flip else blk


def _encoder(**over):
    from adaptpoint_amd.pointnext import PointNextEncoder, fill_parameters_by_name
    return fill_parameters_by_name(PointNextEncoder(**{**R.POINTNEXT_B, **over}))


def _sampled(t, name, keep):
    return t.detach().reshape(-1)[torch.from_numpy(R.sample_index(name, t.numel(), keep))]


def _check_block(gold, tag, out, df, dp, grads, buffers, what, vectors64=False):
    """vectors64: compare the 1-D parameter gradients with the reference's own float64 run (`tag/grad64/`): they are
    per-channel sums with heavy cancellation, and the reference's float32 values sit up to 3e-5 from its float64 ones
    (make_golden_invres._vector_grads64) -- no yardstick for a float64 restatement at 1e-5."""
    errs = {"out": R.rel(_sampled(out, f"{tag}/out", 16384), gold[f"{tag}/out"]),
            "df": R.rel(_sampled(df, f"{tag}/df", 16384), gold[f"{tag}/df"]), "dp": R.rel(dp, gold[f"{tag}/dp"])}
    names = [k[len(tag) + 6:] for k in gold.files if k.startswith(f"{tag}/grad/")]
    assert sorted(names) == sorted(grads)
    for n in names:
        key = f"{tag}/grad64/{n}" if vectors64 and f"{tag}/grad64/{n}" in gold.files else f"{tag}/grad/{n}"
        errs["grad/" + n] = R.rel(_sampled(grads[n], n, 8192), gold[key])
    for k in gold.files:
        if k.startswith(f"{tag}/buf/"):
            n = k[len(tag) + 5:]
            if n.endswith("num_batches_tracked"):
                assert int(buffers[n]) == int(gold[k]), n
            else:
                errs["buf/" + n] = R.rel(buffers[n], gold[k])
    print(what, tag, {k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < BAR, {k: v for k, v in errs.items() if v >= BAR}


def test_state_dict_names_and_shapes_are_the_references(gold):
    want = list(zip(gold["d/names"].tolist(), gold["d/shapes"].tolist()))
    enc = _encoder()
    have = [(n, ",".join(str(s) for s in t.shape)) for n, t in enc.state_dict().items()]
    assert have == want
    assert enc.channel_list == [32, 64, 128, 256, 512] and enc.out_channels == 512
    from adaptpoint_amd.pointnext import InvResMLP
    blk = InvResMLP(64, expansion=4)
    have = [("encoder.1.1." + n, ",".join(str(s) for s in t.shape)) for n, t in blk.state_dict().items()]
    assert have == [w for w in want if w[0].startswith("encoder.1.1.")]
    assert "convs.convs.0.0.weight" in blk.state_dict() and "pwconv.1.1.running_var" in blk.state_dict()


def test_radii_and_nsample_lists_follow_the_reference(gold):
    enc = _encoder()
    np.testing.assert_allclose([r for st in enc.radii for r in st], gold["d/radii_scalar"], rtol=1e-12)
    nested = _encoder(radius=[[0.1], [0.1, 0.2], [0.2, 0.3, 0.4], [0.4], [0.8, 1.0]], nsample=[[16], [32], [32, 24], [16], [8]])
    np.testing.assert_allclose([r for st in nested.radii for r in st], gold["d/radii_nested"], rtol=1e-12)
    assert [r for st in nested.nsample for r in st] == gold["d/nsample_nested"].tolist()
    assert nested.encoder[2][2].convs.grouper.radius == 0.4 and nested.encoder[2][2].convs.grouper.nsample == 24
    from adaptpoint_amd.pointnext import PointNextEncoder
    narrow = PointNextEncoder(**R.NARROW)
    np.testing.assert_allclose([r for st in narrow.radii for r in st], gold["c/radii"], rtol=1e-12)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_composed_block_reproduces_the_reference(gold, cpu_mirrors, tag):
    blk = _block(flip=tag == "b").train()
    p, f, w = R.block_inputs(R.BLOCK['B'], R.BLOCK['N'], R.BLOCK['C'], int(gold["ab/seed"]))
    p.requires_grad_(True)
    f.requires_grad_(True)
    _, out = blk([p, f])
    (out * w).sum().backward()
    _check_block(gold, tag, out, f.grad, p.grad, {n: q.grad for n, q in blk.named_parameters()},
                 dict(blk.named_buffers()), "composed")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_float64_restatement_reproduces_the_reference(gold, oracle, tag):
    blk = _block(flip=tag == "b")
    c = R.BLOCK
    p, f, w = R.block_inputs(c['B'], c['N'], c['C'], int(gold["ab/seed"]))
    idx = torch.from_numpy(oracle.ball_query(c['radius'], c['nsample'], p.numpy(), p.numpy()))
    r = R.run_invres64(blk, p, f, idx, w)
    buffers = {n: r['buffers'].get(n, b) for n, b in blk.named_buffers()}
    _check_block(gold, tag, r['out'], r['df'], r['dp'], r['grads'], buffers, "float64", vectors64=True)
    assert r['margin'] > 0


def test_composed_narrow_encoder_reproduces_the_reference(gold, cpu_mirrors):
    from adaptpoint_amd.pointnext import PointNextEncoder, fill_parameters_by_name
    enc = fill_parameters_by_name(PointNextEncoder(**R.NARROW)).eval()
    pos = torch.from_numpy(R.GI.unit_sphere_cloud(2, 512, seed=931))
    x = torch.cat([pos, pos[:, :, 1:2] - pos[:, :, 1:2].min(1, keepdim=True)[0]], -1).transpose(1, 2).contiguous()
    with torch.no_grad():
        cls = enc.forward_cls_feat(pos, x)
        ps, fs = enc.forward_seg_feat({'pos': pos, 'x': x})
    assert R.rel(cls, gold["c/cls"]) < BAR
    assert len(ps) == len(fs) == 6
    for i, (p, f) in enumerate(zip(ps, fs)):
        assert np.array_equal(p.numpy(), gold[f"c/p{i}"]), i
        assert R.rel(f, gold[f"c/f{i}"]) < BAR, i


def test_fused_request_on_cpu_tensors_runs_composed_and_records_no_fallback(gold, cpu_mirrors):
    from adaptpoint_amd import set_abstraction as SA
    before = dict(SA.FUSED_FALLBACKS)
    blk, ref = _block(fused=True).train(), _block().train()
    p, f, _ = R.block_inputs(2, 128, R.BLOCK['C'], 3)
    _, a = blk([p, f])
    _, b = ref([p, f])
    assert torch.equal(a, b)
    assert SA.FUSED_FALLBACKS == before


def test_settings_outside_the_hot_path_are_refused():
    from adaptpoint_amd.pointnext import InvResMLP, LocalAggregation, PointNextEncoder
    with pytest.raises(NotImplementedError):
        LocalAggregation([64, 64], feature_type='dp_df')
    with pytest.raises(NotImplementedError):
        LocalAggregation([64, 64], reduction='mean')
    with pytest.raises(NotImplementedError):
        InvResMLP(64, group_args={'NAME': 'knn', 'nsample': 16})
    with pytest.raises(NotImplementedError):
        PointNextEncoder(block='ResBlock')


def test_argument_validation_of_the_local_aggregation_entries_needs_no_gpu():
    """Bad sizes and null tensors are rejected before any HIP call; empty work is a no-op."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    EINVAL, P = -1, 4096                                        # P: a non-null address that is never read
    assert lib.apn_la_pool_rows(4, 512) == 32 and lib.apn_la_pool_rows(1, 65) == 2 and lib.apn_la_pool_rows(0, 5) == 0
    fwd = lambda b=2, n=8, c=64, k=32, radius=0.3, U=P, xyz=P, wp=P, ldw=67, idx=P, ext=P, sel=P, ysum=P, part=P: \
        lib.apn_la_pool_fwd(b, n, c, k, radius, U, xyz, wp, ldw, idx, None, ext, sel, ysum, part, None)
    assert fwd(b=0) == 0 and fwd(n=0) == 0                      # empty work
    assert fwd(b=-1) == EINVAL and fwd(n=-1) == EINVAL
    assert fwd(c=48) == EINVAL and fwd(c=1024) == EINVAL and fwd(c=0) == EINVAL
    assert fwd(k=16) == EINVAL and fwd(radius=0.0) == EINVAL and fwd(ldw=2) == EINVAL
    assert fwd(b=1 << 15, n=1 << 15) == EINVAL                  # b * n beyond the index structures
    for null in ("U", "xyz", "wp", "idx", "ext", "sel"):
        assert fwd(**{null: None}) == EINVAL, null
    assert fwd(ysum=None) == EINVAL and fwd(part=None) == EINVAL          # training outputs: both or neither
    assert lib.apn_la_stats_fold(None, 0, 64, 1.0, None, None) == 0
    assert lib.apn_la_stats_fold(None, 4, 64, 1.0, P, None) == EINVAL
    assert lib.apn_la_stats_fold(P, 4, 0, 1.0, P, None) == EINVAL and lib.apn_la_stats_fold(P, -1, 64, 1.0, P, None) == EINVAL

    def bwd(b=2, n=8, c=64, k=32, radius=0.3, ldw=67, null=None):
        ptrs = [P] * 11
        if null is not None:
            ptrs[null] = None
        return lib.apn_la_pool_bwd(b, n, c, k, radius, *ptrs, ldw, P, P, None, None)
    assert bwd(b=0) == 0 and bwd(n=0) == 0
    assert bwd(b=-1) == EINVAL and bwd(c=96) == EINVAL and bwd(k=31) == EINVAL and bwd(radius=0.0) == EINVAL
    assert bwd(ldw=2) == EINVAL
    for null in (0, 1, 2, 3, 4, 5, 6, 7, 9, 10):                # (8: ysum may be null -- eval mode)
        assert bwd(null=null) == EINVAL, null
    assert lib.apn_la_pool_bwd(2, 8, 64, 32, 0.3, *([P] * 11), 67, None, P, None, None) == EINVAL          # dU
