"""GPU: adaptpoint_amd.partseg on the device -- the narrow decoder against the reference-made goldens (composed, and on
the fused + hoisted kernels), one `PartSegStep` replayed from a hipGraph against the same step run eagerly, and
`PartSegEvaluator.validate` against a host loop over the same logits."""
import copy
import gc
import os

import numpy as np
import pytest
import torch

import golden_inputs as GI
import partseg_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partseg_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.mark.parametrize("mode", ["composed", "fused_hoisted"])
@pytest.mark.parametrize("cls_map", R.CLS_MAPS)
def test_part_decoder_on_the_device_meets_reference_goldens(dev, gold, oracle, cls_map, mode):
    """The bars of the G14 device test (tests/test_gpu_propagation.py:188-191): rtol 1e-5 / atol 1e-5 on the output,
    rtol 1e-4 / atol 1e-5 on the gradients."""
    from adaptpoint_amd import propagation
    from adaptpoint_amd.partseg import PointNextPartDecoder
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    on = mode == "fused_hoisted"
    dec = fill_parameters_by_name(PointNextPartDecoder(
        hoisted=on, fused=on, cls2partembed=R.part_embed() if 'pointnext' in cls_map else None,
        **R.decoder_args(cls_map))).to(dev).train()
    p, f, cls, gout = R.pyramid(int(gold["dec/seed"]), oracle.furthest_point_sampling)
    p, f, cls, gout = [q.to(dev) for q in p], [t.to(dev) for t in f], cls.to(dev), gout.to(dev)
    if on:       # the kernels, not the torch form: the last block with its conditioning vector
        conv, bn, _ = propagation.block_parts(dec.decoder[0][0].convs[0])
        cond = dec.conditioning(f, cls)
        assert tuple(cond.shape) == (R.NARROW_B, dec.cond_channels)
        assert propagation.supported(f[1].contiguous(), f[2].contiguous(), conv, bn, cond.contiguous())
    res = R.run_decoder(dec, p, f, cls, gout)
    for k in [k for k in gold.files if k.startswith(f"dec/{cls_map}/")]:
        name = k[len(f"dec/{cls_map}/"):]
        if name == "err64" or name.endswith("num_batches_tracked"):
            continue
        rtol = 1e-5 if name == "out" else 1e-4
        np.testing.assert_allclose(res[name], gold[k], rtol=rtol, atol=1e-5, err_msg=f"{cls_map} {mode}: {name}")


NARROW_MODEL = dict(blocks=(1, 1, 1), strides=(1, 4, 4), width=16, nsample=16, radius=0.2)


def _narrow_model(dev, **kw):
    from adaptpoint_amd.partseg import POINTNEXT_S_ENCODER, BasePartSeg
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    import test_gpu_graph_replay as G
    enc = dict(POINTNEXT_S_ENCODER, **NARROW_MODEL)
    return G._no_dropout(fill_parameters_by_name(BasePartSeg(encoder_args=enc, **kw))).to(dev)


def _batch(dev, B, N, seed):
    pos = torch.from_numpy(GI.unit_sphere_cloud(B, N, seed=seed)).to(dev)
    g = torch.Generator().manual_seed(seed)
    height = pos[:, :, 1:2] - pos[:, :, 1:2].min(1, keepdim=True)[0]
    normals = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g), dim=-1).to(dev)
    x = torch.cat([pos, normals, height], -1).transpose(1, 2).contiguous()
    cls = torch.randint(0, 16, (B, 1), generator=g)
    from adaptpoint_amd.part_metrics import SHAPENETPART_CLS2PARTS
    y = torch.stack([torch.tensor(SHAPENETPART_CLS2PARTS[int(k)])[torch.randint(0, len(SHAPENETPART_CLS2PARTS[int(k)]),
                                                                                 (N,), generator=g)] for k in cls])
    return {'pos': pos, 'x': x, 'y': y.to(dev), 'cls': cls.to(dev)}


def test_partseg_step_replayed_from_a_hipgraph_equals_eager(dev, monkeypatch):
    """One `train_one_epoch` iteration (adaptpoint_amd.partseg.PartSegStep: PointNeXt-S for ShapeNetPart on the fused
    and hoisted kernels, Poly1 focal loss, gradient-norm clipping, capturable fused AdamW) by the method of
    tests/test_gpu_graph_replay.py: three replayed steps against three eager ones from the same snapshot, with a second
    eager run as the run-to-run floor; and two replayed runs from one snapshot leave identical parameters.
    The encoder's set-abstraction blocks have sa_layers=2, the depth the fused kernels cover (the classifier's): with the
    ShapeNetPart configuration's three layers they run on the unfused operators, whose gradient scatter adds with float
    atomics -- the step still replays (measured: equal to eager within the run-to-run floor), not bit for bit."""
    import test_gpu_graph_replay as G
    from adaptpoint_amd import fused, graphs
    from adaptpoint_amd.partseg import BasePartSeg, PartSegStep
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    monkeypatch.setattr(fused, "DETERMINISTIC", True)
    B, N, STEPS = 4, 1024, G.STEPS
    from adaptpoint_amd.partseg import POINTNEXT_S_ENCODER
    model = G._no_dropout(fill_parameters_by_name(BasePartSeg(encoder_args=dict(POINTNEXT_S_ENCODER, sa_layers=2), fused=True,
                                                              hoisted=True))).to(dev)
    assert all(stage[0].hoisted for stage in model.decoder.decoder)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True, fused=True)
    step = PartSegStep(model, optimizer=opt)
    batches = [_batch(dev, B, N, 900 + i) for i in range(STEPS + 1)]
    data = {k: v.clone() for k, v in batches[0].items()}

    def load(i):
        for k in data:
            data[k].copy_(batches[i][k])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            load(STEPS)
            step(data)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    snap = G._snapshot((model,), (opt,))

    def eager_run():
        out = []
        for i in range(STEPS):
            load(i)
            out.append({"loss": step(data)[1].item()})
        return out, [copy.deepcopy(model.state_dict())]
    eager2, eager_w2 = eager_run()
    G._restore((model,), (opt,), snap)
    eager, eager_w = eager_run()
    G._restore((model,), (opt,), snap)
    gc.collect()
    load(STEPS)
    graph, (_, cap_loss), census = graphs.capture(lambda: step(data), leaves=list(model.parameters()),
                                                  what="the part-segmentation step's graph")
    print("part-segmentation step graph:", census)

    def replay_run():
        G._restore((model,), (opt,), snap)
        out = []
        for i in range(STEPS):
            load(i)
            graph.replay()
            torch.cuda.synchronize()
            out.append({"loss": cap_loss.item()})
        return out, copy.deepcopy(model.state_dict())
    replayed, first = replay_run()
    replayed2, second = replay_run()
    G._compare("part-segmentation step", eager, replayed, (model,), eager_w, snap[0], floor=eager_w2, floor_losses=eager2)
    assert [d["loss"] for d in replayed] == [d["loss"] for d in replayed2]
    assert all(torch.equal(first[k], second[k]) for k in first)


class _Recorder(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model, self.logits = model, []

    def forward(self, data):
        out = self.model(data)
        self.logits.append(out.detach().clone())
        return out


def test_evaluator_equals_the_host_loop_over_the_same_logits(dev):
    """70 shapes, batches of 32 (the last one padded and masked), one vote besides the plain pass."""
    from adaptpoint_amd.part_metrics import SHAPENETPART_CLS2PARTS, PartSegEvaluator, finish
    S, N, B = 70, 256, 32
    model = _narrow_model(dev, hoisted=True)
    data = _batch(dev, S, N, 31)
    vote = lambda pos: pos * 1.05
    rec = _Recorder(model)
    eager = PartSegEvaluator(rec, batch_size=B, capture=False, keep_ious=True)
    was = model.training
    res_eager = eager.validate(data['pos'], data['x'], data['y'], data['cls'], num_votes=1, vote_transform=vote)
    assert model.training == was and len(rec.logits) == 6
    # the host loop: the reference's statements over the recorded logits
    table = [list(p) for p in SHAPENETPART_CLS2PARTS]
    state, all_ious = None, []
    for i in range(3):
        logits = ((rec.logits[2 * i] + rec.logits[2 * i + 1]) / 2).cpu().numpy()
        rows = np.arange(32 * i, 32 * i + 32)
        valid = rows < S
        rows = np.where(valid, rows, 32 * i)
        ious = R.shape_ious(R.predict(logits), data['y'].cpu().numpy()[rows], data['cls'].cpu().numpy()[rows], table)
        ious[~valid] = -1.0
        all_ious.append(ious)
        state = R.totals(ious, data['cls'].cpu().numpy().reshape(-1)[rows], 16, state)
    assert state[3] == S
    want = finish(*state)
    assert np.array_equal(eager.ious.cpu().numpy().view(np.int32), np.stack(all_ious).view(np.int32))
    assert res_eager[0] == want[0] and res_eager[1] == want[1] and np.array_equal(res_eager[2], want[2])
    captured = PartSegEvaluator(model, batch_size=B, capture=True, keep_ious=True)
    res = captured.validate(data['pos'], data['x'], data['y'], data['cls'], num_votes=1, vote_transform=vote)
    assert captured.captures == 1 and next(iter(captured.graphs.values())).census.get("memset", 0) == 0
    assert torch.equal(captured.ious, eager.ious)
    assert res[0] == want[0] and res[1] == want[1] and np.array_equal(res[2], want[2])
    res2 = captured.validate(data['pos'], data['x'], data['y'], data['cls'], num_votes=1, vote_transform=vote)
    assert captured.captures == 1 and res2[0] == res[0] and np.array_equal(res2[2], res[2])
