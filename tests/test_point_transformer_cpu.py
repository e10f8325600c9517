"""CPU suite: the Point Transformer modules (adaptpoint_amd/point_transformer.py) against the REFERENCE's `PTSeg` captured in
tests/golden/point_transformer_golden.npz (tests/golden/make_golden_point_transformer.py), the graph-sharing call
forms, the argument checks of the apn_pt_* entries and the plain-value coverage rule of the fused layer."""
import os

import numpy as np
import pytest
import torch

import point_transformer_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5          # relative L2 per tensor, the bar of tests/test_dgcnn_cpu.py
ERR64_KNEE = 2.5e-6  # a tensor whose recorded err64 (the reference's own distance to float64) exceeds this gets 4 x err64


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "point_transformer_golden.npz"))


def _narrow(fused=False):
    from adaptpoint_amd.point_transformer import PTSeg
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return fill_parameters_by_name(PTSeg('PointTransformerBlock', fused=fused, **R.NARROW))


def _shapes(module):
    return [(n, ",".join(str(s) for s in t.shape)) for n, t in module.state_dict().items()]


# the flat bar on every tensor that has a value: 4 x BAR.  Measured 5e-6 at the worst; ONE product rounded in another order
# (the decoder head's linear2 applied to all clouds at once instead of cloud by cloud) measured 2.6e-5 -- the BatchNorms over
# the 16 and 4 rows of the deep levels amplify a last-bit difference that far --, and a host with another thread count
# blocks its matmuls differently.  A dropped or reordered TERM is a per-cent effect, three orders above this
FLAT = 4e-5
# gradients that vanish analytically: a bias in front of a training-mode BatchNorm (through whatever linear steps), or in
# front of the softmax over the slots
_ZERO = ('linear_q.bias', 'linear_k.bias', 'linear_v.bias', 'linear_p.0.bias', 'linear_p.3.bias', 'linear_w.2.bias',
         'linear_w.5.bias', 'linear1.0.bias', 'cls.0.bias')
# the deepest level holds clouds of 1, 2 and 1 points: 62 of its 64 neighbour offsets are exactly zero, BatchNorm(3)
# normalises two distinct values per channel, and the gradient of the Linear(3,3) in front of it is a cancellation
# (err64 2e-2): these two keep the issue's 4 x err64 bar alone (the mirror measures 2e-3 .. 6e-3 there)
DEGENERATE = ('grad/enc5.1.transformer2.linear_p.0.weight', 'grad/dec5.1.transformer2.linear_p.0.weight')


def _analytically_zero(key):
    name = key[len("grad/"):] if key.startswith("grad/") else None
    if name is None:
        return False
    return name.endswith(_ZERO) or (name.endswith('linear2.0.bias') and not name.startswith('dec5.'))


def _bar(err64):
    return 4.0 * err64 if err64 > ERR64_KNEE else BAR


def test_state_dict_names_and_shapes_are_the_references(gold):
    from adaptpoint_amd.point_transformer import PointTransformerBlock, PTSeg
    assert _shapes(PTSeg(PointTransformerBlock, **R.NARROW)) == list(zip(gold["d/narrow_names"].tolist(),
                                                                          gold["d/narrow_shapes"].tolist()))
    full = PTSeg('PointTransformerBlock', R.FULL_BLOCKS)
    assert _shapes(full) == list(zip(gold["d/full_names"].tolist(), gold["d/full_shapes"].tolist()))
    sd = full.state_dict()
    assert sd["enc1.1.transformer2.linear_p.3.weight"].shape == (32, 3)
    assert sd["enc5.2.transformer2.linear_w.2.weight"].shape == (64, 512) and "dec1.1.transformer2.linear_w.3.running_var" in sd
    with pytest.raises(ValueError):
        PTSeg('os.system', R.FULL_BLOCKS)                   # names go through a table, nothing is evaluated


def test_composed_mirror_matches_the_reference_in_training_mode(gold):
    """Logits, every parameter's gradient and the BatchNorm buffers after the step; on CPU tensors the mirror's
    operators are the module's torch statements, the golden's the float32 statements of tests/pointops_reference.py."""
    from adaptpoint_amd.point_transformer import StageGraph
    m = _narrow().train()
    p, x, o, w = R.model_inputs(R.NARROW_SIZES, int(gold["a/seed"]))
    before = StageGraph.builds
    logits = m(p, x, o, keep_graphs=True)
    assert StageGraph.builds - before == 5                  # one graph per level, not two per layer
    (logits * w).sum().backward()
    graphs = m.last_graphs
    for lv in range(5):
        assert np.array_equal(graphs['stage'][lv].numpy(), gold[f"a/graph/stage{lv + 1}"]), lv
    for lv in range(4):
        assert np.array_equal(graphs['down'][lv][0].numpy(), gold[f"a/graph/fps{lv + 2}"]), lv
        assert np.array_equal(graphs['down'][lv][1].numpy(), gold[f"a/graph/down{lv + 2}"]), lv
        assert np.array_equal(graphs['up'][lv].numpy(), gold[f"a/graph/up{lv + 1}"]), lv
    err64 = {n: float(v[0]) for n, v in R.unpack(gold, "a/err64/").items()}
    errs = {"logits": R.rel(logits.detach(), gold["a/logits"])}
    grads, params = R.unpack(gold, "a/grad/"), dict(m.named_parameters())
    assert sorted(grads) == sorted(params)
    for n, g in grads.items():
        mine = params[n].grad.reshape(-1)[torch.from_numpy(R.sample_index(n, params[n].numel()))]
        errs["grad/" + n] = R.rel(mine, g)
    buffers = dict(m.named_buffers())
    for n, b in R.unpack(gold, "a/buf/").items():
        if n.endswith("num_batches_tracked"):
            assert int(buffers[n]) == int(b[0]) == 1, n
        else:
            errs["buf/" + n] = R.rel(buffers[n].reshape(-1), b)
    # The issue's rule (4 x err64 beyond the knee) holds, and is far from tight: the mirror runs the reference's float32
    # statements in the reference's order, so every tensor that HAS a value meets the flat bar as well.  Two groups do not:
    zero = {k for k in errs if _analytically_zero(k)}
    assert len(zero) == 80 and all(err64[k] > 1e3 for k in zero)      # float64 says so: the golden's entries are rounding noise
    over = {k: (v, _bar(err64[k])) for k, v in errs.items() if not v <= _bar(err64[k])}
    flat = {k: v for k, v in errs.items() if k not in zero and k not in DEGENERATE and not v <= FLAT}
    print("worst of the %d tensors under the flat bar: %.1e" % (len(errs) - len(zero) - len(DEGENERATE),
                                                                 max(v for k, v in errs.items() if k not in zero and k not in DEGENERATE)))
    assert not over, over
    assert not flat, flat


def test_composed_mirror_matches_the_reference_in_eval_mode(gold):
    m = _narrow().eval()
    p, x, o, _ = R.model_inputs(R.NARROW_SIZES, int(gold["a/seed"]))
    with torch.no_grad():
        logits = m({'pos': p, 'x': x, 'o': o})              # the reference's dict form
    assert R.rel(logits, gold["b/logits"]) <= BAR


def test_three_list_and_four_list_call_forms_agree_bit_for_bit():
    from adaptpoint_amd.point_transformer import PointTransformerBlock, StageGraph, TransitionDown
    p, x, o, _ = R.layer_inputs((40, 3, 57), 16, 0)
    blk = R.seed_module(PointTransformerBlock(16, 16, 8, 8), 1).train()
    before = StageGraph.builds
    three = blk([p, x, o])
    assert len(three) == 3 and StageGraph.builds - before == 1
    g = StageGraph(p, o, 8)
    blk2 = R.seed_module(PointTransformerBlock(16, 16, 8, 8), 1).train()
    before = StageGraph.builds
    four = blk2([p, x, o, g])
    assert len(four) == 4 and four[3] is g and StageGraph.builds == before
    assert torch.equal(three[1], four[1])
    assert torch.equal(blk.transformer2([p, x, o]), blk.transformer2([p, x, o, g]))
    with pytest.raises(ValueError):
        blk([p, x, o, StageGraph(p, o, 4)])                 # a graph of another nsample
    down = TransitionDown(16, 32, 4, 8)
    assert len(down([p, x, o, g])) == 3                     # the point set changes: the graph is dropped


def test_fused_model_on_cpu_tensors_runs_composed_without_a_fallback_entry(gold):
    from adaptpoint_amd import set_abstraction as SA
    before = dict(SA.FUSED_FALLBACKS)
    m = _narrow(fused=True).eval()
    assert all(blk.transformer2.fused for blk in m.modules() if hasattr(blk, 'transformer2'))
    p, x, o, _ = R.model_inputs(R.NARROW_SIZES, int(gold["a/seed"]))
    with torch.no_grad():
        logits = m(p, x, o)
    assert R.rel(logits, gold["b/logits"]) <= BAR
    assert SA.FUSED_FALLBACKS == before


def test_graphs_handed_in_are_the_graphs_used(gold):
    m = _narrow().eval()
    p, x, o, _ = R.model_inputs(R.NARROW_SIZES, int(gold["a/seed"]))
    from adaptpoint_amd import point_transformer as PT
    with torch.no_grad():
        ref = m(p, x, o, keep_graphs=True)
        graphs = m.last_graphs
        calls = []
        PT.knn_hook = lambda who, k, n, q: calls.append(who)
        try:
            again = m(p, x, o, graphs=graphs)
            assert calls == [] and m.last_graphs is None    # nothing queried, nothing kept unless asked for
            m(p, x, o)
            assert calls.count('stage') == 5 and calls.count('down') == 4 and calls.count('up') == 4
        finally:
            PT.knn_hook = None
    assert torch.equal(ref, again)
    r64 = R.run_model64(_narrow(), p, x, o, graphs, training=False)
    assert R.rel(ref, r64['logits']) < 1e-5


def test_pt_layer_covers_on_plain_values():
    from adaptpoint_amd.point_transformer import pt_layer_covers as covers
    f32 = torch.float32
    for C in (32, 64, 128, 256, 512):
        for k in (1, 8, 16, 32):
            assert covers('cuda', f32, True, C, C, 8, k, 1000)
    assert not covers('cpu', f32, True, 32, 32, 8, 8, 1000) and not covers('cuda', torch.float64, True, 32, 32, 8, 8, 1000)
    assert not covers('cuda', f32, False, 32, 32, 8, 8, 1000) and not covers('cuda', f32, True, 32, 64, 8, 8, 1000)
    assert not covers('cuda', f32, True, 48, 48, 8, 8, 1000) and not covers('cuda', f32, True, 16, 16, 8, 8, 1000)
    assert not covers('cuda', f32, True, 64, 64, 4, 8, 1000) and not covers('cuda', f32, True, 64, 64, 8, 0, 1000)
    assert not covers('cuda', f32, True, 64, 64, 8, 33, 1000) and not covers('cuda', f32, True, 64, 64, 8, 8, 2 ** 24)
    assert covers('cuda', f32, True, 64, 64, 8, 8, 2 ** 24 - 1) and not covers('cuda', f32, True, 64, 64, 8, 8, 0)


def test_argument_validation_of_the_new_entries_needs_no_gpu():
    """Every apn_pt_* entry rejects bad sizes and null pointers before any HIP call and accepts empty work (P: a
    non-null, aligned address that is never read)."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    EINVAL, P = -1, 4096

    def stats(n=16, k=8, c=32, qkv=P, ld=96, h=P, idx=P, wts=P, part=P):
        return lib.apn_pt_rel_stats(n, k, c, qkv, ld, h, idx, wts, part, None)

    def mid(n=16, k=8, c=32, qkv=P, ld=96, h=P, idx=P, wts=P, bn=P, t=P, part=None):
        return lib.apn_pt_mid(n, k, c, qkv, ld, h, idx, wts, bn, t, part, None)

    def attend(n=16, k=8, c=32, qkv=P, ld=96, h=P, idx=P, wts=P, bn=P, t=P, a=P, out=P):
        return lib.apn_pt_attend(n, k, c, qkv, ld, h, idx, wts, bn, t, a, out, None)

    def attend_bwd(n=16, k=8, c=32, qkv=P, ld=96, h=P, idx=P, wts=P, bn=P, t=P, a=P, go=P, g1=P, part=P):
        return lib.apn_pt_attend_bwd(n, k, c, qkv, ld, h, idx, wts, bn, t, a, go, g1, part, None)

    def mid_bwd(n=16, k=8, c=32, qkv=P, ld=96, h=P, idx=P, wts=P, bn=P, de=P, t=P, g1=P, part=P):
        return lib.apn_pt_mid_bwd(n, k, c, qkv, ld, h, idx, wts, bn, de, t, g1, part, None)

    def rel_bwd(n=16, k=8, c=32, qkv=P, ld=96, h=P, idx=P, wts=P, bn=P, de=P, t=P, g1=P, a=P, go=P, dr=P, dh=P, dqkv=P,
                ldg=96, part=P):
        return lib.apn_pt_rel_bwd(n, k, c, qkv, ld, h, idx, wts, bn, de, t, g1, a, go, dr, dh, dqkv, ldg, part, None)

    def scatter(n=16, k=8, c=32, dr=P, go=P, a=P, pcnt_poff=P, plist=P, dqkv=P, ldg=96):
        return lib.apn_pt_scatter_bwd(n, k, c, dr, go, a, pcnt_poff, plist, dqkv, ldg, None)

    pointers = {stats: ["qkv", "h", "idx", "wts", "part"], mid: ["qkv", "h", "idx", "wts", "bn", "t"],
                attend: ["qkv", "h", "idx", "wts", "bn", "t", "a", "out"],
                attend_bwd: ["qkv", "h", "idx", "wts", "bn", "t", "a", "go", "g1", "part"],
                mid_bwd: ["qkv", "h", "idx", "wts", "bn", "de", "t", "g1", "part"],
                rel_bwd: ["qkv", "h", "idx", "wts", "bn", "de", "t", "g1", "a", "go", "dr", "dh", "dqkv", "part"],
                scatter: ["dr", "go", "a", "pcnt_poff", "plist", "dqkv"]}
    for entry, names in pointers.items():
        for name in names:
            assert entry(**{name: None}) == EINVAL, (entry.__name__, name)
        assert entry(n=0) == 0 and entry(n=0, **{names[0]: None}) == 0, entry.__name__         # empty work
        assert entry(n=-1) == EINVAL and entry(n=2 ** 24) == EINVAL, entry.__name__
        assert entry(k=0) == EINVAL and entry(k=33) == EINVAL and entry(k=-1) == EINVAL, entry.__name__
        pitch = {v: 3 * 1024 for v in ("ld", "ldg") if v in entry.__code__.co_varnames[:entry.__code__.co_argcount]}
        for c in (48, 0, 16, 1024, 33):                                                         # with pitches wide enough
            assert entry(c=c, **pitch) == EINVAL, (entry.__name__, c)
    for entry in (stats, mid, attend, attend_bwd, mid_bwd, rel_bwd):
        assert entry(ld=95) == EINVAL and entry(c=64, ld=191) == EINVAL, entry.__name__         # ld >= 3c
    assert rel_bwd(ldg=95) == EINVAL and scatter(ldg=95) == EINVAL

    def colsum(n=16, width=96, src=P, ld=96, part=P):
        return lib.apn_pt_colsum(n, width, src, ld, part, None)
    assert colsum(n=0) == 0 and colsum(n=0, src=None) == 0 and colsum(src=None) == EINVAL and colsum(part=None) == EINVAL
    assert colsum(n=-1) == EINVAL and colsum(n=2 ** 24) == EINVAL and colsum(width=0) == EINVAL
    assert colsum(width=1537, ld=1537) == EINVAL and colsum(ld=95) == EINVAL and colsum(n=0, width=1536, ld=1536) == 0
    assert [lib.apn_pt_colsum_rows(n) for n in (0, 1, 32, 33, 705, 2 ** 24 - 1, 2 ** 24)] == [0, 1, 1, 2, 23, 1024, 0]

    assert lib.apn_pt_rows(0, 8, 32) == 0 and lib.apn_pt_rows(16, 8, 48) == 0 and lib.apn_pt_rows(16, 33, 32) == 0
    assert lib.apn_pt_rows(1, 1, 32) == 1 and lib.apn_pt_rows(705, 16, 64) == 177 and lib.apn_pt_rows(4, 16, 512) == 1
    assert [lib.apn_pt_rows(2 ** 24 - 1, 32, c) for c in (32, 64, 128, 256, 512)] == [2048, 2048, 1024, 256, 128]
    # mid: a workgroup per tile of 8192 / c positions, within the same cap
    assert [lib.apn_pt_mid_rows(705, 16, c) for c in (32, 64, 128, 256, 512)] == [45, 89, 177, 177, 128]
    assert lib.apn_pt_mid_rows(0, 8, 32) == 0 and lib.apn_pt_mid_rows(16, 8, 48) == 0 and lib.apn_pt_mid_rows(1, 1, 512) == 1
    assert [lib.apn_pt_mid_rows(2 ** 24 - 1, 32, c) for c in (32, 512)] == [2048, 128]
    assert lib.apn_pt_fold(P, 4, 0, P, None) == 0 and lib.apn_pt_fold(P, 4, 8, None, None) == EINVAL
    assert lib.apn_pt_fold(None, 4, 8, P, None) == EINVAL and lib.apn_pt_fold(P, 2049, 8, P, None) == EINVAL
    assert lib.apn_pt_fold(P, -1, 8, P, None) == EINVAL and lib.apn_pt_fold(P, 4, -1, P, None) == EINVAL
