"""GPU suite: apn_knn_query (csrc/knn.hip) through `layers.knn_query` against the numpy statement of its contract
(tests/knn_reference.py).

Exact cases: integer coordinates in [-4, 4] -- every squared distance is an integer <= 64 C <= 8192, exact in fp32
under any summation order, and ties are plentiful -- so indices and distances must EQUAL the reference.

Error bars on seeded normal inputs: tau = (C + 3) 2^-24, derived: one rounding in the difference (relative 2^-24 of
the difference, so 2 x 2^-24 of its square), one in the square (or none under an fma), and at most C - 1 in a sum of
non-negative terms, in any order.  numpy, sequential float32 accumulation: measured maxima 4.4, 8.7 and 12.4 x 2^-24 at
C = 3, 64, 128.  With D_k the float64 k-th smallest distance, a returned support lies within D_k (1 + 3 tau) and one
that is not returned beyond D_k (1 - 3 tau): a swap needs two fp32 distances, each within tau of its float64 value, to
compare the other way."""
import gc

import numpy as np
import pytest
import torch

import golden_inputs as GI
import knn_reference as KR

pytestmark = pytest.mark.gpu

EXACT = [(1, 1, 1, 3, 1), (2, 5, 5, 3, 5), (3, 77, 77, 3, 20), (2, 130, 33, 4, 8), (2, 200, 200, 64, 20),
         (1, 257, 257, 128, 40), (1, 300, 300, 5, 64), (2, 1024, 1024, 3, 20)]


def _run(dev, support, query, k):
    from adaptpoint_amd.layers import knn_query
    s = torch.from_numpy(support).to(dev)
    q = s if query is support else torch.from_numpy(query).to(dev)
    idx, d2 = knn_query(s, q, k, return_dist=True)
    assert idx.dtype == torch.int32 and idx.shape == (support.shape[0], query.shape[1], k) and d2.shape == idx.shape
    assert torch.equal(knn_query(s, q, k), idx)                       # dist2 = NULL: the same indices
    return idx.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("B,N,M,C,k", EXACT)
def test_exact_cases_equal_the_reference(dev, B, N, M, C, k):
    support = KR.integer_cloud((B, N, C), seed=N * 131 + C)
    query = support if (N, M) != (130, 33) else KR.integer_cloud((B, M, C), seed=4242)
    idx, d2 = _run(dev, support, query, k)
    ref_idx, ref_d2 = KR.knn(support, query, k)
    assert np.array_equal(idx, ref_idx)
    assert np.array_equal(d2.astype(np.float64), ref_d2)


def test_identical_points_come_back_in_index_order(dev):
    support = np.full((1, 70, 3), 2.5, np.float32)
    idx, d2 = _run(dev, support, support, 20)
    assert np.array_equal(idx, np.broadcast_to(np.arange(20, dtype=np.int32), (1, 70, 20)))
    assert not d2.any()


def test_distinct_points_find_themselves_first(dev):
    support = GI.seeded_normal((2, 300, 3), seed=71).astype(np.float32)
    assert len(np.unique(support.reshape(-1, 3), axis=0)) == 600
    idx, d2 = _run(dev, support, support, 8)
    assert np.array_equal(idx[:, :, 0], np.broadcast_to(np.arange(300, dtype=np.int32), (2, 300)))
    assert not d2[:, :, 0].any() and (d2[:, :, 1] > 0).all()


@pytest.mark.parametrize("C", [3, 64, 128])
def test_error_bars_on_normal_inputs(dev, C):
    B, N, k = 2, 300, 20
    support = GI.seeded_normal((B, N, C), seed=500 + C).astype(np.float32)
    idx, d2 = _run(dev, support, support, k)
    tau = (C + 3) * 2.0 ** -24
    d64 = KR.dist2_64(support, support)                               # (B, N, N), every query
    got64 = np.take_along_axis(d64, idx.astype(np.int64), -1)
    err = np.abs(d2.astype(np.float64) - got64) / np.maximum(got64, 1e-300)
    print(f"C={C}: worst |dist2 - d64| / d64 = {np.where(got64 > 0, err, 0).max() / 2.0 ** -24:.2f} x 2^-24 (bar {C + 3})")
    assert (np.abs(d2.astype(np.float64) - got64) <= tau * got64).all()
    assert (idx >= 0).all() and (idx < N).all()
    assert all(len(np.unique(row)) == k for row in idx.reshape(-1, k))                 # k distinct supports
    Dk = np.sort(d64, -1)[..., k - 1:k]
    assert (got64 <= Dk * (1 + 3 * tau)).all()
    returned = np.zeros_like(d64, dtype=bool)
    np.put_along_axis(returned, idx.astype(np.int64), True, -1)
    assert (np.where(returned, np.inf, d64) >= Dk * (1 - 3 * tau)).all()
    assert (np.diff(d2, axis=-1) >= 0).all()                                            # non-decreasing along k
    assert (np.diff(idx, axis=-1)[np.diff(d2, axis=-1) == 0] > 0).all()                  # equal values: ascending indices


def test_knn_grouper_on_cuda_calls_the_kernel_and_returns_sorted_neighbours(dev, monkeypatch):
    from adaptpoint_amd import layers
    calls = []
    real = layers.knn_query
    monkeypatch.setattr(layers, "knn_query", lambda *a, **k: calls.append(1) or real(*a, **k))
    xyz = torch.from_numpy(GI.unit_sphere_cloud(2, 256, seed=72)).to(dev)
    query = xyz[:, :40].contiguous()
    idx = layers.KnnGrouper(8).neighbours(query, xyz)
    assert len(calls) == 1 and idx.shape == (2, 40, 8) and idx.dtype == torch.int32
    ref_idx, _ = KR.knn(xyz.cpu().numpy(), query.cpu().numpy(), 8)
    d64 = np.take_along_axis(KR.dist2_64(xyz.cpu().numpy(), query.cpu().numpy()), idx.cpu().numpy().astype(np.int64), -1)
    assert (np.diff(d64, axis=-1) >= -6 * 2.0 ** -24 * d64[..., 1:]).all()              # sorted (to fp32 rounding)
    assert (np.sort(idx.cpu().numpy(), -1) == np.sort(ref_idx, -1)).all(-1).mean() >= 0.98
    # float64 inputs are outside the kernel: the cdist / topk line
    layers.KnnGrouper(8).neighbours(query.double(), xyz.double())
    assert len(calls) == 1


def test_two_runs_are_bit_identical(dev):
    support = GI.seeded_normal((2, 500, 64), seed=73).astype(np.float32)
    a, b = _run(dev, support, support, 20), _run(dev, support, support, 20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_replay_from_a_hipgraph_equals_eager_without_a_memset_node(dev):
    from adaptpoint_amd import graphs
    from adaptpoint_amd.layers import knn_query
    x = torch.from_numpy(GI.seeded_normal((2, 300, 64), seed=74).astype(np.float32)).to(dev)

    def step():
        return list(knn_query(x, x, 20, return_dist=True))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up: allocator pools, lazy initialisation
        step()
    torch.cuda.current_stream().wait_stream(side)
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(step, what="the kNN query's graph")
    print("kNN graph:", census)
    assert not census.get("memset", 0) and census.get("kernel", 0) == 1
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)
