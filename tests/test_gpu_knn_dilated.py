"""GPU suite: apn_knn_dilated (csrc/knn.hip) through `layers.knn_dilated` against the numpy statement of the kNN
contract (tests/knn_reference.py): with L = KR.knn(support, query, kd), the result is L[..., slots].

Exact cases: integer coordinates in [-4, 4] -- every squared distance is an integer <= 64 C <= 8192, exact in fp32
under any summation order, and ties are plentiful -- so indices and distances must EQUAL the reference.  The shapes
cross the kernel's boundaries: one rank past a wave (kd = 65), 2, 3 and 4 list registers per lane, kd = n, M != N with
M no multiple of the query tile, several support chunks at C = 64 and C = 128.

Error bars on seeded normal inputs: tests/test_gpu_knn.py's derived bar, tau = (C + 3) 2^-24: a returned distance lies
within tau of its float64 value, and the rank-r entry within D_r (1 + 3 tau) and beyond D_r (1 - 3 tau) of the float64
r-th smallest distance D_r (a swap needs two fp32 distances, each within tau, to compare the other way)."""
import gc

import numpy as np
import pytest
import torch

import golden_inputs as GI
import knn_reference as KR

pytestmark = pytest.mark.gpu

#        B, N,    M,    C,   kd,  k,  d
EXACT = [(1, 65, 65, 3, 65, 5, 13), (2, 130, 33, 4, 128, 16, 8), (2, 257, 257, 3, 129, 43, 3), (1, 256, 256, 3, 256, 16, 16),
         (1, 257, 257, 5, 256, 64, 4), (2, 300, 300, 64, 208, 16, 13), (1, 400, 400, 128, 96, 16, 6),
         (2, 1024, 1024, 3, 208, 16, 13)]


def _raw(s, q, kd, k, d, slots, dist=True):
    """The C entry itself: kd is its own argument there (the Python wrapper always searches k * d, and 208 is no multiple
    of the error-bar case's k = 64)."""
    from adaptpoint_amd.fused import _call, _ptr
    B, N, C = s.shape
    M = q.shape[1]
    idx = torch.empty(B, M, k, dtype=torch.int32, device=s.device)
    d2 = torch.empty(B, M, k, device=s.device) if dist else None
    _call("apn_knn_dilated", s.device, B, N, M, C, kd, k, d, _ptr(slots), s.data_ptr(), q.data_ptr(), idx.data_ptr(), _ptr(d2))
    return idx, d2


def _pair(dev, support, query):
    s = torch.from_numpy(support).to(dev)
    return s, (s if query is support else torch.from_numpy(query).to(dev))


@pytest.mark.parametrize("B,N,M,C,kd,k,d", EXACT)
def test_exact_cases_equal_the_reference(dev, B, N, M, C, kd, k, d):
    from adaptpoint_amd.layers import knn_dilated
    support = KR.integer_cloud((B, N, C), seed=N * 131 + C + kd)
    query = support if N == M else KR.integer_cloud((B, M, C), seed=4243)
    s, q = _pair(dev, support, query)
    ref_idx, ref_d2 = KR.knn(support, query, kd)
    # null slots at the given dilation
    assert kd == k * d
    idx, d2 = knn_dilated(s, q, k, d, return_dist=True)
    assert torch.equal(knn_dilated(s, q, k, d), idx)                           # dist2 = NULL: the same indices
    assert idx.dtype == torch.int32 and idx.shape == (B, M, k) and d2.shape == idx.shape
    ranks = np.arange(k) * d
    assert np.array_equal(idx.cpu().numpy(), ref_idx[..., ranks])
    assert np.array_equal(d2.cpu().numpy().astype(np.float64), ref_d2[..., ranks])
    # a seeded permutation's first k as the slot table
    ranks = np.random.default_rng(kd * 7 + k).permutation(kd)[:k]
    slots = torch.from_numpy(ranks.astype(np.int32)).to(dev)
    idx, d2 = knn_dilated(s, q, k, d, slots=slots, return_dist=True)
    assert np.array_equal(idx.cpu().numpy(), ref_idx[..., ranks])
    assert np.array_equal(d2.cpu().numpy().astype(np.float64), ref_d2[..., ranks])


def test_identical_points_come_back_in_index_order(dev):
    from adaptpoint_amd.layers import knn_dilated
    s = torch.full((1, 300, 3), 2.5, device=dev)
    idx, d2 = knn_dilated(s, s, 16, 13, return_dist=True)
    assert torch.equal(idx.cpu(), (torch.arange(16, dtype=torch.int32) * 13).expand(1, 300, 16))
    assert not d2.any()


@pytest.mark.parametrize("C,k,d", [(3, 20, 1), (64, 16, 4), (128, 9, 7), (5, 64, 1)])
def test_up_to_rank_64_it_is_the_old_kernels_list(dev, C, k, d):
    from adaptpoint_amd.layers import knn_dilated, knn_query
    x = torch.from_numpy(GI.seeded_normal((2, 300, C), seed=80 + C).astype(np.float32)).to(dev)
    idx, d2 = knn_dilated(x, x, k, d, return_dist=True)
    old_idx, old_d2 = knn_query(x, x, k * d, return_dist=True)
    assert torch.equal(idx, old_idx[..., ::d]) and torch.equal(d2, old_d2[..., ::d])


@pytest.mark.parametrize("C", [3, 64, 128])
def test_error_bars_on_normal_inputs(dev, C):
    B, N, kd, k = 2, 300, 208, 64
    ranks = np.append(np.arange(0, 187, 3), 207)                       # 0, 3, ..., 186 and 207: k = 64 ranks
    assert len(ranks) == k
    support = GI.seeded_normal((B, N, C), seed=600 + C).astype(np.float32)
    s, _ = _pair(dev, support, support)
    idx, d2 = _raw(s, s, kd, k, 1, torch.from_numpy(ranks.astype(np.int32)).to(dev))
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    tau = (C + 3) * 2.0 ** -24
    d64 = KR.dist2_64(support, support)                               # (B, N, N), every query
    got64 = np.take_along_axis(d64, idx.astype(np.int64), -1)
    err = np.abs(d2.astype(np.float64) - got64) / np.maximum(got64, 1e-300)
    print(f"C={C}: worst |dist2 - d64| / d64 = {np.where(got64 > 0, err, 0).max() / 2.0 ** -24:.2f} x 2^-24 (bar {C + 3})")
    assert (np.abs(d2.astype(np.float64) - got64) <= tau * got64).all()
    assert (idx >= 0).all() and (idx < N).all()
    assert all(len(np.unique(row)) == k for row in idx.reshape(-1, k))                 # k distinct supports
    Dr = np.sort(d64, -1)[..., ranks]                                                   # the float64 r-th smallest
    assert (got64 <= Dr * (1 + 3 * tau)).all() and (got64 >= Dr * (1 - 3 * tau)).all()
    assert (np.diff(d2, axis=-1) >= 0).all()                                            # non-decreasing along k
    assert (np.diff(idx, axis=-1)[np.diff(d2, axis=-1) == 0] > 0).all()                  # equal values: ascending indices


def test_slots_outside_the_list_are_clamped_into_it(dev):
    from adaptpoint_amd.layers import knn_dilated
    support = KR.integer_cloud((2, 300, 3), seed=91)
    s, _ = _pair(dev, support, support)
    kd = 208
    table = np.arange(16, dtype=np.int32) * 13
    table[3], table[7], table[11] = -1, kd + 5, np.iinfo(np.int32).min
    table[12] = np.iinfo(np.int32).max
    idx, d2 = knn_dilated(s, s, 16, 13, slots=torch.from_numpy(table).to(dev), return_dist=True)
    ref_idx, ref_d2 = KR.knn(support, support, kd)
    ranks = np.clip(table.astype(np.int64), 0, kd - 1)
    assert ranks[3] == 0 and ranks[7] == kd - 1 and ranks[11] == 0 and ranks[12] == kd - 1
    assert np.array_equal(idx.cpu().numpy(), ref_idx[..., ranks])
    assert np.array_equal(d2.cpu().numpy().astype(np.float64), ref_d2[..., ranks])


def test_two_runs_are_bit_identical(dev):
    from adaptpoint_amd.layers import knn_dilated
    x = torch.from_numpy(GI.seeded_normal((2, 500, 64), seed=83).astype(np.float32)).to(dev)
    a, b = knn_dilated(x, x, 16, 13, return_dist=True), knn_dilated(x, x, 16, 13, return_dist=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_replay_from_a_hipgraph_reads_the_slot_table_anew(dev):
    """One kernel and no memset node; overwriting the `slots` buffer between replays changes the replayed result to
    the new table's, without recapture."""
    from adaptpoint_amd import graphs
    from adaptpoint_amd.layers import knn_dilated
    x = torch.from_numpy(GI.seeded_normal((2, 300, 64), seed=84).astype(np.float32)).to(dev)
    tables = [torch.arange(16, dtype=torch.int32) * 13, torch.from_numpy(np.random.default_rng(5).permutation(208)[:16].astype(np.int32))]
    slots = tables[0].to(dev)

    def step():
        return list(knn_dilated(x, x, 16, 13, slots=slots, return_dist=True))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up: allocator pools, lazy initialisation
        step()
    torch.cuda.current_stream().wait_stream(side)
    eager = []
    for t in tables:
        slots.copy_(t)
        eager.append([r.clone() for r in step()])
    assert not torch.equal(eager[0][0], eager[1][0])
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(step, what="the dilated kNN query's graph")
    print("dilated kNN graph:", census)
    assert not census.get("memset", 0) and census.get("kernel", 0) == 1
    for which in (0, 1, 0):
        slots.copy_(tables[which])
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager[which], captured):
            assert torch.equal(a, b)
