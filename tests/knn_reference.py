"""The kNN contract of `apn_knn_query` (include/adaptpoint_amd.h) stated in numpy (tests/test_gpu_knn.py): float64
squared distances by direct differences -- exact for the integer inputs of the exact cases -- and a stable argsort, so
that equal distances keep ascending support indices."""
import numpy as np


def dist2_64(support, query):
    """(B,M,N) float64: d2[b,q,s] = sum_c (query[b,q,c] - support[b,s,c])^2."""
    s, q = np.asarray(support, np.float64), np.asarray(query, np.float64)
    out = np.empty((s.shape[0], q.shape[1], s.shape[1]))
    for b in range(s.shape[0]):                                   # (per cloud: the (M,N,C) differences stay small)
        out[b] = np.square(q[b][:, None, :] - s[b][None, :, :]).sum(-1)
    return out


def knn(support, query, k):
    """-> (idx (B,M,k) int32, dist2 (B,M,k) float64): the k smallest keys (d2, support index), ascending."""
    d = dist2_64(support, query)
    order = np.argsort(d, axis=-1, kind="stable")[..., :k]
    return order.astype(np.int32), np.take_along_axis(d, order, -1)


def integer_cloud(shape, seed, lo=-4, hi=4):
    """Integer coordinates in [lo, hi] as float32: every squared distance is an integer <= 64 C <= 8192, exact in
    fp32 under any summation order, and ties are plentiful."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float32)
