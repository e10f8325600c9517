"""The ball query's register-chunk scan (csrc/ball_query_body.h) at the places its structure can go wrong, bit-exact
against the CPU oracle: a wave holds 1024 support points in registers (lane l, slot s = point 64 s + l), forms the hit
masks of four slots at a time, emits the hits afterwards, tests saturation once per four slots (256 points), carries
count and first hit across register chunks, and fills the rest of the row itself.

Every comparison is `np.array_equal` with `oracle.ball_query` (indices: no tolerance applies)."""
import numpy as np
import pytest
import torch

import golden_inputs as GI

pytestmark = pytest.mark.gpu

FAR = 50.0          # a coordinate no ball of these tests reaches


def _cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def gpu_ball(radius, k, xyz, q, dev, fill=0):
    import pointnet2_batch_cuda as ext
    x, qq = _cu(xyz, dev), _cu(q, dev)
    b, n, _ = x.shape
    m = qq.shape[1]
    idx = torch.full((b, m, k), fill, dtype=torch.int32, device=dev)
    ext.ball_query_wrapper(b, n, m, radius, k, qq, x, idx)
    torch.cuda.synchronize()
    return idx.cpu().numpy()


def _hits(xyz, q, r):
    """Hit counts per query (float64: only used to state what a case covers, never as the reference)."""
    d2 = ((q[:, :, None].astype(np.float64) - xyz[:, None].astype(np.float64)) ** 2).sum(-1)
    return (d2 < float(np.float32(r)) ** 2).sum(-1)


# ------------------------------------------------------------------ chunk and slot edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097])
def test_chunk_and_slot_edges_vs_oracle(dev, oracle, n):
    """Uniform clouds in [-1, 1]^3 whose sizes straddle a slot (64), a group of four slots (256), a register chunk (1024)
    and the LDS staging chunk (4096); tiles of 1, 7, 33 and 129 queries; rows shorter and longer than a wave.  Radii:
    1e-4 (empty balls), the radius at which a ball holds about three points (fewer hits than nsample; clouds of a few
    points: mostly empty), 4.0 (every point hits: the row saturates inside the first four slots)."""
    xyz = GI.seeded_uniform((3, n, 3), seed=900 + n).astype(np.float32)
    few = float((3.0 * 8.0 * 3.0 / (4.0 * np.pi * n)) ** (1.0 / 3.0))
    for m in (1, 7, 33, 129):
        q = GI.seeded_uniform((3, m, 3), seed=1900 + m).astype(np.float32)
        assert _hits(xyz, q, 1e-4).max() == 0 and _hits(xyz, q, 4.0).min() == n
        if n >= 255 and m >= 33:
            h = _hits(xyz, q, few)
            assert 0 < h.max() and np.median(h) < 32        # the middle radius does what its name says
        for k in (1, 5, 32, 64, 65, 100):
            for r in (1e-4, few, 4.0):
                got = gpu_ball(r, k, xyz, q, dev)
                assert np.array_equal(got, oracle.ball_query(r, k, xyz, q)), (n, m, k, r)


@pytest.mark.parametrize("k", [1, 5, 32, 64, 65, 100])
@pytest.mark.parametrize("kth", [255, 256])
def test_saturation_at_a_group_boundary(dev, oracle, k, kth):
    """The k-th hit is point 255 (the last lane of the first four slots: the once-per-group test stops the scan there)
    or point 256 (the first lane of the next group: the scan must go on).  Later hits (257, 300, 599, 1030) must not
    reach the row.  The first k - 1 hits are spread over the first 255 points."""
    n, m = 1100, 9
    xyz = np.full((2, n, 3), FAR, dtype=np.float32)
    early = np.linspace(0, 254, k - 1).astype(np.int64) if k > 1 else np.zeros(0, np.int64)
    assert len(set(early.tolist())) == k - 1
    near = np.concatenate([early, [kth, 257, 300, 599, 1030]])
    xyz[:, near] = (GI.seeded_uniform((2, len(near), 3), seed=7 + k) * 0.1).astype(np.float32)
    q = np.zeros((2, m, 3), dtype=np.float32)
    got = gpu_ball(0.25, k, xyz, q, dev)
    assert np.array_equal(got, oracle.ball_query(0.25, k, xyz, q))
    assert (got[..., -1] == kth).all() and (got < 257).all()


# ------------------------------------------------------------------ where the only hit sits
@pytest.mark.parametrize("n,at", [(1024, 1023), (2000, 1023), (1000, 999), (65, 64), (1025, 1024), (4097, 4096),
                                  (5000, 4095)])
def test_the_only_hit_at_an_edge(dev, oracle, n, at):
    """One support point inside the ball: lane 63 of slot 15, point n - 1 of a ragged last slot, the first point of the
    second register chunk, the first point of the second staging chunk.  The row repeats it (nsample above 64 too)."""
    xyz = np.full((2, n, 3), FAR, dtype=np.float32)
    xyz[:, at] = (0.01, -0.02, 0.03)
    q = np.zeros((2, 5, 3), dtype=np.float32)
    q[1, 3] = FAR / 2                                              # one empty ball among them
    for k in (1, 32, 100):
        got = gpu_ball(0.25, k, xyz, q, dev)
        assert np.array_equal(got, oracle.ball_query(0.25, k, xyz, q)), k
        assert (got[0] == at).all() and (got[1, 3] == 0).all()


def test_first_hit_carried_across_register_chunks(dev, oracle):
    """Hits in the first and in later register chunks of a 3000-point cloud, fewer than nsample: the fill value is the
    hit of the FIRST chunk, the later chunks append behind the carried count."""
    n = 3000
    xyz = np.full((1, n, 3), FAR, dtype=np.float32)
    near = [700, 1023, 1024, 2047, 2999]
    xyz[0, near] = (GI.seeded_uniform((len(near), 3), seed=3) * 0.1).astype(np.float32)
    q = np.zeros((1, 3, 3), dtype=np.float32)
    got = gpu_ball(0.25, 8, xyz, q, dev)
    assert np.array_equal(got, oracle.ball_query(0.25, 8, xyz, q))
    assert got[0, 0].tolist() == near + [700] * 3


# ------------------------------------------------------------------ strictness
@pytest.mark.parametrize("n,places", [(3, (0, 1, 2)), (300, (63, 64, 299)), (1030, (1023, 1024, 1029))])
def test_strict_inequality_at_the_radius(dev, oracle, n, places):
    """Query at the origin, radius 0.25: (0.25, 0, 0) and its negation have d2 == radius2 exactly (0.0625, no rounding)
    and are no hits; (nextafter(0.25, 0), 0, 0) is one."""
    xyz = np.full((1, n, 3), FAR, dtype=np.float32)
    xyz[0, places[0]] = (0.25, 0, 0)
    xyz[0, places[1]] = (-0.25, 0, 0)
    xyz[0, places[2]] = (np.nextafter(np.float32(0.25), np.float32(0)), 0, 0)
    q = np.zeros((1, 2, 3), dtype=np.float32)
    got = gpu_ball(0.25, 4, xyz, q, dev)
    assert np.array_equal(got, oracle.ball_query(0.25, 4, xyz, q))
    assert (got == places[2]).all()


# ------------------------------------------------------------------ duplicates
@pytest.mark.parametrize("n", [130, 1500])
def test_duplicated_support_points_and_queries_on_them(dev, oracle, n):
    """Every third support point is a copy of point 0; the queries ARE support points (d2 == 0)."""
    xyz = GI.seeded_uniform((3, n, 3), seed=41 + n).astype(np.float32)
    xyz[:, ::3] = xyz[:, :1]
    q = xyz[:, :40].copy()
    for k in (5, 32, 100):
        assert np.array_equal(gpu_ball(0.2, k, xyz, q, dev), oracle.ball_query(0.2, k, xyz, q)), k


# ------------------------------------------------------------------ the two empty-row contracts
@pytest.mark.parametrize("n", [200, 1025, 4100])
def test_drop_in_entry_leaves_rows_of_empty_balls_untouched(dev, oracle, n):
    """Point 0 is out of every ball's reach, so a row of the oracle is all zeros exactly where its ball is empty: there
    the caller's contents must survive, everywhere else the row is the oracle's."""
    xyz = GI.seeded_uniform((2, n, 3), seed=5).astype(np.float32)
    xyz[:, 0] = FAR
    q = GI.seeded_uniform((2, 21, 3), seed=6).astype(np.float32)
    q[:, ::2] += 10.0                                              # every other ball is empty for certain
    got = gpu_ball(0.3, 70, xyz, q, dev, fill=99)
    ref = oracle.ball_query(0.3, 70, xyz, q)
    empty = ~ref.any(-1)
    assert empty[:, ::2].all() and not empty.all()
    assert np.array_equal(got, np.where(empty[..., None], 99, ref))


@pytest.mark.parametrize("n,m", [(300, 64), (1024, 512), (1500, 100)])
def test_zero_writing_entry_leaves_zeros(dev, oracle, n, m):
    """`fused.sample_and_query` never pre-zeroes its buffer.  Its queries are support points, so only radius 0
    (d2 = 0 is not < 0) empties the balls: every row must then be written as zeros over the poisoned buffer; at a
    real radius the same call equals the oracle."""
    from adaptpoint_amd.fused import Sampling, sample_and_query
    xyz = GI.unit_sphere_cloud(3, n, seed=8)
    p = _cu(xyz, dev)
    for radius in (0.0, 0.15):
        smp = Sampling(3, m, 32, dev)
        smp.buf.fill_(-1)
        sample_and_query(p, m, radius, 32, out=smp)
        torch.cuda.synchronize()
        ref = oracle.ball_query(radius, 32, xyz, smp.new_p.cpu().numpy())
        assert np.array_equal(smp.idx.cpu().numpy(), ref), radius
        assert radius > 0 or not ref.any()


def test_two_role_launch_writes_zeros(dev, oracle):
    """The search role of the sampler's launch (fps_ball_kernel: 8 waves, zero-writing) on poisoned buffers."""
    from adaptpoint_amd.fused import Sampling, sample_and_query_many
    clouds = [GI.unit_sphere_cloud(2, 1024, seed=60 + i) for i in range(2)]
    ps = [_cu(c, dev) for c in clouds]
    for radius in (0.0, 0.15):
        outs = [Sampling(2, 500, 32, dev) for _ in ps]
        for o in outs:
            o.buf.fill_(-1)
        sample_and_query_many(ps, 500, radius, 32, outs=outs)
        torch.cuda.synchronize()
        for c, o in zip(clouds, outs):
            ref = oracle.ball_query(radius, 32, c, o.new_p.cpu().numpy())
            assert np.array_equal(o.idx.cpu().numpy(), ref), radius
            assert radius > 0 or not ref.any()


# ------------------------------------------------------------------ the large-launch form, every cloud
@pytest.mark.parametrize("m", [512, 500])
def test_large_launch_every_cloud_vs_oracle(dev, oracle, m):
    """264 clouds x 4 tiles of 128 queries >= 1024 workgroups selects the 16-wave form (csrc/ball_query.hip); m = 500
    leaves its last tile ragged.  All 264 clouds are compared."""
    b, n = 264, 200
    xyz = GI.seeded_uniform((b, n, 3), seed=70).astype(np.float32)
    q = GI.seeded_uniform((b, m, 3), seed=71).astype(np.float32)
    q[5, 9] = FAR                                                  # an empty ball
    got = gpu_ball(0.3, 32, xyz, q, dev)
    assert np.array_equal(got, oracle.ball_query(0.3, 32, xyz, q))
    assert (got[5, 9] == 0).all()
