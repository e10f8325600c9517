"""Regenerates tests/golden/online_aug_golden.npz (run in the BUILD container only):

    python tests/golden/make_golden_online_aug.py

The reference's own `PointWOLF_classversion` (openpoints/online_aug/pointwolf.py, its FPS routed to oracle/) and
`rsmix_provider.rsmix` run on CPU under fixed seeds, imported in memory through make_golden's stubs (nothing copied).

  pw_*     B=8, N=2048: the input seed, the torch seed, the draws the reference consumed (recorded as it made them, in
           PointWOLF.draw_params' packed layout), the anchors, its output, and the float64 restatement's distance to it.
  rs<i>_*  B=8, N=2048, C=4, nsample=512, knn on and off, seeds giving a small and a large cut_rad: the numpy seed, the
           labels, the reference's lam / label_a / label_b, and its mixed batch in a compact lossless form (per cloud
           the erased points as a mask, the appended rows; tests/online_aug_reference.rsmix_reconstruct rebuilds it and
           this script asserts that it equals the reference's output bit for bit).

A seed is rejected when any RSMix selection changes under another float64 rounding of the squared distance
(online_aug_reference.rsmix_distance's "reversed" and "exact" orders; a fused multiply-add changes nothing there, as
every product is exact), so the golden does not depend on how the expanded distance rounds.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import online_aug_reference as R  # noqa: E402

OUT = os.path.join(HERE, "online_aug_golden.npz")
B, N, C, NSAMPLE = 8, 2048, 4, 512


def import_online_aug():
    MG.import_reference()                       # stubs + sys.path
    import openpoints.online_aug.pointwolf as ref_pw
    import openpoints.online_aug.rsmix_provider as ref_rs
    ref_pw.furthest_point_sample = MG._OracleOps.furthest_point_sample
    return ref_pw, ref_rs


def record_pointwolf(ref_pw, xyz, seed):
    """Run the reference's PointWOLF on CPU, recording every random tensor it makes, in order."""
    rec = []
    orig_uniform, orig_bern, orig_randint = torch.Tensor.uniform_, torch.bernoulli, torch.randint

    def uniform_(self, *a, **k):
        out = orig_uniform(self, *a, **k)
        rec.append(out.clone())
        return out

    def bernoulli(*a, **k):
        out = orig_bern(*a, **k)
        rec.append(out.clone())
        return out

    def randint(*a, **k):
        out = orig_randint(*a, **k)
        rec.append(out.clone())
        return out

    torch.manual_seed(seed)
    torch.Tensor.uniform_, torch.bernoulli, torch.randint = uniform_, bernoulli, randint
    try:
        _, out = ref_pw.PointWOLF_classversion()(torch.from_numpy(xyz))
    finally:
        torch.Tensor.uniform_, torch.bernoulli, torch.randint = orig_uniform, orig_bern, orig_randint
    # uniform(keep), bernoulli, randint(axis), uniform(degree), uniform(scale), uniform(translation), randint(kernel axis)
    assert len(rec) == 7, len(rec)
    _, keep, code, deg, scale, trl, kcode = rec
    draws = torch.cat([keep.reshape(-1), code.reshape(-1).float(), deg.reshape(-1), scale.reshape(-1),
                       trl.reshape(-1), kcode.reshape(-1).float()]).numpy()
    return out.numpy(), draws


def rsmix_seed(ref_rs, points, knn, want_small, start):
    """The first seed from `start` whose cut_rad is small (0.1 .. 0.3) or large (> 0.75) and whose selections every
    rounding variant agrees on."""
    for seed in range(start, start + 1000):
        np.random.seed(seed)
        cut_rad = np.random.beta(1.0, 1.0)
        if not (0.1 < cut_rad < 0.3 if want_small else cut_rad > 0.75):
            continue
        perm = np.random.choice(B, B, replace=False)
        i1 = np.random.randint(0, N, (B, 1))[:, 0]
        i2 = np.random.randint(0, N, (B, 1))[:, 0]
        sets = [R.rsmix_sets(points, cut_rad, perm, i1, i2, NSAMPLE, knn, order) for order in
                ("reference", "reversed", "exact")]
        if all(np.array_equal(a, b) for s in sets[1:] for a, b in zip(sets[0][0] + sets[0][1], s[0] + s[1])):
            return seed
        print(f"  seed {seed}: a selection depends on the rounding -- rejected")
    raise SystemExit("no seed found")


def main():
    from oracle import oracle as O
    ref_pw, ref_rs = import_online_aug()
    g = {}
    # ---- PointWOLF
    pw_points_seed, pw_seed = 401, 4242
    xyz = np.ascontiguousarray(R.golden_points(pw_points_seed)[:, :, :3])
    out, draws = record_pointwolf(ref_pw, xyz, pw_seed)
    fidx = O.furthest_point_sampling(xyz, 4)
    dist = float(np.abs(R.pointwolf_f64(xyz, fidx, draws).numpy() - out).max())
    print(f"PointWOLF: float64 restatement vs reference {dist:.3e}")
    g.update(pw_points_seed=pw_points_seed, pw_seed=pw_seed, pw_draws=draws, pw_fidx=fidx, pw_out=out,
             pw_restatement_dist=dist)
    # ---- RSMix
    rs_points_seed = 402
    points = R.golden_points(rs_points_seed)
    label = (np.arange(B) * 7 % 15).astype(np.int64).reshape(B, 1)
    g.update(rs_points_seed=rs_points_seed, rs_label=label[:, 0])
    start = 1
    for i, (knn, small) in enumerate([(False, True), (False, False), (True, True), (True, False)]):
        seed = rsmix_seed(ref_rs, points, knn, small, start)
        start = seed + 1
        # which points each cloud erases: the reference's own erase index, recorded from its cut_points* call
        seen = []
        fn_name = "cut_points_knn" if knn else "cut_points"
        orig = getattr(ref_rs, fn_name)

        def wrapped(*a, **k):
            r = orig(*a, **k)
            seen.append(r[0].copy())
            return r
        setattr(ref_rs, fn_name, wrapped)
        try:
            np.random.seed(seed)
            mixed, lam, la, lb = ref_rs.rsmix(points.copy(), label.copy(), beta=1.0, n_sample=NSAMPLE, KNN=knn)
        finally:
            setattr(ref_rs, fn_name, orig)
        erase_idx = seen[0]
        erased = np.zeros((B, N), bool)
        counts_e = np.zeros(B, np.int64)
        appended = []
        for c in range(B):
            if erase_idx[c][0][0] != N:
                e = np.unique(erase_idx[c].reshape(-1))
                erased[c, e] = True
                counts_e[c] = len(e)
                appended.append(mixed[c][N - len(e):])
        appended = np.concatenate(appended, 0).astype(np.float32) if appended else np.zeros((0, C), np.float32)
        assert np.array_equal(R.rsmix_reconstruct(points, erased, appended, counts_e), mixed.astype(np.float32))
        assert np.array_equal(mixed.astype(np.float32), mixed)
        # the restatement reproduces the reference exactly
        np.random.seed(seed)
        m2, lam2, _, lb2, counts = R.rsmix_np(points, label, 1.0, NSAMPLE, knn)
        assert np.array_equal(m2, mixed) and np.array_equal(lam2, lam.astype(np.float32)) and np.array_equal(lb2, lb)
        np.random.seed(seed)
        cut_rad = np.random.beta(1.0, 1.0)
        print(f"RSMix case {i}: knn={knn} seed={seed} cut_rad={cut_rad:.3f} |E|={counts[:B].tolist()} "
              f"|A|={counts[B:].tolist()}")
        g.update({f"rs{i}_knn": knn, f"rs{i}_seed": seed, f"rs{i}_lam": lam.astype(np.float32),
                  f"rs{i}_label_a": np.asarray(la).reshape(B), f"rs{i}_label_b": np.asarray(lb).reshape(B),
                  f"rs{i}_erased": np.packbits(erased, axis=1), f"rs{i}_appended": appended,
                  f"rs{i}_counts": counts})
    np.savez_compressed(OUT, **g)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
