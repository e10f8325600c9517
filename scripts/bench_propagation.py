"""The imitator's four feature-propagation decoders, forward + backward, hoisted (adaptpoint_amd.propagation) against
composed (three_interpolate + cat + pointwise.conv_bn_act), alternating in ONE process.

    python scripts/bench_propagation.py [--batch 32] [--points 1024 2048] [--iters 200] [--warmup 20] [--eager] [--out FILE]

Each form is captured into a hipGraph and the replays are timed (a layer is 12-17 launches of a few microseconds: issued
eagerly the host's launch rate is what gets measured, ~300 us per form whatever the shape); `--eager` times the calls.

Per layer and in total: device-event times of both forms, and the algorithmic multiply-adds and bytes of both forms
computed from the shapes.  `two_launches`: the hoisted block with its product pairs issued as two plain launches each
(what apn_pw_contract2 is there to avoid).  One JSON line per layer and per total.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from adaptpoint_amd import layers, pointwise, propagation

WIDTHS = (64, 128, 256, 512, 1024)          # stage widths on N, N/2 ... N/16 points


def decoder_shapes(N):
    """(C1, C2, O, n, m) of decode_list[0..3]: the coarsest pair first."""
    out = []
    for i in range(4):
        c1, c2 = WIDTHS[-(i + 2)], WIDTHS[-(i + 1)]
        out.append((c1, c2, c1, N >> (3 - i), N >> (4 - i)))
    return out


def algorithmic(B, C1, C2, O, n, m):
    """Multiply-adds and bytes (float32 tensors read or written once per use) of forward + backward, both forms."""
    composed_mac = 3 * B * O * (C1 + C2) * n + 2 * 3 * B * C2 * n
    hoisted_mac = 3 * B * O * (C1 * n + C2 * m) + 2 * 3 * B * O * n
    cat = B * (C1 + C2) * n
    composed_bytes = 4 * (B * C2 * m + B * C2 * n                    # interpolate: read f2, write up
                          + B * C1 * n + B * C2 * n + cat            # cat: read both, write x
                          + cat + 2 * B * O * n                      # conv: read x, write y; bn: write out
                          + 3 * B * O * n + 2 * cat + cat            # backward: g, y, gy; gx written, x and gy read for gW
                          + 2 * cat                                  # the two slice copies of the cat's backward
                          + B * C2 * n + B * C2 * m)                 # interpolate_grad
    hoisted_bytes = 4 * (B * C1 * n + B * C2 * m + B * O * n + B * O * m     # the pair: read f1, f2, write a, u
                         + 2 * B * O * n + B * O * m + B * O * n              # blend: read a, u, write y; bn: write out
                         + 3 * B * O * n + B * O * n + 2 * B * O * m          # backward: g, y, gy; gu zeroed and written
                         + 2 * (B * C1 * n + B * C2 * m) + 2 * (B * O * n + B * O * m))
    return {"composed_mac": composed_mac, "hoisted_mac": hoisted_mac, "composed_bytes": composed_bytes,
            "hoisted_bytes": hoisted_bytes}


class _TwoLaunches:
    """propagation's pair launcher replaced by two plain apn_pw_contract launches each (timing only: the folded
    weight-gradient blocks are not copied into their place): the measurement of what the paired launch saves."""

    def __enter__(self):
        self.orig = propagation._contract2

        def two(dev, a_kcont, b_kcont, probs, splits=None, scratch=None):
            from adaptpoint_amd.fused import _call
            lib = propagation._lib.load()
            for p in probs:
                nb, r, q, k, a, ab, lda, b, bb, ldb, d, db, ldd = p
                if splits:
                    s = lib.apn_pw_contract_splits(nb, r, q, k)
                    sc = torch.empty(s, r, q, device=dev)
                    tmp = torch.empty(r, q, device=dev)
                    _call("apn_pw_contract", dev, nb, r, q, k, a, ab, lda, int(a_kcont), b, bb, ldb, int(b_kcont),
                          tmp.data_ptr(), 0, q, s, sc.data_ptr(), pointwise.PRECISION)
                else:
                    _call("apn_pw_contract", dev, nb, r, q, k, a, ab, lda, int(a_kcont), b, bb, ldb, int(b_kcont),
                          d, db, ldd, 0, None, pointwise.PRECISION)
        propagation._contract2 = two
        return self

    def __exit__(self, *exc):
        propagation._contract2 = self.orig
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--eager", action="store_true", help="time eager calls instead of hipGraph replays")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.batch
    lines = []
    for N in a.points:
        g = torch.Generator().manual_seed(N)
        xyz = [torch.rand(B, N >> i, 3, generator=g).to(dev) for i in range(5)]
        totals = {}
        for li, (C1, C2, O, n, m) in enumerate(decoder_shapes(N)):
            conv = torch.nn.Conv1d(C1 + C2, O, 1, bias=False).to(dev)
            bn = torch.nn.BatchNorm1d(O).to(dev)
            f1 = torch.randn(B, C1, n, generator=g).to(dev).requires_grad_(True)
            f2 = torch.randn(B, C2, m, generator=g).to(dev).requires_grad_(True)
            gout = torch.randn(B, O, n, generator=g).to(dev)
            lvl = 3 - li
            nearest, weights = layers.three_nn_weights(xyz[lvl], xyz[lvl + 1])
            params = [f1, f2, conv.weight, bn.weight, bn.bias]

            def hoisted():
                return torch.autograd.grad(propagation.propagate(f1, f2, nearest, weights, conv, bn), params, gout)

            def composed():
                x = torch.cat([f1, layers.three_interpolate(f2, nearest, weights)], dim=1)
                return torch.autograd.grad(pointwise.conv_bn_act(x, conv, bn), params, gout)

            def two_launches():
                with _TwoLaunches():
                    return hoisted()
            forms = {"hoisted": hoisted, "composed": composed, "two_launches": two_launches}
            if not a.eager:
                from adaptpoint_amd import graphs
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(3):
                        for fn in forms.values():
                            fn()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                keep = {k: graphs.capture(fn, leaves=params, what=k) for k, fn in forms.items()}
                forms = {k: v[0].replay for k, v in keep.items()}
            for _ in range(a.warmup):
                for fn in forms.values():
                    fn()
            torch.cuda.synchronize()
            ev = {k: [] for k in forms}
            for _ in range(a.iters):                    # alternating: both forms see the same clocks and cache state
                for k, fn in forms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    ev[k].append((e0, e1))
            torch.cuda.synchronize()
            res = {"bench": "feature propagation fwd+bwd", "B": B, "N": N, "layer": li, "C1": C1, "C2": C2, "O": O, "n": n, "m": m,
                   "launch": "eager" if a.eager else "hipGraph replay"}
            for k, pairs in ev.items():
                t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs)
                res[k + "_us_median"] = round(t[len(t) // 2], 1)
                res[k + "_us_p10"] = round(t[len(t) // 10], 1)
                res[k + "_us_p90"] = round(t[(9 * len(t)) // 10], 1)
                totals[k] = totals.get(k, 0.0) + t[len(t) // 2]
            res.update(algorithmic(B, C1, C2, O, n, m))
            lines.append(res)
            print(json.dumps(res), flush=True)
        tot = {"bench": "feature propagation fwd+bwd, four decoders", "B": B, "N": N,
               **{k + "_us_median_sum": round(v, 1) for k, v in totals.items()}}
        lines.append(tot)
        print(json.dumps(tot), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
