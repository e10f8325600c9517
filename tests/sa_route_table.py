"""The routing table of `SetAbstraction(fused=True)`: one row per kind of call, with the path it takes, whether its
residual branch runs inside the kernels, what the index stage (`sample` + `index_for`) builds for it, and the fallback
reason it records.  tests/test_sa_route_cpu.py checks `set_abstraction.route` against it on plain values;
tests/test_gpu_sa_route.py runs every row on the device and records what the forward and the index stage actually did."""
from adaptpoint_amd.set_abstraction import SetAbstraction

RESIDENT_INDEX = ("geo", "tmap", "rowmap")


def block(cin, cout, stride=2, nsample=32, radius=0.15, use_res=True, is_head=False):
    """A PointNeXt-S set-abstraction block (cfgs/scanobjectnn/pointnext-s.yaml) with fused=True."""
    return SetAbstraction(cin, cout, layers=1 if is_head else 2, stride=stride, fused=True, is_head=is_head,
                          group_args={'NAME': 'ballquery', 'radius': radius, 'nsample': nsample, 'normalize_dp': True},
                          norm_args={'norm': 'bn'}, act_args={'act': 'relu'}, conv_args={'order': 'conv-norm-act'},
                          use_res=use_res)


def _no_final_relu(b):
    b.convs[1] = b.convs[1][:2]
    return b


def _momentum_none(b):
    b.convs[0][1].momentum = None
    return b


def _no_kernel(c_in, widths, K):
    return f"C_in={c_in} -> {widths}, K={K}: no fused kernel for this shape"


BIG = "N=20000 > 16384: index stage beyond the resident samplers"

# name: (make block, (C_in, B, N), prefer_wide, sampling handed in, CUDA tensors,
#        expected (path, width-generic kernels, residual branch fused, index stage, fallback reason))
ROWS = {
    "stage1":            (lambda: block(32, 64), (32, 32, 1024), False, False, True,
                          ("resident", False, True, RESIDENT_INDEX, None)),
    "stage1-wide":       (lambda: block(32, 64), (32, 32, 1024), True, False, True,
                          ("wide", True, True, ("index", "fq"), None)),
    "stage2":            (lambda: block(64, 128, radius=0.225), (64, 32, 512), False, False, True,
                          ("wide", True, True, ("index", "fq"), None)),
    "stage2-wide":       (lambda: block(64, 128, radius=0.225), (64, 32, 512), True, False, True,
                          ("wide", True, True, ("index", "fq"), None)),
    "stage3":            (lambda: block(128, 256, radius=0.3375), (128, 32, 256), False, False, True,
                          ("wide", True, False, ("index",), None)),
    "stage3-wide":       (lambda: block(128, 256, radius=0.3375), (128, 32, 256), True, False, True,
                          ("wide", True, False, ("index",), None)),
    "stage4":            (lambda: block(256, 512, radius=0.50625), (256, 32, 128), False, False, True,
                          ("wide", True, False, ("index",), None)),
    "stage4-wide":       (lambda: block(256, 512, radius=0.50625), (256, 32, 128), True, False, True,
                          ("wide", True, False, ("index",), None)),
    "identity-skip":     (lambda: block(64, 64), (64, 8, 1024), False, False, True,
                          ("grouped", True, False, (), None)),
    "no-res-relu":       (lambda: block(32, 64, use_res=False), (32, 8, 1024), False, False, True,
                          ("resident", False, False, RESIDENT_INDEX, None)),
    "no-res-no-relu":    (lambda: _no_final_relu(block(32, 64, use_res=False)), (32, 8, 1024), False, False, True,
                          ("resident", False, False, RESIDENT_INDEX, None)),
    "big-cloud":         (lambda: block(32, 64), (32, 1, 20000), False, False, True,
                          ("grouped", False, False, (), BIG)),
    "big-cloud-sampled": (lambda: block(32, 64), (32, 1, 20000), False, True, True,
                          ("wide", True, True, ("index", "fq"), None)),
    "momentum-none":     (lambda: _momentum_none(block(32, 64)), (32, 8, 1024), False, False, True,
                          ("composed", False, False, (), _no_kernel(32, [32, 64], 32))),
    "h-outside-widths":  (lambda: block(32, 96), (32, 8, 1024), False, False, True,
                          ("composed", False, False, (), _no_kernel(32, [48, 96], 32))),
    "k16":               (lambda: block(32, 64, nsample=16), (32, 8, 1024), False, False, True,
                          ("composed", False, False, (), _no_kernel(32, [32, 64], 16))),
    "cpu-tensors":       (lambda: block(32, 64), (32, 2, 256), False, False, False,
                          ("composed", False, False, (), _no_kernel(32, [32, 64], 32))),
    "is-head":           (lambda: block(4, 32, stride=1, use_res=False, is_head=True), (4, 8, 1024), False, False, True,
                          ("stem", False, False, (), None)),
    "all-aggr":          (lambda: block(512, 512, stride=1), (512, 8, 64), False, False, True,
                          ("group_all", False, False, (), None)),
}
