"""CPU suite: the C-ABI library loads and exports exactly what include/adaptpoint_amd.h
declares (no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adaptpoint_amd.h")


def header_prototypes():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"APN_API\s+(?:const\s+char\s*\*|int)\s*(apn_\w+)\s*\(([^)]*)\)\s*;", src):
        args = [a.strip() for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        protos[m.group(1)] = args
    return protos


@pytest.fixture(scope="module")
def lib():
    from adaptpoint_amd import build as apn_build
    path = apn_build.build()           # hipcc cross-compiles gfx950 without a GPU
    return ctypes.CDLL(path)


def test_header_declares_the_nine_reference_entry_points():
    protos = header_prototypes()
    for name in ["apn_ball_query", "apn_group_points", "apn_group_points_grad", "apn_gather_points",
                 "apn_gather_points_grad", "apn_furthest_point_sampling", "apn_three_nn",
                 "apn_three_interpolate", "apn_three_interpolate_grad"]:
        assert name in protos
        assert protos[name][-1].replace(" ", "") == "void*stream"


def test_library_exports_every_declared_symbol(lib):
    for name in header_prototypes():
        assert hasattr(lib, name), f"{name} declared in the header but not exported"


def test_ctypes_signatures_match_header_arity():
    from adaptpoint_amd import _lib
    protos = header_prototypes()
    for name, argtypes in _lib.SIGNATURES.items():
        assert name in protos, name
        assert len(argtypes) == len(protos[name]), name
        for at, decl in zip(argtypes, protos[name]):
            if "*" in decl:
                assert at is ctypes.c_void_p, (name, decl)
            elif decl.startswith("float"):
                assert at is ctypes.c_float, (name, decl)
            elif decl.startswith("double"):
                assert at is ctypes.c_double, (name, decl)
            elif decl.startswith("size_t"):
                assert at is ctypes.c_size_t, (name, decl)
            elif decl.startswith("long long"):
                assert at is ctypes.c_longlong, (name, decl)
            else:
                assert at is ctypes.c_int, (name, decl)


def test_version_and_error_strings(lib):
    lib.apn_version.restype = ctypes.c_int
    assert lib.apn_version() >= 100
    lib.apn_error_string.restype = ctypes.c_char_p
    assert lib.apn_error_string(0) == b"success"
    assert b"invalid" in lib.apn_error_string(-1)


def test_library_carries_its_flag_line_and_the_loader_checks_it(lib, monkeypatch):
    """a library built with the vectoriser back on (or contraction on) must not load silently.  build.py
    stamps the flag line into the library, refuses flag sets that undo the two correctness flags, treats an object whose
    recorded flags differ from today's as stale; _lib.load() refuses a library whose line lacks them."""
    from adaptpoint_amd import _lib, build as apn_build
    lib.apn_build_flags.restype = ctypes.c_char_p
    flags = lib.apn_build_flags().decode().split()
    assert "-fno-slp-vectorize" in flags and "-ffp-contract=off" in flags and "-O3" in flags
    assert _lib.REQUIRED_BUILD_FLAGS == apn_build.REQUIRED_FLAGS
    obj = os.path.join(apn_build.OBJ, "fps.o")
    assert apn_build._same_flags(obj, os.path.join(apn_build.CSRC, "fps.hip"))
    monkeypatch.setattr(apn_build, "CXXFLAGS", apn_build.CXXFLAGS + ["-DAPN_SOMETHING_ELSE"])
    assert not apn_build._same_flags(obj, os.path.join(apn_build.CSRC, "fps.hip"))       # changed flags: stale object
    monkeypatch.setattr(apn_build, "CXXFLAGS", apn_build.CXXFLAGS + ["-fslp-vectorize"])
    with pytest.raises(RuntimeError, match="refused"):
        apn_build.build()
    monkeypatch.setattr(apn_build, "CXXFLAGS", [f for f in apn_build.CXXFLAGS if "slp" not in f])
    with pytest.raises(RuntimeError, match="refused"):
        apn_build.check_flags()


def test_argument_validation_needs_no_gpu(lib):
    """Bad sizes are rejected before any HIP call; zero sizes are no-ops."""
    f = lib.apn_furthest_point_sampling
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
    assert f(-1, 8, 4, None, None, None, None) == -1
    assert f(0, 8, 4, None, None, None, None) == 0
    assert f(2, 8, 0, None, None, None, None) == 0          # m <= 0: the reference kernel returns at once
    assert f(2, 0, 4, None, None, None, None) == -1
    assert f(2, 8, 4, None, None, None, None) == -1          # null pointers
    g = lib.apn_group_points
    g.restype = ctypes.c_int
    g.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 4
    assert g(1, 4, 8, 0, 3, None, None, None, None) == 0
    assert g(1, 4, 8, 1 << 20, 1 << 20, None, None, None, None) == -1   # npoints*nsample overflows int
    t = lib.apn_furthest_point_sampling_tuned
    t.restype = ctypes.c_int
    t.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    assert t(2, 8, 0, None, None, None, 3, 0, None) == 0      # m <= 0 returns before anything is read
    assert t(2, 8, 4, None, None, None, 0, 0, None) == -1
    assert not hasattr(lib, "apn_fps_set_waves") and not hasattr(lib, "apn_fps_set_algo")   # no process-wide state


def test_argument_validation_of_the_adaptpoint_entries_needs_no_gpu():
    """The per-point layer, spectral-norm, anchor-transform and deformation entries reject bad arguments (and accept
    empty work) before any HIP call, like the reference-boundary entries above."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    assert lib.apn_pw_conv_tiles(4, 1000) == 4 * 8
    assert lib.apn_pw_conv_forward(2, 8, 8, 16, 5, None, None, None, None, None) == EINVAL        # precision 2 or 3
    assert lib.apn_pw_conv_forward(0, 8, 8, 16, 3, None, None, None, None, None) == 0             # no clouds
    assert lib.apn_pw_conv_forward(2, 8, 8, 16, 3, None, None, None, None, None) == EINVAL        # null tensors
    assert lib.apn_pw_bn_act(2, 0, 16, None, None, 0, None, None, 1e-5, 0.1, 1, 1, None, None, None, None, None, None) == EINVAL
    assert lib.apn_pw_bn_act(0, 8, 16, None, None, 0, None, None, 1e-5, 0.1, 1, 1, None, None, None, None, None, None) == 0
    assert lib.apn_pw_conv_grad_weight(2, 8, 8, 16, 3, None, None, None, None, None) == EINVAL
    assert lib.apn_pw_conv_max_backward(2, 129, 8, 16, None, None, None, None, None, 1, None, None, None, None, None) == EINVAL
    assert lib.apn_pw_contract(1, 4, 4, 4, None, 0, 4, 1, None, 0, 4, 1, None, 0, 4, 0, None, 3, None) == EINVAL
    # the raw contraction entries: every check returns before any launch (P: a non-null address that is never read)
    P = 4096
    contract = lambda nbatch=1, ldd=4, splits=0, scratch=None, precision=3, a=P, b=P, d=P: lib.apn_pw_contract(
        nbatch, 4, 4, 4, a, 0, 4, 1, b, 0, 4, 1, d, 0, ldd, splits, scratch, precision, None)
    assert contract(ldd=3) == EINVAL                                   # ldd < q
    assert contract(ldd=5, splits=2, scratch=P) == EINVAL              # the split form writes a tight result
    assert contract(splits=2) == EINVAL                                # ... and needs its scratch
    assert contract(splits=-1) == EINVAL
    assert contract(precision=4) == EINVAL and contract(precision=1) == EINVAL
    assert contract(nbatch=65536) == EINVAL and contract(nbatch=0) == EINVAL
    assert contract(a=None) == EINVAL and contract(b=None) == EINVAL and contract(d=None) == EINVAL
    I2, L2, P2 = ctypes.c_int * 2, ctypes.c_longlong * 2, ctypes.c_void_p * 2

    def contract2(nbatch=(1, 1), ldd=(4, 4), splits=(0, 0), scratch=(None, None), precision=3, null=None, a=(P, P)):
        args = [I2(*nbatch), I2(4, 4), I2(4, 4), I2(4, 4), P2(*a), L2(0, 0), I2(4, 4), P2(P, P), L2(0, 0), I2(4, 4), P2(P, P),
                L2(0, 0), I2(*ldd), I2(*splits), P2(*scratch)]
        if null is not None:
            args[null] = None
        return lib.apn_pw_contract2(1, 1, precision, *args, None)
    assert contract2(ldd=(4, 3)) == EINVAL and contract2(ldd=(3, 4)) == EINVAL                 # ldd < q
    assert contract2(splits=(2, 0), scratch=(P, P)) == EINVAL and contract2(splits=(0, 2), scratch=(P, P)) == EINVAL   # both or neither
    assert contract2(splits=(2, 2), scratch=(P, None)) == EINVAL
    assert contract2(precision=4) == EINVAL
    assert contract2(nbatch=(1, 65536)) == EINVAL and contract2(nbatch=(0, 1)) == EINVAL
    assert contract2(a=(P, None)) == EINVAL
    for i in range(15):
        assert contract2(null=i) == EINVAL, i                          # a null array
    # split-K shares: short contractions down to two chunks per share, long ones at least eight, <= 256 workgroups (one per CU)
    assert lib.apn_pw_contract_splits(1, 256, 256, 512) == 8 and lib.apn_pw_contract_splits(32, 512, 1536, 256) == 5
    assert lib.apn_spectral_norm(0, 4, None, 1, 1e-12, None, None, None, None, None, None, None, None) == EINVAL
    assert lib.apn_spectral_norm_blocks(1024, 512) == 512 and lib.apn_spectral_norm_blocks(15, 1) == 1
    assert lib.apn_anchor_transforms(0, None, None, None, 10.0, 3.0, 0.25, None, None, None) == 0
    assert lib.apn_anchor_transforms(4, None, None, None, 10.0, 3.0, 0.25, None, None, None) == EINVAL
    assert lib.apn_deform_forward(2, 5000, 4, None, None, None, None, None, None, 0.5, None, None, None, None) == EINVAL   # n <= 4096
    assert lib.apn_deform_forward(2, 1024, 9, None, None, None, None, None, None, 0.5, None, None, None, None) == EINVAL   # m <= 8
    assert lib.apn_deform_forward(0, 1024, 4, None, None, None, None, None, None, 0.5, None, None, None, None) == 0
    deform_fwd = lambda n=1024, m=4, sigma=0.5: lib.apn_deform_forward(2, n, m, P, P, P, P, P, None, sigma, P, P, P, None)
    assert deform_fwd(n=4097) == EINVAL and deform_fwd(m=9) == EINVAL and deform_fwd(sigma=0.0) == EINVAL    # the limit alone refuses
    # the two backward entries: every check returns before a launch (P: a non-null address that is never read)

    def deform_bwd(b=2, n=1024, m=4, sigma=0.5, null=(), mask=P, g_mask=P):
        ptr = {k: (None if k in null else P) for k in ("xyz", "anchors", "axes", "z", "stat", "g_out", "g_lin", "g_off")}
        return lib.apn_deform_backward(b, n, m, ptr["xyz"], ptr["anchors"], ptr["axes"], mask, sigma, ptr["z"], ptr["stat"],
                                       ptr["g_out"], ptr["g_lin"], ptr["g_off"], g_mask, None)
    everything = ("xyz", "anchors", "axes", "z", "stat", "g_out", "g_lin", "g_off")
    # the limits, with every pointer non-null: only the limit itself can be what refuses the call
    assert deform_bwd(n=4097) == EINVAL and deform_bwd(n=0) == EINVAL and deform_bwd(n=-1) == EINVAL           # 0 < n <= 4096
    assert deform_bwd(m=9) == EINVAL and deform_bwd(m=0) == EINVAL                                             # 0 < m <= 8
    assert deform_bwd(sigma=0.0) == EINVAL and deform_bwd(sigma=-0.5) == EINVAL                                # sigma > 0
    assert deform_bwd(b=-1) == EINVAL
    assert deform_bwd(b=0, null=everything, mask=None, g_mask=None) == 0                                     # no clouds
    for name in everything:
        assert deform_bwd(null=(name,)) == EINVAL, name                                                      # required pointers

    def transforms_grad(n=4, null=()):
        ptr = {k: (None if k in null else P) for k in ("prob", "keep", "axes", "g_prob")}
        return lib.apn_anchor_transforms_grad(n, ptr["prob"], ptr["keep"], ptr["axes"], 10.0, 3.0, 0.25, P, P, ptr["g_prob"], None)
    assert transforms_grad(n=-1) == EINVAL                                                                   # all pointers non-null
    assert transforms_grad(n=0, null=("prob", "keep", "axes", "g_prob")) == 0
    for name in ("prob", "keep", "axes", "g_prob"):
        assert transforms_grad(null=(name,)) == EINVAL, name


def test_argument_validation_of_the_attention_entries_needs_no_gpu():
    """The five apn_attention_* entries reject null pointers, m = 0, an m the kernel has no tile for, b / heads of 0 or
    above 65535 (grid dimensions) and pointers that their 16-byte vector accesses could not take -- all before any launch
    (P: a non-null, 16-byte aligned address that is never read)."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    EINVAL, P = -1, 4096
    assert lib.apn_attention_small_max() == 32

    def prep(b=1, m=32, heads=1, q=P, k=P, v=P, images=P, for_backward=1):
        return lib.apn_attention_prep(b, m, heads, q, k, v, images, for_backward, None)

    def fwd(b=1, m=32, heads=1, images=P, out=P, lse=P):
        return lib.apn_attention_fwd(b, m, heads, images, out, lse, None)

    def bwd(b=1, m=32, heads=1, images=P, out=P, lse=P, g_out=P, scratch=P, dq=P, dk=P, dv=P):
        return lib.apn_attention_bwd(b, m, heads, images, out, lse, g_out, scratch, dq, dk, dv, None)

    def small_fwd(b=1, m=4, heads=1, q=P, k=P, v=P, out=P):
        return lib.apn_attention_small_fwd(b, m, heads, q, k, v, out, None)

    def small_bwd(b=1, m=4, heads=1, q=P, k=P, v=P, g_out=P, dq=P, dk=P, dv=P):
        return lib.apn_attention_small_bwd(b, m, heads, q, k, v, g_out, dq, dk, dv, None)

    pointers = {prep: ["q", "k", "v", "images"], fwd: ["images", "out", "lse"],
                bwd: ["images", "out", "lse", "g_out", "scratch", "dq", "dk", "dv"], small_fwd: ["q", "k", "v", "out"],
                small_bwd: ["q", "k", "v", "g_out", "dq", "dk", "dv"]}
    for entry, names in pointers.items():
        for name in names:
            assert entry(**{name: None}) == EINVAL, (entry.__name__, name)
        assert entry(m=0) == EINVAL and entry(m=-32) == EINVAL and entry(m=33) == EINVAL, entry.__name__
        for bad in (0, -1, 65536):
            assert entry(b=bad) == EINVAL and entry(heads=bad) == EINVAL, (entry.__name__, bad)
    for entry in (prep, fwd, bwd):
        assert entry(m=16) == EINVAL and entry(m=48) == EINVAL                     # whole 32-tiles only
    # float4 / uint4 / bf16x8 accesses: 16-byte alignment of what they reach
    aligned = {prep: ["images"], fwd: ["images", "out"], bwd: ["images", "scratch", "dq", "dk", "dv"]}
    for entry, names in aligned.items():
        for name in names:
            for off in (2, 4, 8):
                assert entry(**{name: P + off}) == EINVAL, (entry.__name__, name, off)
