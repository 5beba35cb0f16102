"""bf16 GEMM kernels against exact references: bitwise equality on the integer operands of
gemm_exact_cases.py (no tolerance anywhere in those tests), and real-valued operands against
the derived per-element bound.  Shapes are the smallest that reach each code path of
csrc/gemm.hip / gemm256.hip; (T, K, N) is always (tokens, reduction length, output width)."""
import functools

import pytest
import torch

import gemm_exact_cases as C

pytestmark = pytest.mark.gpu


def _ext():
    from distributed_pipeline_amd.ops._ext import get_ext
    return get_ext(required=True)


def _restore():
    ext = _ext()
    ext.set_gemm256(True)
    ext.set_gemmp_grid_cap(0)
    ext.set_gemmp_half(-1)
    ext.set_gemmp_dynamic(False)   # the library default (world == 1)
    ext.set_wgrad4w(False)         # the library default


@pytest.fixture(autouse=True)
def _switches():
    """Every launcher switch a test of this module flips is back at its default afterwards."""
    yield
    _restore()


def _set(gemm256=True, cap=0, half=-1, dynamic=False):
    ext = _ext()
    ext.set_gemm256(gemm256)
    ext.set_gemmp_grid_cap(cap)
    ext.set_gemmp_half(half)
    ext.set_gemmp_dynamic(dynamic)


# (id, (T, K, N), switches, persistent kernel expected)
PATHS = (
    [(f"tile128-{s[0]}x{s[1]}x{s[2]}", s, dict(gemm256=False), False) for s in C.SHAPES_128]
    + [(f"tile256-{s[0]}x{s[1]}x{s[2]}", s, {}, True) for s in C.SHAPES_256]
    # 12 tiles on 3 workgroups: 4 tiles each through the cross-tile pipeline, static schedule
    + [("cap3-static", C.SHAPE_STATIC, dict(cap=3), True)]
    # 24 tiles > grid 8 >= 8: gemmp_launch takes the queue (a null queue with dynamic off)
    + [("cap8-queue-off", C.SHAPE_QUEUE, dict(cap=8, dynamic=False), True),
       ("cap8-queue-on", C.SHAPE_QUEUE, dict(cap=8, dynamic=True), True)]
    + [("half2", C.SHAPE_HALF, dict(half=2), True), ("half0", C.SHAPE_HALF, dict(half=0), True)]
)
PATH_IDS = [p[0] for p in PATHS]
PERSISTENT = [p for p in PATHS if p[3]]
PERSISTENT_IDS = [p[0] for p in PERSISTENT]


def _cuda(*ts):
    return [t.cuda() if t is not None else None for t in ts]


@pytest.mark.parametrize("name,shape,sw,persistent", PATHS, ids=PATH_IDS)
def test_forward_exact(name, shape, sw, persistent):
    """gemm_nt (act 0) with and without bias, gemm_nt_into a row slice of a larger buffer, the
    head-major store, and the residual epilogue at p = 0."""
    ext = _ext()
    T, K, N = shape
    x, W, b, res, _ = C.nt_case(11, T, K, N, bias=True, res=True)
    xg, Wg, bg, rg = _cuda(x, W, b, res)
    ref_b, ref_0 = C.ref_nt(x, W, b), C.ref_nt(x, W)
    _set(**sw)
    y, z, mode = ext.gemm_nt(xg, Wg, bg, 0)
    assert z is None and mode == 0
    C.assert_exact(f"{name} gemm_nt bias", y, ref_b)
    y, _, _ = ext.gemm_nt(xg, Wg, None, 0)
    C.assert_exact(f"{name} gemm_nt no bias", y, ref_0)
    # a row slice of a larger buffer: the rows around it keep their fill
    buf = torch.full((T + 256, N), 7.0, device="cuda", dtype=torch.bfloat16)
    ext.gemm_nt_into(xg, Wg, bg, buf[128:128 + T])
    C.assert_exact(f"{name} gemm_nt_into", buf[128:128 + T], ref_b)
    assert bool((buf[:128] == 7).all()) and bool((buf[128 + T:] == 7).all()), f"{name}: gemm_nt_into wrote outside its slice"
    if not persistent:
        assert ext.gemm_nt_res(xg, Wg, bg, rg, 0.0, 1, 0) is None
        return
    for L in (128, 256):
        y, _, _ = ext.gemm_nt(xg, Wg, bg, 0, 0, L)
        C.assert_exact(f"{name} gemm_nt head-major L={L}", y, C.head_major(ref_b, L))
    h = ext.gemm_nt_res(xg, Wg, bg, rg, 0.0, 1234, 5)
    C.assert_exact(f"{name} gemm_nt_res p=0", h, C.ref_nt(x, W, b, res))
    h = ext.gemm_nt_res(xg, Wg, None, rg, 0.0, 1234, 5)
    C.assert_exact(f"{name} gemm_nt_res p=0 no bias", h, C.ref_nt(x, W, None, res))


@pytest.mark.parametrize("name,shape,sw,persistent", PATHS, ids=PATH_IDS)
def test_dgrad_exact(name, shape, sw, persistent):
    """gemm_nn / gemm_nn_into with and without the transposed weight, gemm_nn_acc_ onto an
    integer dx."""
    ext = _ext()
    T, K, N = shape
    dy, W, dx0, ref_acc = C.nn_case(12, T, K, N, acc=True)
    ref = C.ref_nn(dy, W)
    dyg, Wg, dx0g = _cuda(dy, W, dx0)
    WT = Wg.t().contiguous()
    _set(**sw)
    C.assert_exact(f"{name} gemm_nn", ext.gemm_nn(dyg, Wg), ref)
    C.assert_exact(f"{name} gemm_nn wt", ext.gemm_nn(dyg, Wg, wt=WT), ref)
    out = torch.full((T, N), 7.0, device="cuda", dtype=torch.bfloat16)
    ext.gemm_nn_into(dyg, Wg, out)
    C.assert_exact(f"{name} gemm_nn_into", out, ref)
    for wt in (None, WT):
        dx = dx0g.clone()
        ran = ext.gemm_nn_acc_(dyg, Wg, dx, wt=wt)
        assert ran == persistent, f"{name}: gemm_nn_acc_ returned {ran}"
        if ran:
            C.assert_exact(f"{name} gemm_nn_acc_ wt={wt is not None}", dx, ref_acc)
        else:
            C.assert_exact(f"{name} gemm_nn_acc_ declined but wrote", dx, C.d(dx0))


def _dact_all(ext, name, T, K, N, act):
    """dz and every column-sum route against the exact dz and ITS exact column sums."""
    dy, W, aux, dz_ref, cs_ref = C.dact_case(13 + act, T, K, N, act)
    dyg, Wg, auxg = _cuda(dy, W, aux)
    WT = Wg.t().contiguous()
    for wt in (None, WT):
        tag = f"{name} dact act={act} wt={wt is not None}"
        dz, db = ext.gemm_nn_dact(dyg, Wg, auxg, act, False, wt=wt)
        assert db is None
        C.assert_exact(f"{tag} dz", dz, dz_ref)
        dz, db = ext.gemm_nn_dact(dyg, Wg, auxg, act, True, wt=wt)
        C.assert_exact(f"{tag} dz (want_db)", dz, dz_ref)
        C.assert_exact(f"{tag} db", db, cs_ref)
        acc0 = C.int_small(C.generator(99), N)
        acc = acc0.cuda()
        dz, db = ext.gemm_nn_dact(dyg, Wg, auxg, act, True, db_acc=acc, wt=wt)
        assert db is None
        C.assert_exact(f"{tag} dz (db_acc)", dz, dz_ref)
        C.assert_exact(f"{tag} db_acc", acc, C.require_fp32_exact("db_acc", cs_ref + C.d(acc0)))
        part = torch.full((T // 256 * 2, N), float("nan"), device="cuda")
        dz, db = ext.gemm_nn_dact(dyg, Wg, auxg, act, True, part_out=part, wt=wt)
        assert db is None
        C.assert_exact(f"{tag} dz (part_out)", dz, dz_ref)
        acc = acc0.cuda()
        ext.colsum_acc(part, acc)
        C.assert_exact(f"{tag} part_out + colsum_acc", acc, cs_ref + C.d(acc0))


@pytest.mark.parametrize("act", [2, 4])
@pytest.mark.parametrize("name,shape,sw,persistent", PERSISTENT, ids=PERSISTENT_IDS)
def test_dact_exact(name, shape, sw, persistent, act):
    T, K, N = shape
    _set(**sw)
    _dact_all(_ext(), name, T, K, N, act)


@pytest.mark.parametrize("act", [2, 4])
def test_dact_exact_grouped_tile_order(act):
    """(M / 256) % 8 == 0 and N / 256 >= 8: the EPI 4 launch (column-sum partials) walks tiles
    in groups of 8 tile rows (GM = 8 in gemmp_go); the plain dz launch (EPI 3) does not."""
    T, K, N = C.SHAPE_GM8
    _dact_all(_ext(), "gm8", T, K, N, act)


def test_forward_saved_derivative_grouped_tile_order():
    """EPI 6 (y and act' stored) and EPI 8 (act' as u8 codes) take the GM = 8 order at the same
    shape.  GELU / SiLU of an integer are not integers, so the exact statement here is another
    one: an element's value does not depend on which workgroup computes its tile or when, so
    the launch over all 2048 rows must equal, bit for bit, eight launches over 256 rows each
    (one tile row: (M / 256) % 8 != 0, the plain order).  The values themselves are checked
    against float64 in test_act_sweep_gpu.py."""
    ext = _ext()
    T, K, N = C.SHAPE_GM8
    x, W, b, _, _ = C.nt_case(21, T, K, N)
    xg, Wg, bg = _cuda(x, W, b)
    ext.set_gemmp_half(0)   # full tiles in both launches: only the tile order differs
    for act in (1, 3):
        y, dv, mode = ext.gemm_nt(xg, Wg, bg, act, 1)
        assert mode == 1
        y8, _, mode8 = ext.gemm_nt(xg, Wg, bg, act, 2)
        assert mode8 == 2
        for i in range(T // 256):
            rows = slice(i * 256, (i + 1) * 256)
            yi, dvi, mi = ext.gemm_nt(xg[rows], Wg, bg, act, 1)
            assert mi == 1
            C.assert_exact(f"gm8 EPI 6 act={act} y rows {i}", y[rows], yi.double().cpu())
            C.assert_exact(f"gm8 EPI 6 act={act} act' rows {i}", dv[rows], dvi.double().cpu())
            C.assert_exact(f"gm8 EPI 8 act={act} y rows {i}", y8[rows], yi.double().cpu())


# ---- weight gradients -------------------------------------------------------------------
# The split-K plan (wgrad_plan in gemm256.hip; gemm256_wgrad_workspace_floats returns non-zero
# exactly when it merges through the workspace) needs T / 64 >= 4 K-tiles to split at all, so
# T = 128 never splits and T = 256 is the smallest T that can: at every (N, K) below two splits
# of two K-tiles cost 7 + 1.5 * (N K 4 / 1e6) model units against 10 unsplit, so T = 256 splits
# and merges through the workspace (for any CU count >= the 2..6 workgroups launched).  Each
# T = 128 case therefore has its T = 256 partner; T = 1024 splits 8 ways.

@pytest.mark.parametrize("T,N,K", C.WGRAD_SHAPES)
def test_wgrad_exact(T, N, K):
    """dW += dy^T x and db += colsum(dy) onto integer-valued fp32 gradients.  (512, 384, 128)
    runs the 128-tile kernel's atomic merge; (256, 128, 768) the zero-padded 256-tile path."""
    ext = _ext()
    dys, xs, dW0, db0, dW_ref, db_ref = C.wgrad_case(31, T, N, K)
    dy, x, dW, db = _cuda(dys[0], xs[0], dW0, db0)
    ext.gemm_wgrad(dy, x, dW, db)
    C.assert_exact("wgrad dW", dW, dW_ref)
    C.assert_exact("wgrad db", db, db_ref)


@pytest.mark.parametrize("four_w", [True, False], ids=["wgrad4w", "8phase"])
@pytest.mark.parametrize("T,N,K", C.WGRAD_SHAPES)
def test_wgrad_exact_no_bias(T, N, K, four_w):
    ext = _ext()
    dys, xs, dW0, _, dW_ref, _ = C.wgrad_case(32, T, N, K, bias=False)
    dy, x, dW = _cuda(dys[0], xs[0], dW0)
    ext.set_wgrad4w(four_w)
    ext.gemm_wgrad(dy, x, dW, None)
    C.assert_exact("wgrad dW (no bias)", dW, dW_ref)


@pytest.mark.parametrize("tile128", [False, True], ids=["tile256", "tile128"])
def test_wgrad_exact_128_tile_kernel(tile128):
    """(T, N, K) = (128, 128, 128) and (256, 384, 128) on the 128-tile kernel (the only one
    that takes a 128-wide side unpadded), with the 256-tile path on and off."""
    ext = _ext()
    ext.set_gemm256(not tile128)
    for T, N, K in ((128, 128, 128), (256, 384, 128), (256, 256, 256)):
        dys, xs, dW0, db0, dW_ref, db_ref = C.wgrad_case(33, T, N, K)
        dy, x, dW, db = _cuda(dys[0], xs[0], dW0, db0)
        ext.gemm_wgrad(dy, x, dW, db)
        C.assert_exact(f"wgrad dW {T, N, K}", dW, dW_ref)
        C.assert_exact(f"wgrad db {T, N, K}", db, db_ref)


@pytest.mark.parametrize("mode", ["bias", "nobias-wgrad4w", "nobias-8phase"])
@pytest.mark.parametrize("nseg", [2, 3, 8])
@pytest.mark.parametrize("T,N,K", C.WGRAD_MULTI)
def test_wgrad_multi_exact(T, N, K, nseg, mode):
    """One multi-segment launch (always merged through the workspace: >= 2 slabs)."""
    ext = _ext()
    bias = mode == "bias"
    dys, xs, dW0, db0, dW_ref, db_ref = C.wgrad_case(34, T, N, K, nseg, bias)
    dW, db = _cuda(dW0, db0)
    ext.set_wgrad4w(mode == "nobias-wgrad4w")
    assert ext.gemm_wgrad_multi(_cuda(*dys), _cuda(*xs), dW, db)
    C.assert_exact("wgrad_multi dW", dW, dW_ref)
    if bias:
        C.assert_exact("wgrad_multi db", db, db_ref)


@pytest.mark.parametrize("with_db", [True, False])
def test_wgrad_grouped_exact(with_db):
    """Three sites of different shapes and segment counts in one grouped launch."""
    ext = _ext()
    cases = [C.wgrad_case(35 + i, T, N, K, nseg, with_db) for i, (T, N, K, nseg) in enumerate(C.WGRAD_GROUP)]
    dWs = [c[2].cuda() for c in cases]
    dbs = [c[3].cuda() if with_db else None for c in cases]
    assert ext.gemm_wgrad_grouped([_cuda(*c[0]) for c in cases], [_cuda(*c[1]) for c in cases], dWs, dbs)
    for i, c in enumerate(cases):
        C.assert_exact(f"wgrad_grouped site {i} dW", dWs[i], c[4])
        if with_db:
            C.assert_exact(f"wgrad_grouped site {i} db", dbs[i], c[5])


# ---- real-valued operands against the per-element bound ---------------------------------

REAL_PATHS = (
    [(f"{s[0]}x{s[1]}x{s[2]}", s, {}) for s in C.REAL_SHAPES]
    + [("cap3-static", C.SHAPE_STATIC, dict(cap=3)),
       ("cap8-queue-off", C.SHAPE_QUEUE, dict(cap=8, dynamic=False)),
       ("cap8-queue-on", C.SHAPE_QUEUE, dict(cap=8, dynamic=True))]
)
REAL_IDS = [p[0] for p in REAL_PATHS]


@functools.lru_cache(maxsize=None)
def _real_fwd(shape):
    T, K, N = shape
    x, W, b = C.real_operands(C.generator(41), T, K, N)
    r, a = C.real_ref(x, W, b)
    return x, W, b, r, a


@functools.lru_cache(maxsize=None)
def _real_bwd(shape):
    """dy [T, K] ~ randn, W [K, N] ~ 0.05 randn, aux [T, N] ~ randn: dy W with its |dy| |W|."""
    T, K, N = shape
    g = C.generator(42)
    dy = torch.randn(T, K, generator=g).bfloat16()
    W = (torch.randn(K, N, generator=g) * 0.05).bfloat16()
    aux = torch.randn(T, N, generator=g).bfloat16()
    r, a = C.real_ref(dy, W.t())
    return dy, W, aux, r, a


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("name,shape,sw", REAL_PATHS, ids=REAL_IDS)
def test_forward_real_within_bound(name, shape, sw, act):
    ext = _ext()
    T, K, N = shape
    x, W, b, r, a = _real_fwd(shape)
    xg, Wg, bg = _cuda(x, W, b)
    _set(**sw)
    y, z, mode = ext.gemm_nt(xg, Wg, bg, act)
    assert mode == 0
    C.assert_within(f"{name} gemm_nt act={act} y", y, C.act_ref(r, act), C.act_bound(r, a, K, act))
    if z is not None:   # the saved pre-activation (act 1, 3)
        C.assert_within(f"{name} gemm_nt act={act} z", z, r, C.gemm_bound(r, a, K))


@pytest.mark.parametrize("name,shape,sw", REAL_PATHS, ids=REAL_IDS)
def test_dgrad_real_within_bound(name, shape, sw):
    ext = _ext()
    T, K, N = shape
    dy, W, aux, r, a = _real_bwd(shape)
    dyg, Wg, auxg = _cuda(dy, W, aux)
    WT = Wg.t().contiguous()
    _set(**sw)
    bound = C.gemm_bound(r, a, K)
    C.assert_within(f"{name} gemm_nn", ext.gemm_nn(dyg, Wg), r, bound)
    C.assert_within(f"{name} gemm_nn wt", ext.gemm_nn(dyg, Wg, wt=WT), r, bound)
    for act in (1, 2, 3):
        if act == 2:    # aux = y = tanh(z) as the forward stored it; the kernel forms 1 - y^2
            ax = torch.tanh(aux.float()).bfloat16()
            dv = 1 - ax.double() ** 2
        else:
            ax = aux
            dv = C.dact_ref(ax.double(), act)
        dz, db = ext.gemm_nn_dact(dyg, Wg, ax.cuda(), act, False)
        C.assert_within(f"{name} gemm_nn_dact act={act}", dz, r * dv, C.dact_bound(r, a, K, dv))
