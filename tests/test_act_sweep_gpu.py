"""Every bf16 pre-activation through every activation epilogue.

x holds all 65536 bf16 bit patterns ([512, 128]; NaN and +-inf patterns replaced by 0).  With an
identity weight and no bias the GEMM's pre-activation IS x, so the forward epilogues
(gemm_nt act 1..3, want_deriv 0 / 1), the backward epilogues (gemm_nn_dact act 1..4 with
dy W = 1) and the elementwise kernels (bias_act_fwd / bias_act_bwd) are compared, value by
value, with float64 erf / tanh / sigmoid forms.

The persistent 256-tile kernels need an output width that is a multiple of 256, so on that path
the weight is two stacked 128 x 128 identities ([256, 128]: both halves of the output are the
sweep); the 128-tile path (set_gemm256(False)) takes the plain 128 x 128 identity.

Tolerances (none fitted to kernel output):
  one bf16 ulp of the reference (its spacing 2^(e-7); the final round-to-nearest uses half)
  plus an absolute term quoted from csrc/act.h:
  * GELU z Phi(z): act.h states |erf error| < 1.5e-7; Phi = (1 + erf) / 2 halves it and the
    fp32 evaluation of 0.5 + 0.5 erf adds < 2^-24, so |Phi error| < 1.5e-7 and |y error| <
    |z| 1.5e-7.
  * GELU' = Phi(z) + z phi(z): the same 1.5e-7 on Phi plus the pdf term |z| 0.3989 exp(-z^2/2)
    evaluated with the same exp, relative error of order 1.5e-7: (1 + 0.4 |z|) 1.5e-7.
  * tanh_fast: act.h states an absolute error of ~1e-7.
  * SiLU z s(z) and its derivative s (1 + z (1 - s)): one exp, one rcp (1 ulp each) and three
    fp32 roundings give a RELATIVE error < 4 * 2^-23, far inside the half ulp of slack, so no
    absolute term - except where the sigmoid leaves the normal fp32 range: v_rcp_f32 returns 0
    for a result below 2^-126 (s(z) < 2^-126 for z < -87.34, csrc/act.h), and the kernels then
    give 0 for a true |z| s < |z| 2^-126, resp. |1 + z| s < (1 + |z|) 2^-126.  The absolute
    term is (1 + |z|) 2^-126 for both.
"""
import math

import pytest
import torch

import gemm_exact_cases as C

pytestmark = pytest.mark.gpu

FLT_TINY = 2.0 ** -126                  # smallest normal fp32
BF16_MAX = 3.3895313892515355e38        # 0x7f7f
TANH_SWITCH = 2.0 ** -8                 # tanh_fast returns z below this


def _ext():
    from distributed_pipeline_amd.ops._ext import get_ext
    return get_ext(required=True)


@pytest.fixture(params=[256, 128], ids=["tile256", "tile128"])
def tile(request):
    _ext().set_gemm256(request.param == 256)
    yield request.param
    _ext().set_gemm256(True)


def _sweep():
    """All 65536 bf16 bit patterns as [512, 128]; non-finite ones replaced by 0."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.bfloat16).reshape(512, 128).clone()
    x[~torch.isfinite(x)] = 0
    return x


def _bf16_ulp(ref):
    """Spacing of bf16 at |ref| (8 significant bits; 2^-133 in the subnormal range and at 0)."""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))      # |ref| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref), e - 8)


def _tol(kind, z, ref):
    az = z.abs()
    if kind == "gelu":
        a = az * 1.5e-7
    elif kind == "dgelu":
        a = (1 + 0.4 * az) * 1.5e-7
    elif kind == "tanh":
        a = torch.full_like(z, 1e-7)
    elif kind in ("silu", "dsilu"):
        a = (1 + az) * FLT_TINY
    else:               # exact operations on the swept value (1 - y^2, a saved derivative)
        a = torch.zeros_like(z)
    return _bf16_ulp(ref) + a


def _fwd_ref(z, act):
    if act == 1:    # z Phi(z) through erfc: no cancellation in the negative tail
        return 0.5 * z * torch.erfc(-z / math.sqrt(2.0))
    return C.act_ref(z, act)


def _dact_ref(z, act):
    if act == 1:
        return 0.5 * torch.erfc(-z / math.sqrt(2.0)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    if act == 2:    # aux = y = tanh(z): the kernels form 1 - y^2
        return 1 - z * z
    if act == 4:    # aux already is act'
        return z
    return C.dact_ref(z, act)


def _check(name, got, z, ref, kind):
    """got (bf16, any device) against float64 ref over the whole sweep, then the named cases."""
    g = got.detach().cpu().double().reshape(z.shape)
    assert bool(torch.isfinite(g).all()), f"{name}: NaN or inf at z = {z[~torch.isfinite(g)][:8].tolist()}"
    tol = _tol(kind, z, ref)
    err = (g - ref).abs()
    bad = err > tol
    if bool(bad.any()):
        i = torch.where(bad, err - tol, torch.full_like(err, -1.0)).argmax()
        zi, gi, ri = z.flatten()[i].item(), g.flatten()[i].item(), ref.flatten()[i].item()
        raise AssertionError(f"{name}: {int(bad.sum())} of {z.numel()} values outside tolerance; worst at z = {zi!r} "
                             f"(index {int(i)}): got {gi!r} want {ri!r}, |err| {err.flatten()[i].item():.3e} > "
                             f"{tol.flatten()[i].item():.3e}")

    def case(label, mask, want=None):
        assert bool(mask.any()), f"{name}: case '{label}' selects nothing"
        if want is None:
            ok = err[mask] <= tol[mask]
        else:
            ok = g[mask] == want[mask] if torch.is_tensor(want) else g[mask] == want
        assert bool(ok.all()), f"{name}: {label}: z = {z[mask][~ok][:8].tolist()} gave {g[mask][~ok][:8].tolist()}"

    az = z.abs()
    zero_val = {"gelu": 0.0, "tanh": 0.0, "silu": 0.0, "dgelu": 0.5, "dsilu": 0.5, "dtanh": 1.0, "ident": 0.0}[kind]
    case("+-0", z == 0, zero_val)
    if kind != "dtanh":     # (its operand y = tanh(z) lives in [-1, 1])
        case("|z| >= 89 (exp overflows)", az >= 89)
        case("largest finite bf16", az == BF16_MAX)
    if kind == "tanh":
        near = (az >= TANH_SWITCH / 2) & (az <= TANH_SWITCH * 2)
        case("tanh_fast switch at |z| = 2^-8", near)
        # below the switch the result is z itself, bit for bit (tanh(z) = z to 5e-6 there)
        case("tanh_fast below the switch returns z", (az < TANH_SWITCH) & (az >= 2.0 ** -126), z)
        case("tanh saturates to +-1", az >= 89, torch.sign(z))
    if kind in ("gelu", "silu"):
        case("large positive z passes through", z >= 89, z)
        case("large negative z gives 0", z <= -104, 0.0)


KIND_FWD = {1: "gelu", 2: "tanh", 3: "silu"}
KIND_BWD = {1: "dgelu", 2: "dtanh", 3: "dsilu", 4: "ident"}


def _same_value(name, got, x):
    """The pre-activation the GEMM hands its epilogue is x itself: equal as numbers everywhere
    (0 == -0: a sum started from +0 returns +0 for -0 + 0, so the sign of a zero is not kept),
    hence equal bit patterns wherever x != 0."""
    g = got.detach().cpu().reshape(x.shape)
    ne = g != x
    assert not bool(ne.any()), f"{name}: pre-activation differs from x at x = {x[ne][:8].tolist()}: {g[ne][:8].tolist()}"
    nz = x != 0
    assert torch.equal(g.view(torch.int16)[nz], x.view(torch.int16)[nz]), f"{name}: bit patterns differ"


def _identity(tile):
    eye = torch.eye(128, dtype=torch.bfloat16)
    return (torch.cat([eye, eye]) if tile == 256 else eye).cuda()


@pytest.mark.parametrize("want_deriv", [0, 1])
@pytest.mark.parametrize("act", [1, 2, 3])
def test_forward_epilogue_sweep(tile, act, want_deriv):
    ext = _ext()
    x = _sweep()
    W = _identity(tile)
    reps = W.shape[0] // 128
    y, z, mode = ext.gemm_nt(x.cuda(), W, None, act, want_deriv)
    zz = x.double().repeat(1, reps)
    _check(f"gemm_nt act={act} y", y, zz, _fwd_ref(zz, act), KIND_FWD[act])
    if act == 2:
        assert z is None
        return
    # the persistent kernel saves act' when asked (mode 1); the 128-tile kernel the pre-activation
    assert mode == (1 if (want_deriv and tile == 256) else 0)
    if mode == 0:
        _same_value(f"gemm_nt act={act} z", z, x.repeat(1, reps))
    else:
        _check(f"gemm_nt act={act} saved act'", z, zz, _dact_ref(zz, act), KIND_BWD[act])


@pytest.mark.parametrize("want_db", [False, True], ids=["dz", "dz+db"])
@pytest.mark.parametrize("act", [1, 2, 3, 4])
def test_backward_epilogue_sweep(act, want_db):
    """dz = (dy W) * act'(aux) with dy W = 1 exactly (dy selects row 0 of W, a row of ones)."""
    ext = _ext()
    x = _sweep()
    if act == 2:    # aux is y = tanh(z): its domain is [-1, 1]
        x[x.abs() > 1] = 0
    aux = x.repeat(1, 2)
    dy = torch.zeros(512, 128, dtype=torch.bfloat16)
    dy[:, 0] = 1
    W = torch.zeros(128, 256, dtype=torch.bfloat16)
    W[0] = 1
    a = aux.double()
    for wt in (None, W.t().contiguous().cuda()):
        dz, db = ext.gemm_nn_dact(dy.cuda(), W.cuda(), aux.cuda(), act, want_db, wt=wt)
        _check(f"gemm_nn_dact act={act} wt={wt is not None}", dz, a, _dact_ref(a, act), KIND_BWD[act])
        if act == 4:
            _same_value("gemm_nn_dact act=4 (dz = aux)", dz, aux)


@pytest.mark.parametrize("act", [1, 2, 3])
def test_elementwise_sweep(act):
    """bias_act_fwd / bias_act_bwd: act_apply and act_deriv of csrc/act.h."""
    ext = _ext()
    x = _sweep()
    z, y = ext.bias_act_fwd(x.cuda(), None, act)
    _same_value("bias_act_fwd z", z, x)
    _check(f"bias_act_fwd act={act}", y, x.double(), _fwd_ref(x.double(), act), KIND_FWD[act])
    if act == 2:
        x[x.abs() > 1] = 0
    ones = torch.ones(512, 128, dtype=torch.bfloat16, device="cuda")
    dz, db = ext.bias_act_bwd(ones, x.cuda(), act, False)
    assert db is None
    _check(f"bias_act_bwd act={act}", dz, x.double(), _dact_ref(x.double(), act), KIND_BWD[act])
