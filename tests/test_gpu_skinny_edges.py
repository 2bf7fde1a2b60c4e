"""The skinny layer-0 products (csrc/skinny.hip) at their dispatch edges, strides and tails:
every template instance of the three mlvae_skinny_nt kernels on both sides of their thresholds
(the N = 64 LDS form with its 67,584 bytes of static LDS included), one / odd chunk counts, the ks
form's tail loop, K == 0, every NB of skinny_tn with short, ragged and EMPTY frame splits,
skinny_dzw's odd / single tile counts and partial workgroups, skinny_proj's partial column passes
and single biases -- on padded leading dimensions, against tests/skinny_ref.py's fp64 contracts.

Every launch (launch()): integer operands in [-4, 4] place()d between NaN poison with 4096-element
guards, so every sum is exact in fp32 in any order and the result must EQUAL the fp64 reference
cast to the output type (an over-read makes it NaN); every output prefilled with a sentinel that
must survive bit for bit outside the logical region, in a bias that was not passed and in the
float just past the workspace size the API reports.  tn and dzw launch twice: identical bits.
No tolerance appears in this file."""
import pytest
import torch

import skinny_ref as S
from gpu_utils import need_gpu
from skinny_ref import seed_of

pytestmark = pytest.mark.gpu


def _last_error():
    from mlvae_hip._lib import last_error
    return last_error()


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _upload(c, outs_only=False):
    for b in list(c.outs.values()) + ([] if outs_only else list(c.ins.values())):
        b.dev = b.flat.cuda()


def _workspace(kind, c):
    """(ws, need): a SENTINEL workspace of the size the API reports, which must be the twin's."""
    from mlvae_hip._lib import lib
    if kind == "tn":
        need = lib().mlvae_skinny_tn_workspace_size(c.M, c.NB, c.K)
        assert need == S.tn_plan(c.M, c.K)[0] * c.M * c.NB * 4, "S differs from the Python twin"
    else:
        need = lib().mlvae_skinny_dzw_workspace_size(c.M, c.K8)
        assert need == S.dzw_plan(c.M, c.K8)[0] * c.K8 * S.DZW_NB * 4, "G differs from the Python twin"
    return S.make_ws(need), need


def _args(kind, c, ws=None, need=0):
    """The keyword arguments of the case's run_* call, every one explicit (refusals override some)."""
    i, o = c.ins, c.outs
    A = i["A"]
    if kind == "nt":
        a = dict(M=c.M, N=c.N, K=c.K, A=A.dev, a0=A.off, lda=A.ld, Bt=i["Bt"].dev, b0=i["Bt"].off, ldb=i["Bt"].ld,
                 C=o["C"].dev, c0=o["C"].off, ldc=o["C"].ld)
        if c.fp8:
            a.update(A8=a.pop("A"), alpha=torch.tensor([c.alpha], device="cuda"))
        return a
    if kind == "proj":
        return dict(M=c.M, N=c.N, K=c.K, A=A.dev, a0=A.off, lda=A.ld, B=i["B"].dev, b0=i["B"].off, ldb=i["B"].ld,
                    b1=i["b1"].dev if c.bias & 1 else None, b1_0=i["b1"].off,
                    b2=i["b2"].dev if c.bias & 2 else None, b2_0=i["b2"].off, C=o["C"].dev, c0=o["C"].off,
                    ldc=o["C"].ld, c_fp16=c.c_fp16)
    bias = dict(b1=o["b1"].dev if c.bias & 1 else None, b1_0=o["b1"].off,
                b2=o["b2"].dev if c.bias & 2 else None, b2_0=o["b2"].off, ws=ws, ws_bytes=need)
    if kind == "tn":
        return dict(M=c.M, NB=c.NB, K=c.K, A=A.dev, a0=A.off, lda=A.ld, B=i["B"].dev, b0=i["B"].off, ldb=i["B"].ld,
                    nw=c.nw, W=o["W"].dev, w0=o["W"].off, alpha=torch.tensor([c.alpha], device="cuda") if c.fp8 else None,
                    **bias)
    return dict(M=c.M, K8=c.K8, A=A.dev, a0=A.off, lda=A.ld, Wt=i["Wt"].dev, wt0=i["Wt"].off, ldw=i["Wt"].ld,
                zb=i["zb"].dev, z0=i["zb"].off, ldz=i["zb"].ld, Z=S.DZW_Z, dZ=o["dZ"].dev, dz0=o["dZ"].off,
                lddz=o["dZ"].ld, W=o["W"].dev, w0=o["W"].off, **bias)


def _run(kind, c, a):
    if kind == "nt":
        return (S.run_nt_fp8 if c.fp8 else S.run_nt)(**a)
    return {"proj": S.run_proj, "tn": S.run_tn, "dzw": S.run_dzw}[kind](**a)


def _check_outputs(kind, c, ws, need):
    """Values equal the reference exactly, every sentinel intact -> name -> flat host copy."""
    exp, flats = S.expected(kind, c), {}
    for name, b in c.outs.items():
        flat = flats[name] = b.dev.cpu()
        if name not in exp:
            assert torch.equal(_bits(flat), _bits(b.flat)), f"{name} was not passed but was written"
            continue
        mask = b.mask()
        assert torch.equal(_bits(flat)[~mask], _bits(b.flat)[~mask]), f"{name} written outside its logical region"
        got, ref = b.logical(flat), exp[name].to(flat.dtype)
        assert torch.isfinite(got).all(), f"{name}: non-finite result: a poisoned (out-of-range) element was read"
        assert torch.equal(got, ref), f"{name}: {int((got != ref).sum())} of {ref.numel()} elements differ"
    if ws is not None:
        tail = ws[need // 4:].cpu()
        assert torch.equal(_bits(tail), _bits(torch.full_like(tail, S.SENTINEL))), "written past the workspace size"
    return flats


def launch(kind, c):
    """One case under the file's rules; tn and dzw run twice (into fresh sentinel outputs, the
    workspace as the first launch left it) and must give identical bits."""
    need_gpu()
    _upload(c)
    ws, need = _workspace(kind, c) if kind in ("tn", "dzw") else (None, 0)
    rc = _run(kind, c, _args(kind, c, ws, need))
    assert rc == 0, _last_error()
    first = _check_outputs(kind, c, ws, need)
    if kind in ("tn", "dzw"):
        _upload(c, outs_only=True)
        rc = _run(kind, c, _args(kind, c, ws, need))
        assert rc == 0, _last_error()
        again = _check_outputs(kind, c, ws, need)
        assert all(torch.equal(_bits(first[k]), _bits(again[k])) for k in first), "the rerun differs"


def refuse(kind, c, **over):
    """The call with some arguments replaced must return non-zero, set the error text and write
    nothing: every output and the whole workspace still hold the sentinel."""
    need_gpu()
    _upload(c)
    ws, need = _workspace(kind, c) if kind in ("tn", "dzw") else (None, 0)
    a = _args(kind, c, ws, need)
    for k, v in over.items():
        a[k] = v(a) if callable(v) else v
    assert _run(kind, c, a) != 0, "the call must be refused"
    assert _last_error(), "a refusal sets mlvae_last_error()"
    torch.cuda.synchronize()
    for name, b in c.outs.items():
        assert torch.equal(_bits(b.dev.cpu()), _bits(b.flat)), f"a refused call wrote to {name}"
    if ws is not None:
        w = ws.cpu()
        assert torch.equal(_bits(w), _bits(torch.full_like(w, S.SENTINEL))), "a refused call wrote to the workspace"


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", S.NT_CASES, ids=str)
def test_nt(args):
    """mlvae_skinny_nt dispatches (csrc/skinny.hip): the LDS form when K > 0 && K % 256 == 0 &&
    M >= 4096, else the ks form when K % 128 == 0, else the plain kernel; N / 16 picks the template
    instance of each.  K == 0 stores zeros and reads nothing."""
    need_gpu()
    M, N, K, padded = args
    form = "lds" if (K > 0 and K % 256 == 0 and M >= 4096) else ("ks" if K % 128 == 0 else "plain")
    assert S.nt_form(M, N, K) == form
    if K > 0 and padded:
        assert (M, K) in S.NT_SHAPES[form], "the shape is listed under another kernel"
    launch("nt", S.make_nt(M, N, K, padded, seed=seed_of(args)))


@pytest.mark.parametrize("args", S.NT8_CASES, ids=str)
def test_nt_fp8(args):
    need_gpu()
    M, N, K, padded = args
    launch("nt", S.make_nt(M, N, K, padded, fp8=True, seed=seed_of(args)))


@pytest.mark.parametrize("args", S.proj_cases(), ids=str)
def test_proj(args):
    """fp32 cases alternate between mlvae_skinny_proj and mlvae_skinny_proj_ex(c_fp16 = 0)."""
    need_gpu()
    f16, M, N, K, bias, padded = args
    c = S.make_proj(f16, M, N, K, bias, padded, seed=seed_of(args))
    c.c_fp16 = 1 if f16 else (None if bias % 2 == 0 else 0)
    launch("proj", c)


@pytest.mark.parametrize("args", S.TN_CASES, ids=str)
def test_tn(args):
    need_gpu()
    M, NB, nw, bias, K, padded = args
    launch("tn", S.make_tn(M, NB, nw, bias, K, padded, seed=seed_of(args)))


@pytest.mark.parametrize("args", S.TN8_CASES, ids=str)
def test_tn_fp8(args):
    need_gpu()
    M, NB, nw, bias, K, padded = args
    launch("tn", S.make_tn(M, NB, nw, bias, K, padded, fp8=True, seed=seed_of(args)))


@pytest.mark.parametrize("args", S.DZW_CASES, ids=str)
def test_dzw(args):
    need_gpu()
    M, K8, bias, padded = args
    launch("dzw", S.make_dzw(M, K8, bias, padded, seed=seed_of(args)))


# ------------------------------------------------------------------------------------------------
# refusals: non-zero status, nothing written, nothing launched.  Misaligned base pointers appear
# here only: the host check rejects them before any launch.
def _shift(key, by):
    return lambda a: a[key] + by


NT_REFUSED = [dict(N=0), dict(N=8), dict(N=80), dict(K=40), dict(K=-32), dict(lda=100), dict(ldc=34),
              dict(a0=_shift("a0", 1)), dict(b0=_shift("b0", 4)), dict(c0=_shift("c0", 1))]


@pytest.mark.parametrize("over", NT_REFUSED, ids=lambda o: "-".join(o))
def test_nt_refuses(over):
    need_gpu()
    refuse("nt", S.make_nt(77, 32, 96), **over)            # lda 104, ldb 120, ldc 36


def test_nt_refuses_negative_k_at_the_lds_threshold():
    need_gpu()
    refuse("nt", S.make_nt(4173, 32, 256), K=-256)


NT8_REFUSED = [dict(M=4095), dict(K=128), dict(K=0), dict(K=-256), dict(lda=264), dict(alpha=None),
               dict(a0=_shift("a0", 8))]


@pytest.mark.parametrize("over", NT8_REFUSED, ids=lambda o: "-".join(o))
def test_nt_fp8_refuses(over):
    need_gpu()
    refuse("nt", S.make_nt(4173, 32, 256, fp8=True), **over)


PROJ_REFUSED = [(0, dict(K=0)), (0, dict(K=40)), (0, dict(K=12)), (0, dict(N=24)), (1, dict(ldc=148)),
                (0, dict(ldc=146)), (0, dict(b1_0=_shift("b1_0", 1))), (1, dict(c0=_shift("c0", 4)))]


@pytest.mark.parametrize("f16,over", PROJ_REFUSED, ids=lambda o: "-".join(o) if isinstance(o, dict) else str(o))
def test_proj_refuses(f16, over):
    need_gpu()
    c = S.make_proj(f16, 17, 144, 16, 3)                     # lda = ldb 24, ldc 152
    c.c_fp16 = f16
    refuse("proj", c, **over)


TN_REFUSED = [dict(M=100), dict(NB=80), dict(nw=0), dict(nw=16), dict(ws_bytes=lambda a: a["ws_bytes"] - 1),
              dict(ws=None), dict(b0=_shift("b0", 1))]


@pytest.mark.parametrize("over", TN_REFUSED, ids=lambda o: "-".join(o))
def test_tn_refuses(over):
    need_gpu()
    refuse("tn", S.make_tn(64, 16, 15, 3, 65), **over)      # nw = 16 with a bias: nw + 1 > NB


DZW_REFUSED = [dict(Z=16), dict(K8=128), dict(ldz=40), dict(lddz=28), dict(ws_bytes=lambda a: a["ws_bytes"] - 1),
               dict(dz0=_shift("dz0", 1))]


@pytest.mark.parametrize("over", DZW_REFUSED, ids=lambda o: "-".join(o))
def test_dzw_refuses(over):
    need_gpu()
    refuse("dzw", S.make_dzw(129, 256, 3), **over)
