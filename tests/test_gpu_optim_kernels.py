"""csrc/optim.hip kernel by kernel through the C ABI, against the fp64 references of
tests/elbo_optim_ref.py: the gradient sum of squares, the clip, the fused Adam step with its
prologue (clip coefficient, skip flag, bias corrections) and step counter, the column sums in
every path (vector, scalar, bf16, two-level fold, beta / out2) and the data-parallel scalar
header -- at one element, around the quad boundary, and just past each kernel's grid cap.
Tolerances: elbo_optim_ref.TOL; counters, skipped updates and second launches exact."""
import functools
import math

import pytest
import torch

import elbo_optim_ref as R
from gpu_utils import P, need_gpu, rel_err, stream
from mlvae_hip._lib import last_error, lib

pytestmark = pytest.mark.gpu

H = R.ADAM_HYPER
F32_ROUND = 2.0 ** -24     # one rounding of an fp64 result to fp32


def dev(t):
    return t.contiguous().cuda()


def ok(rc):
    assert rc == 0, last_error()
    torch.cuda.synchronize()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def i32(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def sumsq_partials(tensors):
    """One NaN-poisoned partials buffer shared by the tensors, as optim.clip_grad_norm_ lays it out."""
    l = lib()
    counts = [l.mlvae_sumsq_partials_count(t.numel()) for t in tensors]
    buf = torch.full((sum(counts),), float("nan"), device="cuda", dtype=torch.float64)
    off = 0
    for t, c in zip(tensors, counts):
        ok(l.mlvae_grad_sumsq(P(t), t.numel(), buf.data_ptr() + 8 * off, stream()))
        off += c
    return buf


# ------------------------------------------------------------------------------- sum of squares
@pytest.mark.parametrize("n", R.SUMSQ_SIZES)
def test_grad_sumsq(n):
    need_gpu()
    g = R.grad_inputs(n)
    count = lib().mlvae_sumsq_partials_count(n)
    assert count == min((n // 4 + 1 + 255) // 256, 1024)
    parts = sumsq_partials([dev(g)])
    assert parts.numel() == count and not torch.isnan(parts).any()    # every partial written
    ref = R.sumsq(g).item()
    e = abs(parts.sum().item() - ref) / ref
    print(f"sumsq n={n}: {e:.3e} (bound {n * 2.0 ** -52:.3e})")
    assert e <= n * 2.0 ** -52


def test_grad_sumsq_rejects_a_misaligned_pointer():
    need_gpu()
    g = torch.zeros(16, device="cuda")
    parts = torch.zeros(1, device="cuda", dtype=torch.float64)
    assert lib().mlvae_grad_sumsq(P(g, 1), 8, P(parts), stream()) != 0
    assert "aligned" in last_error()


# ------------------------------------------------------------------------------- clip
def _clip(gs, max_norm):
    """mlvae_clip_scale over the tensors (norm_out from the first); returns the norm tensor."""
    parts = sumsq_partials(gs)
    norm = torch.full((1,), -1.0, device="cuda")
    for i, g in enumerate(gs):
        ok(lib().mlvae_clip_scale(P(g), g.numel(), P(parts), parts.numel(), max_norm, P(norm) if i == 0 else None,
                                  stream()))
    return norm


@functools.lru_cache(maxsize=None)
def clip_case():
    gs = [R.grad_inputs(n) for n in R.CLIP_SIZES]
    return gs, math.sqrt(sum(R.sumsq(g).item() for g in gs))


def test_clip_scale_above_max_norm_scales_both_tensors():
    need_gpu()
    gs, total = clip_case()
    assert total > R.CLIP_MAX_NORM
    d = [dev(g) for g in gs]
    norm = _clip(d, R.CLIP_MAX_NORM)
    assert abs(norm.item() - total) <= (F32_ROUND + sum(R.CLIP_SIZES) * 2.0 ** -52) * total
    coef = R.clip_coef(total, R.CLIP_MAX_NORM)
    for g, got in zip(gs, d):
        e = rel_err(got, g.double() * coef)
        print(f"clip_g n={g.numel()}: {e:.3e} (TOL {R.TOL['clip_g']:.3e})")
        assert e <= R.TOL["clip_g"]


@pytest.mark.parametrize("max_norm", [1e4, math.inf])
def test_clip_scale_below_max_norm_keeps_the_bits(max_norm):
    need_gpu()
    gs, total = clip_case()
    d = [dev(g) for g in gs]
    norm = _clip(d, max_norm)
    assert abs(norm.item() - total) <= (F32_ROUND + sum(R.CLIP_SIZES) * 2.0 ** -52) * total
    for g, got in zip(gs, d):
        assert torch.equal(bits(got), bits(g))


def test_clip_scale_nan_gradient_poisons_everything_as_torch_does():
    need_gpu()
    gs, _ = clip_case()
    d = [dev(g) for g in gs]
    d[1][3] = float("nan")
    norm = _clip(d, R.CLIP_MAX_NORM)
    assert math.isnan(norm.item())
    for got in d:
        assert torch.isnan(got).all()


@pytest.mark.parametrize("max_norm", [R.CLIP_MAX_NORM, 1e4])
def test_optim_clip_grad_norm_matches_torch(max_norm):
    need_gpu()
    from mlvae_hip import optim
    gs, total = clip_case()
    cpu = [torch.nn.Parameter(torch.zeros(g.numel(), dtype=torch.float64)) for g in gs]
    gpu = [torch.nn.Parameter(torch.zeros(g.numel(), device="cuda")) for g in gs]
    for pc, pg, g in zip(cpu, gpu, gs):
        pc.grad, pg.grad = g.double().clone(), dev(g)
    want = torch.nn.utils.clip_grad_norm_(cpu, max_norm)
    got = optim.clip_grad_norm_(gpu, max_norm)
    torch.cuda.synchronize()
    assert abs(got.item() - want.item()) <= (F32_ROUND + sum(R.CLIP_SIZES) * 2.0 ** -52) * want.item()
    for pc, pg in zip(cpu, gpu):
        assert rel_err(pg.grad, pc.grad) <= R.TOL["clip_g"]


# ------------------------------------------------------------------------------- Adam
class AdamRun:
    """Device state of one mlvae_adam_step_ex call; every output readable afterwards."""

    def __init__(self, d, step0=0, loss=1.25, err=None, nonfinite0=3, err_skips0=5):
        self.n = d["p"].numel()
        self.p, self.m, self.v, self.g = (dev(d[k]) for k in ("p", "m", "v", "g"))
        self.parts = sumsq_partials([self.g])
        self.loss = None if loss is None else torch.tensor([loss], device="cuda")
        self.step, self.nonfinite, self.err_skips = i32(step0), i32(nonfinite0), i32(err_skips0)
        self.err = None if err is None else i32(err)
        self.norm = torch.full((1,), -1.0, device="cuda")
        self.hyp = torch.full((4,), float("nan"), device="cuda")

    def call(self, advance=1, lr=H["lr"], max_norm=R.ADAM_MAX_NORM, hyp=None, p=None):
        hyp = self.hyp if hyp is None else hyp
        opt = lambda t: None if t is None else P(t)
        rc = lib().mlvae_adam_step_ex(P(self.p) if p is None else p, P(self.m), P(self.v), P(self.g), self.n,
                                      P(self.parts), self.parts.numel(), opt(self.loss), P(self.step),
                                      P(self.nonfinite), opt(self.err), P(self.err_skips), lr, H["b1"], H["b2"],
                                      H["eps"], max_norm, P(self.norm), 0 if hyp is False else P(hyp), advance,
                                      stream())
        torch.cuda.synchronize()
        return rc

    def counters(self):
        return self.step.item(), self.nonfinite.item(), self.err_skips.item()


@functools.lru_cache(maxsize=None)
def adam_case(n):
    d = R.adam_inputs(n)
    return d, math.sqrt(R.sumsq(d["g"]).item())


def check_adam(run, d, t, coef, lr=H["lr"], what=""):
    ref = R.adam_step(d["p"], d["m"], d["v"], d["g"], t, lr, H["b1"], H["b2"], H["eps"], coef=coef)
    for key, got, want in zip(("adam_p", "adam_m", "adam_v"), (run.p, run.m, run.v), ref):
        e = rel_err(got, want)
        print(f"{key} {what}: {e:.3e} (TOL {R.TOL[key]:.3e})")
        assert e <= R.TOL[key], key


@pytest.mark.parametrize("step0", R.ADAM_STEPS0)
@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adam_one_step(n, step0):
    need_gpu()
    d, norm = adam_case(n)
    run = AdamRun(d, step0=step0)
    assert run.call(advance=1) == 0, last_error()
    check_adam(run, d, step0 + 1, R.clip_coef(norm, R.ADAM_MAX_NORM), what=f"n={n} t={step0 + 1}")
    assert run.counters() == (step0 + 1, 3, 5)
    assert abs(run.norm.item() - norm) <= (F32_ROUND + n * 2.0 ** -52) * norm
    hyp = run.hyp.cpu()
    assert hyp[1] == 0
    if norm < R.ADAM_MAX_NORM:
        assert hyp[0] == 1.0      # coef is exactly 1 below max_norm


def test_adam_zero_gradient_and_state_leaves_the_parameters_alone():
    need_gpu()
    n = 185
    d = dict(R.adam_inputs(n), m=torch.zeros(n), v=torch.zeros(n), g=torch.zeros(n))
    run = AdamRun(d)
    assert run.call() == 0, last_error()
    assert torch.equal(bits(run.p), bits(d["p"]))
    assert run.m.abs().max() == 0 and run.v.abs().max() == 0
    assert run.counters() == (1, 3, 5) and run.norm.item() == 0.0


def test_adam_advance_zero_updates_but_keeps_the_counter():
    need_gpu()
    d, norm = adam_case(185)
    a, b = AdamRun(d, step0=41), AdamRun(d, step0=41)
    assert a.call(advance=1) == 0 and b.call(advance=0) == 0, last_error()
    assert a.counters() == (42, 3, 5) and b.counters() == (41, 3, 5)
    for x, y in ((a.p, b.p), (a.m, b.m), (a.v, b.v), (a.hyp, b.hyp)):
        assert torch.equal(bits(x), bits(y))
    check_adam(b, d, 42, R.clip_coef(norm, R.ADAM_MAX_NORM), what="advance=0")


def test_adam_advance_minus_one_reuses_the_prologue_of_the_earlier_call():
    need_gpu()
    da, norm_a = adam_case(185)
    db, _ = adam_case(5)
    a, b = AdamRun(da, step0=7), AdamRun(db, step0=7)
    assert a.call(advance=0) == 0, last_error()
    # another lr, max_norm and (poisoned) partials: none of them may be looked at
    b.parts.fill_(float("nan"))
    assert b.call(advance=-1, lr=7e-2, max_norm=1e-3, hyp=a.hyp) == 0, last_error()
    check_adam(b, db, 8, R.clip_coef(norm_a, R.ADAM_MAX_NORM), what="advance=-1")
    assert b.counters() == (7, 3, 5)
    assert b.norm.item() == -1.0 and torch.isnan(b.hyp).all()     # no prologue ran for b


def test_adam_null_loss_and_null_err_update():
    need_gpu()
    d, norm = adam_case(185)
    run = AdamRun(d, loss=None, err=None)
    assert run.call() == 0, last_error()
    check_adam(run, d, 1, R.clip_coef(norm, R.ADAM_MAX_NORM), what="loss=NULL")
    assert run.counters() == (1, 3, 5)
    run = AdamRun(d, loss=2.0, err=0)     # an err word that is clear
    assert run.call() == 0, last_error()
    check_adam(run, d, 1, R.clip_coef(norm, R.ADAM_MAX_NORM), what="err=0")
    assert run.counters() == (1, 3, 5)


@pytest.mark.parametrize("n", [185, 2097152 + 1027])
@pytest.mark.parametrize("loss,err,want", [
    (math.nan, None, (9, 4, 5)), (math.inf, None, (9, 4, 5)), (-math.inf, 0, (9, 4, 5)),
    (1.25, 1, (9, 3, 6)), (math.nan, 1, (9, 3, 6)),          # the err word beats a non-finite loss
])
def test_adam_skips_are_exact_and_counted(n, loss, err, want):
    need_gpu()
    d, norm = adam_case(n)
    run = AdamRun(d, step0=9, loss=loss, err=err)
    assert run.call(advance=1) == 0, last_error()
    for key, got in (("p", run.p), ("m", run.m), ("v", run.v)):
        assert torch.equal(bits(got), bits(d[key])), key
    assert run.counters() == want
    assert run.hyp[1].item() == 1.0
    assert abs(run.norm.item() - norm) <= (F32_ROUND + n * 2.0 ** -52) * norm


def test_adam_nan_norm_propagates():
    need_gpu()
    d = dict(R.adam_inputs(185))
    d["g"] = d["g"].clone()
    d["g"][17] = float("nan")
    run = AdamRun(d)
    assert run.call() == 0, last_error()
    assert math.isnan(run.norm.item()) and math.isnan(run.hyp[0].item())
    assert torch.isnan(run.p).all() and torch.isnan(run.m).all() and torch.isnan(run.v).all()
    assert run.counters() == (1, 3, 5)     # torch too steps on a finite loss with NaN gradients


def test_adam_ten_step_trajectory():
    need_gpu()
    n = 185
    run = AdamRun(dict(R.adam_inputs(n), m=torch.zeros(n), v=torch.zeros(n)))
    for t in range(1, 11):
        run.g.copy_(R.grad_inputs(n, scale=t))
        run.parts = sumsq_partials([run.g])
        assert run.call(advance=1, max_norm=math.inf) == 0, last_error()
        assert run.hyp[0].item() == 1.0
    assert run.counters() == (10, 3, 5)
    for key, got, want in zip(("adam_p", "adam_m", "adam_v"), (run.p, run.m, run.v), R.adam_trajectory()):
        e = rel_err(got, want)
        print(f"{key} trajectory: {e:.3e} (TOL {R.TOL[key]:.3e})")
        assert e <= R.TOL[key], key


def test_adam_rejects_a_null_hyp_and_a_misaligned_buffer():
    need_gpu()
    d, _ = adam_case(185)
    run = AdamRun(d)
    assert run.call(hyp=False) != 0
    assert run.call(p=P(run.p, 1)) != 0
    assert torch.equal(bits(run.p), bits(d["p"])) and run.counters() == (0, 3, 5)


# ------------------------------------------------------------------------------- column sums
def run_colsum(ptr, N, C, ld, bf16=0, beta=0.0, out=None, out2=None, short=0):
    l = lib()
    size = l.mlvae_colsum_workspace_size(N, C)
    ws = torch.full((size // 4 + 1,), float("nan"), device="cuda")   # an unwritten chunk would show
    out = torch.full((C,), float("nan"), device="cuda") if out is None else out
    rc = l.mlvae_colsum_ex(N, C, ptr, bf16, ld, P(out), None if out2 is None else P(out2), beta, P(ws),
                           size - short, stream())
    torch.cuda.synchronize()
    return rc, out


@functools.lru_cache(maxsize=None)
def colsum_case(N, C, ld):
    d = R.colsum_inputs(N, C, ld)
    return d, R.colsum(d["x"][:, :C]), R.colsum(d["x"][:, :C].to(torch.bfloat16))


def check_colsum(got, ref, what):
    e = rel_err(got, ref)
    print(f"colsum {what}: {e:.3e} (TOL {R.TOL['colsum']:.3e})")
    assert e <= R.TOL["colsum"], what


@pytest.mark.parametrize("N,C,ld", R.COLSUM_SHAPES)
def test_colsum_fp32_aligned_offset_and_rerun(N, C, ld):
    need_gpu()
    d, ref, _ = colsum_case(N, C, ld)
    flat = torch.zeros(N * ld + 4, device="cuda")
    flat[:N * ld] = dev(d["x"].reshape(-1))
    rc, out = run_colsum(P(flat), N, C, ld)
    assert rc == 0, last_error()
    check_colsum(out, ref, "aligned")
    rc, again = run_colsum(P(flat), N, C, ld)
    assert rc == 0 and torch.equal(bits(again), bits(out))
    flat[1:N * ld + 1] = dev(d["x"].reshape(-1))     # base pointer off by one float: the scalar path
    rc, off = run_colsum(P(flat, 1), N, C, ld)
    assert rc == 0, last_error()
    check_colsum(off, ref, "offset by one float")


@pytest.mark.parametrize("N,C,ld", R.COLSUM_SHAPES)
def test_colsum_bf16_aligned_and_offset(N, C, ld):
    need_gpu()
    d, _, ref = colsum_case(N, C, ld)
    xb = dev(d["x"].to(torch.bfloat16).reshape(-1))
    flat = torch.zeros(N * ld + 8, device="cuda", dtype=torch.bfloat16)
    for off in (0, 1):        # one bf16 element = 2 bytes off the 8-byte quad alignment
        flat[off:off + N * ld] = xb
        rc, out = run_colsum(flat.data_ptr() + 2 * off, N, C, ld, bf16=1)
        assert rc == 0, last_error()
        check_colsum(out, ref, f"bf16 offset {off}")


@pytest.mark.parametrize("N,C,ld", [(1000, 70, 72), (1000, 70, 71), (65836, 8, 8)])
def test_colsum_beta_accumulates_and_out2_gets_the_copy(N, C, ld):
    need_gpu()
    d, ref, _ = colsum_case(N, C, ld)
    x = dev(d["x"])
    out, out2 = dev(d["out0"]), torch.full((C,), float("nan"), device="cuda")
    rc, _ = run_colsum(P(x), N, C, ld, beta=1.0, out=out, out2=out2)
    assert rc == 0, last_error()
    check_colsum(out, R.colsum(d["x"][:, :C], 1.0, d["out0"]), "beta=1")
    assert torch.equal(bits(out2), bits(out))
    rc, plain = run_colsum(P(x), N, C, ld, out2=out2)     # beta = 0 ignores what out held
    assert rc == 0 and torch.equal(bits(out2), bits(plain))
    check_colsum(plain, ref, "beta=0 with out2")


def test_colsum_rejects_a_workspace_one_byte_short():
    need_gpu()
    N, C, ld = 130, 64, 64
    x = dev(colsum_case(N, C, ld)[0]["x"])
    rc, out = run_colsum(P(x), N, C, ld, short=1)
    assert rc != 0 and "workspace" in last_error()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------- DP scalar header
def test_dp_scalars_pack_and_unpack():
    need_gpu()
    l = lib()
    loss3 = torch.tensor([1.5, -2.25, 3e-7], device="cuda")
    for e, flag in ((0, 0.0), (7, 1.0)):
        hdr, err = torch.full((4,), float("nan"), device="cuda"), i32(e)
        ok(l.mlvae_dp_scalars(1, P(hdr), P(loss3), P(err), stream()))
        assert torch.equal(bits(hdr[:3]), bits(loss3)) and hdr[3].item() == flag and err.item() == e
    # unpack the summed header of two ranks that both timed out
    hdr, out3, err = torch.tensor([3.0, -4.5, 6e-7, 2.0], device="cuda"), torch.zeros(3, device="cuda"), i32(0)
    ok(l.mlvae_dp_scalars(0, P(hdr), P(out3), P(err), stream()))
    assert torch.equal(bits(out3), bits(hdr[:3])) and err.item() == 1
    # a clear header leaves an err word that is already set alone
    hdr[3], err = 0.0, i32(5)
    ok(l.mlvae_dp_scalars(0, P(hdr), P(out3), P(err), stream()))
    assert err.item() == 5
    err = i32(0)
    ok(l.mlvae_dp_scalars(0, P(hdr), P(out3), P(err), stream()))
    assert err.item() == 0
    assert l.mlvae_dp_scalars(0, None, P(out3), P(err), stream()) != 0
