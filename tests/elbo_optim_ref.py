"""Plain references of the ELBO kernels (csrc/elbo.hip) and the optimizer-step kernels
(csrc/optim.hip), the seeded inputs their kernel tests share, and the tolerance table.

No GPU import.  Every function restates the formula of the reference project's module that the
kernel header cites (ref:src/modules/vanilla_vae.py:37-45, ref:src/modules/decoder.py:37-53,
ref:src/utils/data_utils.py:67-104, SpeechBrain's check_gradients, torch.optim.Adam), in torch
ops, on the fp32 values the kernel is handed.  ``dtype`` chooses the arithmetic: float64 (the
default) is the reference the kernels are held to; float32 is the yardstick of the tolerance
table -- the same formula on a CPU in the kernel's own number format
(tests/test_elbo_optim_ref_cpu.py measures it and ties every function here to torch autograd,
torch.optim.Adam, clip_grad_norm_ and the oracle).
"""
import math

import numpy as np
import torch

NEG_SLOPE = 0.01                                         # nn.LeakyReLU() default
LOG_2PI = float(torch.log(2 * torch.tensor(np.pi)))      # fp32, as ref:src/modules/decoder.py:42
REDUCTIONS = ("mean", "batchmean", "batch")              # the kernels' reduction 0, 1, 2


# ------------------------------------------------------------------------------- lengths
def frame_mask(lens, T):
    """SpeechBrain ``length_to_mask(lens * T, max_len=T)``: arange(T) < fp32(len) * fp32(T), in
    numpy fp32.  Bool [B, T]; a NaN length masks every frame."""
    lim = np.asarray(lens, dtype=np.float32) * np.float32(T)
    with np.errstate(invalid="ignore"):
        return torch.from_numpy(np.arange(T, dtype=np.float32)[None, :] < lim[:, None])


def valid_frames(lens, T):
    """Valid frames per utterance: ceil(fp32(len) * fp32(T)) clamped to [0, T], 0 for a length
    that is not > 0 (NaN included) -- the number of True per row of ``frame_mask``.  int64 [B]."""
    lim = np.asarray(lens, dtype=np.float32) * np.float32(T)
    with np.errstate(invalid="ignore"):
        c = np.where(lim > 0, np.minimum(np.ceil(lim), np.float32(T)), np.float32(0))
    return c.astype(np.int64)


# ------------------------------------------------------------------------------- ELBO
def _mask3(lens, T, dtype):
    return frame_mask(lens, T).to(dtype).unsqueeze(-1)


def reparam_kl_terms(mu, lv, eps):
    """z = eps * exp(0.5 lv) + mu ;  kl = -0.5 (1 + lv - mu^2 - exp(lv)), elementwise."""
    z = eps * torch.exp(0.5 * lv) + mu
    kl = -0.5 * (1 + lv - mu.pow(2) - lv.exp())
    return z, kl


def reparam_kl(ml, eps, lens, T, dtype=torch.float64):
    """ml [B, T, 2Z] = (mu | log_var).  Returns z, kl [B, T, Z] and the masked sum of kl."""
    Z = ml.shape[-1] // 2
    ml = ml.to(dtype)
    z, kl = reparam_kl_terms(ml[..., :Z], ml[..., Z:], eps.to(dtype))
    return z, kl, (kl * _mask3(lens, T, dtype)).sum()


def reparam_kl_bwd(ml, eps, lens, T, dz=None, dkl=None, kl_scale=0.0, count=None,
                   dtype=torch.float64):
    """d/d(ml) of sum(dz * z) + sum(s * kl), with s = dkl (elementwise upstream gradient) or
    kl_scale * mask / (count * Z); ``count`` defaults to the batch's own valid frames."""
    Z = ml.shape[-1] // 2
    ml = ml.to(dtype)
    mu, lv, eps = ml[..., :Z], ml[..., Z:], eps.to(dtype)
    if dkl is not None:
        s = dkl.to(dtype)
    else:
        c = int(valid_frames(lens, T).sum()) if count is None else int(count)
        s = _mask3(lens, T, dtype) * (kl_scale / (c * Z) if c > 0 else 0.0)
    g = dz.to(dtype) if dz is not None else torch.zeros_like(mu)
    dmu = g + s * mu
    dlv = g * 0.5 * eps * torch.exp(0.5 * lv) + s * 0.5 * (lv.exp() - 1)
    return torch.cat([dmu, dlv.expand_as(dmu)], -1)


def recon_terms(mu, lv, x, loss_type):
    """'likelihood' (0): 0.5 (log 2pi + lv + (x - mu)^2 / (exp(lv) + 1e-5));  'mse' (1): (x - mu)^2."""
    if loss_type in (0, "likelihood"):
        return 0.5 * (LOG_2PI + lv + (x - mu) ** 2 / (torch.exp(lv) + 1e-5))
    if loss_type in (1, "mse"):
        return (x - mu) ** 2
    raise ValueError(f"Invalid loss type: {loss_type}")


def recon(mu, lv, x, lens, T, loss_type, weight=None, dtype=torch.float64):
    """Per-element loss [B, T, F], its masked sum, and d/dmu, d/dlv of sum(weight * loss) by
    autograd on the forward (weight None = ones: the elementwise derivatives)."""
    mu = mu.to(dtype).detach().clone().requires_grad_(True)
    lv = lv.to(dtype).detach().clone().requires_grad_(True)
    rec = recon_terms(mu, lv, x.to(dtype), loss_type)
    w = torch.ones_like(rec) if weight is None else weight.to(dtype).expand_as(rec)
    dmu, dlv = torch.autograd.grad((rec * w).sum(), [mu, lv], allow_unused=True)
    dlv = torch.zeros_like(dmu) if dlv is None else dlv
    rec = rec.detach()
    return rec, (rec * _mask3(lens, T, dtype)).sum(), dmu, dlv


def mask_weight(lens, T, scale, C, count=None, dtype=torch.float64):
    """scale * mask / (count * C) as [B, T, 1]: the fused-gradient modes' upstream weight."""
    c = int(valid_frames(lens, T).sum()) if count is None else int(count)
    return _mask3(lens, T, dtype) * (scale / (c * C) if c > 0 else 0.0)


def finalize(sum_kl, sum_rec, count, Z, F, w_kl, w_rec):
    """(kld, recon, total) = (sum_kl / (count Z), sum_rec / (count F), w_kl kld + w_rec recon)."""
    kld = float(sum_kl) / (float(count) * Z)
    rec = float(sum_rec) / (float(count) * F)
    return kld, rec, w_kl * kld + w_rec * rec


def masked_mean(loss, lens, reduction, dtype=torch.float64):
    """apply_lens_to_loss over [B, T, C]: 'mean' sum(loss mask) / sum(mask), 'batchmean'
    sum(loss mask) / B, 'batch' the per-utterance means [B]."""
    loss = loss.to(dtype)
    B, T = loss.shape[:2]
    mask = torch.ones_like(loss) * _mask3(lens, T, dtype)
    lm = loss * mask
    if reduction == "mean":
        return lm.sum() / mask.sum()
    if reduction == "batchmean":
        return lm.sum() / B
    if reduction == "batch":
        return lm.reshape(B, -1).sum(-1) / mask.reshape(B, -1).sum(-1)
    raise ValueError(reduction)


def masked_mean_bwd(g, shape, lens, reduction, dtype=torch.float64):
    """d/dloss of sum(g * masked_mean(loss)): g * mask / denominator, [B, T, C]."""
    B, T, C = shape
    g = g.to(dtype)
    mask = _mask3(lens, T, dtype).expand(B, T, C)
    vf = torch.from_numpy(valid_frames(lens, T)).to(dtype)
    if reduction == "mean":
        return mask * (g.reshape(()) / (vf.sum() * C))
    if reduction == "batchmean":
        return mask * (g.reshape(()) / B)
    if reduction == "batch":
        return mask * (g / (vf * C)).reshape(B, 1, 1)
    raise ValueError(reduction)


def lrelu_bwd(dy, y, dtype=torch.float64):
    """dy * LeakyReLU'(x) from the activation's output y: slope 0.01 wherever y <= 0 (+-0.0
    included: torch's leaky_relu backward tests x > 0), 1 elsewhere."""
    one = torch.ones((), dtype=dtype)
    return dy.to(dtype) * torch.where(y <= 0, one * NEG_SLOPE, one)


# ------------------------------------------------------------------------------- optimizer
def sumsq(g, dtype=torch.float64):
    return (g.to(dtype) ** 2).sum()


def clip_coef(total, max_norm, dtype=torch.float64):
    """clip_grad_norm_'s coefficient: min(max_norm / (total + 1e-6), 1); NaN stays NaN."""
    total = torch.tensor(float(total), dtype=dtype)
    return torch.clamp(max_norm / (total + 1e-6), max=1.0).item()


def adam_step(p, m, v, g, t, lr, b1, b2, eps, coef=1.0, dtype=torch.float64):
    """Step number t (1-based) of torch.optim.Adam (no weight decay, amsgrad off) on the
    gradient coef * g, in torch's order of operations.  Returns the new p, m, v."""
    p, m, v, g = (a.to(dtype) for a in (p, m, v, g))
    g = g * coef
    m = torch.lerp(m, g, 1 - b1)
    v = v * b2 + (1 - b2) * g * g
    bc1 = 1 - b1 ** t
    bc2 = 1 - b2 ** t
    step_size = lr / bc1
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - step_size * (m / denom), m, v


def colsum(x, beta=0.0, out=None, dtype=torch.float64):
    """out[c] = beta * out[c] + sum_n x[n, c]."""
    s = x.to(dtype).sum(0)
    return s if beta == 0.0 else beta * out.to(dtype) + s


# ------------------------------------------------------------------------------- shared inputs
# Every case is the smallest shape that reaches the path it names; the generators are seeded by
# the shape, so the GPU tests and the CPU measurement of TOL see the very same values.
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(k) * 7919 ** i for i, k in enumerate(key, 1)) % (2 ** 31))
    return g


def quirk_len(T):
    """A relative length k / T whose fp32 product with T lands above k (one more valid frame
    than k, like 127/500 at T = 500); T // 3 / T when T has none."""
    for k in range(max(T // 4, 1), T):
        r = np.float32(k / T)
        if r * np.float32(T) > np.float32(k):
            return float(r)
    return float(np.float32(max(T // 3, 1) / T))


def case_lens(B, T):
    """B = 1: full length.  B = 3: full length (above 1 at the large shape), a zero-length
    utterance, and the fp32-quirk fraction."""
    if B == 1:
        return torch.tensor([1.0])
    assert B == 3
    return torch.tensor([1.3 if T > 100 else 1.0, 0.0, quirk_len(T)])


REPARAM_SHAPES = [(1, 1, 1), (3, 17, 5), (3, 343, 256)]    # the last: 263 424 > 1024 x 256
RECON_SHAPES = [(1, 1, 1), (3, 17, 13), (3, 343, 256)]


def reparam_inputs(B, T, Z):
    g = _gen(1, B, T, Z)
    return dict(ml=torch.randn(B, T, 2 * Z, generator=g), eps=torch.randn(B, T, Z, generator=g),
                dz=torch.randn(B, T, Z, generator=g), dkl=torch.randn(B, T, Z, generator=g),
                lens=case_lens(B, T), kl_scale=1e-3)


def recon_inputs(B, T, F):
    """log_var: half the entries from {-20, -3, 0, 3, 10}, half standard normal, so exp(lv) + 1e-5
    is evaluated where the 1e-5 dominates and where it vanishes."""
    g = _gen(2, B, T, F)
    pick = torch.tensor([-20.0, -3.0, 0.0, 3.0, 10.0])[torch.randint(0, 5, (B, T, F), generator=g)]
    lv = torch.where(torch.rand(B, T, F, generator=g) < 0.5, pick, torch.randn(B, T, F, generator=g))
    return dict(mu=torch.randn(B, T, F, generator=g), lv=lv, x=torch.randn(B, T, F, generator=g),
                drec=torch.randn(B, T, F, generator=g), lens=case_lens(B, T), rec_scale=0.7)


FINALIZE_CASES = [(1, 1024), (255, 257), (257, 255), (1024, 1)]   # (nk, nr)
FINALIZE_DIMS = dict(B=3, T=17, Z=5, F=13, w_kl=0.37, w_rec=1.7)


def finalize_inputs(nk, nr):
    g = _gen(3, nk, nr)
    return dict(pk=torch.rand(nk, generator=g) * 40, pr=torch.rand(nr, generator=g) * 900,
                lens=case_lens(3, 17), **FINALIZE_DIMS)


COUNT_CASES = [(B, T) for B in (1, 300) for T in (1, 17, 500)]


def count_lens(B, T):
    """Random lengths; at B = 300 utterances 0, 60, .. are 1.0, 0.0, 127/500, 1.7 and the quirk
    fraction of T; the single utterance of B = 1 is the quirk fraction."""
    lens = torch.rand(B, generator=_gen(4, B, T))
    special = [1.0, 0.0, 127 / 500, 1.7, quirk_len(T)]
    if B == 1:
        lens[0] = special[-1]
    else:
        lens[::B // len(special)][:len(special)] = torch.tensor(special)
    return lens


# (B, T, C): C = 1; B = 300 (more than one pass of 256 threads over the lengths); 263 682 elements
MASKED_MEAN_SHAPES = [(2, 9, 1), (300, 7, 3), (2, 513, 257)]


def masked_mean_inputs(B, T, C):
    """Positive losses (a well-conditioned mean); utterance 0 has every frame valid, utterance 1
    a single frame, the rest random lengths (none empty: 'batch' divides by each one's frames)."""
    g = _gen(5, B, T, C)
    lens = torch.rand(B, generator=g).clamp_min(0.5 / T)
    lens[0], lens[1] = 1.0, 0.5 / T
    return dict(loss=torch.randn(B, T, C, generator=g).abs() + 0.1, lens=lens,
                g1=torch.randn(1, generator=g), gB=torch.randn(B, generator=g))


LRELU_SIZES = [1, 255, 262144 + 77]


def lrelu_inputs(n):
    g = _gen(6, n)
    y = torch.randn(n, generator=g)
    dy = torch.randn(n, generator=g)
    if n == 1:
        y[0] = -0.0
    else:
        sp = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45])
        for r in range(0, n - 5, max((n - 5) // 7, 1)):
            y[r:r + 6] = sp[:min(6, n - r)]
    return dict(dy=dy, y=y)


SUMSQ_SIZES = [1, 3, 4, 5, 1023, 1048576 + 1203]
CLIP_SIZES = (131072 + 9, 7)            # two tensors, one norm (about 362): the first past the grid
CLIP_MAX_NORM = 100.0                   # below that norm: scaled by about 0.28
ADAM_MAX_NORM = 5.0                     # check_gradients' max_grad_norm
ADAM_SIZES = [1, 5, 185, 2097152 + 1027]
ADAM_STEPS0 = [0, 9999, 1000000]          # the counter before the step; at 10^6, 1 - b1^t == 1
ADAM_HYPER = dict(lr=float(np.float32(1e-3)), b1=float(np.float32(0.9)), b2=float(np.float32(0.999)),
                  eps=float(np.float32(1e-8)))   # the fp32 values the C ABI receives


def grad_inputs(n, scale=1.0):
    return torch.randn(n, generator=_gen(7, n)) * scale


def adam_inputs(n):
    g = _gen(8, n)
    return dict(p=torch.randn(n, generator=g), m=torch.randn(n, generator=g) * 0.1,
                v=torch.rand(n, generator=g) * 0.01, g=torch.randn(n, generator=g))


def adam_trajectory(dtype=torch.float64, n=185, steps=10):
    """Ten steps from zero state; step t sees the fp32 gradient grad_inputs(n, scale=t) whatever
    the dtype, and no clipping."""
    p, m, v = adam_inputs(n)["p"], torch.zeros(n), torch.zeros(n)
    for t in range(1, steps + 1):
        p, m, v = adam_step(p, m, v, grad_inputs(n, scale=t), t, dtype=dtype, **ADAM_HYPER)
    return p, m, v


# (N, C, ld): one element; a partial quad; one full column block; the vector path with a scalar
# last quad; ld % 4 != 0 (scalar path); chunks that do not divide N; rows_per > 256 (two-level
# fold); a wide one (32 column blocks)
COLSUM_SHAPES = [(1, 1, 1), (15, 3, 3), (65, 64, 64), (1000, 70, 72), (1000, 70, 71), (130, 64, 64),
                 (65836, 8, 8), (700, 2048, 2048)]


def colsum_inputs(N, C, ld):
    """[N, ld] with a non-zero column mean (what a bias gradient looks like, and a sum whose
    relative error means something); the ld - C padding columns hold 1e6 (must not be read)."""
    g = _gen(9, N, C, ld)
    x = torch.randn(N, ld, generator=g) + 0.5
    x[:, C:] = 1e6
    return dict(x=x, out0=torch.randn(C, generator=g))


# ------------------------------------------------------------------------------- tolerances
# MEASURED[k]: max-abs over max-abs error (gpu_utils.rel_err) of the float32 evaluation of the
# functions above (torch CPU, dtype=torch.float32) against their float64 evaluation, on the
# inputs above, worst case per quantity; measured by test_elbo_optim_ref_cpu.py
# (test_fp32_noise_is_within_a_quarter_of_tol prints the table), recorded here rounded up to two
# digits.  TOL[k] = 4 x MEASURED[k]: the device's expf and fixed-order block folds against the
# CPU's libm and cascaded sums, the ratio csrc/optim.hip colsum_final found between a sequential
# and a pairwise fp32 chain.  Nothing here comes from a kernel's output.
MEASURED = {                      # measured       TOL
    "z": 9.0e-08,                 # 8.922e-08      3.6e-07
    "kl": 4.7e-08,                # 4.620e-08      1.9e-07
    "kl_sum": 1.8e-07,            # 1.795e-07      7.2e-07
    "dml": 9.8e-08,               # 9.779e-08      3.9e-07
    "rec": 1.4e-07,               # 1.361e-07      5.6e-07
    "rec_sum": 1.4e-07,           # 1.361e-07      5.6e-07
    "dmu": 1.5e-07,               # 1.434e-07      6.0e-07
    "dlv": 2.8e-07,               # 2.755e-07      1.1e-06
    "finalize": 8.3e-08,          # 8.287e-08      3.3e-07
    "masked_mean": 9.9e-08,       # 9.844e-08      4.0e-07
    "masked_mean_bwd": 4.5e-08,   # 4.480e-08      1.8e-07
    "clip_g": 5.2e-08,            # 5.173e-08      2.1e-07
    "adam_p": 8.4e-08,            # 8.334e-08      3.4e-07
    "adam_m": 7.6e-08,            # 7.530e-08      3.0e-07
    "adam_v": 9.4e-08,            # 9.317e-08      3.8e-07
    "colsum": 1.6e-07,            # 1.555e-07      6.2e-07
}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
