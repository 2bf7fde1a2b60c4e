"""Timing of the CRDNN front end's kernels (csrc/conv2d.hip) at the CRDNN_CTC recipe's shape:
B = 8, T = 168, F = 120 then 60, channels 1 -> 128 -> 128 and 128 -> 256 -> 256 (DESIGN.md
section 4, "The CRDNN front end").

    python tools/conv2d_bench.py [--rounds 7] [--iters 10] [--no-step]

HIP events around `iters` launches, medians of `rounds` alternating rounds, one JSON line:

(a) each MFMA convolution's forward (pad + weight pack + implicit GEMM, one ABI call) against a
    composition of existing kernels: three ops.w2v_gemm launches (mlvae_gemm_bf16, beta = 1 on the
    second and third) over the overlapping rows of the same reflect-padded bf16 copy, one per time
    tap, K = 3 Cin each.  The composition computes every padded position ((T+2)(F+2) / (T F) of
    the work) and its pad is timed separately (mlvae_conv2d_pad_bf16); its bf16 weights are
    prepared outside the timed region.  Both outputs are compared first (2e-5 max-relative).
(b) achieved TFLOP/s (2 M N 9 Cin flops) of forward, input gradient and weight gradient.
(c) the LayerNorm / pool kernels: ms, and GB/s over the bytes each must move (x read once, y
    written once; backward: x and dy read, dx written).
(d) ms per training step (forward, CTC loss, backward, Adam) of the CRDNN_CTC network with the
    front end (model_cnn.yaml's modules, bf16) next to the network without it (model.yaml's, in
    its fp32 default and in bf16), B = 8, T = 168."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-vae_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

B, T = 8, 168
PEAK_BF16_TFLOPS = 2500.0  # MI355X dense bf16 MFMA peak
PEAK_HBM_GBS = 8000.0


def _timer(iters):
    def run(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    return run


def _alternate(forms, rounds, timer):
    """forms: {name: fn}; medians (ms) of `rounds` alternating rounds after a warm-up."""
    for fn in forms.values():
        fn()
        fn()
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ms[k].append(timer(fn))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                "max_ms": round(max(v), 4)} for k, v in ms.items()}


def conv_case(F, Cin, Cout, rounds, timer):
    from mlvae_hip import ops
    from mlvae_hip._lib import check, lib
    l, s = lib(), torch.cuda.current_stream().cuda_stream
    torch.manual_seed(F + Cin)
    x = torch.randn(B, T, F, Cin, device="cuda")
    w = torch.randn(Cout, Cin, 3, 3, device="cuda") / (9 * Cin) ** 0.5
    bias = torch.randn(Cout, device="cuda")
    dy = torch.randn(B, T, F, Cout, device="cuda")
    y, dx, dw, db = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w), torch.empty_like(bias)
    nb = max(l.mlvae_conv2d_workspace_size(op, B, T, F, Cin, Cout) for op in (0, 1, 2))
    ws = torch.empty(nb // 4 + 1, device="cuda")
    p = lambda t: t.data_ptr()

    def fwd():
        check(l.mlvae_conv2d_fwd(B, T, F, Cin, Cout, p(x), p(w), p(bias), p(y), p(ws), ws.numel() * 4, s))

    def dgrad():
        check(l.mlvae_conv2d_dgrad(B, T, F, Cin, Cout, p(dy), p(w), p(dx), p(ws), ws.numel() * 4, s))

    def wgrad():
        check(l.mlvae_conv2d_wgrad(B, T, F, Cin, Cout, p(dy), p(x), p(dw), p(db), p(ws), ws.numel() * 4, s))

    # the composition: three GEMMs over overlapping rows of the padded copy, every padded position
    Tp, Fp = T + 2, F + 2
    xp = torch.empty(B * Tp * Fp * Cin, device="cuda", dtype=torch.bfloat16)
    wk = [w[:, :, kt].permute(0, 2, 1).reshape(Cout, 3 * Cin).to(torch.bfloat16).contiguous() for kt in range(3)]
    rows = B * Tp * Fp - 2 * Fp - 2  # the last window stays inside the copy
    cfull = torch.empty(B * Tp * Fp, Cout, device="cuda")

    def pad():
        check(l.mlvae_conv2d_pad_bf16(B, T, F, Cin, p(x), p(xp), s))

    def gemm3():
        for kt in range(3):
            ops.w2v_gemm(xp[kt * Fp * Cin:], wk[kt], cfull, rows, Cout, 3 * Cin, Cin, Cout,
                         bias=bias if kt == 0 else None, beta=0.0 if kt == 0 else 1.0)

    fwd()
    pad()
    gemm3()
    torch.cuda.synchronize()
    got = cfull.view(B, Tp, Fp, Cout)[:, :T, :F]
    err = ((got - y).abs().max() / y.abs().max()).item()
    assert err < 2e-5, f"the composition and the kernel disagree: {err:.2e}"
    rec = _alternate({"fwd": fwd, "gemm3": gemm3, "pad": pad, "dgrad": dgrad, "wgrad": wgrad}, rounds, timer)
    flops = 2.0 * B * T * F * Cout * 9 * Cin
    out = {"shape": [B, T, F, Cin, Cout], "kernel_vs_composition_max_rel": float(f"{err:.2e}"), "ms": rec,
           "fwd_over_gemm3_plus_pad": round(rec["fwd"]["median_ms"] /
                                            (rec["gemm3"]["median_ms"] + rec["pad"]["median_ms"]), 3)}
    for k in ("fwd", "dgrad", "wgrad", "gemm3"):
        tf = flops / (rec[k]["median_ms"] * 1e-3) / 1e12
        out[f"{k}_tflops"] = round(tf, 1)
        out[f"{k}_of_peak"] = round(tf / PEAK_BF16_TFLOPS, 4)
    return out


def first_layer(rounds, timer):
    from mlvae_hip import ops
    F, Cout = 120, 128
    x = torch.randn(B, T, F, device="cuda")
    w = (torch.randn(Cout, 1, 3, 3, device="cuda") / 3).requires_grad_(True)
    bias = torch.randn(Cout, device="cuda").requires_grad_(True)
    dy = torch.randn(B, T, F, Cout, device="cuda")
    y = ops.conv2d_3x3(x, w, bias)
    rec = _alternate({"fwd": lambda: ops.conv2d_3x3(x, w, bias),
                      "wgrad": lambda: torch.autograd.grad(y, (w, bias), dy, retain_graph=True)}, rounds, timer)
    nbytes = B * T * F * Cout * 4
    return {"shape": [B, T, F, 1, Cout], "ms": rec,
            "fwd_GBs": round(nbytes / (rec["fwd"]["median_ms"] * 1e-3) / 1e9, 1),
            "wgrad_GBs": round(nbytes / (rec["wgrad"]["median_ms"] * 1e-3) / 1e9, 1)}


def ln_case(F, C, pool, rounds, timer):
    from mlvae_hip import ops
    x = torch.randn(B, T, F, C, device="cuda", requires_grad=True)
    g = torch.ones(F, C, device="cuda", requires_grad=True)
    b = torch.zeros(F, C, device="cuda", requires_grad=True)
    keep = (torch.rand(B, F // 2, device="cuda") >= 0.15).float() / 0.85 if pool else None
    y = ops.layer_norm_fc_act(x, g, b, pool=pool, keep=keep)
    dy = torch.randn_like(y)
    rec = _alternate({"fwd": lambda: ops.layer_norm_fc_act(x, g, b, pool=pool, keep=keep),
                      "bwd": lambda: torch.autograd.grad(y, (x, g, b), dy, retain_graph=True)}, rounds, timer)
    D, Do = F * C, (F // 2 if pool else F) * C
    fb, bb = (D + Do) * 4, (2 * D + Do) * 4  # bytes per frame each pass must move
    return {"shape": [B, T, F, C], "pool": pool, "ms": rec, "fwd_bytes_per_frame": fb, "bwd_bytes_per_frame": bb,
            "fwd_GBs": round(B * T * fb / (rec["fwd"]["median_ms"] * 1e-3) / 1e9, 1),
            "bwd_GBs": round(B * T * bb / (rec["bwd"]["median_ms"] * 1e-3) / 1e9, 1),
            "fwd_of_hbm_peak": round(B * T * fb / (rec["fwd"]["median_ms"] * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
            "bwd_of_hbm_peak": round(B * T * bb / (rec["bwd"]["median_ms"] * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}


def train_step(rounds, timer):
    from mlvae_hip import ops
    from mlvae_hip import optim as hip_optim
    from modules.crdnn import CRDNN, ConvCRDNN
    from modules.linear import Linear
    NPH = 39
    C = NPH + 2
    torch.manual_seed(1)
    feats = torch.randn(B, T, 120, device="cuda")
    lens = torch.ones(B, device="cuda")
    phns = torch.randint(0, NPH, (B, 30), device="cuda", dtype=torch.int32)
    phn_lens = torch.ones(B, device="cuda")
    out = {}
    for name, cls, kw, prec in (("model_cnn_bf16", ConvCRDNN, dict(cnn_blocks=2, time_pooling=True), "bf16"),
                                ("model_fp32", CRDNN, {}, "fp32"), ("model_bf16", CRDNN, {}, "bf16")):
        net = torch.nn.ModuleDict({"crdnn": cls(120, **kw), "output": Linear(512, C)}).cuda().train()
        opt = hip_optim.Adam(net.parameters(), lr=1e-4)

        def step():
            with ops.precision(prec):
                opt.zero_grad()
                pout = ops.log_softmax(net["output"](net["crdnn"](feats)))
                nll = ops.ctc_nll(pout, lens, phns, phn_lens, 1, C - 1)
                (nll / 30.0).mean().backward()
                opt.step()

        out[name] = _alternate({"step": step}, rounds, timer)["step"]
        del net, opt
        torch.cuda.empty_cache()
    out["cnn_over_plain_bf16"] = round(out["model_cnn_bf16"]["median_ms"] / out["model_bf16"]["median_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="skip (d), the training steps")
    args = ap.parse_args()
    from mlvae_hip import ops
    timer = _timer(args.iters)
    rec = {"measurement": "CRDNN front end kernels at the recipe's shape", "B": B, "T": T, "rounds": args.rounds,
           "iters": args.iters, "peak_bf16_tflops": PEAK_BF16_TFLOPS, "peak_hbm_GBs": PEAK_HBM_GBS}
    with ops.precision("bf16"):
        rec["conv"] = [conv_case(120, 128, 128, args.rounds, timer), conv_case(60, 128, 256, args.rounds, timer),
                       conv_case(60, 256, 256, args.rounds, timer)]
        rec["first_layer"] = first_layer(args.rounds, timer)
        rec["ln"] = [ln_case(120, 128, False, args.rounds, timer), ln_case(120, 128, True, args.rounds, timer),
                     ln_case(60, 256, False, args.rounds, timer), ln_case(60, 256, True, args.rounds, timer)]
    if not args.no_step:
        rec["train_step"] = train_step(max(3, args.rounds // 2), _timer(3))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
