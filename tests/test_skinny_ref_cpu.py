"""The skinny-product test harness checks itself (no GPU, no library): every addr_* twin's explicit
flat indexing over the placed, NaN-poisoned buffers must equal the ref_* of the logical operands
exactly (integer operands: every sum is exact), for every case tests/test_gpu_skinny_edges.py
launches -- so a wrong leading dimension, offset or column rule in tests/skinny_ref.py cannot hide
behind the kernel tests that build on it.  The case lists must have the properties they are named
for, from the Python twins of the host-side dispatch alone."""
import pytest
import torch

import skinny_ref as S
from skinny_ref import seed_of

LIMIT = 2.0 ** 24


def _check(kind, c, reduction):
    """addr twin == reference on the logical region, poison never read, nothing written outside the
    logical region, |reference| <= 16 * reduction < 2^24."""
    got, exp = S.addr_case(kind, c), S.expected(kind, c)
    for name, buf in c.outs.items():
        if name not in exp:
            assert got.get(name) is None, name
            continue
        flat = torch.from_numpy(got[name])
        assert torch.isfinite(flat).all(), f"{name}: the emulation read a poisoned element"
        ref = exp[name]
        assert torch.equal(buf.logical(flat), ref), name
        mask = buf.mask()
        assert int(mask.sum()) == ref.numel()
        assert torch.equal(flat[~mask], buf.flat.double()[~mask]), f"{name}: written outside the logical region"
        if ref.numel():
            assert ref.abs().max().item() <= 16 * reduction * getattr(c, "alpha", 1.0) + 8
            assert ref.abs().max().item() < LIMIT
            assert torch.equal(ref, ref.round() if getattr(c, "alpha", 1.0) == 1.0 else (ref * 8).round() / 8)
    for buf in c.ins.values():  # inputs: NaN (0x7F) everywhere but the logical region, finite there
        f = torch.from_numpy(buf.f64())
        m = buf.mask()
        assert torch.isnan(f[~m]).all() and torch.isfinite(f[m]).all()
        assert f[m].abs().max().item() <= 4 if m.any() else True
    return exp


@pytest.mark.parametrize("args", S.NT_CASES, ids=str)
def test_nt_twin(args):
    M, N, K, padded = args
    c = S.make_nt(M, N, K, padded, seed=seed_of(args))
    _check("nt", c, K)
    assert c.ins["A"].ld == K + (8 if padded else 0) and c.ins["Bt"].ld == K + (24 if padded else 0)
    assert c.outs["C"].ld == N + (4 if padded else 0)


@pytest.mark.parametrize("args", S.NT8_CASES, ids=str)
def test_nt_fp8_twin(args):
    M, N, K, padded = args
    c = S.make_nt(M, N, K, padded, fp8=True, seed=seed_of(args))
    _check("nt", c, K)
    assert c.ins["A"].flat.dtype == torch.uint8 and c.ins["A"].ld == K + (16 if padded else 0)
    assert c.alpha == 2.0 ** -3


@pytest.mark.parametrize("args", S.proj_cases(), ids=str)
def test_proj_twin(args):
    f16, M, N, K, bias, padded = args
    c = S.make_proj(f16, M, N, K, bias, padded, seed=seed_of(args))
    exp = _check("proj", c, K)
    assert exp["C"].abs().max().item() <= 2048
    assert torch.equal(exp["C"].to(torch.float16).double(), exp["C"])  # exact in fp16
    assert c.outs["C"].flat.dtype == (torch.float16 if f16 else torch.float32)


def test_proj_cases_cover_every_axis_value_for_both_output_types():
    cases = S.proj_cases()
    assert 28 <= len(cases) <= 32
    for f16 in (0, 1):
        mine = [c for c in cases if c[0] == f16]
        assert {c[1] for c in mine} == set(S.PROJ_MS)
        assert {c[2] for c in mine} == set(S.PROJ_NS)
        assert {c[3] for c in mine} == set(S.PROJ_KS)
        assert {c[4] for c in mine} == {0, 1, 2, 3}
        assert any(not c[5] for c in mine) and any(c[5] for c in mine)
    # the partial last 128-column pass / 512-column workgroup the N values are chosen for
    assert all(n % 128 for n in (144, 528, 1040)) and 528 > 512 and 1040 > 1024


@pytest.mark.parametrize("args", S.TN_CASES, ids=str)
def test_tn_twin(args):
    M, NB, nw, bias, K, padded = args
    c = S.make_tn(M, NB, nw, bias, K, padded, seed=seed_of(args))
    _check("tn", c, K)
    B = c.ins["B"].logical().float()
    first_free = nw + (1 if bias else 0)
    assert (B[:, first_free:] != 0).all(), "B's unused columns must be non-zero"
    if bias:
        assert (B[:, nw] == 1).all()


@pytest.mark.parametrize("args", S.TN8_CASES, ids=str)
def test_tn_fp8_twin(args):
    M, NB, nw, bias, K, padded = args
    c = S.make_tn(M, NB, nw, bias, K, padded, fp8=True, seed=seed_of(args))
    _check("tn", c, K)
    assert c.ins["A"].flat.dtype == torch.uint8 and c.ins["A"].ld == M + (16 if padded else 0)


@pytest.mark.parametrize("args", S.DZW_CASES, ids=str)
def test_dzw_twin(args):
    M, K8, bias, padded = args
    c = S.make_dzw(M, K8, bias, padded, seed=seed_of(args))
    _check("dzw", c, max(M, K8))
    zb = c.ins["zb"].logical().float()
    assert (zb[:, 32] == 1).all() and (zb[:, 33:] == 0).all() and zb.shape[1] == 48  # z | 1 | 0
    if padded:
        assert (c.ins["A"].ld, c.ins["Wt"].ld, c.ins["zb"].ld, c.outs["dZ"].ld) == (K8 + 8, K8 + 16, 56, 36)


def test_nt_case_lists_have_their_properties():
    for form, shapes in S.NT_SHAPES.items():
        for M, K in shapes:
            for N in S.NS:
                assert S.nt_form(M, N, K) == form, (M, N, K)
    assert S.nt_form(4095, 32, 256) == "ks" and S.nt_form(4096, 32, 256) == "lds"  # both sides of M >= 4096
    assert all(K // 256 == 1 and S.nt_form(M, 64, K) == "lds" for M, K in S.NT_ONE_CHUNK)
    assert all((K // 256) % 2 == 1 and K // 256 > 1 and S.nt_form(M, 64, K) == "lds" for M, K in S.NT_ODD_CHUNKS)
    assert all(s in S.NT_SHAPES["lds"] for s in S.NT_ONE_CHUNK + S.NT_ODD_CHUNKS)
    # ks: K / 4 per wave, unrolled by 128, tail by 32 -- both loops run
    assert all(K // 4 >= 128 and (K // 4) % 128 and S.nt_form(M, 16, K) == "ks" for M, K in S.NT_KS_BOTH_LOOPS)
    assert all(s in S.NT_SHAPES["ks"] for s in S.NT_KS_BOTH_LOOPS)
    assert [S.nt_form(M, N, K) for M, N, K in S.NT_TIGHT] == ["plain", "ks", "lds"]
    assert all(S.nt_form(M, N, 0) == "ks" for M, N in S.NT_K0)       # K == 0 never takes the LDS form
    assert any(M >= 4096 for M, _ in S.NT_K0) and any(M < 4096 for M, _ in S.NT_K0)
    assert all(S.nt_form(M, 16, K) == "lds" for M, K in S.NT8_SHAPES)  # the only form the fp8 entry has


def test_tn_case_lists_have_their_properties():
    for M, NB, nw, bias, K in S.TN_EMPTY_SPLIT:
        s, kc, empty = S.tn_plan(M, K)
        assert (s, kc, empty) == (8, 320, [7])
        assert s < -(-K // 256) and kc % 64 == 0
    for M, NB, nw, bias in S.TN_ROWS:
        assert M % 64 == 0 and nw + (1 if bias else 0) <= NB
        for K in S.TN_KS:
            s, kc, empty = S.tn_plan(M, K)
            assert s * kc >= K and not empty
    assert S.tn_plan(64, 1000)[0] == 4                                # several splits in the small cases too
    assert {NB for _, NB, _, _ in S.TN_ROWS} == {16, 32, 48, 64}      # every template instance
    assert any(nw + 1 == NB and b for _, NB, nw, b in S.TN_ROWS)      # the ones column in the last column
    assert {b for _, _, _, b in S.TN_ROWS} == {0, 1, 2, 3}
    assert all(r in S.TN_ROWS for r in S.TN8_ROWS)


def test_dzw_case_lists_have_their_properties():
    plans = {s: S.dzw_plan(*s) for s in S.DZW_SHAPES}
    assert plans[(1, 256)] == (1, [1], [1])
    assert plans[(129, 256)] == (1, [2], [2])
    assert plans[(300, 768)] == (1, [3], [9])
    assert plans[(512, 256)] == (1, [4], [4])
    assert plans[(513, 512)] == (2, [4, 1], [8, 2])
    assert plans[(640, 768)] == (2, [4, 1], [12, 3])
    assert plans[(900, 1024)] == (2, [4, 4], [16, 16])
    assert all(S.dzw_plan(*s)[2][-1] == 1 for s in S.DZW_NTL_1)
    assert all(S.dzw_plan(*s)[1][-1] == 2 for s in S.DZW_NRB_2)
    assert all(any(n % 2 and n > 1 for n in S.dzw_plan(*s)[2]) for s in S.DZW_ODD_NTL)
    assert all(s in S.DZW_SHAPES for s in S.DZW_NTL_1 + S.DZW_NRB_2 + S.DZW_ODD_NTL + S.DZW_TIGHT)
    assert any(M < 128 for M, _ in S.DZW_SHAPES)


def test_sentinel_is_exact_in_every_output_type():
    assert float(torch.tensor(S.SENTINEL)) == S.SENTINEL
    assert torch.isfinite(torch.tensor(S.SENTINEL, dtype=torch.float16))
