"""numpy oracle of the CTC evaluation kernels (csrc/ctc_eval.hip): greedy decode, edit-distance
alignment, the MD / PER counts and Viterbi over the CTC topology, per utterance in host loops --
the form the reference runs on every batch.  Integers, or float64 sums of the fp32 emissions in
frame order, so the kernels are compared for equality.

This file is the DEFINITION of the alignment's tie rule (SpeechBrain's op_table rule as recalled;
SpeechBrain is not available to pin it): at cell (i, j) the diagonal only if its cost is strictly
below both others, else the deletion (from (i - 1, j)) if strictly below the insertion, else the
insertion; row 0 is insertions, column 0 deletions; the backtrace starts at (L_a, L_b)."""
import numpy as np

from hmm_np import round_len

NINF = -np.inf


def greedy_decode(pout, Tb, blank):
    """pout [T, C] -> list: argmax per frame t < Tb (a tie keeps the lowest class), repeats merged,
    blanks dropped."""
    out, prev = [], -1
    for t in range(Tb):
        c = int(np.argmax(pout[t]))  # the first maximum
        if c != blank and c != prev:
            out.append(c)
        prev = c
    return out


def greedy_batch(pout, lens, blank):
    """(pred [B, T] int32 padded with -1, pred_len [B])."""
    pout = np.asarray(pout)
    B, T, _ = pout.shape
    pred, n = np.full((B, T), -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        seq = greedy_decode(pout[b], round_len(lens[b], T), blank)
        pred[b, :len(seq)], n[b] = seq, len(seq)
    return pred, n


def edit_align(a, b):
    """(ali: the token of b aligned to every position of a, -1 for a deletion; (I, D, S, len(a)))."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    la, lb = len(a), len(b)
    cost = np.zeros((la + 1, lb + 1), dtype=np.int64)
    op = np.zeros((la + 1, lb + 1), dtype=np.int8)  # 0 diagonal, 1 deletion, 2 insertion
    cost[:, 0], cost[0, :] = np.arange(la + 1), np.arange(lb + 1)
    op[1:, 0], op[0, 1:] = 1, 2
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            sub = cost[i - 1, j - 1] + (a[i - 1] != b[j - 1])
            dele, ins = cost[i - 1, j] + 1, cost[i, j - 1] + 1
            if sub < dele and sub < ins:
                cost[i, j], op[i, j] = sub, 0
            elif dele < ins:
                cost[i, j], op[i, j] = dele, 1
            else:
                cost[i, j], op[i, j] = ins, 2
    ali = [-1] * la
    i, j, n_ins, n_del, n_sub = la, lb, 0, 0, 0
    while i > 0 or j > 0:
        o = op[i, j]
        if o == 0:
            ali[i - 1] = b[j - 1]
            n_sub += a[i - 1] != b[j - 1]
            i, j = i - 1, j - 1
        elif o == 1:
            n_del += 1
            i -= 1
        else:
            n_ins += 1
            j -= 1
    assert n_ins + n_del + n_sub == cost[la, lb]
    return ali, (n_ins, n_del, n_sub, la)


def md_counts(ali, phn, cnncl):
    """The eight integers of ops.ctc_md_counts for one utterance (equal lengths)."""
    ali, phn, cnncl = np.asarray(ali), np.asarray(phn), np.asarray(cnncl)
    pm, gm, wrong = ali != cnncl, phn != cnncl, ali != phn
    return [int(np.sum(~pm & ~gm)), int(np.sum(pm & gm)), int(np.sum(~pm & gm)), int(np.sum(pm & ~gm)),
            int(np.sum(~gm)), int(np.sum(~gm & wrong)), int(np.sum(gm)), int(np.sum(gm & wrong))]


def align_batch(pred, pred_len, phns, phn_lens, cnncls, cnncl_lens):
    """(ali [B, 2, L] padded with -1, ops [B, 2, 4], counts [B, 8])."""
    phns, cnncls = np.asarray(phns), np.asarray(cnncls)
    B, L = phns.shape
    ali = np.full((B, 2, L), -1, dtype=np.int32)
    ops = np.zeros((B, 2, 4), dtype=np.int32)
    counts = np.zeros((B, 8), dtype=np.int32)
    for b in range(B):
        hyp = list(pred[b, :pred_len[b]])
        for r, (ref, rl) in enumerate(((phns, phn_lens), (cnncls, cnncl_lens))):
            n = round_len(rl[b], L)
            ali[b, r, :n], ops[b, r] = edit_align(ref[b, :n], hyp)
        n = min(round_len(phn_lens[b], L), round_len(cnncl_lens[b], L))
        counts[b] = md_counts(ali[b, 0, :n], phns[b, :n], cnncls[b, :n])
    return ali, ops, counts


def ctc_viterbi(lp, phns, blank):
    """lp [Tb, C] -> (score float64, boundary [Tb] 0/1, infeasible).  delta in float64 in frame
    order; a tie keeps stay, then next, then skip; of the two end nodes a tie keeps the final
    blank.  boundary: 1 at frame 0 and where the path enters phoneme k >= 1.  No path: (0, ones at
    frames 0 .. min(L, Tb) - 1, True)."""
    lp = np.asarray(lp, dtype=np.float64)
    Tb, L = lp.shape[0], len(phns)
    N = 2 * L + 1
    cls = np.full(N, blank, dtype=np.int64)
    cls[1::2] = phns
    skip = np.zeros(N, dtype=bool)
    for n in range(3, N, 2):
        skip[n] = cls[n] != cls[n - 2]
    bound = np.zeros(Tb, dtype=np.int32)
    if Tb == 0:
        return 0.0, bound, True
    e = lp[:, cls]
    d = np.full(N, NINF)
    d[:min(2, N)] = e[0, :min(2, N)]
    code = np.zeros((Tb, N), dtype=np.int8)
    for t in range(1, Tb):
        new = np.full(N, NINF)
        for n in range(N):
            best, c = d[n], 0
            if n >= 1 and d[n - 1] > best:
                best, c = d[n - 1], 1
            if skip[n] and d[n - 2] > best:
                best, c = d[n - 2], 2
            new[n], code[t, n] = best + e[t, n], c
        d = new
    vb, vp = d[N - 1], (d[N - 2] if N >= 2 else NINF)
    u = N - 2 if vp > vb else N - 1
    if not d[u] > NINF:
        bound[:min(L, Tb)] = 1
        return 0.0, bound, True
    score = float(d[u])
    for t in range(Tb - 1, -1, -1):
        c = int(code[t, u]) if t > 0 else 0
        bound[t] = (L >= 1) if t == 0 else (c != 0 and u % 2 == 1 and u >= 3)
        u -= c
    return score, bound, False


def viterbi_batch(pout, lens, phns, phn_lens, blank):
    """(vscore [B] float64, boundary [B, T] int32 with -1 past T_b, infeasible [B])."""
    pout, phns = np.asarray(pout), np.asarray(phns)
    B, T, _ = pout.shape
    L = phns.shape[1]
    vs, bd, inf = np.zeros(B), np.full((B, T), -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        Tb, Lb = round_len(lens[b], T), round_len(phn_lens[b], L)
        vs[b], bd[b, :Tb], inf[b] = ctc_viterbi(pout[b, :Tb], phns[b, :Lb], blank)
    return vs, bd, inf


def error_rate(ops):
    """100 (I + D + S) / sum L_a over [n, 4] rows."""
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, 4)
    return 100.0 * float(ops[:, :3].sum()) / float(ops[:, 3].sum())
