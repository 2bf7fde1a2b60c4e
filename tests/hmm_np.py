"""float64 numpy oracle of the aligner's sequence lattice (csrc/align.hip): forward score,
posterior occupancies (by an explicit beta recursion, not autograd: logaddexp of two -inf has no
gradient), Viterbi with the "stay on a tie" rule, and the frame-accuracy counts.

Chain: phoneme p expands into spp states of classes p * spp + j.  HMM topology: nodes = states,
start in node 0, stay / next, end in the last node.  CTC topology: blank, s0, blank, .., blank;
stay / next / skip over a blank between two different classes; start in node 0 or 1, end in one
of the last two.  A path scores the sum of pout[t, class(node_t)]."""
import numpy as np

HMM, CTC = 0, 1
NINF = -np.inf


def round_len(rel, n):
    """rintf(n * rel) in fp32, half to even, clamped to [0, n] (the kernels' rule)."""
    r = int(np.rint(np.float32(n) * np.float32(rel)))
    return min(max(r, 0), n)


def expand(phns, spp):
    """Phoneme ids -> state classes id * spp + j."""
    phns = np.asarray(phns, dtype=np.int64)
    return (phns[:, None] * spp + np.arange(spp)[None, :]).reshape(-1)


def nodes(states, topo, blank=None):
    """(class of every node, skip[n]: the transition n - 2 -> n is allowed)."""
    states = np.asarray(states, dtype=np.int64)
    if topo == HMM:
        return states, np.zeros(len(states), dtype=bool)
    cls = np.full(2 * len(states) + 1, blank, dtype=np.int64)
    cls[1::2] = states
    skip = np.zeros(len(cls), dtype=bool)
    for n in range(3, len(cls), 2):
        skip[n] = cls[n] != cls[n - 2]
    return cls, skip


def _starts_ends(N, topo):
    k = 2 if topo == CTC else 1
    return list(range(min(k, N))), list(range(max(N - k, 0), N))


def forward_backward(lp, cls, skip, topo):
    """lp [T, C] float64 log-probs -> (score, gamma [T, N]); score -inf when no path exists."""
    T, N = lp.shape[0], len(cls)
    e = lp[:, cls]  # [T, N]
    starts, ends = _starts_ends(N, topo)
    alpha = np.full((T, N), NINF)
    alpha[0, starts] = e[0, starts]
    for t in range(1, T):
        p = alpha[t - 1]
        s1 = np.concatenate([[NINF], p[:-1]])
        s2 = np.where(skip, np.concatenate([[NINF, NINF], p[:-2]])[:N], NINF)
        alpha[t] = e[t] + np.logaddexp(np.logaddexp(p, s1), s2)
    beta = np.full((T, N), NINF)  # without the emission of frame t
    beta[T - 1, ends] = 0.0
    for t in range(T - 2, -1, -1):
        q = beta[t + 1] + e[t + 1]
        u1 = np.concatenate([q[1:], [NINF]])
        u2 = np.concatenate([np.where(skip, q, NINF)[2:], [NINF, NINF]])[:N]
        beta[t] = np.logaddexp(np.logaddexp(q, u1), u2)
    score = np.logaddexp.reduce(alpha[T - 1, ends])
    if not np.isfinite(score):
        return NINF, np.zeros((T, N))
    with np.errstate(invalid="ignore"):
        gamma = np.exp(np.where(np.isfinite(alpha) & np.isfinite(beta), alpha + beta - score, NINF))
    return float(score), gamma


def viterbi(lp, cls):
    """HMM topology: (score, path [T]); delta in float64, a tie keeps "stay"."""
    T, N = lp.shape[0], len(cls)
    e = lp[:, cls]
    d = np.full(N, NINF)
    d[0] = e[0, 0]
    take = np.zeros((T, N), dtype=bool)
    for t in range(1, T):
        below = np.concatenate([[NINF], d[:-1]])
        take[t] = below > d
        d = np.where(take[t], below, d) + e[t]
    path = np.zeros(T, dtype=np.int64)
    u = N - 1
    for t in range(T - 1, -1, -1):
        path[t] = u
        if t > 0 and take[t, u]:
            u -= 1
    return float(d[N - 1]), path


def lattice_batch(pout, lens, phns, phn_lens, spp, topo, blank=None):
    """pout [B, T, C] -> (score [B], dpout [B, T, C] for g = 1, ok [B]).  An HMM utterance with
    T_b < U_b (or no states / frames) and a CTC utterance without a path score 0 with gradient 0."""
    pout = np.asarray(pout, dtype=np.float64)
    B, T, C = pout.shape
    L = np.asarray(phns).shape[1]
    score, dp, ok = np.zeros(B), np.zeros_like(pout), np.zeros(B, dtype=bool)
    for b in range(B):
        Tb, Lb = round_len(lens[b], T), round_len(phn_lens[b], L)
        U = spp * Lb
        if Tb == 0 or (topo == HMM and (U == 0 or Tb < U)):
            continue
        cls, skip = nodes(expand(np.asarray(phns)[b, :Lb], spp), topo, blank)
        s, gamma = forward_backward(pout[b, :Tb], cls, skip, topo)
        if not np.isfinite(s):
            continue
        score[b], ok[b] = s, True
        for n, c in enumerate(cls):  # ascending node order
            dp[b, :Tb, c] += gamma[:, n]
    return score, dp, ok


def viterbi_batch(pout, lens, phns, phn_lens, spp):
    """(vscore [B] float64, align [B, T] with -1 past T_b; infeasible: 0 and all -1)."""
    pout = np.asarray(pout, dtype=np.float64)
    B, T, _ = pout.shape
    L = np.asarray(phns).shape[1]
    vs, al = np.zeros(B), np.full((B, T), -1, dtype=np.int64)
    for b in range(B):
        Tb, Lb = round_len(lens[b], T), round_len(phn_lens[b], L)
        U = spp * Lb
        if Tb == 0 or U == 0 or Tb < U:
            continue
        vs[b], al[b, :Tb] = viterbi(pout[b, :Tb], expand(np.asarray(phns)[b, :Lb], spp))
    return vs, al


def align_counts(align, lens, phns, phn_lens, spp, ends, samples_per_frame):
    """[B, 2] = (frames correct, T_b)."""
    align, phns, ends = np.asarray(align), np.asarray(phns), np.asarray(ends)
    B, T = align.shape
    L = phns.shape[1]
    out = np.zeros((B, 2), dtype=np.int64)
    for b in range(B):
        Tb, Lb = round_len(lens[b], T), round_len(phn_lens[b], L)
        out[b, 1] = Tb
        for t in range(Tb):
            u = align[b, t]
            if u < 0 or Lb == 0 or u // spp >= Lb:
                continue
            k = next((k for k in range(Lb) if t * samples_per_frame < ends[b, k]), Lb - 1)
            out[b, 0] += phns[b, u // spp] == phns[b, k]
    return out


def accuracy_average(counts):
    """accuracy.average: 100 * correct / frames per utterance (fp32), averaged over utterances."""
    c = np.asarray(counts, dtype=np.float32)
    return float(np.mean((c[:, 0] / c[:, 1]) * np.float32(100.0), dtype=np.float32))
