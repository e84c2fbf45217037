"""The reference for the consensus selection (include/slimt_hip.h, slimt_hip_consensus_select): the definition restated with
collections.Counter multisets and Python floats (IEEE doubles), one operation after the other in the defined order. It
shares no code and no algorithm with slimt_amd/csrc/consensus.hip, which counts positions (k_p < c_r) and never builds a
multiset."""
from collections import Counter

import numpy as np

NO_ROW = 0xFFFFFFFF


def grams(tokens, g):
    """the multiset of g-grams of a token list"""
    return Counter(tuple(tokens[p:p + g]) for p in range(len(tokens) - g + 1))


def match_count(h, r, g):
    """M_g(h, r): the sum over the distinct g-grams of the smaller count"""
    a, b = grams(h, g), grams(r, g)
    return sum(min(n, b[x]) for x, n in a.items())


def pair_utility(h, r, max_order, beta2):
    """U(h, r), and the per-order scores it averages ([] when no order counts)"""
    scores = []
    for g in range(1, max_order + 1):
        ch, cr = max(len(h) - g + 1, 0), max(len(r) - g + 1, 0)
        if ch == 0 and cr == 0:
            continue
        scores.append(float((1 + beta2) * match_count(h, r, g)) / float(beta2 * cr + ch))
    total = 0.0
    for f in scores:
        total = total + f
    return (total / float(len(scores)) if scores else 0.0), scores


def rows_of(ids, lengths):
    """the rows as token lists, n_c = min(len[c], T)"""
    ids = np.asarray(ids, dtype=np.uint32)
    T = ids.shape[1] if ids.ndim == 2 else 0
    return [[int(t) for t in ids[c, :min(int(lengths[c]), T)]] for c in range(len(lengths))]


def select(ids, lengths, row_src, B, max_order=4, beta2=4):
    """(utility float64 [N], best uint32 [B]) as the definition gives them"""
    rows = rows_of(ids, lengths)
    N = len(rows)
    utility = np.zeros(N, np.float64)
    best = np.full(B, NO_ROW, np.uint32)
    for b in range(B):
        mine = [c for c in range(N) if int(row_src[c]) == b and len(rows[c]) > 0]  # the competing rows, ascending
        for h in mine:
            refs = [r for r in mine if r != h]
            total = 0.0
            for r in refs:
                total = total + pair_utility(rows[h], rows[r], max_order, beta2)[0]
            utility[h] = total / float(len(refs)) if refs else 0.0
        for h in mine:
            if best[b] == NO_ROW or utility[h] > utility[int(best[b])]:
                best[b] = h
    return utility, best


def bits(utility):
    return np.ascontiguousarray(utility, dtype=np.float64).view(np.uint64)
