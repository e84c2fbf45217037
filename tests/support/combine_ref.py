"""Combined decoding (include/slimt_hip.h, slimt_hip_ctx_set_fanout_combine; slimt_amd/csrc/combine.h) restated in NumPy on
beam_cases.row_scores: `step` is one group's selection by a sort over every column, `translate` steps the oracle's decoder
over the groups' rows as beam_cases.beam_translate does. `crafted` plants the contract's edges in random rows."""
import numpy as np

from support import beam_cases as BC

f32 = np.float32


def step(rows, w, gap=-np.inf):
    """(column, s, lp [m]) of one group's rows [m, N] under weights w [m] and the gap"""
    rows, w = np.asarray(rows, np.float32), np.asarray(w, np.float32)
    m, N = rows.shape
    sc = [BC.row_scores(r) for r in rows]
    lp_at = lambda c: np.asarray([s[4][c] if s[0] else np.nan for s in sc], np.float32)
    if not sc[0][0]:
        return 0, f32(np.nan), lp_at(0)
    with np.errstate(all="ignore"):
        s = (w[0] * sc[0][4]).astype(np.float32)
        for j in range(1, m):
            if w[j] != 0 and sc[j][0]:
                s = np.where(np.isneginf(rows[j]), s, BC.fmaf(np.full(N, w[j], np.float32), sc[j][4], s)).astype(np.float32)
        cand = (rows[0] > -np.inf) & ((rows[0] - sc[0][1]).astype(np.float32) >= f32(gap)) & ~np.isnan(s)
    # candidates first, s descending (floats: +0 == -0), then the primary's logit descending, then the column
    c = min(range(N), key=lambda c: (not cand[c], -float(s[c]) if cand[c] else 0.0, -float(rows[0][c]), c))
    return c, (s[c] if cand[c] else f32(np.nan)), lp_at(c)


def steps(logits, m, w, gap=-np.inf, ids=None):
    """slimt_hip_combine_step's outputs over logits [G m, N]: (column [G], token [G], combined [G], member_scores [G, m])"""
    logits = np.asarray(logits, np.float32)
    got = [step(logits[g:g + m], w, gap) for g in range(0, logits.shape[0], m)]
    col = np.asarray([c for c, _, _ in got], np.uint32)
    return (col, col if ids is None else np.asarray(ids, np.uint32)[col], np.asarray([s for _, s, _ in got], np.float32),
            np.stack([lp for _, _, lp in got]))


def translate(oracle, om, m, ids, lens, row_src, sl, members, w, gap=-np.inf, limit_factor=1.5, eos=0):
    """(out_ids [R, T], out_len [R], scores [R, T], align [R, T, S]) of an armed fan-out call of R = len(row_src) rows"""
    oracle.set_mode(oracle.PORTABLE)
    try:
        ids, lens = np.ascontiguousarray(ids, dtype=np.uint32), np.asarray(lens, dtype=np.uint32)
        row_src = np.asarray(row_src)
        (B, S), R, T = ids.shape, len(row_src), BC.tmax_of(ids.shape[1], limit_factor)
        mask1 = oracle.make_mask(lens, S)
        enc1 = om.encode(om.embed(ids), mask1)
        enc, mask = np.ascontiguousarray(enc1[row_src]), np.ascontiguousarray(mask1[row_src])
        states = np.zeros((m.dec_layers, R, m.D), np.float32)
        out, ln = np.zeros((R, T), np.uint32), np.zeros(R, np.uint32)
        sc, al = np.zeros((R, T), np.float32), np.zeros((R, T, S), np.float32)
        done, prev = np.zeros(R // members, bool), None
        for t in range(T):
            logits, attn = om.decode_step(enc, mask, states, prev, sl)
            logits = np.ascontiguousarray(logits, dtype=np.float32)
            prev = np.zeros(R, np.uint32)
            for g in np.nonzero(~done)[0]:
                r0 = g * members
                c, _, lp = step(logits[r0:r0 + members], w, gap)
                tok = c if sl is None else sl[c]
                for j in range(members):
                    r, L = r0 + j, int(lens[row_src[r0 + j]])
                    out[r, t], sc[r, t], ln[r] = tok, lp[j], t + 1
                    al[r, t, :L] = attn[r, 0, 0, :L]
                prev[r0:r0 + members] = tok
                done[g] = tok == eos
            if done.all():
                break
        return out, ln, sc, al
    finally:
        oracle.set_mode(oracle.FAITHFUL)


def crafted(N, m, G=3, seed=0):
    """logits [G m, N] on quarter steps (ties in s, in l_0 and across columns everywhere): group 0 random with duplicated
    columns, group 1 with -inf entries in the primary and the contrast rows, group 2 a primary with a NaN; a contrast row
    holding a NaN (unusable, so skipped) is group 1's last for m > 2 and, for m = 2, group 0's where N is odd"""
    r = np.random.default_rng(100 * N + 10 * m + seed)
    x = (np.round(r.normal(0, 3, size=(G * m, N)) * 4) / 4).astype(np.float32)
    if N >= 4:
        x[:, N // 2:] = x[:, : N - N // 2]  # every column twice (and the primary's best: the lower column wins)
    x[m, r.integers(0, N, size=max(1, N // 8))] = -np.inf
    if m > 1:
        x[m + 1, r.integers(0, N, size=max(1, N // 8))] = -np.inf
        x[2 * m - 1 if m > 2 else N % 2, N // 3] = np.nan if m > 2 or N % 2 else -np.inf
    x[2 * m, N - 1] = np.nan
    return x
