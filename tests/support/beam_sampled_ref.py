"""Sampling without replacement on a beam call (slimt_hip_ctx_set_beam_sampling): slimt_amd/csrc/beam_sampled.h restated in
NumPy, float32 step by step, and one selection by brute force over every column of every live slot. The beam's arithmetic
(tr_exp, sm_log, fmaf, row_scores) is tests/support/beam_cases.py's; the noise is sampling.h's own bits through
tests/test_sampling_checker.py's host harness (fmaf(0, 1, g) = g)."""
import numpy as np

from support import beam_cases as BC
from test_sampling_checker import harness as sm_harness, row_keys

f32 = np.float32
NINF = f32(-np.inf)


def sb_exp(d):
    d = np.asarray(d, dtype=np.float32)
    inside = d > f32(-28.0)
    return np.where(inside, BC.tr_exp(np.where(inside, d, f32(0))), f32(0)).astype(np.float32)


def sb_log1mexp(d):
    d = np.asarray(d, dtype=np.float32)
    near = d > f32(-0.25)
    dn = np.where(near, d, f32(0))
    p = np.full(d.shape, f32(1.98412698e-4), np.float32)
    for c in (1.38888889e-3, 8.33333333e-3, 4.16666667e-2, 1.66666667e-1, 0.5, 1.0):
        p = BC.fmaf(p, dn, f32(c))
    om_near = np.maximum(-dn * p, f32(1.17549435e-38))
    om_far = f32(1) - sb_exp(np.where(near, f32(-1), d))
    return BC.sm_log(np.where(near, om_near, om_far).astype(np.float32))


def sb_condition(G, Z, psi):
    G, Z, psi = np.broadcast_arrays(*(np.asarray(x, dtype=np.float32) for x in (G, Z, psi)))
    with np.errstate(all="ignore"):
        same = psi == Z
        v = (G - psi) + sb_log1mexp(np.where(same, f32(-1), psi - Z))
        top = G - np.maximum(f32(0), v)
        out = top - BC.sm_log(f32(1) + sb_exp(-np.abs(v)))
    return np.where(same, G, out).astype(np.float32)


def gumbel(K, slot, step, ids):
    """g of every id for slot `slot` of the source keyed K at `step`"""
    k_s = sm_harness().sentence_key(int(K), int(slot))
    return row_keys(k_s, step, np.zeros(len(ids), np.float32), ids, 1.0)


_rows = {}


def _row_scores(l):
    key = l.tobytes()
    if key not in _rows:
        _rows[key] = BC.row_scores(l)
    return _rows[key]


def step_sampled_host(logits, totals, perturbed, flags, beam, keys=None, step=0, eos_id=0, ids=None):
    """slimt_hip_beam_step_sampled's outputs (parent, token, token_score, totals, perturbed, flags), each [B * beam]"""
    logits = np.asarray(logits, dtype=np.float32)
    totals, perturbed = np.asarray(totals, dtype=np.float32), np.asarray(perturbed, dtype=np.float32)
    R, N = logits.shape
    k = int(beam)
    col_ids = np.arange(N, dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32)
    cands = []  # (source, slot, rank, column | -1, lp, phi, G, Z, psi)
    for b in range(R // k):
        K = sm_harness().sentence_key(0, b) if keys is None else int(keys[b])
        for s in range(k):
            r = b * k + s
            if flags[r] == BC.FINISHED:
                cands.append((b, s, 0, -1, f32(0), totals[r], perturbed[r], perturbed[r], perturbed[r]))
            elif flags[r] == BC.LIVE:
                usable, _, _, _, lp = _row_scores(logits[r])
                if not usable:
                    continue
                with np.errstate(all="ignore"):
                    phi = (totals[r] + lp).astype(np.float32)
                    psi = ((phi + gumbel(K, s, step, col_ids)) + f32(0)).astype(np.float32)
                cols = np.nonzero(lp > NINF)[0]
                order = cols[np.lexsort((cols, -psi[cols].astype(np.float64)))][:k]
                for j, c in enumerate(order):
                    cands.append((b, s, j, int(c), lp[c], phi[c], perturbed[r], psi[order[0]], psi[c]))
    parent, token = np.full(R, BC.NONE, np.uint32), np.full(R, BC.NONE, np.uint32)
    score, tot, G = np.zeros(R, np.float32), np.full(R, NINF, np.float32), np.full(R, NINF, np.float32)
    fl = np.zeros(R, np.uint32)
    if not cands:
        return parent, token, score, tot, G, fl
    cand = sb_condition([c[6] for c in cands], [c[7] for c in cands], [c[8] for c in cands])
    taken = {}
    for i in sorted(range(len(cands)), key=lambda i: (cands[i][0], -float(cand[i]), cands[i][1], cands[i][2])):
        b, s, _, c, lp, phi = cands[i][:6]
        n = taken.get(b, 0)
        if n == k:
            continue
        taken[b] = n + 1
        r = b * k + n
        parent[r], tot[r], G[r] = s, phi, cand[i]
        if c < 0:
            fl[r] = BC.FINISHED
        else:
            token[r], score[r] = col_ids[c], lp
            fl[r] = BC.FINISHED if token[r] == eos_id else BC.LIVE
    return parent, token, score, tot, G, fl


def start_state(B, beam):
    totals, flags = BC.start_state(B, beam)
    return totals, totals.copy(), flags


def sampled_beam_translate(oracle, om, m, ids, lens, sl, k, keys, mode=0, limit_factor=1.5, eos=0):
    """(out_ids [B,k,T], out_len, totals, token_scores, align, perturbed [B,k]) of the armed call: BC.beam_translate's
    search over the oracle's decode_step in PORTABLE mode with `step_sampled_host` as the selection"""
    oracle.set_mode(oracle.PORTABLE)
    try:
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lens = np.asarray(lens, dtype=np.uint32)
        B, S = ids.shape
        T, R = BC.tmax_of(S, limit_factor), B * k
        row_src = np.repeat(np.arange(B), k)
        mask1 = oracle.make_mask(lens, S)
        enc1 = om.encode(om.embed(ids), mask1)
        enc, mask = np.ascontiguousarray(enc1[row_src]), np.ascontiguousarray(mask1[row_src])
        states = np.zeros((m.dec_layers, R, m.D), np.float32)
        totals, G, flags = start_state(B, k)
        hyps = [dict(tok=[], sc=[], al=[]) for _ in range(R)]
        prev = None
        for t in range(T):
            logits, attn = om.decode_step(enc, mask, states, prev, sl)
            logits = np.ascontiguousarray(logits, dtype=np.float32)
            parent, token, score, totals, G, flags = step_sampled_host(logits, totals, G, flags, k, keys, t, eos, sl)
            new_hyps, new_states, prev = [], np.zeros_like(states), np.zeros(R, np.uint32)
            for r in range(R):
                b = r // k
                if flags[r] == BC.DEAD:
                    new_hyps.append(dict(tok=[], sc=[], al=[]))
                    continue
                p = b * k + int(parent[r])
                h = hyps[p]
                if token[r] != BC.NONE:
                    row = np.zeros(S, np.float32)
                    row[: int(lens[b])] = attn[p, 0, 0, : int(lens[b])]
                    h = dict(tok=h["tok"] + [int(token[r])], sc=h["sc"] + [score[r]], al=h["al"] + [row])
                new_hyps.append(h)
                new_states[:, r] = states[:, p]
                if flags[r] == BC.LIVE:
                    prev[r] = token[r]
            hyps, states = new_hyps, new_states
            if not (flags == BC.LIVE).any():
                break
        out, ln = np.zeros((B, k, T), np.uint32), np.zeros((B, k), np.uint32)
        tot, pert = np.full((B, k), NINF, np.float32), np.full((B, k), NINF, np.float32)
        sc, al = np.zeros((B, k, T), np.float32), np.zeros((B, k, T, S), np.float32)
        for b in range(B):
            rows = slice(b * k, (b + 1) * k)
            order = BC.final_order(totals[rows], [len(h["tok"]) for h in hyps[rows]], flags[rows], mode)
            for j, s in enumerate(order):
                h, n = hyps[b * k + s], len(hyps[b * k + s]["tok"])
                if flags[b * k + s] == BC.DEAD:
                    continue
                out[b, j, :n], ln[b, j], tot[b, j], pert[b, j] = h["tok"], n, totals[b * k + s], G[b * k + s]
                sc[b, j, :n] = h["sc"]
                if n:
                    al[b, j, :n] = np.stack(h["al"])
        return out, ln, tot, sc, al, pert
    finally:
        oracle.set_mode(oracle.FAITHFUL)
