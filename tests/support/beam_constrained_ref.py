"""Beam search under step constraints: the rows z' from constraints_ref.sets, a step as beam_cases.beam_step_host over them,
the search as beam_cases.beam_translate with that step, the kernel test's crafted state. A setting is constraints_ref's."""
from unittest import mock

import numpy as np

from support import beam_cases as BC
from support import constraints_ref as CR

F = np.float32


def z_rows(logits, hists, flags, cn, ids, eos):
    """(z' [R, N], banned columns [R], lifted [R]); only live rows are constrained"""
    z = np.array(logits, dtype=F)
    R, N = z.shape
    nb, lifted = np.zeros(R, np.uint32), np.zeros(R, bool)
    for r in np.flatnonzero(np.asarray(flags) == BC.LIVE):
        grams, other, seen = CR.sets(hists[r], cn, N, ids, eos)
        banned, theta, l = grams | other, F(cn[1]), z[r].copy()
        with np.errstate(invalid="ignore", over="ignore"):
            zz = np.where(seen, np.where(l > 0, l * (F(1.0) / theta), l * theta), l).astype(F)
        valid = ~np.isnan(zz)
        nb[r], lifted[r] = banned.sum(), valid.any() and not (valid & ~banned).any()
        z[r] = zz if lifted[r] else np.where(banned, F(-np.inf), zz)
    return z, nb, lifted


def step(logits, totals, flags, k, eos, ids, hists, cn):
    z, nb, lifted = z_rows(logits, hists, flags, cn, ids, eos)
    out = BC.beam_step_host(z, totals, flags, k, eos, ids)
    parent, token = out[0], out[1]
    new = []
    for r in range(len(hists)):
        p = None if parent[r] == BC.NONE else hists[r - r % k + int(parent[r])]
        new.append([] if p is None else list(p) + ([] if token[r] == BC.NONE else [int(token[r])]))
    return out, new, nb, lifted


def translate(oracle, om, m, ids, lens, sl, k, cn, mode=0, trace=None):
    """BC.beam_translate under the setting; trace (a dict) also gets `lifts`, the live slots that lifted their bans"""
    hists, real, trace = [[] for _ in range(len(ids) * k)], BC.beam_step_host, {} if trace is None else trace

    def constrained(logits, totals, flags, beam, eos_id=0, ids=None):
        with mock.patch.object(BC, "beam_step_host", real):
            out, hists[:], _, lifted = step(logits, totals, flags, beam, eos_id, ids, hists, cn)
        trace["lifts"] = trace.get("lifts", 0) + int(lifted.sum())
        return out
    with mock.patch.object(BC, "beam_step_host", constrained):
        return BC.beam_translate(oracle, om, m, ids, lens, sl, k, mode, trace=trace)


def violations(out, ln, cn, eos=0):  # hypotheses that repeat an n-gram of the setting's size or end in EOS before min_length
    (n, _, min_length, _), bad = cn, 0
    for h in ([int(x) for x in h[:L]] for h, L in zip(out.reshape(-1, out.shape[-1]), ln.reshape(-1))):
        grams = [tuple(h[q:q + n]) for q in range(len(h) - n + 1)] if n else []
        bad += len(set(grams)) < len(grams) or bool(h and h[-1] == eos and len(h) - 1 < min_length)
    return bad


VARIANTS = {"step 0": (0, (1, 1.3, 1)), "n = 8, eos banned": (20, (8, 1.3, 21)), "n = 1, eos free": (20, (1, 0.7, 20))}


def crafted(N, k, B, with_ids, variant):
    """(logits, totals, flags, histories [R][t], t, setting, ids, eos, roles): quarter-step rows, histories ending in the window
    they begin with (h[7] is banned under n = 8), an id without a column suppressed, the edges on the rows `roles` names"""
    t, (n, theta, min_length) = VARIANTS[variant]
    r, R = np.random.default_rng(100 * N + 10 * k + B + t + n), B * k
    ids, eos = CR.layout(N, with_ids)
    tok = (lambda c: int(c)) if ids is None else (lambda c: int(ids[c]))
    cn = (n, theta, min_length, (2 if with_ids else N + 5,))
    logits = (np.round(r.normal(0, 3, size=(R, N)) * 4) / 4).astype(F)
    if t == 0:
        return (logits,) + BC.start_state(B, k) + ([[] for _ in range(R)], t, cn, ids, eos, {})
    totals, flags = (-np.round(r.uniform(0, 6, size=R) * 2) / 2).astype(F), np.full(R, BC.LIVE, np.uint32)
    hists = [[tok(c) for c in r.integers(0, N, t)] for _ in range(R)]
    for h in hists:
        h[t - 7:] = h[:7]
    top, roles = int(np.argmax(logits[0])), {"max banned": 0}
    logits[0, top] += F(1.0)
    hists[0][7] = tok(top)  # the row's one maximum is banned
    if k >= 3:  # a second live slot of the source with the same row and total, and another history
        logits[1], totals[1] = logits[0], totals[0]
        hists[1][7] = tok((top + 1) % N)
        roles["twin"] = 1
    for role, row in zip(("finished", "lifts", "seen", "dead"), range(2 if k >= 3 else 1, R)):
        roles[role] = row
        if role == "finished":
            flags[row], totals[row] = BC.FINISHED, 0.5  # ahead of every live candidate
        elif role == "dead":
            flags[row], totals[row] = BC.DEAD, -np.inf
        elif role == "lifts":  # under n = 1 every valid column is in the history: all of them, or the two that are not NaN
            if N <= t:
                hists[row][:N] = [tok(c) for c in range(N)]
            else:
                logits[row, 2:] = np.nan
                hists[row][:2] = [tok(0), tok(1)]
        elif N >= 17:  # seen: a positive and a negative logit, neither banned under n = 8
            logits[row, 3], logits[row, 4] = 2.0, -2.0
            hists[row][7:10] = [tok(5), tok(3), tok(4)]
    return logits, totals, flags, hists, t, cn, ids, eos, roles
