"""Diverse beam search (include/slimt_hip.h, slimt_hip_ctx_set_beam_groups): a step as, per group, beam_cases.row_scores and
a sort of ALL the group's candidates by the contract's order under the count; the search as beam_cases.beam_translate with
that step and the groups' start state patched in."""
from unittest import mock

import numpy as np

from support import beam_cases as BC

F = np.float32


def start_state(B, k, G):
    """slot j g of every group live at +0, the others dead"""
    totals, flags = np.full((B, k), -np.inf, F), np.zeros((B, k), np.uint32)
    totals[:, ::k // G], flags[:, ::k // G] = 0.0, BC.LIVE
    return totals.reshape(-1), flags.reshape(-1)


def step(logits, totals, flags, k, G, penalty, eos=0, ids=None):
    """slimt_hip_beam_step_grouped's outputs (parent, token, token_score, totals, flags), each [B * k]"""
    logits = np.asarray(logits, dtype=F)
    totals, flags = np.asarray(totals, dtype=F), np.asarray(flags, dtype=np.uint32)
    R, g = logits.shape[0], k // G
    parent, token = np.full(R, BC.NONE, np.uint32), np.full(R, BC.NONE, np.uint32)
    score, tot, fl = np.zeros(R, F), np.full(R, -np.inf, F), np.zeros(R, np.uint32)
    for b in range(R // k):
        taken = []  # the columns the groups before this one were extended with
        for j in range(G):
            aug, cand, slot, logit, col, lps, carried = [], [], [], [], [], [], []
            for s in range(j * g, (j + 1) * g):
                r = b * k + s
                if flags[r] == BC.FINISHED:
                    one = (totals[r:r + 1], totals[r:r + 1], [s], [F(0)], [0], [F(0)], [True])
                elif flags[r] == BC.LIVE and BC.row_max(logits[r])[0]:
                    lp = BC.row_scores(logits[r])[4]
                    with np.errstate(all="ignore"):
                        c = (totals[r] + lp).astype(F)
                    n = np.zeros(len(c), F)
                    for x in taken:
                        n[x] += 1
                    a = np.where(n == 0, c, c - (F(penalty) * n).astype(F)).astype(F)  # the product in f32, then one f32 subtraction
                    keep = np.flatnonzero(c != -np.inf)
                    one = (a[keep], c[keep], np.full(len(keep), s), logits[r, keep], keep, lp[keep], np.zeros(len(keep), bool))
                else:
                    continue
                for lst, x in zip((aug, cand, slot, logit, col, lps, carried), one):
                    lst.append(np.asarray(x))
            if not aug:
                continue
            aug, cand, slot, logit, col, lps, carried = (np.concatenate(x) for x in (aug, cand, slot, logit, col, lps, carried))
            # aug descending (+0 == -0), slot ascending, logit descending, column ascending
            order = np.lexsort((col, -logit.astype(np.float64), slot, -aug.astype(np.float64)))[:g]
            for i, o in enumerate(order):
                r = b * k + j * g + i
                parent[r], tot[r] = slot[o], cand[o]
                if carried[o]:
                    fl[r] = BC.FINISHED
                else:
                    token[r] = col[o] if ids is None else ids[col[o]]
                    score[r] = lps[o]
                    fl[r] = BC.FINISHED if token[r] == eos else BC.LIVE
                    taken.append(int(col[o]))
    return parent, token, score, tot, fl


def translate(oracle, om, m, ids, lens, sl, k, G, penalty, mode=0):
    """BC.beam_translate in G groups, and group_of [B, k] (the final slot / g in the output's order, NONE for a dead slot)"""
    group_of, order = [], BC.final_order

    def grouped(logits, totals, flags, beam, eos_id=0, ids=None):
        return step(logits, totals, flags, beam, G, penalty, eos_id, ids)

    def ordered(totals, lens_b, flags, mode):
        slots = order(totals, lens_b, flags, mode)
        group_of.append([BC.NONE if flags[s] == BC.DEAD else s // (k // G) for s in slots])
        return slots
    with mock.patch.object(BC, "beam_step_host", grouped), mock.patch.object(BC, "start_state", lambda B, beam: start_state(B, beam, G)), \
            mock.patch.object(BC, "final_order", ordered):
        out = BC.beam_translate(oracle, om, m, ids, lens, sl, k, mode)
    return out + (np.asarray(group_of, np.uint32),)
