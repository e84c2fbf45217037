"""The cases tests/test_gpu_score_candidates.py compares with the checker and with slimt_hip_score on the duplicated sources,
and tests/test_candidate_case_fixtures.py checks for sitting where they claim (CPU). One table, like score_cases.py.

What the table is built around (slimt_amd/csrc/score_candidates.hip, engine.cpp score_device):
  * an attention workgroup walks a run of G = capi.CANDIDATE_RUN consecutive candidates of a chunk and restages K / V when the
    next LIVE candidate (target length > 0) names another source than the one staged;
  * chunks hold max(1, 8192 // T) whole candidates; runs are counted from the chunk's first candidate;
  * the attention keeps a second key per lane for sources above 64 tokens; its LDS is 8 S d_head bytes (64 KiB at 128 x 64).
Nothing here calls the library: counts, runs and chunk splits are written by hand and checked by arithmetic. The rank
checker (rank_reference) is the numpy float32 loop the issue defines; tests/test_candidate_case_fixtures.py works rows by hand."""
from collections import namedtuple

import numpy as np

from slimt_amd.capi import CANDIDATE_RUN as G
from support import model_shapes as MS
from support import score_cases as SC

NONE = 0xFFFFFFFF
CHUNK_ROWS = SC.CHUNK_ROWS

# model: a score_cases.MODELS name; ids / lens: the B sources; t_ids [N, T] / t_len [N]: the candidates; cand_src [N]
Case = namedtuple("Case", "model ids lens sl t_ids t_len cand_src")


def sorted_src(counts):
    return np.repeat(np.arange(len(counts), dtype=np.uint32), counts)


def build(model, S, T, src_lens, cand_src, t_len, seed, n_sl="model"):
    from slimt_amd import synth
    V = SC.dims_of(model)[5]
    if n_sl == "model":
        n_sl = None if V <= 517 else MS.SHORTLIST
    sl = None if n_sl is None else synth.make_shortlist(V, n_sl)
    ids, lens = SC.source(V, len(src_lens), S, seed, src_lens)
    cand_src = np.asarray(cand_src, np.uint32)
    t_len = np.asarray(t_len, np.uint32)
    assert cand_src.shape == t_len.shape
    t_ids = SC.random_targets(np.random.default_rng(seed), len(t_len), T, sl, V)
    return Case(model, ids, lens, sl, t_ids, t_len, cand_src)


def duplicated(c):
    """the score_cases.Inputs of the same work done the parent's way: every candidate with its own copy of its source"""
    return SC.Inputs(c.ids[c.cand_src], c.lens[c.cand_src], c.sl, c.t_ids, c.t_len, set())


def permuted(c, perm):
    perm = np.asarray(perm)
    return c._replace(t_ids=np.ascontiguousarray(c.t_ids[perm]), t_len=c.t_len[perm], cand_src=c.cand_src[perm])


def cycle_lengths(n, T, first=1):
    """n live target lengths walking 1 .. T"""
    return [1 + (first - 1 + i) % T for i in range(n)]


# ---- fan / order / entry points / alternatives -----------------------------------------------------------------------------
FAN_S, FAN_T = 7, 5
FAN_SRC_LENS = (7, 1, 4, 6)
FAN_COUNTS = (0, 1, 3, G + 1)
FAN_T_LEN = [5] + [0, 1, 5] + ([3, 5, 0, 2, 4] + cycle_lengths(G + 1, FAN_T))[:G + 1]


def fan():
    return build("micro", FAN_S, FAN_T, FAN_SRC_LENS, sorted_src(FAN_COUNTS), FAN_T_LEN, seed=501)


def order_perms(n):
    """reversed, and interleaved by source (stride 3 walks the sorted list so that neighbours differ in source wherever
    the sources' candidates allow it)"""
    inter = sorted(range(n), key=lambda i: (i % 3, i))
    return {"reversed": list(range(n))[::-1], "interleaved": inter}


# ---- runs ---------------------------------------------------------------------------------------------------------------------
RUN_COUNTS = {"one-G-1": (G - 1,), "one-G": (G,), "one-G+1": (G + 1,), "one-2G+1": (2 * G + 1,),
              "edge-G-G": (G, G), "mid-G-1-G+1": (G - 1, G + 1)}


def runs(name):
    counts = RUN_COUNTS[name]
    return build("micro", FAN_S, FAN_T, (7, 3)[:len(counts)], sorted_src(counts), cycle_lengths(sum(counts), FAN_T, 2), seed=520)


# ---- dead candidates: (counts, the empty candidates) ----------------------------------------------------------------------------
DEAD_CASES = {
    "first-in-run": ((G, G), [0]),
    "first-of-source-mid-run": ((G - 1, G + 1), [G - 1]),
    "first-of-source-on-edge": ((G, G), [G]),
    "last": ((G, G + 1), [2 * G]),
    "run-between-sources": ((2 * G, G), list(range(G, 2 * G))),
    "whole-source": ((G, G, G), list(range(G, 2 * G))),
    "all": ((G + 1,), list(range(G + 1))),
}


def dead(name):
    counts, empty = DEAD_CASES[name]
    t_len = cycle_lengths(sum(counts), FAN_T, 3)
    for i in empty:
        t_len[i] = 0
    return build("micro", FAN_S, FAN_T, (7, 2, 5)[:len(counts)], sorted_src(counts), t_len, seed=530)


# ---- keys: both key registers and the largest LDS image, restaged inside a run ------------------------------------------------
KEY_S = (64, 65, 128)
KEY_MODELS = SC.SOURCE_MODELS  # head sizes 16, 32, 64
KEY_SRC = (0, 1, 0)


def keys(model, S):
    return build(model, S, FAN_T, (S, 1), KEY_SRC, (5, 4, 3), seed=540 + S)


# ---- rows: past the 128-row GEMM tiles ------------------------------------------------------------------------------------------
ROWS_COUNTS, ROWS_T = (9, 8, 8), 41


def rows():
    t_len = [ROWS_T - (i % 4) for i in range(sum(ROWS_COUNTS))]
    return build("mini", SC.ROW_S, ROWS_T, (7, 2, 5), sorted_src(ROWS_COUNTS), t_len, seed=550)


# ---- chunks: two candidates per chunk ------------------------------------------------------------------------------------------
CHUNK_S, CHUNK_T, CHUNK_SRC = SC.CHUNK_S, 2731, (0, 0, 0, 1)


def chunks():
    return build("micro", CHUNK_S, CHUNK_T, (4, 3), CHUNK_SRC, (CHUNK_T, CHUNK_T - 5, CHUNK_T, CHUNK_T), seed=560,
                 n_sl=MS.SHORTLIST)


# ---- more candidates than the context has sentences ----------------------------------------------------------------------------
MANY_B, MANY_N = 2, 40


def many():
    return build("micro", FAN_S, FAN_T, (7, 3), sorted_src((13, 27)), [i % (FAN_T + 1) for i in range(MANY_N)], seed=570)


# ---- what the fixtures test measures ---------------------------------------------------------------------------------------------
def chunk_split(c):
    """[(first candidate, candidates)] of the call's chunks"""
    N, T = c.t_ids.shape
    per = max(1, CHUNK_ROWS // T)
    return [(b0, min(per, N - b0)) for b0 in range(0, N, per)]


def stagings(c):
    """per chunk and run: the sources staged in order, as the kernel's rule gives them"""
    out = []
    for b0, nb in chunk_split(c):
        for r0 in range(b0, b0 + nb, G):
            staged, seq = None, []
            for i in range(r0, min(r0 + G, b0 + nb)):
                if c.t_len[i] == 0:
                    continue
                if int(c.cand_src[i]) != staged:
                    staged = int(c.cand_src[i])
                    seq.append(staged)
            out.append(seq)
    return out


# ---- rank ---------------------------------------------------------------------------------------------------------------------------
def rank_reference(scores, t_len, cand_src, B, mean):
    """(totals float32 [N], best uint32 [B]): the float32 loop of the definition"""
    scores = np.asarray(scores, np.float32)
    N, T = scores.shape
    totals = np.zeros(N, np.float32)
    best = np.full(B, NONE, np.uint32)
    top = [None] * B
    with np.errstate(all="ignore"):
        for c in range(N):
            n = min(int(t_len[c]), T)
            s = np.float32(0.0)
            for t in range(n):
                s = np.float32(s + scores[c, t])
            totals[c] = s
            if n == 0:
                continue
            key = np.float32(s / np.float32(n)) if mean else s
            if np.isnan(key):
                continue
            b = int(cand_src[c])
            if top[b] is None or key > top[b]:  # (a tie keeps the lower c; +0 == -0)
                top[b], best[b] = key, c
    return totals, best


RANK_SIZES = ((1, 1), (64, 7), (65, 130), (1000, 130))  # (N, B)
RANK_T = 6


def rank_inputs(N, B, seed):
    """crafted scores: small integers over eight (exact sums: exact ties), with -inf, NaN, +0 / -0 rows, empty candidates;
    shuffled sources that leave some source without a candidate"""
    rng = np.random.default_rng(seed)
    sc = (rng.integers(-24, 1, size=(N, RANK_T)) / 8.0).astype(np.float32)
    t_len = rng.integers(0, RANK_T + 1, size=N).astype(np.uint32)
    src = rng.integers(0, max(1, B - B // 4), size=N).astype(np.uint32)  # the last quarter of the sources: no candidate
    kind = rng.integers(0, 10, size=N)
    for c in range(N):
        if kind[c] == 0:
            sc[c, rng.integers(0, RANK_T)] = -np.inf
        elif kind[c] == 1:
            sc[c, rng.integers(0, RANK_T)] = np.nan
        elif kind[c] == 2:
            sc[c] = 0.0 if c % 2 else -0.0
        elif kind[c] == 3 and c:
            sc[c], t_len[c], src[c] = sc[c - 1], t_len[c - 1], src[c - 1]  # an exact tie with the neighbour
    if N == 1:
        t_len[0] = RANK_T
    return sc, t_len, src
