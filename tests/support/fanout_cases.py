"""The cases tests/test_gpu_fanout.py compares with the checkers and with slimt_hip_translate on the duplicated sources, and
tests/test_fanout_case_fixtures.py proves able to catch the bugs they are for (CPU, on the oracle). One table, like
candidate_cases.py.

A fan-out call (include/slimt_hip.h, slimt_hip_translate_fanout) decodes N rows over B sources encoded once; row r
translates source row_src[r]. Its checker is an existing checker on the duplicated batch ids[row_src], lens[row_src]:
sampled_translate (test_sampling_checker.py), forced_translate (test_forced_prefix_checker.py), truncated_translate
(test_truncation_checker.py) and the oracle's greedy translate. What the table is built around
(slimt_amd/csrc/decode_fanout.hip):
  * an attention workgroup owns 16 consecutive rows and walks them as runs of consecutive rows that name one source, staging
    that source's K / V once per run: N = 1, 16, 17, 33, a run of 20, one staging per row, sources without rows;
  * a second key per lane for sources above 64 tokens; LDS of 8 S d_head bytes beside the Q operands (d_head 16, 32, 64).
What a sampled case must show, or a bug hides (asserted by the fixture test on the CPU):
  (a) every source with two or more rows has two rows whose token sequences differ -- else a wrong key or row index hides;
  (b) under greedy no two sources of the batch have the same translation -- else a wrong row_src lookup hides;
  (c) at S = 32 the rows end at three or more different lengths -- else a wrong per-row out_len / finished hides."""
from collections import namedtuple

import numpy as np

TEMPERATURES = (0.7, 1.0)
TOP_K, TOP_P = 4, 0.9  # the truncated parity runs

# preset + dims (None: the preset's own) + eos_bias + model_seed: the synthetic model; S, B: the sources; row_src [N];
# n_sl: shortlist size (None: the full vocabulary); seed: of the batch; key_seed: keys = keys_of(key_seed, N)
Case = namedtuple("Case", "name preset dims eos_bias model_seed S B row_src n_sl seed key_seed")


def sorted_src(counts):
    return np.repeat(np.arange(len(counts), dtype=np.uint32), counts)


def case(name, preset, eos_bias, S, B, row_src, n_sl, dims=None, model_seed=1234, seed=None, key_seed=None):
    row_src = np.asarray(row_src, dtype=np.uint32)
    assert row_src.ndim == 1 and row_src.size >= 1 and int(row_src.max()) < B
    return Case(name, preset, dims, eos_bias, model_seed, S, B, row_src, n_sl, 61 + S + B if seed is None else seed,
                S + B if key_seed is None else key_seed)


def model_of(c, synth_models=None):
    from slimt_amd import synth
    if c.dims is not None:
        return synth.make_model(c.preset, seed=c.model_seed, eos_bias=c.eos_bias, dims=c.dims)
    if synth_models is not None:
        return synth_models(c.preset, c.eos_bias, c.model_seed)
    return synth.make_model(c.preset, seed=c.model_seed, eos_bias=c.eos_bias)


def inputs(c, V):
    """(ids [B, S], lens [B], shortlist | None, keys uint64 [N])"""
    from slimt_amd import synth
    from test_sampling_checker import keys_of
    ids, lens = synth.make_batch(V, c.B, c.S, seed=c.seed, ragged=True)
    sl = None if c.n_sl is None else synth.make_shortlist(V, c.n_sl)
    return ids, lens, sl, keys_of(c.key_seed, c.row_src.size)


def duplicated(ids, lens, row_src):
    """the same work done the parent's way: every row with its own copy of its source"""
    return np.ascontiguousarray(ids[row_src]), np.ascontiguousarray(lens[row_src])


def prefixes(c, V, sl, Tm, seed=7):
    """forced prefixes of the N rows: lengths walking 0 .. min(3, Tm), ids from the output layer's columns"""
    N = c.row_src.size
    r = np.random.default_rng(seed + c.seed)
    p_len = (np.arange(N) % (min(3, Tm) + 1)).astype(np.uint32)
    pool = np.arange(1, V, dtype=np.uint32) if sl is None else sl[sl != 0]
    p_ids = np.zeros((N, Tm), np.uint32)
    for n in range(N):
        p_ids[n, : p_len[n]] = r.choice(pool, size=int(p_len[n]))
    return p_ids, p_len


# ---- parity: checked against the checkers AND the duplicated call, every kind of call ------------------------------------
# The first three are the issue's (n rows per source, sorted); the others' seeds were chosen so that (a)-(c) hold.
DH16 = (64, 128, 4, 1, 1, 517)  # a model_shapes member with d_head 16 (per-stage kernels only)
PARITY = [
    case("s8", "tiny11", 6.0, 8, 5, sorted_src([4] * 5), 4096),
    case("s32", "tiny11", 6.0, 32, 5, sorted_src([7] * 5), 4096),
    case("full", "tiny11", 7.0, 8, 3, sorted_src([6] * 3), None),
    case("s64", "tiny11", 8.0, 64, 3, sorted_src([2, 3, 2]), 4096),
    case("s100", "tiny11", 6.0, 100, 2, [0, 1, 1], 4096),
    # (base: below an EOS bias of 14 the greedy translations of this batch's sources coincide -- one loop of tokens -- and (b) fails)
    case("base32", "base", 14.0, 32, 3, sorted_src([3, 1, 4]), 4096),
    case("dh16", "tiny11", 2.0, 13, 4, sorted_src([3, 2, 0, 3]), None, dims=DH16, model_seed=1238),
]
EXEMPT_FROM_C = {"s8", "full"}  # (the issue's two S = 8 cases: two or three distinct lengths)


def parity(name):
    return next(c for c in PARITY if c.name == name)


# ---- tiling edges: compared with the duplicated call (and plain translate) on the device ---------------------------------
EDGE_S, EDGE_B = 8, 5


def edges():
    """name -> row_src over EDGE_B sources"""
    B = EDGE_B
    r = np.random.default_rng(5)
    every = np.arange(B, dtype=np.uint32)
    out = {
        "n1": [3],
        "n16": sorted_src([4, 3, 3, 3, 3]),                    # one full workgroup
        "n17": sorted_src([4, 3, 3, 3, 4]),                    # a run crosses the 16-row boundary; 15 dead waves behind it
        "n33": sorted_src([7, 7, 6, 7, 6]),                    # three workgroups, the last with one row
        "run20": sorted_src([2, 20, 1, 1, 1]),                 # one source owns 20 consecutive rows (rows 2 .. 21)
        "arange": every,                                       # one staging per row: plain translate
        "shuffled": r.permutation(sorted_src([7, 7, 6, 7, 6])),
        "none_first": sorted_src([0, 5, 4, 4, 4]),
        "none_middle": sorted_src([5, 4, 0, 4, 4]),
        "none_last": sorted_src([5, 4, 4, 4, 0]),
        "reversed": sorted_src([3, 4, 3, 4, 3])[::-1].copy(),
    }
    return {k: np.asarray(v, dtype=np.uint32) for k, v in out.items()}


def edge_case(name):
    return case("edge_" + name, "tiny11", 6.0, EDGE_S, EDGE_B, edges()[name], 4096)


def one_token():
    """S = 1: one step, and every source is the lone EOS -- no condition can hold; compared on the device all the same"""
    return case("s1", "tiny11", 6.0, 1, 5, sorted_src([4] * 5), 4096)


def single_source():
    return case("b1", "tiny11", 6.0, 8, 1, np.zeros(17, np.uint32), 4096)


def runs_of(row_src):
    """(first row, rows, source) of every staging the kernel does: runs of equal sources inside each 16-row workgroup"""
    out = []
    for m0 in range(0, len(row_src), 16):
        tile = row_src[m0:m0 + 16]
        r0 = 0
        while r0 < len(tile):
            r1 = r0 + 1
            while r1 < len(tile) and tile[r1] == tile[r0]:
                r1 += 1
            out.append((m0 + r0, r1 - r0, int(tile[r0])))
            r0 = r1
    return out
