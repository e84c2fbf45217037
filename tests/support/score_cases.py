"""The cases tests/test_gpu_score_shapes.py, tests/test_gpu_score_edges.py and tests/test_gpu_option_shapes.py compare with the
oracle, and tests/test_score_case_fixtures.py checks for being worth comparing (CPU). One table, like model_shapes.py, so that
the GPU tests and the CPU proof of their coverage cannot drift.

What the table is built around (slimt_amd/csrc/score_tall.hip, engine.cpp score_device, device_common.h forced_column):
  * the scorer's kernels are instantiated per emb size / 64 (scan, output layer) and per head size (attention): the shapes of
    model_shapes.SHAPES reach every pair that exists;
  * the tall path changes tiling with the number of target rows B * T: 128-row GEMM tiles from 1024 rows, other row blocks at
    512 / 2048 / 4096, one output-layer workgroup per 128 rows, a dead-tile mask per 16 rows, chunks of whole sentences of
    at most max(T, 8192) rows;
  * the attention kernel keeps a second key per lane for sources above 64 tokens;
  * the column of a target is found by a 64-ary search over the shortlist, one round per factor 64 of its size.
Nothing here calls the library: shapes, row counts and chunk splits are written by hand and checked by arithmetic."""
from collections import namedtuple

import numpy as np

from support import model_shapes as MS
from support.model_values import score_bound

FILL = np.float32(-7.25)  # what the output buffers hold before a call: entries the call does not write keep it

# ---- models of the edge cases: the smallest that reach each edge --------------------------------------------------------
# name: (preset, dims or None); eos_bias 3.0, seed 1234 throughout (scoring never stops at EOS, any values serve)
MODELS = {
    "micro": ("micro", None),                          # (64, 128, 4, 2, 2, 512): head size 16
    "head64": ("micro", (64, 128, 1, 1, 1, 512)),      # head size 64
    "mini": ("mini", None),                            # (128, 256, 8, 2, 2, 2048): head size 16, two 64-column slices
    "tiny11": ("tiny11", None),                        # head size 32; the flagship shape, only where the issue names it
    "v517": ("micro", (64, 128, 4, 1, 1, 517)),        # a full vocabulary that is no multiple of 16
    "v8192": ("micro", (64, 128, 4, 1, 1, 8192)),      # room for shortlists of 64^2 + 1 ids
}


def make_model(name):
    from slimt_amd import synth
    preset, dims = MODELS[name]
    return synth.make_model(preset, seed=1234, eos_bias=3.0, dims=dims)


def dims_of(name):
    from slimt_amd import synth
    preset, dims = MODELS[name]
    return dims if dims is not None else synth.PRESETS[preset]


# ids / lens: the source batch; sl: the shortlist or None; t_ids / t_len: the targets; minus_inf: the (b, t) the case places a
# missing token at ON PURPOSE (an empty set: every target is drawn from the output layer's ids, every score is finite)
Inputs = namedtuple("Inputs", "ids lens sl t_ids t_len minus_inf")


def spread(B, hi, lo=0):
    return [lo + (b * (hi - lo)) // max(1, B - 1) for b in range(B)]


def source(V, B, S, seed, lens=None):
    """lens None: ragged lengths with lens[0] = 0 and lens[-1] = S; else the given ones over full rows of tokens"""
    from slimt_amd import synth
    ids, ln = synth.make_batch(V, B, S, seed=seed, ragged=lens is None and S > 1)
    if lens is not None:
        ln = np.asarray(lens, np.uint32)
    elif B >= 2:
        ln[0], ln[-1] = 0, S
    return ids, ln.astype(np.uint32)


def shortlist(V, n):
    """None: the full vocabulary; n: n sorted ids drawn from all of 1 .. V - 1 (NOT synth.make_shortlist, whose first 100 ids
    are 0 .. 99: below 100 ids a column would equal its token)"""
    if n is None:
        return None
    return np.sort(np.random.default_rng(1000 + n).choice(np.arange(1, V, dtype=np.uint32), size=n, replace=False))


def pool_of(sl, V):
    return sl[sl != 0] if sl is not None else np.arange(1, V, dtype=np.uint32)


def random_targets(rng, B, T, sl, V):
    return rng.choice(pool_of(sl, V), size=(B, T)).astype(np.uint32)


# ---- section 2: the scorer over the accepted family (every model_shapes.SHAPES entry) -----------------------------------------
# kind: (B, S, T, shortlist size). short: T odd and above tmax_of(13) = 19 (the forced-prefix path refuses it); long: S above 64
# on every head size, over the full vocabulary (V = 517, 1003 ...: widths that are no multiple of 16)
SHAPE_CASES = {"short": (5, 13, 27, MS.SHORTLIST), "long": (3, 70, 21, None)}


def shape_inputs(s, kind):
    """Target lengths spread over 0 .. T, both ends included, and turned by one place: sentence 0 (no source token at all:
    lens[0] = 0) gets all T rows and the sentence of S source tokens keeps rows too, instead of pairing lens 0 with length 0."""
    from slimt_amd import synth
    B, S, T, n_sl = SHAPE_CASES[kind]
    V = s.dims[5]
    ids, lens = source(V, B, S, seed=B * 100 + S + 7)
    sl = None if n_sl is None else synth.make_shortlist(V, n_sl)
    t_len = spread(B, T)
    t_len = np.asarray(t_len[-1:] + t_len[:-1], np.uint32)
    t_ids = random_targets(np.random.default_rng(s.seed + S), B, T, sl, V)
    return Inputs(ids, lens, sl, t_ids, t_len, set())


# ---- section 3: the edges ------------------------------------------------------------------------------------------------------
def _model_shortlist(name):
    """the output layer of an edge case that is not about the layer's width: the full vocabulary at 512 ids, else 200 ids"""
    return None if dims_of(name)[5] <= 517 else MS.SHORTLIST


def _plain(name, B, S, T, t_len, seed, lens=None):
    from slimt_amd import synth
    V = dims_of(name)[5]
    n_sl = _model_shortlist(name)
    sl = None if n_sl is None else synth.make_shortlist(V, n_sl)
    ids, ln = source(V, B, S, seed, lens)
    t_ids = random_targets(np.random.default_rng(seed), B, T, sl, V)
    return Inputs(ids, ln, sl, t_ids, np.asarray(t_len, np.uint32), set())


# source lengths: 1, 2, 3, 5 (fewer keys than d_head / 4 float4 rows, clamped j0), 63 / 64 / 65 (the second key register comes
# alive above 64), 127 / 128 (the last lane of it; 128 is the limit)
SOURCE_LENGTHS = (1, 2, 3, 5, 63, 64, 65, 127, 128)
SOURCE_MODELS = ("micro", "tiny11", "head64")  # head sizes 16, 32, 64
SOURCE_B, SOURCE_T = 6, 5


def source_length_lens(S):
    """{0, 1, S, S - 1}, and 64 and 65 where S is above 64 (else S - 2 and S again)"""
    return [0, 1, S, S - 1] + ([64, 65] if S > 64 else [max(0, S - 2), S])


def source_length_inputs(name, S):
    return _plain(name, SOURCE_B, S, SOURCE_T, [5, 4, 5, 5, 1, 5], seed=300 + S, lens=source_length_lens(S))


# row counts: (B, T) with B * T on and next to every switch of the tall path. A product of two odd numbers where the count is
# odd, so that sentences straddle the 16-row tiles and 128-row blocks; powers of two have no such factors, there the case has
# several sentences per block or several blocks per sentence
ROW_COUNTS = (127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
ROW_CASES = [(1, 127), (4, 32), (3, 43), (7, 73), (16, 32), (3, 171), (3, 341), (32, 32), (5, 205), (23, 89), (8, 256), (3, 683),
             (5, 819), (16, 256), (17, 241)]
ROW_MODELS = ("micro", "mini")
TINY_ROW_CASES = [(32, 32), (1, 1025)]  # the flagship shape on both sides of the 128-row GEMM tiles, nothing more
ROW_S = 7


def row_inputs(name, B, T):
    """every sentence of full length (the last row of the call is live) but the first, which stops three rows early"""
    t_len = [T] * B
    if B > 1:
        t_len[0] = T - 3
    return _plain(name, B, ROW_S, T, t_len, seed=B * 7 + T)


# dead tiles and blocks in one call: sentence 1 (rows 300 .. 599) leaves the 128-row block of rows 384 .. 511 dead altogether;
# sentence 2 lives in rows 600 .. 604 only, so block 4 (rows 512 .. 639) has one live 16-row tile among seven dead ones; sentence
# 4 ends at row 1329 = 83 * 16 + 1 and sentence 5 at row 1516 = 94 * 16 + 12: the last live row of a tile in mid-tile
DEAD_B, DEAD_T, DEAD_LEN = 6, 300, [300, 0, 5, 300, 130, 17]
DEAD_MODELS = ("micro", "mini")


def dead_inputs(name):
    return _plain(name, DEAD_B, ROW_S, DEAD_T, DEAD_LEN, seed=611)


# chunks: (B, T, sentences per chunk written by hand). Chunks hold max(1, 8192 // T) whole sentences
CHUNK_ROWS = 8192
CHUNK_CASES = [(2, 8191, [1, 1]), (2, 8192, [1, 1]), (2, 8193, [1, 1]), (3, 4096, [2, 1]), (4, 2731, [2, 2]), (4, 2730, [3, 1])]
CHUNK_S = 4


def chunk_inputs(B, T):
    """micro over a 200-id shortlist: sentence 1 stops five rows early, the others are full"""
    from slimt_amd import synth
    V = dims_of("micro")[5]
    sl = synth.make_shortlist(V, MS.SHORTLIST)
    ids, ln = source(V, B, CHUNK_S, seed=B + T)
    t_len = [T] * B
    t_len[1] = T - 5
    t_ids = random_targets(np.random.default_rng(B + T), B, T, sl, V)
    return Inputs(ids, ln, sl, t_ids, np.asarray(t_len, np.uint32), set())


# output-layer width: (model, shortlist size or None). Below 64 columns some of the four waves have no column tile at all and
# merge their start values; 72 and 517 leave the last tile partly filled. Every size is accepted: the library has no rule on a
# shortlist's size
WIDTH_CASES = [("micro", 8), ("micro", 16), ("micro", 24), ("micro", 48), ("micro", 56), ("micro", 64), ("micro", 72),
               ("micro", None), ("v517", None)]
WIDTH_B = 2


def width_inputs(name, n):
    """T = the layer's width; both sentences hold every id of the layer once, in two orders"""
    V = dims_of(name)[5]
    sl = shortlist(V, n)
    N = V if sl is None else len(sl)
    ids, ln = source(V, WIDTH_B, ROW_S, seed=40 + N)
    rng = np.random.default_rng(N)
    cols = np.arange(V, dtype=np.uint32) if sl is None else sl
    t_ids = np.stack([rng.permutation(cols), rng.permutation(cols)]).astype(np.uint32)
    return Inputs(ids, ln, sl, t_ids, np.full(WIDTH_B, N, np.uint32), set())


# column search: hand-built sorted shortlists of the v8192 model. 64 is the last size searched in one round, 65 the first in
# two, 4096 = 64^2 the last in two, 4097 the first in three. Every size is accepted as it stands
SEARCH_SIZES = (64, 65, 128, 4095, 4096, 4097)
SEARCH_V = 8192
SEARCH_EDGE = 10  # ids 0 .. 9 and the top ten are in no list: there is an id below sl[0] and one above sl[N - 1]
SEARCH_GAPS = 128


def search_shortlist(N):
    """N sorted ids; the short lists hold even ids only, so that every entry of theirs is followed by a gap (64 entries: 64 gaps)"""
    ids = np.arange(SEARCH_EDGE, SEARCH_V - SEARCH_EDGE, 2 if N <= 128 else 1, dtype=np.uint32)
    return np.sort(np.random.default_rng(N).choice(ids, size=N, replace=False))


def search_tokens(sl):
    """(tokens, present): every entry of the list once, the id below sl[0], and for up to SEARCH_GAPS gaps spread over the list
    the id just past a present one -- the last of them is the id above sl[N - 1]; shuffled"""
    nxt = sl + 1
    gaps = nxt[~np.isin(nxt, sl)]
    gaps = gaps[np.linspace(0, len(gaps) - 1, min(SEARCH_GAPS, len(gaps))).astype(np.int64)]
    toks = np.concatenate([sl, [sl[0] - 1], gaps]).astype(np.uint32)
    toks = np.random.default_rng(len(sl)).permutation(toks)
    return toks, np.isin(toks, sl)


def search_inputs(N):
    """the tokens as two target rows (the second padded with sl[0] behind its length)"""
    sl = search_shortlist(N)
    toks, present = search_tokens(sl)
    T = (len(toks) + 1) // 2
    t_ids = np.full(2 * T, sl[0], np.uint32)
    t_ids[:len(toks)] = toks
    ids, ln = source(SEARCH_V, 2, ROW_S, seed=N)
    minus_inf = {(int(i) // T, int(i) % T) for i in np.flatnonzero(~present)}
    return Inputs(ids, ln, sl, t_ids.reshape(2, T), np.asarray([T, len(toks) - T], np.uint32), minus_inf)


SEARCH_PREFIX_S = 64  # forced prefixes of tmax_of(64) = 96 tokens


def search_prefix_inputs(N, Tmax):
    """the same tokens as full-length forced prefixes of B sentences (the rest of the last one: entries of the list again).
    The lists hold no EOS (id 0), so no sentence ends before Tmax. Returns (ids, lens, sl, p_ids, p_len, present [B, Tmax])"""
    sl = search_shortlist(N)
    toks, present = search_tokens(sl)
    B = -(-len(toks) // Tmax)
    p = np.resize(sl, B * Tmax).astype(np.uint32)
    p[:len(toks)] = toks
    ok = np.ones(B * Tmax, bool)
    ok[:len(toks)] = present
    ids, ln = source(SEARCH_V, B, SEARCH_PREFIX_S, seed=N + 1)
    return ids, ln, sl, p.reshape(B, Tmax), np.full(B, Tmax, np.uint32), ok.reshape(B, Tmax)


# missing tokens (mini over a 200-id shortlist), T = 130: at t = 0, on the row that ends the first 128-row block (sentence 0's
# row 127), on the last row of a sentence (sentence 1), on every row of a sentence (sentence 2)
MISSING_B, MISSING_T, MISSING_LEN = 4, 130, [130, 50, 20, 130]
MISSING_AT = sorted({(0, 0), (0, 127), (1, 49)} | {(2, t) for t in range(20)})


def missing_inputs():
    c = _plain("mini", MISSING_B, ROW_S, MISSING_T, MISSING_LEN, seed=77)
    absent = np.setdiff1d(np.arange(1, dims_of("mini")[5], dtype=np.uint32), c.sl)
    t_ids = c.t_ids.copy()
    rng = np.random.default_rng(78)
    for b, t in MISSING_AT:
        t_ids[b, t] = rng.choice(absent)
    return c._replace(t_ids=t_ids, minus_inf=set(MISSING_AT))


# every edge case above as (kind, model, argument): what the CPU fixture test walks, and the GPU module by kind
EDGE_CASES = ([("source", n, S) for n in SOURCE_MODELS for S in SOURCE_LENGTHS]
              + [("rows", n, bt) for n in ROW_MODELS for bt in ROW_CASES] + [("rows", "tiny11", bt) for bt in TINY_ROW_CASES]
              + [("dead", n, None) for n in DEAD_MODELS] + [("chunk", "micro", c[:2]) for c in CHUNK_CASES]
              + [("width", n, w) for n, w in WIDTH_CASES] + [("search", "v8192", N) for N in SEARCH_SIZES]
              + [("missing", "mini", None)])


def edge_id(case):
    kind, name, arg = case
    if isinstance(arg, tuple):
        arg = "B%d-T%d" % arg
    return "-".join(str(x) for x in (kind, name, arg) if x is not None or kind == "width").replace("None", "full")


def edges_of(kind):
    return [c for c in EDGE_CASES if c[0] == kind]


def edge_inputs(case):
    kind, name, arg = case
    if kind == "source":
        return source_length_inputs(name, arg)
    if kind == "rows":
        return row_inputs(name, *arg)
    if kind == "dead":
        return dead_inputs(name)
    if kind == "chunk":
        return chunk_inputs(*arg)
    if kind == "width":
        return width_inputs(name, arg)
    if kind == "search":
        return search_inputs(arg)
    assert kind == "missing", kind
    return missing_inputs()


# ---- section 4: the translate options over the family ------------------------------------------------------------------------
# (B, S) of every shape: a partly filled tile under a 200-id shortlist, and more than one tile over the full vocabulary
# (model_shapes.translate_shortlist). Both are vouched cases of every shape: their greedy batches are not degenerate
OPTION_CASES = [(5, 13), (21, 32)]
OPTION_TEMPERATURE = 0.7


def option_inputs(s, B, S):
    """(ids, lens, shortlist): the batch model_shapes.translate_reference translates"""
    from slimt_amd import synth
    ids, lens = MS.batch(s, B, S, salt=2)
    n_sl = MS.translate_shortlist(S)
    return ids, lens, None if n_sl is None else synth.make_shortlist(s.dims[5], n_sl)


def option_prefix(s, B, S, sl, Tmax):
    """random targets of full length Tmax (no EOS), forced over prefixes of 0 .. Tmax tokens"""
    t = random_targets(np.random.default_rng(s.seed + B + S), B, Tmax, sl, s.dims[5])
    return t, np.asarray(spread(B, Tmax), np.uint32)


def option_modes(s, S):
    """decode modes 0 (automatic) and 1 (per-stage kernels), and 2 (persistent decoder, 16 sentences per workgroup) where the
    shape has one"""
    return (0, 1) + ((2,) if MS.expected_plan(s, S)[1] else ())


# ---- the comparison every GPU test of the three modules makes -----------------------------------------------------------------
def bounds(peaks, b, n):
    return np.array([score_bound(peaks[t, b]) for t in range(n)])


def check_scores(got, want, ln, peaks, fill=None):
    """scores [B, T] against the checker's float64 ones: -inf exactly where the checker has it, finite elsewhere and within
    model_values.score_bound of the row's largest |logit| (peaks [steps][B]); with `fill`, entries behind ln[b] keep it"""
    worst, widest = 0.0, 0.0
    for b in range(len(ln)):
        n = int(ln[b])
        g, w = got[b, :n].astype(np.float64), want[b, :n]
        assert np.array_equal(np.isneginf(g), np.isneginf(w)), (b, np.flatnonzero(np.isneginf(g) != np.isneginf(w)))
        fin = np.isfinite(w)
        assert np.all(np.isfinite(g[fin])), (b, g)
        bound = bounds(peaks, b, n)
        ratio = np.zeros(n)
        ratio[fin] = np.abs(g[fin] - w[fin]) / bound[fin]
        if fin.any():
            t = int(np.argmax(ratio))
            worst = max(worst, float(ratio[t]))
            widest = max(widest, float(bound[fin].max()))
            assert ratio[t] <= 1.0, (b, t, got[b, t], want[b, t], bound[t])
        if fill is not None:
            assert np.all(got[b, n:] == fill), b
    print("scores: at most %.3f of the bound; largest |logit| %.1f%s"
          % (worst, peaks.max(initial=0), "" if widest <= 5e-5 else "; bound 8 ulp(L) = %.3g" % widest))


def check_align(al, want, lens, ln, fill=None):
    """alignment rows [B, T, S] bit for bit; with `fill`, rows behind ln[b] and columns from lens[b] on keep it"""
    for b in range(len(ln)):
        n, L = int(ln[b]), int(lens[b])
        assert np.array_equal(al[b, :n, :L].view(np.uint32), want[b, :n, :L].view(np.uint32)), b
        if fill is not None:
            assert np.all(al[b, n:] == fill) and np.all(al[b, :, L:] == fill), b


def reference(oracle, m, om, c):
    """(scores float64, alignment rows, row peaks) of case c from the teacher-forced checker in PORTABLE mode"""
    from support.model_values import Recording
    from test_score_checker import teacher_forced
    rec = Recording(om)
    sc, al = teacher_forced(oracle, rec, m, c.ids, c.lens, c.sl, c.t_ids, c.t_len)
    peaks = rec.row_peaks() if rec.logits else np.zeros((0, len(c.t_len)))
    return sc, al, peaks


def check_case(got, ref, c, align=True):
    sc, al = got
    w_sc, w_al, peaks = ref
    check_scores(sc, w_sc, c.t_len, peaks, FILL)
    if align:
        check_align(al, w_al, c.lens, c.t_len, FILL)
    else:
        assert al is None
