"""GPU checks of the consensus selection over unit rows (include/slimt_hip.h, slimt_hip_consensus_select_units*,
slimt_hip_ctx_set_fanout_consensus_units): the rows' ids are expanded through the unit table with a few lines of NumPy and
tests/support/consensus_ref.py, which is general in what a token is and in the order, gives the reference. Integer counts
and doubles in a fixed order: utilities are compared as uint64 bits and best exactly -- no tolerance anywhere."""
import numpy as np
import pytest
import torch

from support import consensus_ref as R
from support import fanout_cases as FC

pytestmark = pytest.mark.gpu

X, A, B_, C_ = 0, 7, 0x110041, 0xFFFFFFF0  # the unit alphabet (0 is a unit like any other: the rows' zero padding must not match it)
V = 50
PIECE_LENGTHS = (0, 1, 2, 7)


def make_table(size=V, seed=3):
    """ids 0..5 by hand -- 0: nothing (EOS), 1: [X], 2: [X, X], 3: [A, B, C], 4: [A], 5: [B, C] -- then random pieces of 0, 1,
    2 and 7 units over the alphabet; ids from V up to `size` (a model's vocabulary) expand to nothing"""
    rnd = np.random.default_rng(seed)
    pieces = [[], [X], [X, X], [A, B_, C_], [A], [B_, C_]]
    pieces += [list(rnd.choice([X, A, B_, C_], PIECE_LENGTHS[v % 4])) for v in range(6, V)]
    off = np.zeros(size + 1, np.uint32)
    off[1:V + 1] = np.cumsum([len(p) for p in pieces])
    off[V + 1:] = off[V]
    return off, np.asarray([u for p in pieces for u in p], np.uint32)


OFF, UNITS = make_table()


def expand(ids, lens):
    """the unit rows as a padded matrix and their lengths (an id >= V expands to nothing)"""
    rows = [[int(u) for v in ids[c, :min(int(lens[c]), ids.shape[1])] if v < V for u in UNITS[OFF[v]:OFF[v + 1]]]
            for c in range(len(lens))]
    mat = np.zeros((len(rows), max(1, max(map(len, rows), default=1))), np.uint32)
    for c, r in enumerate(rows):
        mat[c, :len(r)] = r
    return mat, np.asarray([len(r) for r in rows], np.uint32)


def reference(ids, lens, src, B, G, beta2):
    return R.select(*expand(ids, lens), src, B, G, beta2)


def row_of(rnd, u):
    """random ids (6..V-1) that expand to exactly u units, pieces of nothing sprinkled in"""
    want = [7] * (u // 7) + [2] * (u % 7 // 2) + [1] * (u % 7 % 2) + [0] * int(rnd.integers(1, 3))
    rnd.shuffle(want)
    return [int(rnd.choice([v for v in range(6, V) if PIECE_LENGTHS[v % 4] == n])) for n in want]


def pack(sources, seed=0):
    """sources: lists of id rows -> (ids [N, T], lens, row_src, B): the sources' rows interleaved, one more source without rows"""
    rows = [(b, r) for b, rs in enumerate(sources) for r in rs]
    order = np.random.default_rng(seed).permutation(len(rows))
    ids = np.zeros((len(rows), max(1, max(len(r) for _, r in rows))), np.uint32)
    for c, k in enumerate(order):
        ids[c, :len(rows[k][1])] = rows[k][1]
    return (ids, np.asarray([len(rows[k][1]) for k in order], np.uint32), np.asarray([rows[k][0] for k in order], np.uint32),
            len(sources) + 1)


def small_cases():
    rnd = np.random.default_rng(11)
    by_units = lambda *lengths: [row_of(rnd, u) for u in lengths]
    return pack([by_units(5),                       # one row: no reference, utility 0
                 by_units(3, 4),
                 by_units(0, 1, 2),                 # three rows (odd pair dealing); a row of tokens that spell nothing
                 by_units(1, 2, 3, 4, 5, 6, 7),     # orders without a gram on one side or both
                 by_units(63, 64, 65),              # the lane chunk
                 by_units(255, 256, 257, 261, 262), # the partner tile and its look-ahead
                 by_units(1023, 1024, 1024),
                 [[1] * 20, [1] * 6, [2] * 5, [4] * 3],  # one unit repeated against shorter runs of it: clipping
                 by_units(*rnd.integers(0, 31, 17)),     # more pairs than one chunk of waves, more rows than waves
                 by_units(*rnd.integers(0, 41, 64))])


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(R.bits(got[0]), R.bits(want[0])), (what, got[0], want[0])


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).cuda()


def _select_device(ctx, ids, lens, src, B, G, beta2):
    N, T = ids.shape
    d_ids, d_len, d_src = _dev(ids), _dev(lens), _dev(src)
    d_util = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
    d_best = torch.full((B,), 12345, dtype=torch.int32, device="cuda")
    ctx.consensus_select_units_device(d_ids.data_ptr(), d_len.data_ptr(), d_src.data_ptr(), N, T, B, G, beta2,
                                      d_util.data_ptr(), d_best.data_ptr())
    ctx.synchronize()
    return d_util.cpu().numpy(), d_best.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def micro(hip, synth_models):
    m = synth_models("micro", 3.0)
    gm = hip.Model(m)
    gm.set_consensus_units(*make_table(m.V))
    ctx = hip.Context(gm, 4, 8)
    yield gm, ctx, m.V
    ctx.close()
    gm.close()


@pytest.mark.parametrize("beta2", [1, 4, 16])
@pytest.mark.parametrize("G", [1, 4, 6])
def test_host_and_device_calls_equal_the_reference(hip, micro, G, beta2):
    ids, lens, src, B = small_cases()
    want = reference(ids, lens, src, B, G, beta2)
    assert want[1][-1] == R.NO_ROW and (want[0] > 0).sum() > 90  # (the case is what it says: a source without rows, live pairs)
    _same(hip.consensus_select_units(ids, lens, src, B, OFF, UNITS, G, beta2), want, "host")
    _same(_select_device(micro[1], ids, lens, src, B, G, beta2), want, "device")


def test_two_segmentations_of_one_text_agree_fully_where_the_token_utility_sees_nothing_shared(hip):
    ids = np.zeros((3, 6), np.uint32)
    ids[0, :3], ids[1], ids[2, :2] = [3, 3, 3], [4, 5, 4, 5, 4, 5], [1, 2]  # ABCABCABC twice, and XXX
    lens, src = np.asarray([3, 6, 2], np.uint32), np.zeros(3, np.uint32)
    for G in range(1, 7):
        util, best = hip.consensus_select_units(ids[:2], lens[:2], src[:2], 1, OFF, UNITS, G, 4)
        assert list(util) == [1.0, 1.0] and best[0] == 0, G
    util, best = hip.consensus_select_units(ids, lens, src, 1, OFF, UNITS, 6, 4)
    assert list(util) == [0.5, 0.5, 0.0] and best[0] == 0
    util, _ = hip.consensus_select(ids[:2], lens[:2], src[:2], 1, 4, 4)
    assert list(util) == [0.0, 0.0]


def test_the_device_call_marks_what_it_cannot_select_and_the_host_call_refuses_it(hip, micro):
    gm, ctx, model_V = micro
    rnd = np.random.default_rng(5)
    fine = [row_of(rnd, u) for u in (9, 12, 10)]

    def check(bad_rows, what, message):
        ids, lens, src, B = pack([fine, bad_rows], seed=1)
        util, best = _select_device(ctx, ids, lens, src, B, 6, 4)
        mine = src == 0
        w_util, w_best = reference(ids[mine], lens[mine], src[mine], 1, 6, 4)  # (the other source alone)
        assert list(best) == [np.flatnonzero(mine)[int(w_best[0])], R.NO_ROW, R.NO_ROW], what
        assert np.array_equal(R.bits(util[mine]), R.bits(w_util)) and np.array_equal(R.bits(util[~mine]), R.bits(np.zeros((~mine).sum()))), what
        with pytest.raises(hip.SlimtHipError, match=message):
            hip.consensus_select_units(ids, lens, src, B, OFF, UNITS, 6, 4)

    check([row_of(rnd, 3) for _ in range(65)], "65 rows", "more than 64 rows")
    check([row_of(rnd, 1025), row_of(rnd, 7)], "1025 units", "expands to 1025 units")
    # an id >= V: nothing on the device, refused by the host call
    ids, lens, src, B = pack([fine])
    ids[0, 1], ids[2, 0] = model_V + 5, 0xFFFFFFFF
    _same(_select_device(ctx, ids, lens, src, B, 6, 4), reference(ids, lens, src, B, 6, 4), "id >= V")
    with pytest.raises(hip.SlimtHipError, match="is not below V"):
        hip.consensus_select_units(ids, lens, src, B, OFF, UNITS, 6, 4)
    # tables
    ids, lens, src, B = pack([fine])
    down = OFF.copy()
    down[9] = down[8] - 1
    with pytest.raises(hip.SlimtHipError, match="offsets decrease"):
        hip.consensus_select_units(ids, lens, src, B, down, UNITS, 6, 4)
    long = np.concatenate([OFF, [OFF[-1] + 256]]).astype(np.uint32)
    with pytest.raises(hip.SlimtHipError, match="expands to 256 units"):
        hip.consensus_select_units(ids, lens, src, B, long, np.zeros(int(long[-1]), np.uint32), 6, 4)
    with pytest.raises(hip.SlimtHipError, match="not the model's vocabulary"):
        gm.set_consensus_units(OFF, UNITS)
    # no table on the model: the device call and the arming are refused; the table can be set again
    gm.set_consensus_units(None)
    with pytest.raises(hip.SlimtHipError, match="no unit table"):
        _select_device(ctx, ids, lens, src, B, 6, 4)
    with pytest.raises(hip.SlimtHipError, match="no unit table"):
        ctx.set_fanout_consensus_units(6, 4, np.zeros(B, np.uint32), np.zeros(len(lens)))
    gm.set_consensus_units(*make_table(model_V))
    _same(_select_device(ctx, ids, lens, src, B, 6, 4), reference(ids, lens, src, B, 6, 4), "table set again")


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_armed_fanout_call_keeps_every_output_and_selects_over_the_unit_rows(hip, synth_models):
    c = FC.case("units", "tiny11", 6.0, 8, 3, FC.sorted_src([4] * 3), 4096)
    m = synth_models("tiny11", 6.0)
    gm = hip.Model(m)
    # (pieces of the whole vocabulary: the model's ids are anywhere in it)
    rnd = np.random.default_rng(9)
    n_units = rnd.choice(PIECE_LENGTHS, m.V)
    off = np.concatenate([[0], np.cumsum(n_units)]).astype(np.uint32)
    units = rnd.choice([X, A, B_, C_], int(off[-1])).astype(np.uint32)
    gm.set_consensus_units(off, units)
    ids, lens, sl, keys = FC.inputs(c, m.V)
    N = c.row_src.size
    kw = dict(scores=True, sampling=(1.0, keys), want_align=True, truncation=(FC.TOP_K, FC.TOP_P))
    ctx = hip.Context(gm, max(N, c.B), c.S)

    def check(got, best, util, what):
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), what
        assert np.array_equal(_bits32(got[2]), _bits32(want[2])), what
        live = np.arange(got[0].shape[1])[None, :] < got[1][:, None]
        assert np.array_equal(_bits32(got[3])[live], _bits32(want[3])[live]), what
        alone = hip.consensus_select_units(got[0], got[1], c.row_src, c.B, off, units, 6, 4)
        _same((util, best), alone, what)
        rows = [[int(u) for v in got[0][r, :got[1][r]] for u in units[off[v]:off[v + 1]]] for r in range(N)]
        mat = np.zeros((N, max(map(len, rows))), np.uint32)
        for r, x in enumerate(rows):
            mat[r, :len(x)] = x
        _same(alone, R.select(mat, [len(x) for x in rows], c.row_src, c.B, 6, 4), what)
        assert len({float(u) for u in util}) > 2, what

    try:
        want = ctx.translate_fanout(ids, lens, c.row_src, sl, **kw)
        got = ctx.translate_fanout(ids, lens, c.row_src, sl, consensus=("units", 6, 4), **kw)
        check(got, got[-2], got[-1], "translate_fanout")
        got = ctx.translate_fanout_pinned(ids, lens, c.row_src, sl, consensus=("units", 6, 4), **kw)
        check(got, got[-2], got[-1], "translate_fanout_async")
        # tokens armed, then units: the last arming wins
        t_best, t_util = np.full(c.B, 12345, np.uint32), np.full(N, -7.0)
        best, util = np.full(c.B, 12345, np.uint32), np.full(N, -7.0)
        ctx.set_fanout_consensus(4, 4, t_best, t_util)
        ctx.set_fanout_consensus_units(6, 4, best, util)
        check(ctx.translate_fanout(ids, lens, c.row_src, sl, **kw), best, util, "units armed last")
        assert (t_best == 12345).all() and (t_util == -7.0).all()
        # a plain translate finds it armed: refused, and consumed
        best[...], util[...] = 12345, -7.0
        ctx.set_fanout_consensus_units(6, 4, best, util)
        with pytest.raises(hip.SlimtHipError, match="not a fan-out call"):
            ctx.translate(ids, lens, sl)
        got = ctx.translate_fanout(ids, lens, c.row_src, sl, **kw)
        assert len(got) == len(want) and np.array_equal(got[0], want[0]) and (best == 12345).all() and (util == -7.0).all()
    finally:
        ctx.close()
        gm.close()


def test_frontend_chrf_pick_is_the_reference_pick_among_the_samples(hip):
    """text -> text: every segment's winner is the sample of translate(samples=n) that the reference picks among the samples'
    ids expanded through the vocabulary's table, which the model uploads on first use"""
    import io
    import random
    import sentencepiece
    from slimt_amd import frontend, synth
    rnd = random.Random(7)
    words = ["".join(rnd.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 8))) for _ in range(1500)]
    corpus = []
    for _ in range(3000):
        s = " ".join(rnd.choice(words) for _ in range(rnd.randint(3, 18)))
        corpus.append(s[0].upper() + s[1:] + rnd.choice(".?!"))
    out = io.BytesIO()
    sentencepiece.SentencePieceTrainer.train(sentence_iterator=iter(corpus), model_writer=out, vocab_size=512,
                                             model_type="unigram", pad_id=-1, unk_id=1, bos_id=-1, eos_id=0, minloglevel=2)
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    cfg = frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph")
    model = frontend.Model(cfg, frontend.Package(model=synth.write_bin(m), vocabulary=out.getvalue()), device=0)
    svc = frontend.Service(workers=1, max_words=256, wrap_length=24)
    try:
        sources, n, sampling = corpus[:3], 5, (1.0, 11)
        alts = svc.translate(model, sources, sampling=sampling, samples=n)
        won = svc.sample_and_select(model, sources, n, sampling, utility="chrf")
        off, units = model.consensus_units()
        assert np.array_equal(off, model.vocabulary.consensus_units(m.V)[0])
        processed = model.processor.process_many(sources, svc.wrap_length, svc.workers)
        drawn = svc._translate_samples(model, [segs for _, segs in processed], n, sampling)  # [sample][text][segment]
        segments = 0
        for t, (r, w) in enumerate(zip(alts, won)):
            assert len(w.utility) == len(w.sample_index) == len(processed[t][1]) >= 1
            for i in range(len(processed[t][1])):
                rows = [[int(u) for v in drawn[j][t][i][0] for u in units[off[v]:off[v + 1]]] for j in range(n)]
                mat = np.zeros((n, max(1, max(map(len, rows)))), np.uint32)
                for j, x in enumerate(rows):
                    mat[j, :len(x)] = x
                w_util, w_best = R.select(mat, [len(x) for x in rows], np.zeros(n, np.uint32), 1, 6, 4)
                j = int(w_best[0])
                assert w.sample_index[i] == j and R.bits([w.utility[i]])[0] == R.bits(w_util[j:j + 1])[0], (t, i)
                assert np.array_equal(_bits32(w.token_scores[i]), _bits32(r.samples[j].token_scores[i])), (t, i)
                segments += 1
            if len(processed[t][1]) == 1:
                assert w.target.text == r.samples[w.sample_index[0]].target.text
        assert segments >= 3
        with pytest.raises(ValueError):
            svc.sample_and_select(model, sources, n, sampling, utility="bleu")
    finally:
        svc.close()
        model.close()
