"""The table of tests/support/shortlist_cases.py reaches the edges it claims (CPU; nothing here runs on a device): for every
case the oracle's list equals the independent set construction of tests/test_shortlist.py, and the window a patch id falls in,
need, the list lengths, the bitmap sizes, the token counts and the full lists are what the GPU test relies on -- computed from
the reference's bitmap before and after the patch. A later edit of the table cannot quietly lose an edge.

The model-bound cases keep the precedent of test_model_shape_fixtures.py: the greedy translation the device is compared with
is not degenerate (eos_bias and seed of every model were chosen here, on the oracle)."""
import numpy as np
import pytest

from support import shortlist_cases as T
from test_model_shape_fixtures import fixture_problems
from test_shortlist import numpy_generate


def check_reference(oracle, c):
    """the oracle's list of case c, checked against numpy_generate; returns (list, dissection)"""
    got = T.reference(oracle, c)
    want = numpy_generate(c.blob, c.Vt, c.ids if c.twin is None else c.twin, c.lens, c.shared)
    assert np.array_equal(got, want), c.name
    frequent = T.parse(c.blob)[0]
    assert got.size > 0, "an empty output layer is outside the contract"
    assert np.all(np.diff(got.astype(np.int64)) > 0) and got[-1] < c.Vt
    assert np.array_equal(got[: min(frequent, c.Vt)], np.arange(min(frequent, c.Vt)))
    d = T.dissect(c, got)
    assert d.patch.size <= d.need and (d.patch.size == d.need or got.size == c.Vt)  # the patch stops short only when ids run out
    assert np.all(d.patch >= frequent)
    return got, d


@pytest.mark.parametrize("name", T.case_names())
def test_every_case_has_its_reference(oracle, name):
    c = T.case(name)
    assert c.ids.max() < c.Vs and (c.twin is None or (c.shared and c.ids.max() >= c.Vt and c.twin.max() < c.Vt))
    check_reference(oracle, c)


def test_window_cases_reach_the_second_window(oracle):
    got, d = check_reference(oracle, T.case("patch-second-window"))
    assert d.need == 7 and d.patch.size == 7
    assert d.windows.tolist() == [1] * 7 and d.lanes.tolist() == [1, 1, 1, 1, 2, 2, 2]  # two neighbouring words of window 1
    assert not d.before[2174] and 2174 not in got  # the eighth hole stays
    assert not d.before[T.WINDOW_END: T.WINDOW_END + 64].any()  # ... and so does everything behind the list
    got, d = check_reference(oracle, T.case("patch-straddles-windows"))
    assert d.need == 7 and d.patch.size == 7
    assert d.windows.tolist() == [0, 0, 0, 1, 1, 1, 1] and d.lanes.tolist() == [63, 63, 63, 0, 0, 5, 5]
    assert 2246 not in got
    for name in T.WINDOW_HOLES:  # frequent in mid-word: the first window's first word is masked below bit 8
        c = T.case(name)
        assert T.parse(c.blob)[0] % 32 == 8
        assert T.dissect(c, T.reference(oracle, c)).list_lengths.max() > 2000  # the long list


def test_patch_counts(oracle):
    got, d = check_reference(oracle, T.case("patch-not-needed"))
    assert d.need == 0 and d.patch.size == 0 and got.size % 8 == 0 and got.size < 640 and not d.before[64]
    got, d = check_reference(oracle, T.case("patch-runs-out"))
    assert d.need == 7 and d.patch.tolist() == [150, 201] and got.size == 203
    got, d = check_reference(oracle, T.case("frequent-above-V"))
    assert got.size == 645 and d.patch.size == 0 and d.need == 3
    got, d = check_reference(oracle, T.case("frequent-0"))
    assert d.patch.tolist() == [0, 1] and got.size == 8
    for V in (517, 1003):
        got, d = check_reference(oracle, T.case("full-%d" % V))
        assert got.size == V and V % 8 and d.need and d.patch.size == 0


def test_sizes(oracle):
    d2 = check_reference(oracle, T.case("wpt2"))[1]
    d3 = check_reference(oracle, T.case("wpt3"))[1]
    assert 1024 < d2.TW <= 2048 < d3.TW <= 3072 and T.case("wpt2").Vt % 32 and T.case("wpt3").Vt % 32
    for d in (d2, d3):  # lists past 128 and 256 entries: more than one trip of the 64-entry loop
        assert (d.list_lengths > 128).any() and (d.list_lengths > 256).any()
        assert d.patch.size == d.need
    got, d = check_reference(oracle, T.case("wpt3"))
    assert got[-1] // 32 >= 2048  # ids of the third word of a thread
    assert check_reference(oracle, T.case("tokens-40x32"))[1].n_tok > 1024
    assert check_reference(oracle, T.case("tokens-140x128"))[1].n_tok > 16384 and T.case("tokens-140x128").paths == (1,)
    for name in T.case_names():
        if name != "tokens-140x128":
            assert T.case(name).paths == (1, 2), name
    assert {(T.case(n).Vs, T.case(n).Vt) for n in T.case_names()} >= {(3000, 1003), (600, 1003), (300, 2048), (2048, 300)}


def test_duplicates(oracle):
    for name in ("duplicates", "duplicates-shared"):
        c = T.case(name)
        check_reference(oracle, c)
        assert c.ids.size == 192 and np.all(c.ids[:, 0] == 9)  # in every sentence, hence in every 64-token chunk
        words = T.words_of(c.ids, c.lens)
        frequent, _, off, _ = T.parse(c.blob)
        assert c.Vs - 1 in words and any(off[w] == off[w + 1] for w in words)  # the last word; words without a list
        assert off[10] - off[9] > 64
    c = T.case("duplicates-shared")
    assert c.Vs > c.Vt and (T.words_of(c.ids, c.lens) >= c.Vt).any()


def _padding_shows(c):
    return not np.array_equal(numpy_generate(c.blob, c.Vt, c.ids, c.lens, c.shared),
                              numpy_generate(c.blob, c.Vt, c.ids, np.full_like(c.lens, c.ids.shape[1]), c.shared))


def test_padding_would_show(oracle):
    """A generator that takes padding for words gives another list: in most stand-alone cases and in at least one model-bound
    case of every encoder set-up."""
    shows = [n for n in T.case_names() if T.case(n).twin is None and _padding_shows(T.case(n))]
    assert {"patch-second-window", "patch-not-needed", "duplicates", "wpt2", "tokens-40x32", "src3000-tgt1003"} <= set(shows), shows
    for enc in T.ENCODERS:
        assert any(_padding_shows(T.model_case(mc)[1]) for mc in T.MODEL_CASES if mc[0] == enc), enc
    for name, _, _, _ in T.MERGED:
        if name != "eight-one-tile":
            assert any(_padding_shows(c) for c in T.merged_batches(name)[1]), name


@pytest.mark.parametrize("mc", T.MODEL_CASES, ids=T.model_case_id)
def test_model_cases(oracle, mc):
    """Every model-bound case has its reference; its batch holds only words both vocabularies know (padding included: the
    host checks every id); and the translation it is compared through is not degenerate where the table vouches for it."""
    enc, what, B, S, mode = mc
    name, c = T.model_case(mc)
    V = T.model_V(name)
    assert c.Vt == V and c.ids.max() < min(V, c.Vs)
    got, d = check_reference(oracle, c)
    if what == "lex100":
        assert d.n_tok > 1024 and (d.list_lengths > 64).any()
    if what == "full":
        assert got.size == V and V % 8
    if what in T.WINDOW_HOLES:
        assert d.windows.max() == 1 and d.need == 7
    if what == "patch-not-needed":
        assert d.need == 0
    if V == 33003:
        assert d.TW > 1024
    if (what, B, S) in T.VOUCHED:
        sl, out, ln, al = T.translation(oracle, name, c)
        assert not fixture_problems(B, out, ln, out.shape[1]), (name, what, B, S, ln.tolist())


def test_model_table_covers_the_launch_edges():
    dims = {n: T.MODELS[n][0] for n in T.MODELS}
    assert dims["tiny-1003"][:3] == dims["tiny-33003"][:3] == (256, 1536, 8) and dims["base-1003"][:3] == (512, 2048, 8)
    assert T.model_V("tiny-1003") % 32 and (T.model_V("tiny-33003") + 31) // 32 > 1024
    seen = {(mc[0], mc[1]) for mc in T.MODEL_CASES}
    for enc in ("rows64", "rows32", "wide"):  # each encoder: many tokens, the full list, both source vocabularies
        assert {(enc, "lex100"), (enc, "full"), (enc, "src3000"), (enc, "src600")} <= seen
    shapes = {(mc[2], mc[3]) for mc in T.MODEL_CASES}
    assert {(40, 32), (5, 13), (1, 1), (9, 40), (9, 70)} <= shapes
    assert any(mc[4] == 1 for mc in T.MODEL_CASES)
    assert T.GENERATORS["src3000"][0] > T.model_V("tiny-1003") > T.GENERATORS["src600"][0]


def test_hint_cases_alternate_between_the_extremes(oracle):
    """the small list is a few dozen ids, the large one is past the 16384 columns at which the host changes the decoder tiling"""
    sizes = [T.reference(oracle, T.hint_case(B, S)).size for B, S in T.HINT_SHAPES]
    assert sizes[0] == sizes[2] and sizes[1] == sizes[3]
    assert 0 < sizes[0] <= 128 and sizes[1] > 16384, sizes
    c = T.hint_case(40, 32)
    sl, out, ln, al = T.translation(oracle, T.HINT_MODEL, c)
    assert not fixture_problems(40, out, ln, out.shape[1]), ln.tolist()


def test_merged_cases(oracle):
    """2, 5 and 8 sub-batches of different B and S_j <= S; one launch with fewer tiles than shortlists; the lists of one launch
    differ from each other; the repeated word's ids are in every sub-batch's list and nowhere by leaking alone"""
    assert {len(m[2]) for m in T.MERGED} >= {2, 5, 8}
    for name, S, shapes, word in T.MERGED:
        S_, cases = T.merged_batches(name)
        assert S_ == S and max(Sj for _, Sj in shapes) == S and len(cases) == len(shapes) <= 8
        lists = [check_reference(oracle, c)[0] for c in cases]
        assert len({l.tobytes() for l in lists}) == len(lists), name  # every sub-batch has ITS list
        if name in ("two", "five", "eight"):
            assert len({B for B, _ in shapes}) > 1 and len({Sj for _, Sj in shapes}) > 1
        if name == "eight-one-tile":
            assert sum(B for B, _ in shapes) <= 16 and S == 1
        if word is not None:
            frequent, _, off, ids = T.parse(cases[0].blob)
            own = ids[int(off[word]): int(off[word + 1])]
            own = own[own >= frequent]
            assert own.size and all(np.isin(own, l).all() for l in lists)
            # ... which no other word of the later sub-batches selects: a claim left behind by sub-batch 0 would lose them
            for c in cases[1:]:
                others = T.words_of(c.ids, c.lens)
                rest = np.concatenate([ids[int(off[w]): int(off[w + 1])] for w in np.unique(others[others != word])])
                assert not np.isin(own, rest).all()
