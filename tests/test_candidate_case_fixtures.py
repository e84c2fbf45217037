"""CPU proof that the cases of tests/support/candidate_cases.py sit where they claim relative to the attention's run length G
and the 8192-row chunks (in the manner of test_score_case_fixtures.py), and the numpy rank checker against hand-worked rows.
Nothing here needs a GPU or calls the library's compute."""
import re
import os

import numpy as np

from support import candidate_cases as CC
from support import score_cases as C

G = CC.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_length_is_the_headers_and_the_kernels():
    hdr = open(os.path.join(ROOT, "include", "slimt_hip.h")).read()
    krn = open(os.path.join(ROOT, "slimt_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"#define SLIMT_HIP_CANDIDATE_RUN (\d+)", hdr).group(1)) == G
    assert int(re.search(r"constexpr int kScoreCandidateRun = (\d+);", krn).group(1)) == G
    assert G >= 2


def test_fan_is_the_issues():
    c = CC.fan()
    assert c.model == "micro" and c.ids.shape == (4, 7) and c.t_ids.shape == (1 + 3 + G + 1, 5)
    assert list(c.lens) == [7, 1, 4, 6]
    assert [int((c.cand_src == b).sum()) for b in range(4)] == [0, 1, 3, G + 1]
    assert list(c.cand_src) == sorted(c.cand_src)
    assert {0, 1, 5} <= set(int(x) for x in c.t_len)
    perms = CC.order_perms(len(c.t_len))
    assert perms["reversed"] == list(range(len(c.t_len)))[::-1]
    for p in perms.values():
        assert sorted(p) == list(range(len(c.t_len)))
    inter = c.cand_src[np.asarray(perms["interleaved"])]
    assert np.count_nonzero(np.diff(inter.astype(int))) >= 5  # not sorted: sources alternate
    assert max(len(s) for s in CC.stagings(CC.permuted(c, perms["interleaved"]))) > max(len(s) for s in CC.stagings(c)) - 1


def test_runs_sit_on_and_around_the_run_length():
    assert [sum(v) for v in CC.RUN_COUNTS.values()] == [G - 1, G, G + 1, 2 * G + 1, 2 * G, 2 * G]
    assert any(sum(v) % G for v in CC.RUN_COUNTS.values())  # a last, partial run
    assert CC.stagings(CC.runs("one-2G+1")) == [[0], [0], [0]]  # one staging per run
    assert CC.stagings(CC.runs("edge-G-G")) == [[0], [1]]       # the change is on the run's edge
    assert CC.stagings(CC.runs("mid-G-1-G+1")) == [[0, 1], [1]]  # ... in mid-run
    for name in CC.RUN_COUNTS:
        assert np.all(CC.runs(name).t_len > 0)


def test_dead_cases_are_what_their_names_say():
    st = {n: CC.stagings(CC.dead(n)) for n in CC.DEAD_CASES}
    t = {n: CC.dead(n).t_len for n in CC.DEAD_CASES}
    assert t["first-in-run"][0] == 0 and st["first-in-run"] == [[0], [1]]
    c = CC.dead("first-of-source-mid-run")
    assert c.t_len[G - 1] == 0 and c.cand_src[G - 1] == 1 != c.cand_src[G - 2] and (G - 1) % G
    assert st["first-of-source-mid-run"] == [[0], [1]]  # the empty candidate stages nothing: source 1 comes with the next run
    c = CC.dead("first-of-source-on-edge")
    assert c.t_len[G] == 0 and c.cand_src[G] == 1 and st["first-of-source-on-edge"] == [[0], [1]]
    assert t["last"][-1] == 0 and len(t["last"]) % G == 1 and st["last"] == [[0], [1], []]
    assert st["run-between-sources"] == [[0], [], [1]]  # a run whose candidates are all dead
    c = CC.dead("whole-source")
    assert np.all(c.t_len[c.cand_src == 1] == 0) and st["whole-source"] == [[0], [], [2]]
    assert np.all(t["all"] == 0) and st["all"] == [[], []]


def test_keys_rows_chunks_and_many():
    assert CC.KEY_S == (64, 65, 128) and [C.dims_of(n)[0] // C.dims_of(n)[2] for n in CC.KEY_MODELS] == [16, 32, 64]
    c = CC.keys("head64", 128)
    st = CC.stagings(c)  # restaged inside a run, and back to the long source
    assert list(c.lens) == [128, 1] and sum(st, []) == [0, 1, 0] and max(len(s) for s in st) >= 2 and 8 * 128 * 64 == 64 << 10
    c = CC.rows()
    assert c.model == "mini" and c.t_ids.shape == (25, 41) and 25 * 41 == 1025 > 1024 and len(c.lens) == 3
    c = CC.chunks()
    assert c.t_ids.shape == (4, 2731) and CC.chunk_split(c) == [(0, 2), (2, 2)] and 3 * 2731 > CC.CHUNK_ROWS >= 2 * 2731
    assert list(c.cand_src) == [0, 0, 0, 1] and CC.stagings(c) == [[0], [0, 1]]
    c = CC.many()
    assert len(c.lens) == CC.MANY_B == 2 and len(c.t_len) == CC.MANY_N == 40 and 0 in c.t_len


def test_rank_checker_against_hand_worked_rows():
    f = np.float32
    inf, nan = f(-np.inf), f(np.nan)
    sc = np.array([[-1.0, -2.0, 9.0],    # 0: source 0, n 2: total -3, mean -1.5
                   [-0.5, -0.5, -0.5],   # 1: source 0, n 3: total -1.5, mean -0.5 (wins both)
                   [-1.0, -0.5, 0.0],    # 2: source 0, n 2: total -1.5 (ties 1 as a sum: the lower index stays), mean -0.75
                   [nan, 0.0, 0.0],      # 3: source 1: NaN never competes
                   [inf, 0.0, 0.0],      # 4: source 1, n 1: -inf competes (and is alone)
                   [5.0, 5.0, 5.0],      # 5: source 2, n 0: 0.0, never competes
                   [-0.0, -0.0, -0.0],   # 6: source 3, n 3: +0 + -0 ... = +0
                   [0.0, 0.0, 0.0],      # 7: source 3: equal to 6 as a float: the lower index stays
                   [-4.0, 1.0, 1.0],     # 8: source 5, n 3: total -2, mean -2/3
                   [-1.0, 0.0, 0.0]],    # 9: source 5, n 1: total -1 (wins the sum), mean -1 (loses the mean)
                  np.float32)
    t_len = np.array([2, 3, 2, 3, 1, 0, 3, 3, 3, 1], np.uint32)
    src = np.array([0, 0, 0, 1, 1, 2, 3, 3, 5, 5], np.uint32)
    tot, best = CC.rank_reference(sc, t_len, src, 6, mean=False)
    assert np.array_equal(tot[[0, 1, 2, 5, 8, 9]], f([-3, -1.5, -1.5, 0, -2, -1])) and np.isnan(tot[3]) and tot[4] == inf
    assert not np.signbit(tot[6]) and tot[6] == 0
    assert list(best) == [1, 4, CC.NONE, 6, CC.NONE, 9]
    tot_m, best_m = CC.rank_reference(sc, t_len, src, 6, mean=True)
    assert np.array_equal(tot_m.view(np.uint32), tot.view(np.uint32))
    assert list(best_m) == [1, 4, CC.NONE, 6, CC.NONE, 8]
    # a total that depends on the order of the adds: ascending t from +0
    big = np.array([[1e8, 1.0, -1e8, 1.0]], np.float32)
    assert CC.rank_reference(big, [4], [0], 1, False)[0][0] == f(f(f(f(1e8) + f(1)) - f(1e8)) + f(1)) == f(1.0)


def test_rank_inputs_hold_what_the_issue_lists():
    for (N, B) in CC.RANK_SIZES:
        sc, t_len, src = CC.rank_inputs(N, B, seed=N + B)
        assert sc.shape == (N, CC.RANK_T) and src.max() < B
        if N < 64:
            continue
        tot, best = CC.rank_reference(sc, t_len, src, B, False)
        live = t_len > 0
        assert np.isnan(tot[live]).any() and np.isneginf(tot[live]).any() and (~live).any()
        assert np.signbit(sc).any() and (sc == 0).all(axis=1).any()  # -0 rows and +0 rows
        assert (best == CC.NONE).any() and np.any(np.diff(src.astype(int)) < 0)
        ok = live & ~np.isnan(tot)
        ties = sum(int(np.sum(tot[ok & (src == b)] == tot[best[b]]) > 1) for b in range(B) if best[b] != CC.NONE)
        assert ties > 0
