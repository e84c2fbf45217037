"""One affine case at the extremes of the int8 formats, shared by tests/test_oracle.py (the oracle against an int64 numpy
sum: the reference itself is pinned there) and tests/test_gpu_qmm.py (the kernels against the oracle).

W ([N][K], int8): row 0 = all -128 (a value quantisation never produces but a model file may hold), row 1 = all +127,
row 2 = all -127, row 3 = +127 / -127 alternating, row 4 = all +127 but one 126 (an odd accumulator against the row of
zeros), the others uniform over [-128, 127].
x ([M][K], float32) under a_quant = 8: a row saturating at +1000 (q = 127), one at -1000 (q = -127, never -128), one on
exact .5 ties (q * 8 = k + 0.5: round to even), one of zeros, the others normal(0, 2). With many rows the four are repeated at
the edges of the 128-row tiles (rows 127 / 128, 1023 / 1024) and at the end of the ragged last tile.

Closed forms of the shifted accumulator accS = sum_k (q_k + 127) W_k:
  q = +127 (254 shifted): -254 * 128 K, 254 * 127 K, -254 * 127 K and 0 on rows 0..3 of W;
  q = -127 (0 shifted):   0 everywhere -- a clamp to -128 would give -1 * colsum instead;
  q = 0  (127 shifted):   127 * colsum = -127 * 128 K, 127 * 127 K, -127 * 127 K and 0.
At K = 4096 the first is -133,169,152: past 2^24 from K = 1536 on, where float(accS) rounds and the ONE conversion the
reference makes (float(accS) * u + prepared bias) differs from float(acc) + float(127 colsum)."""
import numpy as np

A_QUANT = 8.0
KS = (64, 256, 1536, 2048, 4096)
MS = (5, 1024, 1100)
NS = (7, 72, 517)
SAT_POS, SAT_NEG, TIES, ZEROS = 0, 1, 2, 3


def special_rows(M):
    """{row of x: kind}"""
    rows = {0: SAT_POS, 1: SAT_NEG, 2: TIES, 3: ZEROS}
    if M >= 1024:
        rows.update({127: SAT_POS, 128: SAT_NEG, 1023: TIES, 1022: ZEROS, M - 1: SAT_POS, M - 2: SAT_NEG, M - 3: ZEROS, M - 4: TIES})
    if M > 1024:
        rows.update({1024: SAT_NEG, 1025: SAT_POS})
    return rows


def make(M, K, N):
    r = np.random.Generator(np.random.PCG64(1000003 * M + 1009 * K + N))
    W = r.integers(-128, 128, size=(N, K)).astype(np.int8)
    W[0], W[1], W[2] = -128, 127, -127
    W[3] = np.where(np.arange(K) % 2 == 0, 127, -127)
    W[4] = 127  # (the one 126 is placed below, once x is known)
    x = r.normal(0, 2.0, size=(M, K)).astype(np.float32)
    ties = (((np.arange(K) * 7) % 201 - 100) + 0.5) / np.float32(A_QUANT)  # q * 8 = j + 0.5, j in -100 .. 100: exact in float32
    values = {SAT_POS: 1000.0, SAT_NEG: -1000.0, TIES: ties, ZEROS: 0.0}
    for row, kind in special_rows(M).items():
        x[row] = values[kind]
    # row 4's one 126: 127 colsum = 127 * (127 K - 1) is odd, so past 2^24 (K >= 1536) float(accS) MUST round against the row
    # of zeros. Its place is the first at which, in one of the first five rows, converting the signed accumulator and
    # 127 colsum separately gives another float than converting accS once (the defect the float comparisons are for).
    q5 = quantised(x[:5])
    for j in range(K):
        w = np.full(K, 127, np.int64)
        w[j] = 126
        acc, shift = (q5 + 127) @ w, 127 * int(w.sum())
        if K < 1536 or (np.float32(shift) + (acc - shift).astype(np.float32) != acc.astype(np.float32)).any():
            W[4, j] = 126
            break
    else:
        raise AssertionError("no place for the 126 separates the two conversions")
    bias = r.normal(0, 0.05, size=N).astype(np.float32)
    bq = float(np.float32(127.0 / r.uniform(0.3, 1.0)))
    return x, W, bias, A_QUANT, bq


def quantised(x):
    """int64 [M][K]: round to nearest even, clamped to [-127, 127]"""
    return np.clip(np.rint(x.astype(np.float64) * A_QUANT), -127, 127).astype(np.int64)


def accumulators_int64(x, W):
    return (quantised(x) + 127) @ W.astype(np.int64).T


def check_closed_forms(acc, M, K):
    """the extreme accumulators of `acc` ([M][N], any integer type), exactly"""
    acc = np.asarray(acc).astype(np.int64)
    want = {SAT_POS: (-254 * 128 * K, 254 * 127 * K, -254 * 127 * K, 0),
            SAT_NEG: (0, 0, 0, 0),
            ZEROS: (-127 * 128 * K, 127 * 127 * K, -127 * 127 * K, 0)}
    for row, kind in special_rows(M).items():
        if kind in want:
            assert tuple(acc[row, :4].tolist()) == want[kind], (row, kind, acc[row, :4].tolist(), want[kind])
    assert not acc[1].any()  # a row of -127s, shifted, is all zeros: accS is 0 in EVERY column
