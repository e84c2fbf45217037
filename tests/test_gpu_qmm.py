"""GPU parity of the slimt::qmm boundary (QMM.hh:48-63), through the C ABI.
int32 accumulators: bit-exact. Floats: bit-exact against the oracle in
PORTABLE order, and within 1e-4 (north_star) of the FAITHFUL reference order --
for these ops the two orders coincide, the epilogue being pure IEEE mul/add."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def make_case(seed, M, K, N, x_scale=2.0):
    r = rng(seed)
    x = r.normal(0, x_scale, size=(M, K)).astype(np.float32)
    W = np.clip(np.rint(r.normal(0, 32, size=(N, K))), -127, 127).astype(np.int8)
    bias = r.normal(0, 0.05, size=N).astype(np.float32)
    aq = float(np.float32(127.0 / r.uniform(4, 12)))
    bq = float(np.float32(127.0 / r.uniform(0.3, 1.0)))
    return x, W, bias, aq, bq


def test_mfma_operand_layout_asymmetric(hip, oracle):
    """A = one-hot rows against an asymmetric W catches any row/col/k swap of
    the MFMA fragment maps (cdna guide: 'A=I-check with ASYMMETRIC B')."""
    M, K, N = 16, 64, 16
    x = np.zeros((M, K), dtype=np.float32)
    for i in range(M):
        x[i, (i * 5 + 3) % K] = 1.0  # q = 1 at a distinct k per row
    W = ((np.arange(N)[:, None] * 7 + np.arange(K)[None, :] * 3) % 251 - 125).astype(np.int8)
    got = hip.affine_acc_i32(x, W, 1.0)
    want = oracle.affine_acc(x, W, 1.0)
    assert np.array_equal(got, want)


# the GEMM shape census of SURVEY App. D (decoder M=B, encoder M=B*S) + edges
SHAPES = [
    (1, 64, 8), (3, 64, 16), (16, 64, 16), (17, 128, 24), (5, 256, 40),
    (64, 256, 256), (64, 256, 512), (64, 256, 1536), (64, 1536, 256), (64, 256, 4096),
    (256, 512, 512), (2048, 256, 256), (300, 256, 1536), (130, 2048, 512), (33, 512, 2048),
    # many rows: slimt_hip_affine takes the 128-row tiling (gemm_tile.hip): a ragged last row
    # block, K in one / three / four 512-deep chunks, N not a multiple of the 128-column block
    (1100, 512, 512), (1024, 1536, 256), (1300, 2048, 576), (2048, 256, 1536),
    # K that no model preset has (3, 5, 7, 11, 16 and 64 k-steps of 64), N that is no multiple of 8
    (19, 192, 40), (70, 320, 517), (5, 448, 7), (33, 704, 1), (130, 1024, 1003), (21, 4096, 72),
    # the edges of the 128-row tiling's dispatch: M = 1023 / 1024, N = 48 / 64 / 72, K it does not take with M >= 1024
    (1023, 512, 512), (1024, 512, 48), (1024, 512, 72), (1024, 192, 256), (1024, 320, 256), (1024, 1024, 64),
]


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_affine_accumulators_bit_exact(hip, oracle, M, K, N):
    x, W, bias, aq, bq = make_case(M + K + N, M, K, N)
    got = hip.affine_acc_i32(x, W, aq)
    want = oracle.affine_acc(x, W, aq)
    assert got.dtype == np.int32 and np.array_equal(got, want)


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_affine_and_dot_float(hip, oracle, M, K, N):
    x, W, bias, aq, bq = make_case(7 * M + K + N, M, K, N)
    for b in (bias, None):  # affine / dot
        got = hip.affine(x, W, b, aq, bq)
        for mode in (oracle.PORTABLE, oracle.FAITHFUL):
            oracle.set_mode(mode)
            want = oracle.affine(x, W, b, aq, bq)
            assert np.array_equal(got, want), np.abs(got - want).max()
    oracle.set_mode(oracle.FAITHFUL)


def test_affine_saturation_and_ties(hip, oracle):
    """activations that saturate the +-127 clamp and sit on exact .5 ties."""
    M, K, N = 32, 256, 64
    x, W, bias, aq, bq = make_case(5, M, K, N)
    aq = 8.0
    x[0, :] = 1000.0
    x[1, :] = -1000.0
    x[2, :] = (np.arange(K) - 128 + 0.5) / 8.0  # q*aq lands on k + 0.5 exactly
    x[3, :] = 0.0
    W[0, :] = 127
    W[1, :] = -127
    got_acc = hip.affine_acc_i32(x, W, aq)
    assert np.array_equal(got_acc, oracle.affine_acc(x, W, aq))
    assert got_acc[0, 0] == 254 * 127 * K and got_acc[1, 0] == 0
    got = hip.affine(x, W, bias, aq, bq)
    assert np.array_equal(got, oracle.affine(x, W, bias, aq, bq))


@pytest.mark.parametrize("M,K,N,n_idx", [(1, 64, 512, 8), (16, 256, 2048, 256), (64, 256, 32000, 4096),
                                         (7, 512, 4000, 1000), (21, 256, 1003, 200)])
def test_affine_with_select(hip, oracle, M, K, N, n_idx):
    x, W, bias, aq, bq = make_case(M + n_idx, M, K, N)
    r = rng(n_idx)
    idx = np.sort(r.choice(N, size=n_idx, replace=False)).astype(np.uint32)
    got = hip.affine_with_select(x, W, bias, aq, bq, idx)
    want = oracle.affine_select(x, W, bias, aq, bq, idx)
    assert got.shape == (M, n_idx) and np.array_equal(got, want)
    # and it is the column gather of the full affine (Intgemm.inl.cc:36-87)
    if N <= 4096:
        assert np.array_equal(got, hip.affine(x, W, bias, aq, bq)[:, idx])


def test_affine_non_finite_activations(hip, oracle):
    """NaN / inf activations quantise like intgemm's PrepareA: NaN -> -127,
    +inf -> 127, -inf -> -127 (accumulators stay exact)."""
    M, K, N = 16, 64, 32
    x, W, bias, aq, bq = make_case(77, M, K, N)
    x[0, 0], x[1, 5], x[2, 9] = np.nan, np.inf, -np.inf
    got = hip.affine_acc_i32(x, W, aq)
    assert np.array_equal(got, oracle.affine_acc(x, W, aq))


def test_affine_leading_dims_flatten(hip, oracle):
    """M = x.size / x.dim(-1): leading dims flatten (Intgemm.inl.cc:101-104)."""
    x, W, bias, aq, bq = make_case(9, 6 * 5, 128, 96)
    got = hip.affine(x.reshape(6, 5, 128), W, bias, aq, bq)
    assert got.shape == (6, 5, 96)
    assert np.array_equal(got.reshape(30, 96), oracle.affine(x, W, bias, aq, bq))


def test_affine_rejects_bad_shapes(hip):
    x = np.zeros((4, 100), dtype=np.float32)
    W = np.zeros((16, 100), dtype=np.int8)
    with pytest.raises(hip.SlimtHipError):
        hip.affine(x, W, None, 1.0, 1.0)  # K % 64 != 0, like intgemm's own constraint
    with pytest.raises(hip.SlimtHipError, match="4160"):
        hip.affine(np.zeros((4, 4160), np.float32), np.zeros((16, 4160), np.int8), None, 1.0, 1.0)  # K > 4096
    with pytest.raises(hip.SlimtHipError):
        hip.affine_with_select(np.zeros((4, 64), np.float32), np.zeros((16, 64), np.int8),
                               np.zeros(16, np.float32), 1.0, 1.0, np.array([99], np.uint32))


def test_linearity_property_full_size(hip):
    """Size-independent property at the bench's full decode size: the int32
    accumulators are linear in the quantised activations, so
    acc(q1 + q2) - 127*colsum == acc(q1) + acc(q2) - 2*127*colsum, checked via
    accS(a) + accS(b) - accS(a+b) == accS(0)."""
    M, K, N = 256, 256, 4096
    r = rng(123)
    a = r.integers(-60, 61, size=(M, K)).astype(np.float32)
    b = r.integers(-60, 61, size=(M, K)).astype(np.float32)
    W = r.integers(-127, 128, size=(N, K)).astype(np.int8)
    z = np.zeros_like(a)
    sa, sb, sab, s0 = (hip.affine_acc_i32(v, W, 1.0) for v in (a, b, a + b, z))
    assert np.array_equal(sa.astype(np.int64) + sb - sab, s0.astype(np.int64))
    assert np.array_equal(s0[0], 127 * W.astype(np.int64).sum(axis=1))


# ---- the extremes of the int8 formats (tests/support/qmm_extremes.py; the oracle's side is pinned in tests/test_oracle.py) ----

def _extreme_shapes():
    from support import qmm_extremes as X
    return [(M, K, N) for K in X.KS for M in X.MS for N in X.NS]


@pytest.fixture(scope="module")
def extreme_cases(oracle):
    """(x, W, bias, aq, bq, the oracle's accumulators) per shape, computed once and never written to"""
    from support import qmm_extremes as X
    cache = {}

    def get(M, K, N):
        if (M, K, N) not in cache:
            x, W, bias, aq, bq = X.make(M, K, N)
            acc = oracle.affine_acc(x, W, aq)
            for a in (x, W, bias, acc):
                a.setflags(write=False)
            cache[(M, K, N)] = (x, W, bias, aq, bq, acc)
        return cache[(M, K, N)]

    return get


@pytest.mark.parametrize("M,K,N", _extreme_shapes())
def test_extremes_accumulators_bit_exact_and_closed_forms(hip, extreme_cases, M, K, N):
    """Weights of -128 and rows of one sign against activations that saturate, tie and vanish: int32 accumulators equal
    to the oracle's and to the closed forms (accS == -254 * 128 * K for a saturated-positive row against an all -128
    column; 0 for a saturated-negative row, which a clamp to -128 would turn into -colsum), K up to 4096 (|accS| up to
    133,169,152 < 2^31), M at and past the 128-row tiling's threshold, N that is no multiple of 8."""
    from support import qmm_extremes as X
    x, W, _, aq, _, want = extreme_cases(M, K, N)
    got = hip.affine_acc_i32(x, W, aq)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    X.check_closed_forms(got, M, K)


@pytest.mark.parametrize("M,K,N", _extreme_shapes())
def test_extremes_affine_dot_and_select_bit_exact(hip, oracle, extreme_cases, M, K, N):
    """The floats of the same case: affine, dot (no bias) and affine_with_select (the four extreme columns and every
    third of the others) equal to the oracle's bit for bit. From K = 1536 on the one-signed columns' accumulators pass 2^24,
    where float(accS) rounds: a kernel that converts the signed accumulator and 127 colsum separately differs there. M >=
    1024 takes the 128-row tiling (gemm_tile.hip), which the suite's other extremes (M = 32) never reach."""
    x, W, bias, aq, bq, acc = extreme_cases(M, K, N)
    if K >= 1536:
        a = acc.astype(np.int64)
        assert (a.astype(np.float32).astype(np.int64) != a).any()  # this case does exercise the rounding conversion
        shift = 127 * W.astype(np.int64).sum(axis=1)[None, :]  # ... and the split conversion is another float somewhere in it
        assert ((a - shift).astype(np.float32) + shift.astype(np.float32) != a.astype(np.float32)).any()
    oracle.set_mode(oracle.PORTABLE)
    try:
        for b in (bias, None):
            got = hip.affine(x, W, b, aq, bq) if b is not None else hip.dot(x, W, aq, bq)
            want = oracle.affine(x, W, b, aq, bq)
            assert np.array_equal(got, want), (b is None, np.abs(got - want).max())
        idx = np.unique(np.concatenate([np.arange(min(4, N)), np.arange(4, N, 3)])).astype(np.uint32)
        got = hip.affine_with_select(x, W, bias, aq, bq, idx)
        want = oracle.affine_select(x, W, bias, aq, bq, idx)
        assert got.shape == (M, idx.size) and np.array_equal(got, want), np.abs(got - want).max()
    finally:
        oracle.set_mode(oracle.FAITHFUL)
