"""Every sentence length at every padded width, on every translate entry point, with every output inside guard bands.

The other GPU tests draw ragged lengths from [S / 4, S] and read outputs that the wrappers allocated at exactly their size
and zero-filled. Here:
  * a batch holds EVERY length 0, 1, ..., S (B = S + 1, shuffled), at padded widths on both sides of each encoder's and
    each K/V reader's range boundaries (1..32: the fused encoder, 64- and 32-row tiles; 33..64: the tall encoder and the
    32-row fallback; 65..128: the per-sentence encoder; D = 512: encode_wide);
  * merged launches hold sub-batches padded to fewer tokens than the launch with lengths 0, 1, S_j - 1 and S_j, and
    device lengths past their own row (S_j + 1, S, 0xFFFFFFFF);
  * every output (out_ids, out_len, align, scores) lies inside a larger allocation filled with a pattern; the 4 KiB on
    either side must stay unchanged, and the interior must equal the checker's arrays (PORTABLE order) exactly -- the
    entries past a sentence's length included, which the kernels write as zeros (include/slimt_hip.h).
Scores are compared where they are defined (t < out_len) with the float64 teacher-forced log-softmax."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_scores import _check_scores, _teacher_forced

pytestmark = pytest.mark.gpu

GUARD = 4096  # bytes on either side of every output (>= S * 4 for every S here)
PAT = 0xA5A5A5A5
LF = 1.5
ORACLE_THREADS = 16


@pytest.fixture(scope="module")
def engines(hip, oracle, synth_models):
    cache = {}

    def get(preset):
        if preset not in cache:
            m = synth_models(preset, 6.0)  # eos_bias 6: sentences end at different steps
            cache[preset] = (m, hip.Model(m), oracle.OracleModel(m, threads=ORACLE_THREADS))
        return cache[preset]

    yield get
    for _, gm, _ in cache.values():
        gm.set_kv_cache_format(0)
        gm.close()


def _tmax(S):
    return max(int(np.float32(LF) * np.float32(S)), 1)


class _Buffers:
    """The arrays of one call. where: "device" (one torch.empty per array), "pinned" (slimt_hip_host_alloc) or "host"
    (numpy). Outputs sit GUARD bytes into an allocation filled with PAT; check() asserts the guards and returns the
    interiors."""

    def __init__(self, hip, where):
        self.hip, self.where = hip, where
        self.outs, self.keep, self.pins = [], [], []

    def _raw(self, n_words):
        if self.where == "device":
            t = torch.full((n_words,), np.int32(np.uint32(PAT).view(np.int32)).item(), dtype=torch.int32, device="cuda")
            return t, t.data_ptr(), None
        if self.where == "pinned":
            p = C.c_void_p()
            self.hip._chk(self.hip.lib().slimt_hip_host_alloc(n_words * 4, C.byref(p)))
            self.pins.append(p)
            a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n_words,))
            a[:] = PAT
            return a, a.ctypes.data, a
        a = np.full(n_words, PAT, dtype=np.uint32)
        return a, a.ctypes.data, a

    def inp(self, a):
        """An input array where this call wants it; returns (address, host view or None)."""
        a = np.ascontiguousarray(a, dtype=np.uint32)
        if self.where == "device":
            t = torch.from_numpy(a.reshape(-1).view(np.int32)).cuda()
            self.keep.append(t)
            return t.data_ptr(), None
        raw, ptr, host = self._raw(max(a.size, 1))
        host[:a.size] = a.reshape(-1)
        self.keep.append(raw)
        return ptr, host[:a.size].reshape(a.shape)

    def out(self, name, dtype, shape):
        """An output: (interior address, interior host view or None)."""
        n = int(np.prod(shape))
        g = GUARD // 4
        raw, ptr, host = self._raw(n + 2 * g)
        self.outs.append((name, dtype, shape, raw, n))
        return ptr + GUARD, None if host is None else host[g:g + n].view(dtype).reshape(shape)

    def check(self):
        """Asserts every guard word unchanged; returns {name: interior array}."""
        g = GUARD // 4
        got = {}
        for name, dtype, shape, raw, n in self.outs:
            a = raw.cpu().numpy().view(np.uint32) if self.where == "device" else raw.copy()
            for side, band, base in (("before", a[:g], -GUARD), ("after", a[g + n:], 4 * n)):
                bad = np.nonzero(band != PAT)[0]
                assert bad.size == 0, f"{name}: guard {side} the output changed at byte offset {base + 4 * int(bad[0])} " \
                                      f"(relative to the output's start; {bad.size} words changed)"
            got[name] = a[g:g + n].view(dtype).reshape(shape)
        return got

    def free(self):
        for p in self.pins:
            self.hip.lib().slimt_hip_host_free(p)
        self.pins = []
        self.keep = []


def _want(oracle, om, ids, lens, sl):
    oracle.set_mode(oracle.PORTABLE)
    try:
        return om.translate(ids, lens, sl, LF, 0, want_align=True)[:3]
    finally:
        oracle.set_mode(oracle.FAITHFUL)


def _assert_equal(got, want, what, ok=None):
    """tokens, lengths, alignment rows (whole arrays: the entries past a length included); ok: the sentences to compare."""
    out, ln, al = got
    w_out, w_ln, w_al = want
    sel = slice(None) if ok is None else ok
    bad = np.nonzero(ln[sel] != w_ln[sel])[0]
    assert bad.size == 0, f"{what}: out_len differs first at sentence {bad[0]}: {ln[sel][bad[0]]} != {w_ln[sel][bad[0]]}"
    bad = np.nonzero((out[sel] != w_out[sel]).any(axis=1))[0]
    assert bad.size == 0, f"{what}: out_ids differ first at sentence {bad[0]}"
    bad = np.nonzero((al[sel] != w_al[sel]).any(axis=(1, 2)))[0]
    assert bad.size == 0, f"{what}: alignment rows differ first at sentence {bad[0]}"


def _lengths_0_to_S(S, seed):
    lens = np.arange(S + 1, dtype=np.uint32)
    np.random.Generator(np.random.PCG64(seed)).shuffle(lens)
    return lens


# ---- unmerged calls ------------------------------------------------------------------------------------------------------

ENTRY_WHERE = {"translate": "host", "async": "pinned", "device": "device",
               "generated": "host", "async_generated": "pinned", "device_generated": "device"}


def _call(hip, ctx, entry, ids, lens, sl=None, gen=None, scores=False):
    """One unmerged call through the C ABI on guard-banded arrays; returns ((out, len, align), scores|None)."""
    L = hip.lib()
    B, S = ids.shape
    T = _tmax(S)
    bufs = _Buffers(hip, ENTRY_WHERE[entry])
    try:
        p_ids, _ = bufs.inp(ids)
        p_len, _ = bufs.inp(lens)
        p_sl, n_sl = (bufs.inp(sl)[0], sl.size) if sl is not None and gen is None else (None, 0)
        p_out, _ = bufs.out("out_ids", np.uint32, (B, T))
        p_ol, _ = bufs.out("out_len", np.uint32, (B,))
        p_al, _ = bufs.out("align", np.float32, (B, T, S))
        if scores:
            p_sc, _ = bufs.out("scores", np.float32, (B, T))
            ctx.set_scores([p_sc])
        a = (p_ids, p_len, B, S)
        o = (LF, 0, p_out, p_ol, p_al)
        if entry == "translate":
            rc = L.slimt_hip_translate(ctx.h, *a, p_sl, n_sl, *o)
        elif entry == "async":
            rc = L.slimt_hip_translate_async(ctx.h, *a, p_sl, n_sl, *o)
        elif entry == "device":
            rc = L.slimt_hip_translate_device(ctx.h, *a, p_sl, n_sl, *o, 0)
        elif entry == "generated":
            rc = L.slimt_hip_translate_generated(ctx.h, gen.h, *a, *o)
        elif entry == "async_generated":
            rc = L.slimt_hip_translate_async_generated(ctx.h, gen.h, *a, *o)
        else:
            rc = L.slimt_hip_translate_device_generated(ctx.h, gen.h, *a, *o, 0)
        hip._chk(rc)
        ctx.synchronize()
        got = bufs.check()
        return (got["out_ids"], got["out_len"], got["align"]), got.get("scores")
    finally:
        bufs.free()


# decode modes by padded width: where a mode has no variant for a width the library quietly takes another (plan() only
# tells fused from per-stage), so each mode is listed with the widths it really reaches:
#   0 auto, 1 per-stage launches, 2 / 4 / 5 the 16- / 8- / 4-sentence tilings: every width here (D = 256; D = 512: 0-2);
#   3 the 32-sentence tiling and 6 the clusters of four 16-sentence workgroups: D = 256 with S <= 32 only.
def _modes(preset, S):
    if preset == "base":
        return (0, 1, 2)
    return (0, 1, 2, 3, 4, 5, 6) if S <= 32 else (0, 1, 2, 4, 5)


# preset, S, encode_rows to force as well, the generated twins' entry points
SPECTRUM = [
    ("tiny11", 1, (32, 64), ("generated",)),
    ("tiny11", 5, (32, 64), ("device_generated",)),
    ("tiny11", 16, (32, 64), ("async_generated",)),
    ("tiny11", 17, (32, 64), ()),
    ("tiny11", 31, (32, 64), ()),
    ("tiny11", 32, (32, 64), ("generated", "async_generated", "device_generated")),
    ("tiny11", 33, (32,), ("device_generated",)),          # the tall encoder; 32 rows: the fused 32-row fallback
    ("tiny11", 48, (32,), ("generated",)),
    ("tiny11", 64, (32,), ("async_generated",)),
    ("tiny11", 65, (), ("generated", "async_generated", "device_generated")),  # the per-sentence encoder
    ("tiny11", 128, (), ()),
    ("base", 8, (), ("device_generated",)),                 # encode_wide, D = 512
    ("base", 32, (), ()),
]


@pytest.mark.parametrize("preset,S,enc_rows,gen_entries", SPECTRUM, ids=[f"{p}-S{s}" for p, s, _, _ in SPECTRUM])
def test_every_length_at_every_width(hip, oracle, engines, preset, S, enc_rows, gen_entries):
    """B = S + 1 sentences of lengths 0..S: every decode mode, K/V cache format and entry point == the checker, bit for bit,
    with no write outside the outputs and none left out inside them."""
    from slimt_amd import synth
    m, gm, om = engines(preset)
    B = S + 1
    ids, _ = synth.make_batch(m.V, B, S, seed=900 + S)
    lens = _lengths_0_to_S(S, seed=S)
    sl = synth.make_shortlist(m.V, 1024 if preset == "tiny11" else 512)
    want = _want(oracle, om, ids, lens, sl)
    ctx = hip.Context(gm, B, S)
    try:
        for mode in _modes(preset, S):
            ctx.set_decode_mode(mode)
            _assert_equal(_call(hip, ctx, "device", ids, lens, sl)[0], want, f"device, mode {mode}")
        ctx.set_decode_mode(0)
        for rows in enc_rows:
            ctx.set_encode_rows(rows)
            _assert_equal(_call(hip, ctx, "device", ids, lens, sl)[0], want, f"device, encode rows {rows}")
        ctx.set_encode_rows(0)
        for fmt in (1, 2, 0):
            gm.set_kv_cache_format(fmt)
            _assert_equal(_call(hip, ctx, "device", ids, lens, sl)[0], want, f"device, K/V format {fmt}")
        for entry in ("translate", "async"):
            _assert_equal(_call(hip, ctx, entry, ids, lens, sl)[0], want, entry)
        got, sc = _call(hip, ctx, "device", ids, lens, sl, scores=True)
        _assert_equal(got, want, "device, scored")
        _check_scores(sc, _teacher_forced(oracle, om, m, ids, lens, sl, got[0], got[1]), got[1])
        if gen_entries:
            blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
            gsl = oracle.OracleShortlist(blob, m.V, m.V).generate(ids, lens)
            g_want = _want(oracle, om, ids, lens, gsl)
            gen = hip.ShortlistGenerator(blob, m.V, m.V)
            try:
                for entry in gen_entries:
                    _assert_equal(_call(hip, ctx, entry, ids, lens, gen=gen)[0], g_want, entry)
            finally:
                gen.close()
    finally:
        gm.set_kv_cache_format(0)
        ctx.close()


# ---- merged launches -----------------------------------------------------------------------------------------------------

def _edge_batch(V, B, Sj, seed, lens_at=()):
    """B sentences padded to Sj holding the lengths 0, 1, Sj - 1 and Sj (and ragged others); lens_at: {row: length}
    overrides."""
    from slimt_amd import synth
    ids, lens = synth.make_batch(V, B, Sj, seed=seed, ragged=True)
    edges = [0, 1, max(Sj - 1, 0), Sj]
    rows = np.random.Generator(np.random.PCG64(seed)).permutation(B)[:len(edges)]
    lens[rows] = edges[:len(rows)]
    for r, v in dict(lens_at).items():
        lens[r] = v
    return ids, lens.astype(np.uint32)


def _many(hip, gm, batches, S, sls, mode, where="device", gen=None, ctx=None):
    """batches: [(ids, lens)] padded to their own S_j <= S; sls: per batch a shortlist or None. One merged call on
    guard-banded outputs (device: translate_many_device[_generated]; pinned: translate_many_async[_generated]).
    ctx: run on this context (default: a fresh one). Returns per batch (out, len, align)."""
    own_ctx = ctx is None
    if own_ctx:
        ctx = hip.Context(gm, hip.translate_many_rows([b[0].shape[0] for b in batches]), S)
    ctx.set_decode_mode(mode)
    per = []
    try:
        args, host = [], []
        for (ids, lens), sl in zip(batches, sls):
            B, Sj = ids.shape
            T = _tmax(Sj)
            bufs = _Buffers(hip, where)
            per.append(bufs)
            p_ids, h_ids = bufs.inp(ids)
            p_len, h_len = bufs.inp(lens)
            p_sl = bufs.inp(sl)[0] if (sl is not None and where == "device") else 0
            p_out, h_out = bufs.out("out_ids", np.uint32, (B, T))
            p_ol, h_ol = bufs.out("out_len", np.uint32, (B,))
            p_al, h_al = bufs.out("align", np.float32, (B, T, Sj))
            args.append((p_ids, p_len, B, p_sl, 0 if sl is None else sl.size, p_out, p_ol, p_al, Sj))
            host.append((h_ids, h_len, h_out, h_ol, h_al))
        if where == "device":
            ctx.translate_many_device(args, S, LF, 0, steps_hint=_tmax(S), generator=gen)
        else:
            assert all(s is sls[0] for s in sls), "translate_many_async takes one host shortlist"
            ctx.translate_many_async(host, None if gen is not None else sls[0], LF, 0, generator=gen)
        ctx.synchronize()
        res = []
        for bufs in per:
            got = bufs.check()
            res.append((got["out_ids"], got["out_len"], got["align"]))
        return res
    finally:
        for bufs in per:
            bufs.free()
        if own_ctx:
            ctx.close()


def _many_checked(hip, gm, batches, S, sls, mode, where="device", gen=None):
    """_many with the guard assertion naming the batch."""
    try:
        return _many(hip, gm, batches, S, sls, mode, where, gen)
    except AssertionError as e:
        raise AssertionError(f"mode {mode}, {where}{', generated' if gen else ''}: {e}") from None


def _forms(m, preset):
    from slimt_amd import synth
    n = 1024 if preset == "tiny11" else 512
    shared = synth.make_shortlist(m.V, n, seed=5)
    own = [synth.make_shortlist(m.V, n - 8 * k, seed=6 + k) for k in range(8)]
    return {"shared": lambda k: [shared] * k, "own": lambda k: own[:k], "full": lambda k: [None] * k}


# preset, launch S, [(B_j, S_j)] (every S_j < S but one), decode modes
MERGED = [
    ("tiny11", 32, [(9, 8), (21, 31), (6, 17)], (0, 2, 3, 4, 5)),
    ("tiny11", 24, [(5, 1), (17, 12), (3, 23), (8, 2), (20, 24), (4, 16), (6, 5), (11, 20)], (0, 2, 4, 5)),
    ("tiny11", 48, [(7, 33), (5, 47), (9, 20)], (0, 2, 4, 5)),
    ("tiny11", 64, [(4, 40), (6, 63)], (0, 2, 5)),
    ("base", 32, [(7, 10), (12, 25)], (0, 2)),
]


def _merged_id(c):
    return f"{c[0]}-S{c[1]}-k{len(c[2])}"


@pytest.mark.parametrize("preset,S,shapes,modes", MERGED, ids=[_merged_id(c) for c in MERGED])
def test_merged_sub_batches_at_their_length_edges(hip, oracle, engines, preset, S, shapes, modes):
    """Sub-batches padded to S_j < S with lengths 0, 1, S_j - 1 and S_j: each == the checker at its own S_j (and so its own
    unmerged call) -- shared shortlist, one per batch, the full vocabulary, generated in the launch; device and pinned."""
    from slimt_amd import synth
    m, gm, om = engines(preset)
    batches = [_edge_batch(m.V, B, Sj, seed=40 + 7 * j + S) for j, (B, Sj) in enumerate(shapes)]
    for name, make in _forms(m, preset).items():
        sls = make(len(batches))
        wants = [_want(oracle, om, ids, lens, sl) for (ids, lens), sl in zip(batches, sls)]
        for mode in modes if name == "shared" else modes[:2]:
            res = _many_checked(hip, gm, batches, S, sls, mode)
            for j, (got, want) in enumerate(zip(res, wants)):
                _assert_equal(got, want, f"{name}, mode {mode}, batch {j} (S_j = {shapes[j][1]})")
        if name != "full":
            # the unmerged call of each batch gives the same (implied by the checker; the direct statement)
            ctx = hip.Context(gm, max(b for b, _ in shapes), S)
            try:
                for j, ((ids, lens), sl) in enumerate(zip(batches, sls)):
                    _assert_equal(_call(hip, ctx, "device", ids, lens, sl)[0], wants[j], f"{name}, unmerged batch {j}")
            finally:
                ctx.close()
        if name == "shared":
            res = _many_checked(hip, gm, batches, S, sls, 0, where="pinned")
            for j, (got, want) in enumerate(zip(res, wants)):
                _assert_equal(got, want, f"pinned, batch {j}")
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    osl = oracle.OracleShortlist(blob, m.V, m.V)
    gsls = [osl.generate(ids, lens) for ids, lens in batches]
    wants = [_want(oracle, om, ids, lens, sl) for (ids, lens), sl in zip(batches, gsls)]
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    try:
        for where in ("device", "pinned"):
            for mode in modes[:2] if where == "device" else modes[:1]:
                res = _many_checked(hip, gm, batches, S, [None] * len(batches), mode, where=where, gen=gen)
                for j, (got, want) in enumerate(zip(res, wants)):
                    _assert_equal(got, want, f"generated, {where}, mode {mode}, batch {j}")
    finally:
        gen.close()


# device lengths past the sub-batch's own row: in the first and the last sub-batch
PAST = [
    ("tiny11", 32, [(9, 8), (21, 31), (6, 17)], (0, 2, 5)),
    ("tiny11", 24, [(5, 3), (17, 12), (3, 23), (8, 2)], (0, 4)),
    ("tiny11", 48, [(7, 33), (5, 47), (9, 20)], (0, 2, 5)),
]


@pytest.mark.parametrize("preset,S,shapes,modes", PAST, ids=[_merged_id(c) for c in PAST])
def test_merged_device_lengths_past_the_row(hip, oracle, engines, preset, S, shapes, modes):
    """include/slimt_hip.h, slimt_hip_batch: a device length past the batch's own padded width S_j is S_j. The sentence
    equals the checker at length S_j (and its own unmerged translate_device call with the same length), every other
    sentence is unaffected, and nothing is written outside the batch's outputs -- shared, per-batch and generated lists."""
    from slimt_amd import synth
    m, gm, om = engines(preset)
    k = len(shapes)
    batches, clamped = [], []
    for j, (B, Sj) in enumerate(shapes):
        bad = {}
        if j in (0, k - 1):
            bad = {0: Sj + 1, B // 2: S, B - 1: 0xFFFFFFFF}  # (the last row: its alignment row ends the caller's array)
        ids, lens = _edge_batch(m.V, B, Sj, seed=60 + 5 * j + S, lens_at=bad)
        batches.append((ids, lens))
        clamped.append(np.minimum(lens, Sj).astype(np.uint32))
    forms = _forms(m, preset)
    for name in ("shared", "own"):
        sls = forms[name](k)
        wants = [_want(oracle, om, ids, cl, sl) for (ids, _), cl, sl in zip(batches, clamped, sls)]
        for mode in modes:
            res = _many_checked(hip, gm, batches, S, sls, mode)
            for j, (got, want) in enumerate(zip(res, wants)):
                _assert_equal(got, want, f"{name}, mode {mode}, batch {j} (S_j = {shapes[j][1]})")
        ctx = hip.Context(gm, max(b for b, _ in shapes), S)
        try:
            for j in (0, k - 1):
                ids, lens = batches[j]
                _assert_equal(_call(hip, ctx, "device", ids, lens, sls[j])[0], wants[j], f"{name}, unmerged batch {j}")
        finally:
            ctx.close()
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    osl = oracle.OracleShortlist(blob, m.V, m.V)
    gsls = [osl.generate(ids, cl) for (ids, _), cl in zip(batches, clamped)]
    wants = [_want(oracle, om, ids, cl, sl) for (ids, _), cl, sl in zip(batches, clamped, gsls)]
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    try:
        res = _many_checked(hip, gm, batches, S, [None] * k, modes[0], gen=gen)
        for j, (got, want) in enumerate(zip(res, wants)):
            _assert_equal(got, want, f"generated, batch {j}")
    finally:
        gen.close()


def test_merged_async_rejects_host_lengths_past_the_row(hip, oracle, engines):
    """slimt_hip_translate_many_async validates host lengths against each batch's own S_j: a non-zero status, every output
    and guard untouched, and the next call on the context succeeds."""
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    S, shapes = 32, [(9, 8), (21, 31), (6, 17)]
    sl = synth.make_shortlist(m.V, 1024, seed=5)
    good = [_edge_batch(m.V, B, Sj, seed=80 + j) for j, (B, Sj) in enumerate(shapes)]
    ctx = hip.Context(gm, hip.translate_many_rows([b for b, _ in shapes]), S)
    try:
        for j_bad in (0, len(shapes) - 1):
            per, host = [], []
            try:
                for j, (ids, lens) in enumerate(good):
                    B, Sj = ids.shape
                    lens = lens.copy()
                    if j == j_bad:
                        lens[B - 1] = Sj + 1
                    bufs = _Buffers(hip, "pinned")
                    per.append(bufs)
                    h = (bufs.inp(ids)[1], bufs.inp(lens)[1], bufs.out("out_ids", np.uint32, (B, _tmax(Sj)))[1],
                         bufs.out("out_len", np.uint32, (B,))[1], bufs.out("align", np.float32, (B, _tmax(Sj), Sj))[1])
                    host.append(h)
                with pytest.raises(hip.SlimtHipError):
                    ctx.translate_many_async(host, sl, LF, 0)
                ctx.synchronize()
                for bufs in per:
                    for name, a in bufs.check().items():
                        assert (a.view(np.uint32) == PAT).all(), f"batch {j_bad} rejected, but {name} was written"
            finally:
                for bufs in per:
                    bufs.free()
        res = _many(hip, gm, good, S, [sl] * len(good), 0, where="pinned", ctx=ctx)  # the same context
        for j, ((ids, lens), got) in enumerate(zip(good, res)):
            _assert_equal(got, _want(oracle, om, ids, lens, sl), f"after the rejected calls, batch {j}")
    finally:
        ctx.close()
