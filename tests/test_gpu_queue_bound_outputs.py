"""Queue-bound decoder launches at the process's hardware-queue count (decoder_plan.h; engine.cpp spreads the context
streams evenly over the queues: level_hardware_queues). Eight contexts of one model translate concurrently, B = 256 and
B = 64 at S = 32, their K/V caches in the tight (16-bit) and in the 24-bit form: tokens, lengths and alignment rows of
every sentence equal the checker's, and a launch that found more contexts pending than there are queues took the
queue-bound plan and waited for no admission event. Then two of the contexts go on alone, and their launches wait for
admission events again -- the first of them for launches of the queue-bound phase."""
import threading
import time

import numpy as np
import pytest

W, S, CALLS = 8, 32, 4
_want = {}


def _jobs_and_want(oracle, synth_models, B):
    from slimt_amd import synth
    m = synth_models("tiny11", 6.0)
    if B not in _want:  # (the checker's results do not depend on the cache form: once per batch size)
        # (B = 256: four distinct batches, contexts w and w + 4 take the same one -- the checker needs 9 s for each)
        distinct = [synth.make_batch(m.V, B, S, seed=9900 + 16 * B + i, ragged=True) for i in range(4 if B > 64 else W)]
        jobs = [distinct[w % len(distinct)] for w in range(W)]
        sl = synth.make_shortlist(m.V, 1024)
        om = oracle.OracleModel(m, threads=8)
        oracle.set_mode(oracle.PORTABLE)
        want = [om.translate(ids, lens, sl, 1.5, 0, want_align=True)[:3] for ids, lens in distinct]
        want = [want[w % len(distinct)] for w in range(W)]
        oracle.set_mode(oracle.FAITHFUL)
        _want[B] = (jobs, sl, want)
    return (m,) + _want[B]


def _ask_for(form, m, gm):
    """The cache form, asked for explicitly on a model of the test's own: "16" = packed, the tight form tried first
    around 127 colsum; "24" = packed, 24 bits only."""
    if form == "24":
        gm.set_kv_cache_format(2)
        return
    centres = np.zeros((m.dec_layers, 2, m.D), dtype=np.int64)
    for l in range(m.dec_layers):
        for t, name in enumerate("kv"):
            Wm = np.ascontiguousarray(m.params[f"decoder_l{l + 1}_context_W{name}"].data).reshape(m.D, m.D)
            centres[l, t] = 127 * Wm.astype(np.int64).sum(axis=1)
    gm.set_kv_cache_format(0)
    gm.set_kv_centres(centres.astype(np.int32))
    gm.debug_kv_tight_limit(2 ** 15)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["16", "24"])
@pytest.mark.parametrize("B", [256, 64])
def test_queue_bound_launches_equal_the_checker(hip, oracle, synth_models, B, form):
    m, jobs, sl, want = _jobs_and_want(oracle, synth_models, B)
    gm = hip.Model(m)
    _ask_for(form, m, gm)
    ctxs = [hip.Context(gm, B, S) for _ in range(W)]
    try:
        plans = [[] for _ in range(W)]
        bad, errors = [], []
        start = threading.Barrier(W)

        def check(w, got, tag):
            for name, a, b in zip(("tokens", "lengths", "alignment"), got, want[w]):
                if not np.array_equal(a, b):
                    rows = np.unique(np.nonzero(np.asarray(a) != np.asarray(b))[0])[:8].tolist()
                    bad.append((w, tag, name, rows))

        def work(w):
            try:
                start.wait()
                for it in range(CALLS):
                    got = ctxs[w].translate(jobs[w][0], jobs[w][1], sl, want_align=True)
                    f = ctxs[w].debug_kv_formats(m.dec_layers, B)
                    plans[w].append(dict(ctxs[w].debug_decoder_plan(), tight=f is not None and (f == 2).mean() >= 0.5))
                    check(w, got, it)
            except Exception as e:  # (reported below, on the test's thread)
                errors.append((w, repr(e)))

        ts = [threading.Thread(target=work, args=(w,)) for w in range(W)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert not bad, bad
        queues = hip.lib().slimt_hip_hw_queues() or 4
        flat = [p for ps in plans for p in ps]
        if form == "16":
            assert sum(p["tight"] for p in flat) >= len(flat) // 2, flat  # (a sentence-layer that does not fit falls back)
        else:
            assert not any(p["tight"] for p in flat), flat
        for p in flat:
            assert p["queues"] == queues, (queues, p)
            assert p["in_flight"] == min(p["contexts"], queues), p
            assert p["rows"] in (4, 8, 16, 32), p
            if p["contexts"] > queues:  # queue-bound: the queues order the decoders, no admission wait
                assert p["n"] == 0 and p["eighths"] == 8 * m.dec_layers, p
            else:
                assert p["n"] > 0, p
        if queues < W:  # the eight contexts met the queues at least once
            assert any(p["contexts"] > queues and p["n"] == 0 for p in flat), flat
        # two contexts go on alone: once the others' launches are 25 ms old these wait for admission events again
        # (n > 0), the first ones for launches of the queue-bound phase
        waited = 0
        for it in range(CALLS):
            if it == 1:
                time.sleep(0.05)
            for w in (0, 1):
                check(w, ctxs[w].translate(jobs[w][0], jobs[w][1], sl, want_align=True), ("alone", it))
                p = ctxs[w].debug_decoder_plan()
                assert (p["n"] > 0) == (p["contexts"] <= queues), p
                waited += p["n"] > 0
        assert not bad, bad
        if queues >= 2:
            assert waited > 0
    finally:
        for c in ctxs:
            c.close()
        gm.close()
