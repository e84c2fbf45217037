"""The queue-aware decoder plan on the GPU (slimt_amd/csrc/decoder_plan.h): eight contexts of one model translate
concurrently at the process's hardware-queue count, their batches in the tight (16-bit) K/V form the library
calibrates for itself. Whatever tiling each launch took, tokens, lengths and alignment rows equal the checker's; a
launch with the packed cache that found more contexts pending than there are queues took the 4-sentence tiling and
waited for no admission event."""
import threading

import numpy as np
import pytest


@pytest.mark.gpu
def test_concurrent_contexts_take_the_queue_bound_plan(hip, oracle, synth_models):
    from slimt_amd import synth
    m = synth_models("tiny11", 6.0)
    B, S, W, calls = 128, 24, 8, 3
    jobs = [synth.make_batch(m.V, B, S, seed=8800 + i, ragged=True) for i in range(W)]
    sl = synth.make_shortlist(m.V, 1024)
    om = oracle.OracleModel(m, threads=8)
    oracle.set_mode(oracle.PORTABLE)
    want = [om.translate(ids, lens, sl, 1.5, 0, want_align=True)[:3] for ids, lens in jobs]
    oracle.set_mode(oracle.FAITHFUL)
    gm = hip.Model(m)
    ctxs = [hip.Context(gm, B, S) for _ in range(W)]
    try:
        plans = [[] for _ in range(W)]
        bad, errors = [], []
        start = threading.Barrier(W)

        def work(w):
            try:
                start.wait()
                for it in range(calls):
                    got = ctxs[w].translate(jobs[w][0], jobs[w][1], sl, want_align=True)
                    # (forms: None while the batch's caches are all in one form -- the f32 batch the library calibrates
                    # the tight form's centres from -- else 2 per sentence-layer in the tight form)
                    f = ctxs[w].debug_kv_formats(m.dec_layers, B)
                    plans[w].append(dict(ctxs[w].debug_decoder_plan(), tight=f is not None and (f == 2).mean() >= 0.5))
                    if not all(np.array_equal(a, b) for a, b in zip(got, want[w])):
                        bad.append((w, it))
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
        assert sum(p["tight"] for p in flat) >= len(flat) // 2, flat  # (a sentence-layer that does not fit falls back)
        assert all(p["queues"] == queues for p in flat), (queues, flat)
        for p in flat:
            assert p["in_flight"] == min(p["contexts"], queues), p
            if p["contexts"] > queues and p["tight"]:  # queue-bound: 4 x 32 workgroups of 4 sentences fit the budget
                assert (p["rows"], p["n"], p["eighths"]) == (4, 0, 8 * m.dec_layers), p
            elif p["contexts"] <= queues:  # the budget's plan: the fewest sentences that fit 7/8 of the CUs, then waits
                assert p["rows"] in (4, 8, 16, 32) and p["n"] > 0, p
        if queues < W:  # the eight contexts met the queues at least once, in the tight form
            assert any(p["contexts"] > queues and p["tight"] for p in flat), flat
    finally:
        for c in ctxs:
            c.close()
        gm.close()
