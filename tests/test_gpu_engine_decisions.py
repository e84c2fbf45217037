"""What the engine decides for a call, and what the call then produces, against a fixture recorded before
translate_device became a sequence of stages (tests/golden/engine_decisions.json): a table of single-context cases at the
smallest shapes at which each launch decision can flip -- the K/V slot predicates and the mid / long borders (S), tile remainders (B), the
calibration batch and the tight form behind it, decode modes, K/V formats, the decoder budget, listed / generated / no
shortlists, a merged launch, and one case per per-call option. Per case: ctx.plan(S); after each call the decoder's plan
(without the process's queue count), the K/V forms recorded, both watches, and a CRC of every output; then the launches
per SLIMT_HIP_K_* family. Equality, no tolerance: the engine's code may move, its decisions and results may not.
One family is counted at a time, so the launch counts come from nine more runs of the case's call on the same context,
behind the observed ones: in a two-call case they are those of the later state (after the calibration: the packed or
tight form), not of the first call.

The last test is of another kind: slimt_hip_translate_many_async with SLIMT_MERGE_DENSE=0, in a child process (the variable
is read once per process), where the merge plan's tile-aligned rows exceed the workspace although the batches' sum fits.

`python tests/test_gpu_engine_decisions.py --record FILE` writes the table's records (how the fixture was made, at the
commit before the stages; the recorder uses nothing but slimt_amd.capi and slimt_amd.synth)."""
import json
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_decisions.json")

pytestmark = pytest.mark.gpu

# (D, F, H, Le, Ld, V): the tiny11 and base shapes with the vocabulary cut to 4,096 (model creation and the output layer stay
# small; ctx.plan() is recorded, so a shape the persistent kernels stopped accepting would show), mini for the stage-wise
# path, and tiny11 with all 32,000 columns for the 32-sentence tiling
SHAPES = {
    "tiny11": (256, 1536, 8, 6, 2, 4096),
    "base": (512, 2048, 8, 6, 2, 4096),
    "mini": (128, 256, 8, 2, 2, 2048),
    "tiny11_full": (256, 1536, 8, 6, 2, 32000),
}
_MODELS = {}


def host_model(shape):
    from slimt_amd import synth
    if shape not in _MODELS:
        _MODELS[shape] = synth.make_model(dims=SHAPES[shape], eos_bias=6.0)  # eos_bias 6: sentences end at different steps
    return _MODELS[shape]


def case(name, shape="tiny11", B=17, S=12, n_sl=512, kind="pinned", calls=1, mode=None, fmt=None, budget=None, **opt):
    return dict(name=name, shape=shape, B=B, S=S, n_sl=n_sl, kind=kind, calls=calls, mode=mode, fmt=fmt, budget=budget, opt=opt)


CASES = (
    # sentence lengths: the 24-bit slot misses S = 5, the 20-bit one S = 4 and 12; 32 | 33 and 64 | 65 are the mid / long borders
    # (from S = 64 on 17 sentences are 1024 rows: the first call is the calibration batch, the second takes the packed forms)
    [case("tiny11_S%d" % S, S=S, calls=2 if S >= 64 else 1) for S in (4, 5, 8, 12, 32, 33, 64, 65, 128)]
    # (base, D = 512: the packed forms end at S = 32; 33 is the per-stage encoder in front of the persistent decoder)
    + [case("base_S%d" % S, shape="base", S=S) for S in (4, 5, 8, 12, 32, 33)]
    # batch sizes: one sentence, a tile and a remainder (17, above), whole tiles
    + [case("tiny11_B%d" % B, B=B) for B in (1, 64)]
    # B * S >= 1024, twice with a synchronize between: the calibration batch (cached as f32), then the tight form
    + [case("tiny11_calibrate_then_tight", B=64, S=32, calls=2)]
    + [case("mini_stagewise", shape="mini")]
    # all 32,000 columns: the 32-sentence tiling, and expect_large_output for the call behind it
    + [case("tiny11_full_vocabulary_twice", shape="tiny11_full", B=64, n_sl=0, calls=2)]
    + [case("tiny11_mode%d" % mode, B=64, mode=mode) for mode in range(1, 7)]
    + [case("tiny11_kv_format%d" % fmt, S=32, fmt=fmt) for fmt in (1, 2, 3)]
    + [case("tiny11_budget0", budget=0), case("tiny11_budget224", budget=224)]
    + [case("tiny11_no_shortlist", n_sl=0)]
    + [case("tiny11_generated_shortlist", kind="generated")]
    + [case("tiny11_merged_two_lengths", kind="merged")]
    + [case("tiny11_scored", kind="host", scores=True),
       case("tiny11_forced_prefix", kind="host", prefix=True),
       case("tiny11_sampled", kind="host", sampling=True),
       case("tiny11_truncated", kind="host", sampling=True, truncation=(8, 0.9)),
       case("tiny11_fanout_consensus", kind="fanout"),
       case("tiny11_beam2", kind="beam")]
)


def crc(*arrays):
    c = 0
    for a in arrays:
        if a is not None:
            c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


def make_call(hip, ctx, m, k):
    """The case's call as a function without arguments: it returns the CRC of everything the call wrote."""
    from slimt_amd import synth
    B, S, opt = k["B"], k["S"], k["opt"]
    ids, lens = synth.make_batch(m.V, B, S, seed=100 * S + B, ragged=True)
    sl = synth.make_shortlist(m.V, k["n_sl"]) if k["n_sl"] else None
    T = max(int(np.float32(1.5) * np.float32(S)), 1)
    if k["kind"] == "pinned":
        return lambda: crc(*ctx.translate_pinned(ids, lens, sl, want_align=True))
    if k["kind"] == "generated":
        gen = hip.ShortlistGenerator(synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1), m.V, m.V)
        return lambda: crc(*ctx.translate_pinned(ids, lens, want_align=True, generator=gen))
    if k["kind"] == "merged":  # two batches padded to different lengths S_j, one launch pair
        bufs, pins = [], []
        for j, (Bj, Sj) in enumerate(((B, S), (B - 6, S - 4))):
            bi, bl = synth.make_batch(m.V, Bj, Sj, seed=300 + j, ragged=True)
            Tj = max(int(np.float32(1.5) * np.float32(Sj)), 1)
            ps = [hip._Pinned() for _ in range(5)]
            pins += ps
            b = (ps[0].array(np.uint32, (Bj, Sj)), ps[1].array(np.uint32, (Bj,)), ps[2].array(np.uint32, (Bj, Tj)),
                 ps[3].array(np.uint32, (Bj,)), ps[4].array(np.float32, (Bj, Tj, Sj)))
            b[0][...], b[1][...] = bi, bl
            bufs.append(b)

        def merged():
            for b in bufs:
                b[2][...], b[3][...], b[4][...] = 0, 0, 0
            ctx.translate_many_async(bufs, sl)
            ctx.synchronize()
            return crc(*[a for b in bufs for a in b[2:]])
        merged.keep = pins
        return merged
    if k["kind"] == "fanout":  # two sampled rows per source, the consensus pick among them
        row_src = np.repeat(np.arange(B, dtype=np.uint32), 2)
        keys = hip.sampling_keys(7, row_src.size)
        return lambda: crc(*ctx.translate_fanout(ids, lens, row_src, sl, want_align=True, scores=True, sampling=(0.8, keys),
                                                 consensus=(4, 4)))
    if k["kind"] == "beam":
        return lambda: crc(*ctx.translate_beam(ids, lens, 2, sl, want_align=True))
    kw = {}
    if opt.get("scores"):
        kw["scores"] = True
    if opt.get("prefix"):
        pre = np.zeros((B, T), dtype=np.uint32)
        pre[:, :2] = np.asarray(sl if sl is not None else np.arange(m.V), dtype=np.uint32)[np.arange(2 * B).reshape(B, 2) % 64 + 2]
        kw["prefix"] = (pre, np.arange(B, dtype=np.uint32) % 3)
    if opt.get("sampling"):
        kw["sampling"] = (0.8, hip.sampling_keys(11, B))
    if opt.get("truncation"):
        kw["truncation"] = opt["truncation"]
    return lambda: crc(*ctx.translate(ids, lens, sl, want_align=True, **kw))


def ctx_rows(B):
    return 2 * B  # a fan-out context is made for this many rows (max_batch bounds N)


def observe(ctx, gm, m, k, out_crc):
    plan = ctx.debug_decoder_plan()
    plan.pop("queues")  # (the process's hardware queues: the machine's, not the engine's decision)
    fmts = ctx.debug_kv_formats(m.dec_layers, ctx_rows(k["B"]))
    return dict(crc=out_crc, decoder_plan=plan, kv_formats=None if fmts is None else np.bincount(fmts.ravel(), minlength=4).tolist(),
                kv_watch=list(gm.debug_kv_watch()), kv_tight_watch=list(gm.debug_kv_tight_watch()))


def run_case(hip, k):
    """One model, one context: the case's calls with nothing profiled and everything observed after each, then the same call
    once per kernel family for the launch counts (one family is counted at a time)."""
    m = host_model(k["shape"])
    gm = hip.Model(m, device=0)
    ctx = hip.Context(gm, ctx_rows(k["B"]), k["S"])
    try:
        if k["fmt"] is not None:
            gm.set_kv_cache_format(k["fmt"])
        if k["budget"] is not None:
            gm.set_decoder_budget(k["budget"])
        if k["mode"] is not None:
            ctx.set_decode_mode(k["mode"])
        rec = dict(plan_S=list(ctx.plan(k["S"])), calls=[])
        call = make_call(hip, ctx, m, k)
        for _ in range(k["calls"]):
            out_crc = call()
            ctx.synchronize()
            rec["calls"].append(observe(ctx, gm, m, k, out_crc))
        launches = {}
        for family in range(1, 10):  # SLIMT_HIP_K_GEMM_ENC .. SLIMT_HIP_K_CONSENSUS
            ctx.profile_enable(family)
            call()
            ctx.synchronize()
            launches[str(family)] = int(ctx.profile_read()["launches"])
        ctx.profile_enable(0)
        rec["launches"] = launches
        return rec
    finally:
        ctx.close()
        gm.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_table_and_fixture_name_the_same_cases(golden):
    assert sorted(golden) == sorted(k["name"] for k in CASES)


@pytest.mark.parametrize("k", CASES, ids=[k["name"] for k in CASES])
def test_decisions_and_results_equal_the_recorded_ones(hip, golden, k):
    got = json.loads(json.dumps(run_case(hip, k)))  # (as the fixture was written: lists, string keys)
    assert got == golden[k["name"]]


def merge_dense_off_probe(hip):
    """In a process started with SLIMT_MERGE_DENSE=0: two pinned batches with one shortlist on a context of max_batch 70.
    17 + 17 sentences are 64 tile-aligned rows: one merged launch pair. 33 + 33 are 66 rows densely -- the check in front of
    the merge plan passes -- and 128 aligned ones: the check behind the plan sends the call batch by batch. Either way every
    batch equals its own translate call. Returns the persistent decoder's launches of the two calls and that equality."""
    from slimt_amd import synth
    m = host_model("tiny11")
    gm = hip.Model(m, device=0)
    ctx = hip.Context(gm, 70, 12)
    sl = synth.make_shortlist(m.V, 512)
    out = {}
    try:
        for name, sizes in (("fits", (17, 17)), ("exceeds", (33, 33))):
            bufs, pins, alone = [], [], []
            for j, (Bj, Sj) in enumerate(zip(sizes, (12, 8))):
                bi, bl = synth.make_batch(m.V, Bj, Sj, seed=500 + j, ragged=True)
                alone.append(ctx.translate_pinned(bi, bl, sl, want_align=True))
                Tj = max(int(np.float32(1.5) * np.float32(Sj)), 1)
                ps = [hip._Pinned() for _ in range(5)]
                pins += ps
                b = (ps[0].array(np.uint32, (Bj, Sj)), ps[1].array(np.uint32, (Bj,)), ps[2].array(np.uint32, (Bj, Tj)),
                     ps[3].array(np.uint32, (Bj,)), ps[4].array(np.float32, (Bj, Tj, Sj)))
                b[0][...], b[1][...], b[2][...], b[3][...], b[4][...] = bi, bl, 0, 0, 0
                bufs.append(b)
            ctx.profile_enable(hip.K_DECODE_FUSED)
            ctx.translate_many_async(bufs, sl)
            ctx.synchronize()
            launches = int(ctx.profile_read()["launches"])
            ctx.profile_enable(hip.K_NONE)
            equal = all(np.array_equal(b[2], a[0]) and np.array_equal(b[3], a[1]) and np.array_equal(b[4], a[2])
                        for b, a in zip(bufs, alone))
            out[name] = dict(launches=launches, equal=bool(equal))
        return out
    finally:
        ctx.close()
        gm.close()


def test_merge_plan_rows_are_checked_against_the_workspace_again():
    """(The capacity check of slimt_hip_translate_many_async behind build_merge_plan; without it the 128-row launch would
    be queued on a workspace of 70.)"""
    import subprocess
    env = dict(os.environ, SLIMT_MERGE_DENSE="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--merge-dense-off"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == {"fits": {"launches": 1, "equal": True}, "exceeds": {"launches": 2, "equal": True}}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from slimt_amd import capi
    if sys.argv[1] == "--merge-dense-off":
        assert os.environ.get("SLIMT_MERGE_DENSE") == "0"
        print(json.dumps(merge_dense_off_probe(capi)))
        sys.exit(0)
    assert sys.argv[1] == "--record", sys.argv
    records = {}
    for k_ in CASES:
        records[k_["name"]] = run_case(capi, k_)
        print(k_["name"], json.dumps(records[k_["name"]]), flush=True)
    with open(sys.argv[2], "w") as fh:  # one line per case
        fh.write("{\n" + ",\n".join(json.dumps(n) + ": " + json.dumps(records[n], sort_keys=True) for n in sorted(records)) + "\n}\n")
