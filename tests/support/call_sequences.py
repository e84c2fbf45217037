"""A catalogue of calls and of call sequences on ONE long-lived context (tests/test_gpu_call_sequences.py runs them on the
GPU, tests/test_call_sequence_fixtures.py proves on the CPU that they can catch what they are for).

A *call* is a small record: a name, a kind (its entry point), a shape, a seed and options. `run(call, hip, ctx, env)`
makes the call on `ctx` with every destination pre-filled with PAT and returns every output as {name: array}; a region the
call must not write is then part of the comparison. `oracle_expected(call, env)` gives, per output, what the CPU oracle
(PORTABLE order) and the checkers of the features' own test files say: ("exact", array) -- compared as bits --,
("approx", float64 array, tolerance) -- the output has no bit-exact checker: its expected BITS are the call on a fresh
model and a fresh context, and that fresh result is held against the float64 array within the project's tolerance --, or
None -- no oracle function at all (fresh model and context only).

A *sequence* is a hand-written list of call names and setters ("@mode:N", "@rows:N", "@kv:N") on one model and one context,
aimed at one piece of the state a context or a model carries from call to call; STATE_COVERAGE says which.
"""
import ctypes as C

import numpy as np

PAT = 0xA5A5A5A5
LF = 1.5
TOL = 5e-5  # the project's bound for scores against a float64 checker (tests/test_gpu_forced_prefix.py)
CTX_SHAPE = (70, 128)  # the largest B of the catalogue and the largest S a context takes: every sequence's context
ORACLE_THREADS = 16
EOS_BIAS = 6.0  # sentences end at different steps
GEN = dict(frequent=100, best=2, seed=21, empty_fraction=0.3, min_count=1)  # the lexical shortlist of the generated calls


def tmax(S):
    return max(int(np.float32(LF) * np.float32(S)), 1)


# ---- the calls ------------------------------------------------------------------------------------------------------------

class Call:
    def __init__(self, name, kind, B, S, seed, **opt):
        self.name, self.kind, self.B, self.S, self.seed, self.opt = name, kind, B, S, seed, opt

    def __repr__(self):
        return self.name


def _t(name, B, S, seed, entry="host", sl="A", **opt):
    return Call(name, "translate", B, S, seed, entry=entry, sl=sl, **opt)


PROBE = dict(B=70, S=12, seed=7001)  # several decoder tiles and a partly filled last one (70 = 4 x 16 + 6)
MERGED_SUBS = ((9, 8, 7101), (21, 12, 7102), (6, 5, 7103))  # 16 + 32 + 16 rows of the context's 70: one merged launch
FALLBACK_SUBS = ((20, 8, 7111), (20, 12, 7112), (20, 5, 7113))  # 96 rows: more than the context holds, batch by batch

_CALLS = [
    # translate: host shortlists, the full vocabulary, alignment on and off
    _t("probe", **PROBE, align=True),
    _t("tr_A", 21, 13, 7002, align=True),
    _t("tr_A2", 21, 13, 7002, sl="A2", align=True),
    _t("tr_B", 21, 13, 7002, sl="B", align=True),
    _t("tr_full", 21, 13, 7002, sl=None, align=True),
    _t("tr_A_noalign", 21, 13, 7002),
    _t("tr_gen", 21, 13, 7002, entry="generated", sl="gen", align=True),
    _t("tr_dev_B", 21, 13, 7002, entry="device", sl="B", align=True),
    _t("tr_dev_gen", 17, 16, 7003, entry="device_generated", sl="gen", align=True),
    _t("tr_pinned", 17, 16, 7003, entry="pinned", align=True),
    _t("tr_pinned_gen", 21, 13, 7002, entry="pinned_generated", sl="gen", align=True),
    # the output layer's memory: 32000 columns against 1024 (S <= 32)
    _t("out_full", 37, 32, 7004, entry="device", sl=None, align=True),
    _t("out_1024", 37, 32, 7004, entry="device", sl="S1024", align=True),
    # the packed cache's forms: batch sizes 37 / 5 / 64, S on both sides of the narrow form's exclusions
    _t("kv_37x32", 37, 32, 7005, entry="device", align=True),
    _t("kv_5x4", 5, 4, 7006, entry="device", align=True),
    _t("kv_64x8", 64, 8, 7007, entry="device", align=True),
    _t("kv_37x12", 37, 12, 7008, entry="device", align=True),
    _t("kv_37x13", 37, 13, 7009, entry="device", align=True),
    # the encoders and decoders: every S where the code takes another path; three long sentences
    _t("enc_32", 9, 32, 7010, entry="device", align=True),
    _t("enc_40", 7, 40, 7011, entry="device", align=True),
    _t("enc_64", 5, 64, 7012, entry="device", align=True),
    _t("enc_65", 3, 65, 7013, entry="device", align=True),
    _t("enc_128", 3, 128, 7014, entry="device", align=True),
    # (one token more than any context takes: refused, with an error and every destination as it was)
    _t("enc_129", 3, 129, 7015, entry="device", align=True, refused=True),
    _t("enc_5", 11, 5, 7016, entry="device", align=True),
    # options: scores + prefix + sampling; truncated sampling at two B x n_shortlist sizes
    _t("tr_scored", 21, 13, 7017, align=True, scores=True),
    _t("tr_opts", 13, 12, 7018, align=True, scores=True, prefix=True, sampling=0.7),
    _t("trunc_8x520", 8, 8, 7019, sl="S520", align=True, scores=True, sampling=1.0, trunc=(40, 0.9)),
    _t("trunc_40x4096", 40, 8, 7020, sl="S4096", align=True, scores=True, sampling=1.0, trunc=(40, 0.9)),
    # asynchronous calls on pinned arrays (sequence 8 queues them)
    _t("as_scored", 19, 10, 7021, entry="pinned", align=True, scores=True),
    _t("as_prefix", 9, 24, 7022, entry="pinned", sl="B", align=True, scores=True, prefix=True),
    _t("as_sampled", 33, 6, 7023, entry="pinned", sl="S4096", scores=True, sampling=1.0),
    # merged launches
    Call("many_dev", "many", 0, 12, 0, where="device", subs=MERGED_SUBS, sls="shared"),
    Call("many_own", "many", 0, 12, 0, where="device", subs=MERGED_SUBS, sls="own"),
    Call("many_gen", "many", 0, 12, 0, where="device", subs=MERGED_SUBS, sls="gen"),
    Call("many_pinned", "many", 0, 12, 0, where="pinned", subs=MERGED_SUBS, sls="shared"),
    Call("many_pinned_gen", "many", 0, 12, 0, where="pinned", subs=MERGED_SUBS, sls="gen"),
    Call("many_fallback", "many", 0, 12, 0, where="device", subs=FALLBACK_SUBS, sls="shared"),
    # fan-out: pageable, pinned, device; once with the consensus armed
    Call("fo_host", "fanout", 5, 9, 7030, where="host", counts=(3, 1, 0, 4, 2), sampling=1.0),
    Call("fo_pinned", "fanout", 5, 9, 7031, where="pinned", counts=(1, 2, 3, 2, 1), sampling=0.7),
    Call("fo_device", "fanout", 4, 7, 7032, where="device", counts=(2, 2, 1, 3), sampling=None),
    Call("fo_consensus", "fanout", 6, 8, 7033, where="host", counts=(4, 3, 5, 1, 0, 4), sampling=1.0, consensus=(4, 4)),
    # the one-pass scorer: short and long T, alternatives on pageable destinations, candidates at two N
    Call("sc_short", "score", 5, 13, 7040, T=4, alt=0),
    Call("sc_long", "score", 5, 13, 7041, T=27, alt=0),
    Call("sc_alt_short", "score", 4, 9, 7042, T=3, alt=5),
    Call("sc_alt_long", "score", 4, 9, 7043, T=21, alt=8),
    Call("cand_small", "candidates", 4, 7, 7044, T=6, counts=(2, 1, 0, 3)),
    Call("cand_large", "candidates", 4, 7, 7045, T=9, counts=(17, 20, 1, 25)),
    # the step-wise API and the cross-attention diagnostic
    Call("step_a", "stepwise", 6, 9, 7050, steps=2),
    Call("step_b", "stepwise", 4, 11, 7051, steps=2),
    Call("step_more", "refused_step", 6, 9, 7050),
    Call("begin_again", "refused_begin", 6, 9, 7050),
    Call("xattn", "xattn", 5, 10, 7052),
    # slimt_hip_debug_kv_formats: did the LAST batch's encoder record the forms of a packed cache (kv_fmt_valid)?
    Call("kv_some", "kv_forms", 0, 0, 0, want=1),
    Call("kv_none", "kv_forms", 0, 0, 0, want=0),
]
CALLS = {c.name: c for c in _CALLS}
assert len(CALLS) == len(_CALLS)

# the kinds whose launches take tiles by ticket, by the launcher in engine.cpp that they reach (sequence 7)
TICKETED = ("tr_A", "tr_full", "tr_gen", "tr_dev_gen", "tr_pinned", "enc_40", "enc_64", "many_dev", "many_gen", "many_pinned",
            "many_pinned_gen", "many_fallback", "fo_host", "fo_pinned", "fo_device", "fo_consensus", "tr_opts", "trunc_8x520",
            "tr_A_noalign", "sc_short", "cand_small", "step_a")

# ---- the sequences --------------------------------------------------------------------------------------------------------
SEQUENCES = {}
SEQUENCE_DOC = {}
STATE_COVERAGE = {}  # state item -> the sequences that aim at it


def _seq(name, covers, doc, items):
    SEQUENCES[name] = tuple(items)
    SEQUENCE_DOC[name] = doc
    for s in covers:
        STATE_COVERAGE.setdefault(s, []).append(name)


_seq("shortlist_cache", ("sl_host", "shortlist"),
     """The host shortlist cache (sl_host: re-uploaded only when it changes): everything that overwrites ctx->shortlist
     between two host calls with list A, then A', of A's size and different only in its last id.""",
     ["tr_A", "tr_gen", "tr_A", "tr_dev_B", "tr_A", "step_b", "tr_A", "many_gen", "tr_A", "many_own", "tr_A", "tr_A2",
      "tr_full", "tr_A", "tr_pinned_gen", "tr_A", "tr_B", "tr_A2", "tr_A"])
_seq("output_layer", ("expect_large_output", "n_sl", "out_sl", "kv_tight"),
     """The last decoder launch's column count picks the next encoder's tiling and tight reader: full vocabulary (32000
     columns) and a 1024-entry list at S = 32 in mode 0, in turn.""",
     ["@mode:0", "out_full", "out_1024", "out_full", "out_1024"])
_seq("cache_forms", ("kv_fmt_valid", "kv_fmt_B", "kv_tight", "kv_gen", "kv_auto_wide", "kv_tight_off", "kv_call_seq"),
     """kv_fmt_valid / kv_fmt_B / kv_tight describe the LAST batch's packed-cache forms: batch sizes 37 -> 5 -> 64 -> 37, S on
     both sides of the narrow form's exclusions (4, 8, 12, 13, 32), the cache format stepped 0 -> 1 -> 2 -> 0.""",
     ["kv_37x32", "kv_5x4", "kv_64x8", "kv_37x12", "@kv:1", "kv_37x13", "kv_none", "kv_5x4", "@kv:2", "kv_64x8", "kv_37x32", "@kv:0",
      "kv_37x13", "kv_5x4", "kv_37x12", "kv_64x8", "kv_37x32"])
_seq("encoder_decoder_variants", ("decode_mode", "encode_rows", "kv_ready", "have_encoder_out", "decode_ready", "kv_fmt_valid"),
     """Every encoder (S = 32, 40, 64, 65, 128, 129, 5; rows 0 / 32 / 64) and decoder (modes 0..5) on one context, the
     step-wise mode 1 directly before and after fused ones: ctx->kv changes between f32 and packed under one pointer. The
     per-stage encoder of mode 1 records no cache forms: the forms of the packed batch before it must not be reported
     for its batch (kv_fmt_valid is reset by encode_device itself, the per-stage path assigns it nowhere).""",
     ["@mode:0", "enc_32", "kv_some", "@mode:1", "enc_40", "kv_none", "@mode:2", "enc_64", "@rows:32", "enc_40", "@mode:1", "enc_65", "@mode:3",
      "enc_32", "@rows:64", "enc_64", "@mode:4", "enc_128", "@mode:1", "enc_129", "@mode:5", "enc_5", "@rows:0", "enc_65",
      "@mode:1", "enc_5", "@mode:0", "enc_128", "enc_40", "@mode:1", "enc_32", "@mode:0", "enc_129"])
_seq("stepwise_between_translates", ("have_encoder_out", "decode_ready", "kv_ready", "logits", "attn_dbg"),
     """The step-wise API around a translate call: a decode_step and a decode_begin behind it, with no new encode, are
     refused (the translate path keeps neither the encoder output nor the step-wise decoder's state); a new round equals
     the first.""",
     ["step_a", "tr_A", "step_more", "begin_again", "step_a", "xattn", "tr_dev_B", "step_more", "step_a"])
_seq("growing_workspaces", ("score_ws", "score_io", "cand_align", "cand_rank", "alt_stage", "tr_logits", "align", "logits",
                            "attn_dbg", "fo_stage", "cs_stage", "fp_stage", "sm_stage", "sc_stage", "shortlist"),
     """Every workspace that grows lazily: small, then large, then small again, with other kinds in between.""",
     ["sc_short", "tr_A", "sc_long", "sc_short", "cand_small", "cand_large", "cand_small", "sc_alt_short", "sc_alt_long",
      "sc_alt_short", "trunc_8x520", "trunc_40x4096", "trunc_8x520", "fo_consensus", "tr_A", "fo_host", "tr_opts",
      "fo_consensus", "tr_scored", "tr_opts", "many_gen", "xattn", "step_b", "sc_long"])
_seq("launch_bookkeeping", ("ticket_base", "enc_ticket_base", "xarr_base", "xclaim_base", "gen_epoch", "gen_flag"),
     """One call of every kind that launches a ticketed kernel, the same B = 70 probe after each: a base advanced by
     anything but the launch's real grid shows as untouched pattern rows or wrong rows in the probe.""",
     [x for name in TICKETED for x in (name, "probe")])
_seq("queued_async", ("sc_stage", "fp_stage", "sm_stage", "gate_*"),
     """Four asynchronous calls of different kinds and shapes queued with ONE synchronize at the end: staging buffers are
     reused while the call before is still in the stream.""",
     ["<queue", "as_scored", "as_prefix", "as_sampled", "many_pinned", ">queue", "tr_A"])

SHUFFLE_SEEDS = (11, 22, 33)
SHUFFLE_LENGTH = 25
NOT_SHUFFLED = ("step_more", "begin_again", "kv_some", "kv_none")  # (they mean something only behind a certain call)


def shuffle(seed):
    names = sorted(n for n in CALLS if n not in NOT_SHUFFLED)
    r = np.random.default_rng(seed)
    return tuple(names[i] for i in r.integers(0, len(names), size=SHUFFLE_LENGTH))


for _s in SHUFFLE_SEEDS:
    _seq("shuffle_%d" % _s, (), "25 calls drawn from the whole catalogue: the transitions nobody thought of.", shuffle(_s))

HAND_WRITTEN = [n for n in SEQUENCES if not n.startswith("shuffle_")]
BASE_SEQUENCES = ("shortlist_cache", "cache_forms", "launch_bookkeeping")  # D = 512 as well: encode_wide, other cache-form rules
STATE_ITEMS = ("sl_host", "kv_fmt_valid", "kv_fmt_B", "kv_tight", "kv_gen", "expect_large_output", "kv_ready",
               "have_encoder_out", "decode_ready", "n_sl", "out_sl", "decode_mode", "encode_rows", "ticket_base",
               "enc_ticket_base", "xarr_base", "xclaim_base", "gen_epoch", "gen_flag", "score_ws", "score_io", "cand_align",
               "cand_rank", "alt_stage", "tr_logits", "align", "logits", "attn_dbg", "fo_stage", "cs_stage", "fp_stage",
               "sm_stage", "sc_stage", "shortlist", "kv_auto_wide", "kv_tight_off", "kv_call_seq", "gate_*")


def calls_of(seq):
    return [x for x in SEQUENCES[seq] if x[0] not in "@<>"]


# ---- the environment: one model and what every call of it shares ------------------------------------------------------------

class Env:
    """One synthetic model with its oracle, its shortlists and its inputs; with `hip` the device model and generator."""

    def __init__(self, preset, oracle, synth_models, hip=None, share=None):
        """share: another Env of the preset -- its oracle objects, lists and expected results are used, not built again."""
        from slimt_amd import synth
        self.preset, self.oracle, self.hip = preset, oracle, hip
        self.m = synth_models(preset, EOS_BIAS)
        self.V = self.m.V
        if share is not None:
            assert share.preset == preset
            self.om, self.blob, self.osl, self._sl, self._exp = share.om, share.blob, share.osl, share._sl, share._exp
        else:
            self.om = oracle.OracleModel(self.m, threads=ORACLE_THREADS)
            self.blob = synth.make_lexical_shortlist(self.V, self.V, GEN["frequent"], GEN["best"], seed=GEN["seed"],
                                                     empty_fraction=GEN["empty_fraction"], min_count=GEN["min_count"])
            self.osl = oracle.OracleShortlist(self.blob, self.V, self.V)
            self._sl, self._exp = {}, {}
        self.gm = self.gen = None
        if hip is not None:
            self.gm = hip.Model(self.m)
            self.gen = hip.ShortlistGenerator(self.blob, self.V, self.V)

    def close(self):
        if self.gen is not None:
            self.gen.close()
        if self.gm is not None:
            self.gm.set_kv_cache_format(0)
            self.gm.close()
        self.gm = self.gen = None

    def batch(self, B, S, seed):
        from slimt_amd import synth
        return synth.make_batch(self.V, B, S, seed=seed, ragged=True)

    def translate(self, ids, lens, sl):
        O = self.oracle
        O.set_mode(O.PORTABLE)
        try:
            return self.om.translate(ids, lens, sl, LF, 0, want_align=True)[:3]
        finally:
            O.set_mode(O.FAITHFUL)

    def shortlist(self, name):
        """None: the full vocabulary. S<n>: n ids. B: another list. A: a list whose LAST id the translation of the batch of
        `tr_A` emits -- the ids of S1024 up to the largest emitted one (ids a greedy translation never emits can be taken
        out of its list without changing it) --, and A2: A with that last id replaced by the next free one."""
        from slimt_amd import synth
        if name is None:
            return None
        if name not in self._sl:
            if name[0] == "S":
                self._sl[name] = synth.make_shortlist(self.V, int(name[1:]), seed=5)
            elif name == "B":
                self._sl[name] = synth.make_shortlist(self.V, 1016, seed=6)
            else:
                c = CALLS["tr_A"]
                s0 = self.shortlist("S1024")
                out, ln, _ = self.translate(*self.batch(c.B, c.S, c.seed), s0)
                emitted = np.unique(np.concatenate([out[b, :ln[b]] for b in range(c.B)]))
                last = int(emitted.max())
                keep = s0[s0 < last]
                spare = keep[~np.isin(keep, emitted)]
                drop = spare[::-1][:(keep.size + 1) % 8]  # the size stays a multiple of 8, like every list's
                a = np.concatenate([keep[~np.isin(keep, drop)], [last]]).astype(np.uint32)
                assert a.size % 8 == 0 and a.size > 256 and (np.diff(a.astype(np.int64)) > 0).all()
                a2 = a.copy()
                a2[-1] = last + 1
                assert last + 1 < self.V
                self._sl["A"], self._sl["A2"] = a, a2
        return self._sl[name]


# ---- inputs of a call (the same on the oracle's side and the device's) ------------------------------------------------------

def _keys(call, n):
    return (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(call.seed)).astype(np.uint64)


def _prefix(call, env, sl, B, T):
    r = np.random.default_rng(call.seed + 1)
    pool = np.arange(2, env.V, dtype=np.uint32) if sl is None else sl[sl >= 2]
    p_ids = r.choice(pool, size=(B, T)).astype(np.uint32)
    p_len = r.integers(0, min(T, 4) + 1, size=B).astype(np.uint32)
    p_len[0] = 0
    return p_ids, p_len


def _row_src(counts):
    return np.repeat(np.arange(len(counts), dtype=np.uint32), counts)


def _targets(call, env, sl, N, T):
    r = np.random.default_rng(call.seed + 2)
    pool = np.arange(env.V, dtype=np.uint32) if sl is None else sl
    t_ids = r.choice(pool, size=(N, T)).astype(np.uint32)
    t_len = r.integers(0, T + 1, size=N).astype(np.uint32)
    t_len[0] = T
    return t_ids, t_len


def inputs(call, env):
    """Everything the call reads, as host arrays."""
    k, o = call.kind, call.opt
    if k == "many":
        subs = [env.batch(B, S, seed) for B, S, seed in o["subs"]]
        if o["sls"] == "shared":
            sls = [env.shortlist("A")] * len(subs)
        elif o["sls"] == "own":
            sls = [env.shortlist(n) for n in ("A", "B", "S520")][:len(subs)]
        else:
            sls = [env.osl.generate(ids, lens) for ids, lens in subs]
        return dict(subs=subs, sls=sls)
    if k == "kv_forms":
        return {}
    ids, lens = env.batch(call.B, call.S, call.seed)
    d = dict(ids=ids, lens=lens)
    if k == "translate":
        d["sl"] = env.osl.generate(ids, lens) if o["sl"] == "gen" else env.shortlist(o["sl"])
        if o.get("sampling") is not None:
            d["keys"] = _keys(call, call.B)
        if o.get("prefix"):
            d["p_ids"], d["p_len"] = _prefix(call, env, d["sl"], call.B, tmax(call.S))
    elif k == "fanout":
        d["sl"] = env.shortlist("S4096")
        d["row_src"] = _row_src(o["counts"])
        d["keys"] = _keys(call, d["row_src"].size)
    elif k == "score":
        d["sl"] = env.shortlist("A")
        d["t_ids"], d["t_len"] = _targets(call, env, d["sl"], call.B, o["T"])
    elif k == "candidates":
        d["sl"] = env.shortlist("A")
        d["cand_src"] = _row_src(o["counts"])
        d["t_ids"], d["t_len"] = _targets(call, env, d["sl"], d["cand_src"].size, o["T"])
    elif k in ("stepwise", "refused_step", "refused_begin", "xattn"):
        d["sl"] = env.shortlist("B")
        r = np.random.default_rng(call.seed + 3)
        d["prev"] = r.choice(d["sl"], size=(4, call.B)).astype(np.uint32)
        d["yq"] = r.normal(0, 1, size=(call.B, env.m.D)).astype(np.float32)
    return d


# ---- what the oracle says ---------------------------------------------------------------------------------------------------

def _exact(*arrays_by_name):
    return {n: ("exact", np.ascontiguousarray(a)) for n, a in arrays_by_name}


def oracle_expected(call, env):
    """{output name: ("exact", array) | ("approx", float64 array, tol) | None}, made once per call and environment."""
    if call.name not in env._exp:
        env._exp[call.name] = _oracle_expected(call, env)
    return env._exp[call.name]


def _decoded(call, env, ids, lens, sl, o, keys, p_ids=None, p_len=None):
    """(out, len, align, scores float64 | None, score tolerance) of a translate-like call by its options' own checker"""
    from test_sampling_checker import sampled_translate
    from test_truncation_checker import truncated_translate
    from test_forced_prefix_checker import forced_translate
    O, om, m = env.oracle, env.om, env.m
    T = o.get("sampling")
    if o.get("trunc"):
        return truncated_translate(O, om, m, ids, lens, sl, keys, T, o["trunc"][0], o["trunc"][1], p_ids, p_len) + (TOL * max(1.0, 1.0 / T),)
    if T is not None:
        return sampled_translate(O, om, m, ids, lens, sl, keys, T, p_ids, p_len) + (TOL * max(1.0, 1.0 / T),)
    if o.get("scores") or p_len is not None:
        if p_len is None:
            p_ids, p_len = np.zeros((ids.shape[0], tmax(ids.shape[1])), np.uint32), np.zeros(ids.shape[0], np.uint32)
        return tuple(forced_translate(O, om, m, ids, lens, sl, p_ids, p_len)) + (TOL,)
    return env.translate(ids, lens, sl) + (None, TOL)


def _live(sc, ln):
    """the checker's scores where a translate call writes them (t < out_len), NaN elsewhere"""
    sc = np.array(sc, dtype=np.float64)
    sc[np.arange(sc.shape[1])[None, :] >= np.asarray(ln)[:, None]] = np.nan
    return sc


def _oracle_expected(call, env):
    from test_score_checker import teacher_forced
    from support import consensus_ref
    k, o, inp = call.kind, call.opt, inputs(call, env)
    if k == "translate" and o.get("refused"):
        B, S, T = call.B, call.S, tmax(call.S)
        pat = lambda dtype, shape: np.full(shape, PAT, np.uint32).view(dtype)
        return _exact(("out_ids", pat(np.uint32, (B, T))), ("out_len", pat(np.uint32, (B,))), ("align", pat(np.float32, (B, T, S))))
    if k == "translate":
        out, ln, al, sc, tol = _decoded(call, env, inp["ids"], inp["lens"], inp["sl"], o, inp.get("keys"), inp.get("p_ids"), inp.get("p_len"))
        e = _exact(("out_ids", out), ("out_len", ln))
        if o.get("align"):
            e["align"] = ("exact", al)
        if o.get("scores"):
            e["scores"] = ("approx", _live(sc, ln), tol)
        return e
    if k == "many":
        e = {}
        for j, ((ids, lens), sl) in enumerate(zip(inp["subs"], inp["sls"])):
            out, ln, al = env.translate(ids, lens, sl)
            e.update(_exact(("out_ids_%d" % j, out), ("out_len_%d" % j, ln), ("align_%d" % j, al)))
        return e
    if k == "fanout":
        src = inp["row_src"]
        d_ids, d_lens = np.ascontiguousarray(inp["ids"][src]), np.ascontiguousarray(inp["lens"][src])
        out, ln, al = _decoded(call, env, d_ids, d_lens, inp["sl"], o, inp["keys"])[:3]
        e = _exact(("out_ids", out), ("out_len", ln), ("align", al))
        if o.get("consensus"):
            util, best = consensus_ref.select(out, ln, src, call.B, *o["consensus"])
            e.update(_exact(("best", best), ("utility", util)))
        return e
    if k in ("score", "candidates"):
        src = inp.get("cand_src")
        ids, lens = (inp["ids"], inp["lens"]) if src is None else (np.ascontiguousarray(inp["ids"][src]), np.ascontiguousarray(inp["lens"][src]))
        sc, al = teacher_forced(env.oracle, env.om, env.m, ids, lens, inp["sl"], inp["t_ids"], inp["t_len"])
        e = {"scores": ("approx", sc, TOL), "align": ("approx", al.astype(np.float64), 0.0)}
        if o.get("alt"):  # tests/test_gpu_score_alternatives.py: ids and ranks exact, entries behind t_len not written
            from test_alternatives_checker import alternatives
            alt = alternatives(env.oracle, env.om, env.m, ids, lens, inp["sl"], np.ascontiguousarray(inp["t_ids"]), inp["t_len"], o["alt"])
            dead = np.arange(o["T"])[None, :] >= inp["t_len"][:, None].astype(np.int64)
            a_ids, rank = alt.ids.copy(), alt.rank.copy()
            a_ids[dead], rank[dead] = PAT, PAT
            e.update(alt_ids=("exact", a_ids), rank=("exact", rank), alt_scores=("approx", np.asarray(alt.scores, np.float64), TOL))
        return e
    if k in ("stepwise", "xattn"):  # tests/test_gpu_engine.py, tests/test_gpu_cross_attention_orders.py: all bit-exact
        O, om, m = env.oracle, env.om, env.m
        O.set_mode(O.PORTABLE)
        try:
            mask = O.make_mask(inp["lens"], call.S)
            enc = om.encode(om.embed(inp["ids"]), mask)
            if k == "xattn":
                joined, attn = om.cross_attention(m.dec_layers - 1, inp["yq"], enc, mask)
                return _exact(("joined", joined), ("attn", attn))
            e = _exact(("enc_out", enc))
            states = np.zeros((m.dec_layers, call.B, m.D), np.float32)
            for t in range(o["steps"]):
                logits, attn = om.decode_step(enc, mask, states, None if t == 0 else inp["prev"][t], inp["sl"])
                e.update(_exact(("logits_%d" % t, logits), ("attn_%d" % t, attn), ("states_%d" % t, states.copy())))
            return e
        finally:
            O.set_mode(O.FAITHFUL)
    if k == "kv_forms":
        return _exact(("recorded", np.array([o["want"]], np.uint32)))
    assert k in ("refused_step", "refused_begin")
    return {}


# ---- running a call on the device -------------------------------------------------------------------------------------------

class Arena:
    """The arrays of one call. where: "device" (torch), "pinned" (slimt_hip_host_alloc) or "host" (numpy). Every output is
    filled with PAT before the call; collect() returns them as host arrays."""

    def __init__(self, hip, where):
        self.hip, self.where = hip, where
        self.outs, self.keep, self.pins = [], [], []

    def _raw(self, n_words):
        n_words = max(int(n_words), 2) + 1  # (room to start 64-bit arrays at a multiple of 8)
        if self.where == "device":
            import torch
            t = torch.full((n_words,), int(np.uint32(PAT).view(np.int32)), dtype=torch.int32, device="cuda")
            self.keep.append(t)
            return t, t.data_ptr(), None
        if self.where == "pinned":
            p = C.c_void_p()
            self.hip._chk(self.hip.lib().slimt_hip_host_alloc(n_words * 4, C.byref(p)))
            self.pins.append(p)
            a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n_words,))
        else:
            a = np.empty(n_words, dtype=np.uint32)
            self.keep.append(a)
        a[:] = PAT
        return a, a.ctypes.data, a

    def inp(self, a):
        """An input where the call wants it: its address (None for None)."""
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        words = a.reshape(-1).view(np.uint32)
        raw, ptr, host = self._raw(words.size)
        skip = (ptr % 8) // 4
        if host is None:
            import torch
            raw[skip:skip + words.size] = torch.from_numpy(words.view(np.int32).copy()).cuda()
        else:
            host[skip:skip + words.size] = words
        return ptr + 4 * skip

    def out(self, name, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize // 4
        raw, ptr, host = self._raw(n)
        skip = (ptr % 8) // 4
        self.outs.append((name, np.dtype(dtype), tuple(shape), raw, skip, n))
        return ptr + 4 * skip

    def collect(self):
        got = {}
        for name, dtype, shape, raw, skip, n in self.outs:
            a = raw.cpu().numpy().view(np.uint32) if self.where == "device" else np.array(raw, copy=True)
            got[name] = a[skip:skip + n].copy().view(dtype).reshape(shape)
        return got

    def free(self):
        for p in self.pins:
            self.hip.lib().slimt_hip_host_free(p)
        self.pins, self.keep, self.outs = [], [], []


WHERE = {"host": "host", "generated": "host", "pinned": "pinned", "pinned_generated": "pinned", "device": "device",
         "device_generated": "device"}


def start(call, hip, ctx, env):
    """Queues the call on ctx; returns finish() -> {name: array}, to be called after the context's synchronize (a blocking
    call has finished by then anyway)."""
    L, vp = hip.lib(), C.c_void_p
    k, o, inp = call.kind, call.opt, inputs(call, env)
    if k == "translate":
        entry = o["entry"]
        ar = Arena(hip, WHERE[entry])
        B, S, T = call.B, call.S, tmax(call.S)
        sl = inp["sl"]
        p_ids, p_len = ar.inp(inp["ids"]), ar.inp(inp["lens"])
        p_sl, n_sl = (None, 0) if (sl is None or o["sl"] == "gen") else (ar.inp(sl), sl.size)
        p_out, p_ol = ar.out("out_ids", np.uint32, (B, T)), ar.out("out_len", np.uint32, (B,))
        p_al = ar.out("align", np.float32, (B, T, S)) if o.get("align") else None
        if o.get("scores"):
            ctx.set_scores([ar.out("scores", np.float32, (B, T))])
        if o.get("prefix"):
            ctx.set_target_prefix([(ar.inp(inp["p_ids"]), ar.inp(inp["p_len"]))])
        if o.get("sampling") is not None:
            ctx.set_sampling(o["sampling"], [ar.inp(inp["keys"])])
        if o.get("trunc"):
            ctx.set_sampling_truncation(*o["trunc"])
        a = (vp(p_ids), vp(p_len), B, S)
        s = (vp(p_sl), n_sl)
        r = (LF, 0, vp(p_out), vp(p_ol), vp(p_al))
        if entry == "host":
            rc = L.slimt_hip_translate(ctx.h, *a, *s, *r)
        elif entry == "pinned":
            rc = L.slimt_hip_translate_async(ctx.h, *a, *s, *r)
        elif entry == "device":
            rc = L.slimt_hip_translate_device(ctx.h, *a, *s, *r, 0)
        elif entry == "generated":
            rc = L.slimt_hip_translate_generated(ctx.h, env.gen.h, *a, *r)
        elif entry == "pinned_generated":
            rc = L.slimt_hip_translate_async_generated(ctx.h, env.gen.h, *a, *r)
        else:
            rc = L.slimt_hip_translate_device_generated(ctx.h, env.gen.h, *a, *r, 0)
        if o.get("refused"):
            if rc == 0:
                ar.outs.append(("not_refused", np.dtype(np.uint32), (1,), ar.outs[0][3], 0, 1))
            rc = 0
        finish = _finish(hip, rc, [ar])
        if not o.get("scores"):
            return finish

        def defined():  # include/slimt_hip.h: scores at t >= out_len[b] are not defined -- they count as not written
            got = finish()
            past = np.arange(T)[None, :] >= got["out_len"][:, None].astype(np.int64)
            got["scores"].view(np.uint32)[past] = PAT
            return got

        return defined
    if k == "many":
        ars, args, host = [], [], []
        where = o["where"]
        gen = env.gen if o["sls"] == "gen" else None
        for j, ((ids, lens), sl) in enumerate(zip(inp["subs"], inp["sls"])):
            ar = Arena(hip, where)
            ars.append(ar)
            B, Sj = ids.shape
            T = tmax(Sj)
            p = (ar.inp(ids), ar.inp(lens), ar.out("out_ids_%d" % j, np.uint32, (B, T)), ar.out("out_len_%d" % j, np.uint32, (B,)),
                 ar.out("align_%d" % j, np.float32, (B, T, Sj)))
            p_sl = ar.inp(sl) if (gen is None and where == "device") else 0
            args.append((p[0], p[1], B, p_sl, 0 if gen is not None else sl.size, p[2], p[3], p[4], Sj))
            host.append((_view(p[0], np.uint32, (B, Sj)), _view(p[1], np.uint32, (B,)), _view(p[2], np.uint32, (B, T)),
                         _view(p[3], np.uint32, (B,)), _view(p[4], np.float32, (B, T, Sj))) if where == "pinned" else None)
        try:
            if where == "device":
                ctx.translate_many_device(args, call.S, LF, 0, steps_hint=tmax(call.S), generator=gen)
            else:
                ctx.translate_many_async(host, None if gen is not None else inp["sls"][0], LF, 0, generator=gen)
        except Exception:
            for ar in ars:
                ar.free()
            raise
        return _finish(hip, 0, ars)
    if k == "fanout":
        ar = Arena(hip, o["where"])
        B, S, T, src = call.B, call.S, tmax(call.S), inp["row_src"]
        N, sl = src.size, inp["sl"]
        a = (vp(ar.inp(inp["ids"])), vp(ar.inp(inp["lens"])), B, S, vp(ar.inp(src)), N, vp(ar.inp(sl)), sl.size, LF, 0,
             vp(ar.out("out_ids", np.uint32, (N, T))), vp(ar.out("out_len", np.uint32, (N,))), vp(ar.out("align", np.float32, (N, T, S))))
        if o.get("sampling") is not None:
            ctx.set_sampling(o["sampling"], [ar.inp(inp["keys"])])
        if o.get("consensus"):
            ctx.set_fanout_consensus(o["consensus"][0], o["consensus"][1], ar.out("best", np.uint32, (B,)), ar.out("utility", np.float64, (N,)))
        fn = {"host": L.slimt_hip_translate_fanout, "pinned": L.slimt_hip_translate_fanout_async}.get(o["where"])
        rc = fn(ctx.h, *a) if fn else L.slimt_hip_translate_fanout_device(ctx.h, *a, 0)
        return _finish(hip, rc, [ar])
    if k in ("score", "candidates"):
        ar = Arena(hip, "host")  # pageable destinations: the staging buffers are the context's
        B, S, T, sl = call.B, call.S, o["T"], inp["sl"]
        N = B if k == "score" else inp["cand_src"].size
        if o.get("alt"):
            ctx.set_score_alternatives(o["alt"], ar.out("alt_ids", np.uint32, (N, T, o["alt"])), ar.out("alt_scores", np.float32, (N, T, o["alt"])),
                                       ar.out("rank", np.uint32, (N, T)))
        a = (vp(ar.inp(inp["ids"])), vp(ar.inp(inp["lens"])), B, S, vp(ar.inp(sl)), sl.size, vp(ar.inp(inp["t_ids"])), vp(ar.inp(inp["t_len"])), T)
        r = (vp(ar.out("scores", np.float32, (N, T))), vp(ar.out("align", np.float32, (N, T, S))))
        if k == "score":
            rc = L.slimt_hip_score(ctx.h, *a, *r)
        else:
            rc = L.slimt_hip_score_candidates(ctx.h, *a, vp(ar.inp(inp["cand_src"])), N, *r)
        return _finish(hip, rc, [ar])
    if k in ("stepwise", "xattn"):
        got = {}
        enc = ctx.encode(inp["ids"], inp["lens"])[0]
        ctx.decode_begin(inp["sl"])
        if k == "xattn":
            got["joined"], got["attn"] = ctx.debug_cross_attention(env.m.dec_layers - 1, inp["yq"], call.B, call.S, env.m.H)
        else:
            got["enc_out"] = enc
            for t in range(o["steps"]):
                got["logits_%d" % t], got["attn_%d" % t], got["states_%d" % t] = ctx.decode_step(None if t == 0 else inp["prev"][t])
        return lambda: got
    if k == "kv_forms":
        seen = ctx.debug_kv_formats(env.m.dec_layers, CTX_SHAPE[0])
        return lambda: {"recorded": np.array([0 if seen is None else 1], np.uint32)}
    if k == "refused_step":
        # Context.decode_step sizes its outputs by the wrapper's own record of the last encode / decode_begin (B, S, N);
        # the translate call in between went past the wrapper, so the record is put back to the round this step continues
        ctx.B, ctx.S, ctx.N = call.B, call.S, inp["sl"].size
        try:
            lg, at, st = ctx.decode_step(inp["prev"][2])
        except hip.SlimtHipError:
            return lambda: {}
        return lambda: {"logits_unrefused": lg, "attn_unrefused": at, "states_unrefused": st}
    assert k == "refused_begin"
    try:
        ctx.decode_begin(inp["sl"])
    except hip.SlimtHipError:
        return lambda: {}
    return lambda: {"decode_begin": np.zeros(1, np.uint32)}


def _view(addr, dtype, shape):
    n = int(np.prod(shape))
    return np.ctypeslib.as_array(C.cast(C.c_void_p(addr), C.POINTER(C.c_uint32)), shape=(n,)).view(dtype).reshape(shape)


def _finish(hip, rc, arenas):
    if rc != 0:
        for ar in arenas:
            ar.free()
        hip._chk(rc)

    def finish():
        got = {}
        try:
            for ar in arenas:
                got.update(ar.collect())
        finally:
            for ar in arenas:
                ar.free()
        return got

    return finish


def run(call, hip, ctx, env):
    """The call, finished: {output name: array}."""
    finish = start(call, hip, ctx, env)
    ctx.synchronize()
    return finish()


def apply_setter(item, ctx, env):
    what, value = item[1:].split(":")
    if what == "mode":
        ctx.set_decode_mode(int(value))
    elif what == "rows":
        ctx.set_encode_rows(int(value))
    else:
        assert what == "kv"
        env.gm.set_kv_cache_format(int(value))


def differing_rows(got, want):
    """rows (first axis) at which two arrays of one shape differ as bits"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape %s %s, expected %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    g = np.ascontiguousarray(got).reshape(got.shape[0], -1).view(np.uint8)
    w = np.ascontiguousarray(want).reshape(want.shape[0], -1).view(np.uint8)
    return np.nonzero((g != w).any(axis=1))[0].tolist()
