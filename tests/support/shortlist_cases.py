"""The cases tests/test_gpu_shortlist_paths.py compares with the oracle's ShortlistGenerator::generate id for id, and
tests/test_shortlist_case_fixtures.py checks for reaching the edges they claim (CPU). One table, like score_cases.py and
alternatives_cases.py, so that the GPU test and the CPU proof of its coverage cannot drift.

What the table is built around (slimt_amd/csrc/shortlist_device.h):
  * shortlist_mark: a wave takes 64 tokens at a time, claims each source word once (source bitmap) and ORs the word's list into
    the target bitmap 64 entries per step -- lists above 64 entries take the `k += 64` loop, above 128 more than one trip of it;
    padding is no word;
  * shortlist_compact: 1024 threads over TW = ceil(V_tgt / 32) bitmap words, wpt = ceil(TW / 1024) words per thread; the
    multiple-of-eight patch adds the lowest need = (8 - ones % 8) % 8 unset ids >= frequent, found 64 words at a time from
    word frequent / 32 on (windows), `need` split over the lanes of a window and over windows;
  * in an encoder launch the bitmaps live in LDS as tb (TW words) | sb (SW = ceil(V_src / 32) words) | scan.
Nothing here calls the library; every claim is checked by arithmetic on the lists themselves (dissect)."""
import struct
from collections import namedtuple

import numpy as np

# blob: the binary lexical shortlist; Vs / Vt: the generator's vocabularies; ids / lens: the batch; shared: shared vocabulary;
# paths: the stand-alone generators the case runs on (1: slimt_hip_shortlist_generate, 2: ..._generate_device);
# twin: None, or the batch with every source id >= Vt replaced by a word below `frequent` that has the same list -- the input
#       on which the independent set construction (test_shortlist.numpy_generate) states what such a batch selects: under a
#       shared vocabulary the reference marks target_table[word], which does not exist for word >= Vt (undefined there); the
#       device and the oracle ignore the mark and keep the word's list
Case = namedtuple("Case", "name blob Vs Vt ids lens shared paths twin")

WINDOW = 64  # bitmap words the patch searches at a time


def blob_from_lists(V_src, V_tgt, frequent, best, lists):
    """A binary lexical shortlist (header, magic and checksum as synth.make_lexical_shortlist writes them) from explicit lists:
    {source word: sorted unique target ids}; every other word's list is empty. The last word of the vocabulary needs a list
    (ShortlistGenerator::load's content check wants every offset but the last below the size, Shortlist.cc:18-21)."""
    from slimt_amd import synth
    assert V_src - 1 in lists and len(lists[V_src - 1]), "the last source word needs a list"
    counts = np.zeros(V_src, dtype=np.uint64)
    for w, l in lists.items():
        l = np.asarray(l, dtype=np.int64)
        assert 0 <= w < V_src and l.size and np.all(np.diff(l) > 0) and 0 <= l[0] and l[-1] < V_tgt, w
        counts[w] = l.size
    offsets = np.zeros(V_src + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts)
    flat = np.concatenate([np.asarray(lists[w], dtype=np.uint32) for w in sorted(lists)])
    body = struct.pack("<4Q", frequent, best, offsets.size, flat.size) + offsets.tobytes() + flat.tobytes()
    return struct.pack("<2Q", synth.SHORTLIST_MAGIC, synth.shortlist_checksum(body)) + body


def parse(blob):
    """(frequent, best, offsets uint64 [V_src + 1], lists uint32)"""
    frequent, best, n_off, n_ids = struct.unpack_from("<4Q", blob, 16)
    off = np.frombuffer(blob, dtype=np.uint64, count=n_off, offset=48)
    return frequent, best, off, np.frombuffer(blob, dtype=np.uint32, count=n_ids, offset=48 + 8 * n_off)


def words_of(ids, lens):
    return np.concatenate([ids[b, : int(lens[b])] for b in range(ids.shape[0])])


def batch_of(rows, S, pad):
    """rows of source words, padded to S with `pad` (a word whose list would show if padding were taken for words)"""
    ids = np.full((len(rows), S), pad, dtype=np.uint32)
    for b, r in enumerate(rows):
        ids[b, : len(r)] = r
    return ids, np.asarray([len(r) for r in rows], dtype=np.uint32)


def padded(blob, Vt, ids, lens, below):
    """ids with the padding of every row replaced by ONE word < `below` that no sentence holds and whose list selects an id the
    batch does not (the largest such word): a generator that takes padding for words then gives another list. synth.make_batch
    pads with 0, the EOS every sentence ends with -- such padding can never show. Unchanged when no word serves."""
    frequent, _, off, lists = parse(blob)
    chosen = np.zeros(Vt, dtype=bool)
    chosen[: min(frequent, Vt)] = True
    used = np.unique(words_of(ids, lens))
    for w in used:
        chosen[lists[int(off[w]): int(off[w + 1])]] = True
    for w in range(min(below, len(off) - 1) - 1, 0, -1):
        l = lists[int(off[w]): int(off[w + 1])]
        if l.size and w not in used and not chosen[l].all():
            out = ids.copy()
            for b in range(ids.shape[0]):
                out[b, int(lens[b]):] = w
            return out
    return ids


Dissected = namedtuple("Dissected", "before need patch windows lanes list_lengths TW n_tok")


def dissect(c, final):
    """What `final` (the reference's list for case c) says about the edges: the bitmap before the patch (frequent ids, the
    words' own ids under a shared vocabulary, the lists of the batch's words), need, the ids the patch added, and for each of
    them the 64-word window (0 = the one that starts at word frequent / 32) and the lane (word within the window) it fell in;
    the lengths of the lists the batch uses; TW; the token count of the padded batch."""
    frequent, _, off, lists = parse(c.blob)
    before = np.zeros(c.Vt, dtype=bool)
    before[: min(frequent, c.Vt)] = True
    lengths = []
    for w in np.unique(words_of(c.ids, c.lens)):
        if c.shared and w < c.Vt:
            before[w] = True
        l = lists[int(off[w]): int(off[w + 1])]
        before[l] = True
        lengths.append(l.size)
    after = np.zeros(c.Vt, dtype=bool)
    after[final] = True
    assert not (before & ~after).any()
    patch = np.flatnonzero(after & ~before)
    fw = frequent // 32
    windows = (patch // 32 - fw) // WINDOW
    lanes = (patch // 32 - fw) % WINDOW
    return Dissected(before, int((8 - before.sum() % 8) % 8), patch, windows, lanes, np.asarray(lengths), (c.Vt + 31) // 32,
                     c.ids.size)


# ---- crafted cases ---------------------------------------------------------------------------------------------------------
# The window cases: frequent = 40, in the middle of bitmap word 1 -- the patch's first window is words 1 .. 64 (ids 32 .. 2079),
# its second words 65 .. 128 (ids 2080 .. 4127). Word 7's list covers every id from 40 to 2304 but eight holes: 40 frequent ids
# + 2257 listed ones = 2297 = 8 * 287 + 1, so the patch needs 7 of the 8 holes and must leave the highest alone.
WINDOW_FREQUENT = 40
WINDOW_END = 2305
WINDOW_HOLES = {
    # none in the first window; four in word 66, four in word 67 (the patch takes three of those)
    "patch-second-window": [2115, 2121, 2132, 2143, 2144, 2149, 2161, 2174],
    # three in word 64, the last of the first window (its lane 63); two in word 65 and three in word 70 (two taken) of the second
    "patch-straddles-windows": [2049, 2062, 2079, 2080, 2087, 2244, 2245, 2246],
}


def window_case(name, Vt=4500, Vs=50):
    """Vs >= 50. Word 33 (a list of one id far above everything else) is the padding."""
    big = np.setdiff1d(np.arange(WINDOW_FREQUENT, WINDOW_END), WINDOW_HOLES[name])
    lists = {7: big, 20: [45, 46], 33: [Vt - 100], Vs - 1: [41]}
    blob = blob_from_lists(Vs, Vt, WINDOW_FREQUENT, big.size, lists)
    ids, lens = batch_of([[7, 3, 11, 0], [20, Vs - 1, 7], [7], [3, 0]], 6, 33)
    return Case(name, blob, Vs, Vt, ids, lens, False, (1, 2), None)


def not_needed_case(Vt=640, Vs=20):
    """64 frequent ids + 8 listed ones = 72: need = 0, nothing is added although ids are free right behind `frequent`"""
    lists = {5: [70, 71, 100, 101, 333, 400, 500, Vt - 1], 9: [90], Vs - 1: [70]}
    blob = blob_from_lists(Vs, Vt, 64, 8, lists)
    ids, lens = batch_of([[5, 2, 0], [Vs - 1, 5], [5, 5, 5, 0]], 5, 9)
    return Case("patch-not-needed", blob, Vs, Vt, ids, lens, False, (1, 2), None)


def runs_out_case():
    """V_tgt = 203: 100 frequent ids + 101 listed = 201, need = 7, two ids are free: the list ends at 203, off a multiple of 8"""
    lists = {5: np.setdiff1d(np.arange(100, 203), [150, 201]), 19: [100]}
    blob = blob_from_lists(20, 203, 100, 101, lists)
    ids, lens = batch_of([[5, 2, 0], [19, 5]], 4, 2)
    return Case("patch-runs-out", blob, 20, 203, ids, lens, False, (1, 2), None)


def full_case(V, rows=None):
    """every id selected: words 2 and 3 list the even and the odd ids; count = V, no multiple of 8, nothing left to patch.
    rows (B, S): a random batch of the V words with 2 and 3 planted, for the model-bound runs; else three short rows."""
    lists = {2: np.arange(0, V, 2), 3: np.arange(1, V, 2), V - 1: [5]}
    blob = blob_from_lists(V, V, 10, (V + 1) // 2, lists)
    if rows is None:
        ids, lens = batch_of([[2, 9, 0], [V - 1, 3], [0]], 4, 8)
    else:
        from slimt_amd import synth
        ids, lens = synth.make_batch(V, rows[0], rows[1], seed=V + rows[0], ragged=True)
        ids[0, 0], ids[1, 0] = 2, 3
    return Case("full-%d" % V, blob, V, V, ids, lens, False, (1, 2), None)


def frequent_0_case():
    """frequent = 0: the patch starts at id 0. Six listed ids, need = 2: ids 0 and 1 are added"""
    lists = {5: [3, 9, 64, 65, 300], 8: [2], 19: [7]}
    blob = blob_from_lists(20, 640, 0, 5, lists)
    ids, lens = batch_of([[5, 2, 0], [19, 5], [4]], 4, 8)
    return Case("frequent-0", blob, 20, 640, ids, lens, False, (1, 2), None)


DUP_B, DUP_S = 12, 16  # 192 tokens: three 64-token chunks of four sentences each


def duplicates_case(shared):
    """word 9 (70 ids: past the first 64 entries) opens every sentence -- four times in every 64-token chunk --, next to words
    without a list and the last word of the vocabulary. shared: V_src = 700 above V_tgt = 640, and word 650 (no target id of that
    number exists) in three sentences; its twin is word 3, below frequent = 16, with the same list (the last word's is word 2)."""
    Vs, Vt = 700, 640
    lists = {9: np.arange(100, 240, 2), 3: [300, 301, 302], 650: [300, 301, 302], 21: [611], 2: [17, 639], Vs - 1: [17, 639]}
    blob = blob_from_lists(Vs, Vt, 16, 70, lists)
    rng = np.random.default_rng(5)
    rows = []
    for b in range(DUP_B):
        n = int(rng.integers(3, DUP_S + 1)) if b else DUP_S
        r = [9] + [int(x) for x in rng.choice([4, 5, 6, 9, 30, 31, 500], size=n - 2)] + [0]
        if b % 5 == 1:
            r[1] = Vs - 1
        if shared and b % 4 == 2:
            r[1] = 650
        rows.append(r)
    ids, lens = batch_of(rows, DUP_S, 21)
    twin = None
    if shared:
        twin = ids.copy()
        twin[twin == 650] = 3
        twin[twin == Vs - 1] = 2
    return Case("duplicates-shared" if shared else "duplicates", blob, Vs, Vt, ids, lens, shared, (1, 2), twin)


# ---- sized cases: synth.make_lexical_shortlist --------------------------------------------------------------------------------
# name: (V_src, V_tgt, frequent, best, B, S, shared, seed, paths)
SIZED = {
    "wpt2": (2000, 32768 + 37, 100, 300, 7, 16, False, 31, (1, 2)),   # TW = 1026: two words per thread, the last word 5 bits
    "wpt3": (2000, 70001, 100, 300, 7, 16, False, 32, (1, 2)),        # TW = 2188: three words per thread, the last word 17 bits
    "tokens-40x32": (4000, 4000, 50, 20, 40, 32, False, 33, (1, 2)),  # above 1024 tokens (the model-bound twin: MODEL_CASES)
    "tokens-140x128": (4096, 4096, 100, 20, 140, 128, False, 34, (1,)),  # above 16384: 16 workgroups, every wave loops
    "src3000-tgt1003": (3000, 1003, 100, 6, 9, 12, False, 35, (1, 2)),
    "src600-tgt1003": (600, 1003, 100, 6, 9, 12, False, 36, (1, 2)),
    "src300-tgt2048": (300, 2048, 100, 3, 2, 5, False, 4, (1, 2)),
    "src2048-tgt300": (2048, 300, 100, 50, 16, 32, False, 5, (1, 2)),
    "shared-500": (512, 500, 100, 20, 7, 16, True, 2, (1, 2)),
    "frequent-above-V": (645, 645, 700, 2, 3, 4, False, 9, (1, 2)),   # no room for the patch: all 645 ids, off a multiple of 8
}

_BLOBS = {}


def lexical(Vs, Vt, frequent, best, seed):
    from slimt_amd import synth
    key = (Vs, Vt, frequent, best, seed)
    if key not in _BLOBS:
        _BLOBS[key] = synth.make_lexical_shortlist(Vs, Vt, frequent, best, seed=seed)
    return _BLOBS[key]


def sized_case(name):
    from slimt_amd import synth
    Vs, Vt, frequent, best, B, S, shared, seed, paths = SIZED[name]
    blob = lexical(Vs, Vt, frequent, best, seed)
    below = min(Vs, Vt) if shared else Vs
    ids, lens = synth.make_batch(below, B, S, seed=seed, ragged=True)
    return Case(name, blob, Vs, Vt, padded(blob, Vt, ids, lens, below), lens, shared, paths, None)


CRAFTED = {
    "patch-second-window": lambda: window_case("patch-second-window"),
    "patch-straddles-windows": lambda: window_case("patch-straddles-windows"),
    "patch-not-needed": not_needed_case,
    "patch-runs-out": runs_out_case,
    "full-517": lambda: full_case(517),
    "full-1003": lambda: full_case(1003),
    "frequent-0": frequent_0_case,
    "duplicates": lambda: duplicates_case(False),
    "duplicates-shared": lambda: duplicates_case(True),
}

_CASES = {}


def case_names():
    return list(CRAFTED) + list(SIZED)


def case(name):
    if name not in _CASES:
        _CASES[name] = CRAFTED[name]() if name in CRAFTED else sized_case(name)
    return _CASES[name]


def reference(oracle, c):
    """the oracle's ShortlistGenerator::generate of the case's batch"""
    return oracle.OracleShortlist(c.blob, c.Vs, c.Vt, shared=c.shared, check=True).generate(c.ids, c.lens)


# ---- model-bound cases: the generators inside an encoder launch ------------------------------------------------------------------
# name: (dims, eos_bias, seed): chosen on the CPU (test_shortlist_case_fixtures.py has the conditions) -- with eos_bias 6.0 a
# (256, 1536, 8, 2, 2, 33003) model ends every sentence at step 1
MODELS = {
    "tiny-1003": ((256, 1536, 8, 2, 2, 1003), 4.5, 1234),    # target words 31.3: no multiple of 32
    "tiny-33003": ((256, 1536, 8, 1, 2, 33003), 1.5, 1235),  # TW = 1032: two words per thread in the launch
    "base-1003": ((512, 2048, 8, 1, 2, 1003), 3.0, 1234),    # the wide encoder
}
# how each model's context is set up: (model, set_encode_rows) -- the 64-row, the 32-row and the D = 512 encoder
ENCODERS = {"rows64": ("tiny-1003", 64), "rows32": ("tiny-1003", 32), "wide": ("base-1003", 0), "rows64-33003": ("tiny-33003", 64),
            "rows32-33003": ("tiny-33003", 32)}

_MODELS = {}


def model(name):
    from slimt_amd import synth
    if name not in _MODELS:
        dims, eos_bias, seed = MODELS[name]
        _MODELS[name] = synth.make_model("tiny11", seed=seed, eos_bias=eos_bias, dims=dims)
    return _MODELS[name]


def model_V(name):
    return MODELS[name][0][5]


# the lexical shortlists of the model-bound runs: name -> (V_src or None = the model's, frequent, best, seed)
GENERATORS = {
    "lex": (None, 24, 4, 41),        # small lists: ids differ from batch to batch, padding shows
    "lex100": (None, 8, 100, 42),    # lists past 64 entries; 40 x 32 tokens select most of a small vocabulary
    "src3000": (3000, 24, 4, 43),    # SW = 94 words of source bitmap between tb and scan, above the model's 32
    "src600": (600, 24, 4, 44),      # SW = 19, below
}


def generator_blob(model_name, gen):
    V = model_V(model_name)
    Vs, frequent, best, seed = GENERATORS[gen]
    return lexical(Vs or V, V, frequent, best, seed), Vs or V


def model_batch(model_name, gen, B, S):
    """a ragged batch of the words both vocabularies hold, padded with a word whose list shows (see padded)"""
    from slimt_amd import synth
    blob, Vs = generator_blob(model_name, gen)
    V = model_V(model_name)
    ids, lens = synth.make_batch(min(V, Vs), B, S, seed=B * 100 + S + 3, ragged=S > 1)
    return padded(blob, V, ids, lens, min(V, Vs)), lens


# (encoder set-up, generator or crafted case, B, S, decode mode). S <= 32: in the launch; (9, 40): the 64-row encoder with one
# sentence per workgroup; (9, 70): the per-sentence encoder behind the two-kernel generator on the context's stream, the count
# read by the persistent decoder on the device; mode 1: the per-stage kernels behind one read-back
MODEL_CASES = (
    [(enc, "lex100", 40, 32, 0) for enc in ("rows64", "rows32", "wide", "rows64-33003")]
    + [(enc, "lex", 5, 13, 0) for enc in ("rows64", "rows32", "wide", "rows64-33003", "rows32-33003")]
    + [(enc, "lex", 1, 1, 0) for enc in ("rows64", "rows32", "wide")]
    + [("rows64", "lex", 9, 40, 0), ("rows32", "lex", 9, 40, 0), ("rows64", "lex", 9, 70, 0), ("rows64-33003", "lex", 9, 70, 0)]
    + [("rows64", "lex", 5, 13, 1)]
    + [(enc, g, 9, 12, 0) for enc in ("rows64", "rows32", "wide") for g in ("src3000", "src600")]
    + [(enc, "full", 5, 13, 0) for enc in ("rows64", "rows32", "wide")]
    + [(enc, c, 0, 0, 0) for enc in ("rows64-33003", "rows32-33003")
       for c in ("patch-second-window", "patch-straddles-windows", "patch-not-needed")]
)
# the cases whose greedy translation the fixture test holds to test_model_shape_fixtures.fixture_problems
VOUCHED = [("lex100", 40, 32), ("lex", 5, 13), ("lex", 9, 40), ("lex", 9, 70)]


def model_case_id(mc):
    enc, what, B, S, mode = mc
    return "%s-%s%s%s" % (enc, what, "-%dx%d" % (B, S) if B else "", "-mode%d" % mode if mode else "")


_MODEL_CASES = {}


def model_case(mc):
    """(model name, Case): the generator's blob and the batch of one MODEL_CASES entry"""
    enc, what, B, S, _ = mc
    name = ENCODERS[enc][0]
    key = (name, what, B, S)
    if key not in _MODEL_CASES:
        V = model_V(name)
        if what == "full":
            c = full_case(V, (B, S))
        elif what in WINDOW_HOLES:
            c = window_case(what, Vt=V)
        elif what == "patch-not-needed":
            c = not_needed_case(Vt=V)
        else:
            blob, Vs = generator_blob(name, what)
            ids, lens = model_batch(name, what, B, S)
            c = Case(what, blob, Vs, V, ids, lens, False, (), None)
        _MODEL_CASES[key] = c
    return name, _MODEL_CASES[key]


_TRANSLATIONS = {}


def translation(oracle, model_name, c):
    """(shortlist, out, len, align) of the PORTABLE oracle for case c on the model, with the oracle's own list for the batch;
    computed once per (model, batch)"""
    key = (model_name, c.name, c.ids.shape, c.ids.tobytes(), c.lens.tobytes())
    if key not in _TRANSLATIONS:
        sl = reference(oracle, c)
        om = _oracle_model(oracle, model_name)
        oracle.set_mode(oracle.PORTABLE)
        try:
            out, ln, al, _ = om.translate(c.ids, c.lens, sl, 1.5, 0, want_align=True)
        finally:
            oracle.set_mode(oracle.FAITHFUL)
        _TRANSLATIONS[key] = (sl, out, ln, al)
    return _TRANSLATIONS[key]


_ORACLE_MODELS = {}


def _oracle_model(oracle, name):
    if name not in _ORACLE_MODELS:
        _ORACLE_MODELS[name] = oracle.OracleModel(model(name))
    return _ORACLE_MODELS[name]


# ---- the stale size hint: one context, the smallest and the largest list the blob allows, in turn ------------------------------
HINT_MODEL, HINT_ENCODER_ROWS = "tiny-33003", 64
HINT_GENERATOR = "lex100"
HINT_SHAPES = [(1, 1), (40, 32), (1, 1), (40, 32)]


def hint_case(B, S):
    return model_case(("rows64-33003", HINT_GENERATOR, B, S, 0))[1]


# ---- merged launches: (name, launch S, [(B_j, S_j)], repeated word or None) -----------------------------------------------------
MERGED = [
    ("two", 24, [(33, 24), (5, 19)], None),
    ("five", 16, [(20, 16), (7, 13), (33, 16), (1, 9), (16, 12)], None),
    ("eight", 13, [(5, 13), (17, 9), (3, 13), (20, 11), (1, 1), (9, 13), (2, 5), (12, 13)], None),
    ("eight-one-tile", 1, [(1, 1), (2, 1)] * 4, None),   # one or two one-token sentences each: fewer tiles than shortlists
    ("repeated-word", 12, [(6, 12), (9, 10), (4, 12)], 77),  # word 77 in every sub-batch: claimed once PER sub-batch
]
MERGED_MODEL, MERGED_GENERATOR = "tiny-1003", "lex"


def merged_batches(name):
    """[Case] of one MERGED entry: every sub-batch with its own words (one-token sentences: a word each, not the EOS)"""
    from slimt_amd import synth
    _, S, shapes, word = next(m for m in MERGED if m[0] == name)
    blob, Vs = generator_blob(MERGED_MODEL, MERGED_GENERATOR)
    V = model_V(MERGED_MODEL)
    out = []
    for j, (B, Sj) in enumerate(shapes):
        ids, lens = synth.make_batch(V, B, Sj, seed=900 + 31 * j + B, ragged=Sj > 1)
        if Sj == 1:
            ids[:, 0] = np.random.default_rng(j).integers(2, V, size=B)
        if word is not None:
            ids[:, 0] = word
        out.append(Case("%s-%d" % (name, j), blob, Vs, V, padded(blob, V, ids, lens, V), lens, False, (), None))
    return S, out
