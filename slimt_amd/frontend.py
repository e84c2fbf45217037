"""The reference's Python API over the HIP engine: what
`bindings/python/slimt.cpp:144-221` exposes -- Package, Config, preset, Model,
Service.translate / .pivot, Response, AnnotatedText, Range, Encoding -- with one
addition, the `device` the model's weights live on.

    from slimt_amd import frontend as slimt
    model = slimt.Model(slimt.preset.tiny(), slimt.Package(model="model.bin",
                        vocabulary="vocab.spm", shortlist="lex.s2t.bin"), device=0)
    service = slimt.Service(workers=4)
    responses = service.translate(model, ["Hello world. How are you?"], html=False)
    responses[0].target.text, responses[0].alignments

Text in, text out: TextProcessor (text.py) splits and tokenises, the C++ batching
service (host/Service.{hh,cc} through include/slimt_hip_service.h: token-budget batches
of at most `max_words` padded tokens formed by the reference's rule, Batcher.cc:95-120,
double-buffered pinned workers, the batch's lexical shortlist generated on the device)
translates, and the returned ids / alignment rows become the Response
(Request.cc:136-170). The compute is the C-ABI library's; nothing here falls back
to a CPU model.
"""
from __future__ import annotations

import functools
import threading
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import capi, synth
from .text import AnnotatedText, Encoding, Range, TextProcessor, Vocabulary  # noqa: F401 (API surface)
from .text import _Lazy

Alignment = np.ndarray  # [target token][source token] f32, p(source | target); indexes like a list of rows


@dataclass
class Package:  # slimt.cpp:182-191: paths (or bytes) of the three model files
    model: str | bytes = ""
    vocabulary: str | bytes = ""
    shortlist: str | bytes = ""
    ssplit: str | bytes = ""  # optional non-breaking-prefix list (Package.hh ssplit)


@dataclass
class Config:  # Model::Config, Model.hh:33-51
    encoder_layers: int = 6
    decoder_layers: int = 2
    feed_forward_depth: int = 2
    num_heads: int = 8
    split_mode: str = "sentence"


class preset:  # Model.cc:206-245
    @staticmethod
    def tiny() -> Config:
        return Config(6, 2, 2, 8, "sentence")

    @staticmethod
    def base() -> Config:
        return Config(6, 2, 2, 8, "sentence")

    @staticmethod
    def nano() -> Config:
        return Config(4, 2, 2, 8, "sentence")


@dataclass
class Response:  # Response.hh: source / target with sentence + token ranges, soft alignments
    source: AnnotatedText = field(default_factory=AnnotatedText)
    target: AnnotatedText = field(default_factory=AnnotatedText)
    alignments: List[Alignment] = field(default_factory=list)
    # translate(..., scores=True): per target sentence, the log-probability of each of its target tokens (EOS included)
    # and their sum (no length normalisation); empty otherwise
    token_scores: List[np.ndarray] = field(default_factory=list)
    sentence_scores: List[float] = field(default_factory=list)
    # translate(..., samples=n): the n alternatives of this text, each a Response of its own (alternative j holds sample j of
    # every sentence); this Response is alternative 0. Empty otherwise
    samples: List["Response"] = field(default_factory=list)
    # sample_and_select(): per sentence (segment) of this text, the winning sample's utility among the segment's samples and
    # its index j among them; empty otherwise
    utility: List[float] = field(default_factory=list)
    sample_index: List[int] = field(default_factory=list)
    # beam_search(): the k alternatives of this text, each a Response of its own (alternative j holds the rank-j hypothesis
    # of every sentence, with scores); this Response is rank 0. hypothesis_scores: per sentence, the hypothesis' total
    # log-probability as the engine returned it (-inf where a sentence has fewer than j + 1 hypotheses). Empty otherwise
    nbest: List["Response"] = field(default_factory=list)
    hypothesis_scores: List[float] = field(default_factory=list)

    def to(self, encoding: Encoding) -> None:
        self.source.to(encoding)
        self.target.to(encoding)
        for r in self.samples + self.nbest:
            if r is not self:
                r.to(encoding)


def _target_boundaries(vocabulary, begin: int, words) -> List[int]:
    """Token boundaries (byte offsets in the target text) of a decoded sentence that starts at `begin`."""
    return [begin + o for o in vocabulary.decode_boundaries(words)]


def _blob(x) -> bytes:
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    with open(x, "rb") as f:
        return f.read()


@dataclass
class PairScore:  # Service.score: one (source, given target) pair
    source_ids: List[int]         # the source as tokenised, EOS included
    target_ids: List[int]         # the target as tokenised, EOS included
    token_scores: np.ndarray      # float32 [len(target_ids)]: log-probability of each target token given those before it
    score: float                  # their sum: the log-probability of the target given the source
    alignment: np.ndarray         # float32 [len(target_ids), len(source_ids)]
    # Service.score(..., alternatives=k) only (else None):
    ranks: Optional[List[int]] = None   # per target token: how many tokens of the output layer the model preferred to it
    #                                     (0: it is the model's choice; None: the token is outside the layer)
    alternatives: Optional[List[List[Tuple[str, float]]]] = None  # per target token: the (up to) k most probable
    #                                     (piece string, log-probability) pairs of its position, best first


class Model:
    """slimt::Model (Model.hh:31-83): vocabulary + text processor + the transformer's weights on
    `device` + the optional lexical shortlist generator."""

    _next_id = 0

    def __init__(self, config: Config, package: Package, device: int = 0):
        self.config = config
        self.id = Model._next_id
        Model._next_id += 1
        self.vocabulary = Vocabulary(package.vocabulary)
        self.processor = TextProcessor(config.split_mode, self.vocabulary,
                                       _blob(package.ssplit) if package.ssplit else b"")
        host = synth.model_from_bin(_blob(package.model), heads=config.num_heads,
                                    enc_layers=config.encoder_layers, dec_layers=config.decoder_layers)
        if self.vocabulary.size() > host.V:
            raise ValueError("vocabulary has %d pieces, the model's embedding %d rows"
                             % (self.vocabulary.size(), host.V))
        self.device = device
        capi.request_hw_queues(32)  # a Service runs `workers` x 2 streams on this device (no-op once HIP is up)
        self.engine = capi.Model(host, device)
        self.dims = (host.D, host.F, host.V)
        self.shortlist_generator = None
        self.shortlist_blob = b""
        if package.shortlist:  # Model::make_shortlist_generator, Model.cc:60-72
            self.shortlist_blob = _blob(package.shortlist)
            # ShortlistGenerator(view, source, target): shared = false, check = false (Model.cc:73-80, Shortlist.hh:47-52)
            self.shortlist_generator = capi.ShortlistGenerator(self.shortlist_blob, host.V, host.V,
                                                               shared=False, check=False, device=device)

    def close(self) -> None:
        if self.shortlist_generator is not None:
            self.shortlist_generator.close()
            self.shortlist_generator = None
        self.engine.close()


class _LazyAlignment:
    """One sentence's [target tokens, source tokens] matrix inside a call's block of alignment rows;
    materialised (a reshaped view, no copy) on first use. Indexes, iterates and converts like the
    array it stands for."""
    __slots__ = ("_block", "_a", "_b", "_rows", "_cols", "_arr")

    def __init__(self, block, a, b, rows, cols):
        self._block, self._a, self._b, self._rows, self._cols, self._arr = block, a, b, rows, cols, None

    def array(self) -> np.ndarray:
        if self._arr is None:
            self._arr = self._block[self._a:self._b].reshape(self._rows, self._cols) if self._b > self._a else \
                np.zeros((self._rows, self._cols), np.float32)
        return self._arr

    def __array__(self, dtype=None, copy=None):
        a = self.array()
        return a if dtype is None else a.astype(dtype)

    def __len__(self):
        return self._rows

    def __getitem__(self, i):
        return self.array()[i]

    def __iter__(self):
        return iter(self.array())

    @property
    def shape(self):
        return (self._rows, self._cols)


@dataclass
class _Unit:  # one segment of one request
    request: int
    index: int
    words: List[int]


class Service:
    """slimt::Async (Frontend.hh:20-78) behind the binding's blocking calls (slimt.cpp:44-135)."""

    def __init__(self, workers: int = 1, cache_size: int = 0, max_words: int = 1024, wrap_length: int = 128,
                 tgt_length_limit_factor: float = 1.5):
        if workers < 1:
            raise ValueError("workers must be >= 1")
        self.workers = workers
        self.cache_size = cache_size  # accepted for signature parity; no translation cache here
        self.max_words = max_words
        self.wrap_length = wrap_length
        self.limit_factor = tgt_length_limit_factor
        self.pipeline_documents = 256  # translate(): documents per pipelined chunk (one chunk: no pipeline)
        self._engines = {}  # model id -> capi.BatchService (host/Service over its C ABI)
        self._beam_contexts = {}  # model id -> capi.Context (beam_search)
        self._lock = threading.Lock()

    # -- batching ---------------------------------------------------------------------------------
    def _batches(self, units: Sequence[_Unit]) -> List[List[_Unit]]:
        """The reference's batch-forming rule (Batcher::generate, slimt/Batcher.cc:95-120), as the C++
        Service's LengthQueue applies it: walk the lengths UPWARDS, arrival order inside a length, and
        keep adding sentences while (count + 1) * length fits the word budget -- a batch is as wide as
        the last sentence added, and a sentence's padding (hence its length limit floor(1.5 S)) is the
        same here, in host/Service.cc and in the reference."""
        order = sorted(units, key=lambda u: (len(u.words), u.request, u.index))
        out, cur = [], []
        for u in order:
            if cur and (len(cur) + 1) * len(u.words) > self.max_words:
                out.append(cur)
                cur = []
            cur.append(u)
        if cur:
            out.append(cur)
        return out

    # the engine's longest source (the reference wraps at 128, Frontend.hh:27, and its batcher leaves
    # slack above that for the rare longer segment, Batcher.cc:83-88)
    ENGINE_LIMIT = 128

    def _split_long(self, words: List[int], eos: int) -> List[List[int]]:
        """A segment longer than the engine takes (only a pivot's second hop can produce one: its
        input is the first model's output re-tokenised, not wrapped text) goes through in pieces of
        at most ENGINE_LIMIT tokens, every piece ending in EOS."""
        if len(words) <= self.ENGINE_LIMIT:
            return [words]
        body = list(words[:-1]) if words and words[-1] == eos else list(words)
        step = self.ENGINE_LIMIT - 1
        return [body[i:i + step] + [eos] for i in range(0, len(body), step)]

    def _engine(self, model: Model, scores: bool = False, temperature: float = 0.0, truncation=None) -> "capi.BatchService":
        """The C++ batching service for `model` (host/Service.{hh,cc} behind include/slimt_hip_service.h):
        token-budget batches under the rule of _batches, `workers` double-buffered workers with pinned
        staging, the batch's lexical shortlist generated on the device (Model.cc:117-120). Units,
        batches, padding and result routing used to be Python objects; they are C++ now, and one call
        carries a whole translate(). A scoring service is one of its own (scores are set before its first call), and so
        is a sampling one for each temperature: the temperature is a service-wide setting of the C++ service, so every
        distinct temperature a caller uses keeps its own service -- workers, contexts and pinned staging -- until close().
        None is evicted before that (another thread's call may be in flight on it): a caller that sweeps temperatures
        closes the Service between them, or uses capi.Context.set_sampling, where the temperature is per call. The same
        holds for each truncation (top_k, top_p) of a sampling service."""
        trunc = None if truncation is None else (int(truncation[0]), float(truncation[1]))
        with self._lock:
            eng = self._engines.get((model.id, scores, float(temperature), trunc))
            if eng is None:
                V = model.dims[2]
                eng = capi.BatchService([model.engine], max_words=max(self.max_words, 1),
                                        wrap_length=min(self.ENGINE_LIMIT, max(self.max_words, 1)),
                                        limit_factor=self.limit_factor, workers_per_device=self.workers, pad_id=0,
                                        eos_id=model.vocabulary.eos_id(), alignments=True,
                                        lexical_shortlist=model.shortlist_blob, source_vocab=V, target_vocab=V,
                                        shared_vocab=False, check=False,  # as Model.cc:73-80 constructs it
                                        scores=scores, temperature=float(temperature), truncation=trunc)
                self._engines[(model.id, scores, float(temperature), trunc)] = eng
        return eng

    def _translate_samples(self, model: Model, per_request: List[List[List[int]]], samples: int, sampling, truncation=None):
        """`samples` histories lists shaped like _translate_segments': list j holds sample j of every segment, drawn from
        one encoding of the segment under capi.sampling_key(seed, its index in this call's flat list * samples + j)
        (include/slimt_hip_service_samples.h). Always scored. A segment above ENGINE_LIMIT tokens is refused."""
        flat = [seg for segs in per_request for seg in segs]
        if any(len(seg) > self.ENGINE_LIMIT for seg in flat):
            raise ValueError(f"samples: a segment has more than {self.ENGINE_LIMIT} tokens")
        out = [[[None] * len(segs) for segs in per_request] for _ in range(samples)]
        if not flat:
            return out
        res = self._engine(model, False, sampling[0], truncation).translate_samples(flat, samples, seed=int(sampling[1]))
        e = 0
        for r, segs in enumerate(per_request):
            for i in range(len(segs)):
                for j in range(samples):
                    out[j][r][i] = (res.target(e).tolist(), res.alignment(e).copy(), res.token_scores(e).copy())
                    e += 1
        res.close()
        return out

    def _translate_segments(self, model: Model, per_request: List[List[List[int]]], scores: bool = False, sampling=None,
                            truncation=None):
        """per request, per segment: (target ids, alignment, token scores | None). sampling: (temperature, seed) -- one
        draw per segment under capi.sampling_key(seed, the segment's index in this call's flat list); truncation:
        (top_k, top_p) of those draws"""
        eos = model.vocabulary.eos_id()
        flat, owner = [], []  # the sentences of the one request the C++ service gets; (request, index, piece)
        pieces_of = {}
        limit = self.ENGINE_LIMIT
        if all(len(seg) <= limit for segs in per_request for seg in segs):  # the usual call: nothing to split
            flat = [seg for segs in per_request for seg in segs]
        else:
            for r, segs in enumerate(per_request):
                for i, seg in enumerate(segs):
                    if len(seg) <= limit:
                        flat.append(seg)
                        owner.append((r, i, 0))
                        continue
                    pieces = self._split_long(list(seg), eos)
                    pieces_of[(r, i)] = len(pieces)
                    for k, piece in enumerate(pieces):
                        flat.append(piece)
                        owner.append((r, i, k))
        histories = [[None] * len(segs) for segs in per_request]
        if not flat:
            return histories
        if sampling is not None:
            res = self._engine(model, scores, sampling[0], truncation).translate(flat, seed=int(sampling[1]))
        elif truncation is not None:
            raise ValueError("truncation: only with sampling=(temperature, seed)")
        else:
            res = self._engine(model, scores).translate(flat)
        targets, t_off = res.targets.copy(), res.target_offsets.astype(np.int64)
        tok_sc = res.scores.copy() if scores else None
        align, a_off = res.alignments.copy(), res.align_offsets.astype(np.int64)
        src_len = res.source_lengths
        res.close()
        # per sentence: (target ids, alignment); the alignment is cut out of the call's one block when
        # somebody asks for it (_LazyAlignment): most callers read a few, and 24,000 reshaped views
        # per call were a tenth of a second of interpreter time
        parts = {}
        words_all = targets.tolist()
        to, ao, sl = t_off.tolist(), a_off.tolist(), src_len.tolist()
        if not pieces_of:
            n = 0
            for hist in histories:
                for i in range(len(hist)):
                    words = words_all[to[n]:to[n + 1]]
                    hist[i] = (words, _LazyAlignment(align, ao[n], ao[n + 1], len(words), sl[n]),
                               tok_sc[to[n]:to[n + 1]] if scores else None)
                    n += 1
            return histories
        for n, (r, i, k) in enumerate(owner):
            words = words_all[to[n]:to[n + 1]]
            alignment = _LazyAlignment(align, ao[n], ao[n + 1], len(words), sl[n])
            sc = tok_sc[to[n]:to[n + 1]] if scores else None
            if (r, i) in pieces_of:
                parts[(r, i, k)] = (words, alignment.array(), sl[n], sc)
            else:
                histories[r][i] = (words, alignment, sc)
        for (r, i), n in pieces_of.items():
            # a split segment: targets concatenated (inner EOS dropped), alignment rows block-diagonal
            # over the pieces' source tokens (the pieces' inner EOS columns dropped, the last one kept); scores
            # concatenated like the targets (the inner EOS tokens' dropped with them)
            got = [parts[(r, i, k)] for k in range(n)]
            widths = [L - 1 for _, _, L, _ in got[:-1]] + [got[-1][2]]
            total = sum(widths)
            out_words, rows, col, out_sc = [], [], 0, []
            for k, (words, alignment, L, sc) in enumerate(got):
                last = k == n - 1
                keep = len(words) if last or not len(words) or words[-1] != eos else len(words) - 1
                for t in range(keep):
                    row = np.zeros(total, np.float32)
                    row[col:col + widths[k]] = np.asarray(alignment[t], np.float32)[:widths[k]]
                    rows.append(row)
                out_words.extend(int(w) for w in words[:keep])
                if scores:
                    out_sc.append(sc[:keep])
                col += widths[k]
            histories[r][i] = (out_words, np.stack(rows) if rows else np.zeros((0, total), np.float32),
                               np.concatenate(out_sc) if scores else None)
        return histories

    # -- the binding's calls -----------------------------------------------------------------------
    def _respond_many(self, model: Model, sources: Sequence[AnnotatedText], histories) -> List[Response]:
        """Request::complete (Request.cc:136-170) for a whole call: every sentence's ids decoded in
        one SentencePiece batch, the source's gaps kept, target token ranges resolved on demand."""
        flat = [h[0] for hist in histories for h in hist]  # lists of ids
        decoded = model.vocabulary.decode_text_batch(flat, self.workers) if flat else []
        out, k, v = [], 0, model.vocabulary
        for source, hist in zip(sources, histories):
            # AnnotatedText.append_lazy_sentence per sentence, written out: the target text is joined once per
            # response, sentences recorded directly (this loop holds the interpreter lock while the
            # engine's threads wait for the next chunk)
            resp = Response(source=source)
            parts, sent, alignments = [], resp.target._sent, resp.alignments
            src_sent, data, prev_end, pos = source._sent, source.data, 0, 0
            for s, (words, alignment, sc) in enumerate(hist):
                w = src_sent[s]
                lazy = type(w) is _Lazy
                gap = data[prev_end:(w.begin if lazy else w[0])]  # source.gap_bytes(s)
                prev_end = w.end if lazy else w[-1]
                text = decoded[k].encode("utf-8")
                begin = pos + len(gap)
                pos = begin + len(text)
                parts.append(gap)
                parts.append(text)
                sent.append(_Lazy(begin, pos, len(words), functools.partial(_target_boundaries, v, begin, words)))
                alignments.append(alignment)
                if sc is not None:
                    resp.token_scores.append(sc)
                    resp.sentence_scores.append(float(np.sum(sc, dtype=np.float64)))
                k += 1
            parts.append(data[prev_end:] if hist else data)  # the gap behind the last sentence
            resp.target.data = b"".join(parts)
            out.append(resp)
        return out

    def translate(self, model: Model, texts: Sequence[str], html: bool = False,
                  encoding: Encoding = Encoding.UTF8, scores: bool = False, sampling=None, truncation=None,
                  samples: Optional[int] = None) -> List[Response]:
        """scores: every Response also carries token_scores (per target sentence, each target token's log-probability,
        EOS included; a wrapped segment's pieces concatenated) and sentence_scores (their sums).
        sampling: (temperature, seed) -- each sentence is one draw from the model at that temperature instead of the
        greedy translation, reproducible for a seed: the key of a segment is capi.sampling_key(seed, its index among the
        call's segments), so the same call gives the same text whatever the batcher does; with scores=True the scores are
        the draws' log-probabilities at that temperature. A sampled call goes to the engine as one request. Every
        distinct temperature keeps a batching service of its own until close() (_engine).
        truncation: (top_k, top_p) with sampling -- the draws come from the top_k most probable tokens (0: all) and the
        nucleus of mass top_p (1.0: all) of each step (include/slimt_hip.h, slimt_hip_ctx_set_sampling_truncation).
        samples: n >= 1 with sampling -- n draws of every sentence from ONE encoding of it (include/slimt_hip.h,
        slimt_hip_translate_fanout): each Response carries `samples`, its n alternatives as Responses (alternative j holds
        sample j of every sentence, always with scores; the Response returned is alternative 0). Sample j of the call's
        segment i is drawn under capi.sampling_key(seed, i * n + j)."""
        if html:
            raise NotImplementedError("HTML markup transfer is outside the ported path (SURVEY.md §2)")
        if samples is not None:
            if sampling is None or int(samples) < 1:
                raise ValueError("samples: n >= 1, and only with sampling=(temperature, seed)")
            processed = model.processor.process_many(texts, self.wrap_length, self.workers)
            per_sample = self._translate_samples(model, [segs for _, segs in processed], int(samples), sampling, truncation)
            alts = [self._respond_many(model, [src for src, _ in processed], h) for h in per_sample]
            out = alts[0]
            for r, resp in enumerate(out):
                resp.samples = [a[r] for a in alts]
                resp.to(encoding)
            return out
        # Large calls go through in chunks of documents, pipelined: while the engine translates chunk k
        # (a C call: no interpreter lock held), this thread splits and tokenises chunk k + 1 and
        # assembles the responses of chunk k - 1. Batches are formed per chunk (as they are per
        # arrival window in the reference's Async service).
        chunk = self.pipeline_documents
        if truncation is not None and sampling is None:
            raise ValueError("truncation: only with sampling=(temperature, seed)")
        if len(texts) <= chunk or sampling is not None:  # (sampled: one request, so that the segments' indices are the call's)
            processed = model.processor.process_many(texts, self.wrap_length, self.workers)
            histories = self._translate_segments(model, [segs for _, segs in processed], scores, sampling, truncation)
            out = self._respond_many(model, [src for src, _ in processed], histories)
        else:
            from concurrent.futures import ThreadPoolExecutor
            out, pending = [], []
            with ThreadPoolExecutor(max_workers=2) as pool:
                def finish(item):
                    processed, fut = item
                    out.extend(self._respond_many(model, [src for src, _ in processed], fut.result()))
                for k in range(0, len(texts), chunk):
                    processed = model.processor.process_many(texts[k:k + chunk], self.wrap_length, self.workers)
                    pending.append((processed, pool.submit(self._translate_segments, model, [segs for _, segs in processed],
                                                           scores)))
                    while len(pending) > 2:
                        finish(pending.pop(0))
                while pending:
                    finish(pending.pop(0))
        for r in out:
            r.to(encoding)
        return out

    def score(self, model: Model, sources: Sequence[str], targets: Sequence[str], alternatives: int = 0) -> List["PairScore"]:
        """Teacher-forced scoring of given translations (include/slimt_hip_service_score.h): targets[i] against
        sources[i], each text ONE sentence as the model's vocabulary tokenises it, EOS appended -- no sentence splitting,
        no wrapping: a source of more than ENGINE_LIMIT tokens is refused, a target may be any length. Every target
        position goes through the decoder in one pass; the output layer is the one translate() uses (the model's lexical
        shortlist per batch, else the full vocabulary), so a target token outside it scores -inf. Returns one PairScore
        per pair: the token ids of both sides, each target token's log-probability, their sum, and the
        [target tokens, source tokens] alignment (head 0 of the last decoder layer).
        alternatives = k (1..8; include/slimt_hip_service_alternatives.h): each PairScore also carries `alternatives` -- per
        target token the k most probable pieces of its position with their log-probabilities -- and `ranks`, each given
        token's place in that order (rank r < k means alternatives[t][r] is the token itself)."""
        if len(sources) != len(targets):
            raise ValueError(f"score: {len(targets)} targets for {len(sources)} sources")
        v = model.vocabulary
        eos = v.eos_id()
        src = [ids + [eos] for ids in v.encode_ids_batch(list(sources), self.workers)] if sources else []
        tgt = [ids + [eos] for ids in v.encode_ids_batch(list(targets), self.workers)] if targets else []
        for i, ids in enumerate(src):
            if len(ids) > self.ENGINE_LIMIT:
                raise ValueError(f"score: source {i} has {len(ids)} tokens, more than {self.ENGINE_LIMIT}")
        if not src:
            return []
        res = self._engine(model).score(src, tgt, alternatives) if alternatives else self._engine(model).score(src, tgt)
        out = []
        for i in range(len(src)):
            sc = res.token_scores(i).copy()
            out.append(PairScore(source_ids=src[i], target_ids=tgt[i], token_scores=sc,
                                 score=float(np.sum(sc, dtype=np.float64)), alignment=res.alignment(i).copy()))
            if alternatives:
                a_ids, a_sc, a_rank = res.alternatives(i)
                out[-1].ranks = [None if r == 0xFFFFFFFF else int(r) for r in a_rank]
                out[-1].alternatives = [[(v.piece(w), float(s)) for w, s in zip(row_ids, row_sc) if w != 0xFFFFFFFF]
                                        for row_ids, row_sc in zip(a_ids, a_sc)]
        res.close()
        return out

    def rerank(self, model: Model, sources: Sequence[str], candidates: Sequence[Sequence[str]],
               mean: bool = False) -> List[Tuple[List["PairScore"], Optional[int]]]:
        """Ranks candidates[i], the candidate translations of sources[i], from ONE encoding of each source
        (include/slimt_hip_service_candidates.h); texts are tokenised as score() tokenises them. Returns per source the
        candidates' PairScores in the given order and the index of the best one -- the largest summed log-probability, with
        mean=True the largest sum per token; the first of equals -- or None for a source without candidates."""
        if len(sources) != len(candidates):
            raise ValueError(f"rerank: {len(candidates)} candidate lists for {len(sources)} sources")
        v = model.vocabulary
        eos = v.eos_id()
        src = [ids + [eos] for ids in v.encode_ids_batch(list(sources), self.workers)] if sources else []
        for i, ids in enumerate(src):
            if len(ids) > self.ENGINE_LIMIT:
                raise ValueError(f"rerank: source {i} has {len(ids)} tokens, more than {self.ENGINE_LIMIT}")
        if not src:
            return []
        flat = [t for cs in candidates for t in cs]
        enc = [ids + [eos] for ids in v.encode_ids_batch(flat, self.workers)] if flat else []
        at, tgt = 0, []
        for cs in candidates:
            tgt.append(enc[at:at + len(cs)])
            at += len(cs)
        res, c_off, _, best = self._engine(model).score_candidates(src, tgt, mean=mean)
        out = []
        for i in range(len(src)):
            pairs = []
            for j, e in enumerate(range(int(c_off[i]), int(c_off[i + 1]))):
                sc = res.token_scores(e).copy()
                pairs.append(PairScore(source_ids=src[i], target_ids=tgt[i][j], token_scores=sc,
                                       score=float(np.sum(sc, dtype=np.float64)), alignment=res.alignment(e).copy()))
            out.append((pairs, None if best[i] == 0xFFFFFFFF else int(best[i])))
        res.close()
        return out

    def sample_and_rerank(self, model: Model, sources: Sequence[str], n: int, sampling, truncation=None, mean: bool = False):
        """translate(samples=n) followed by rerank() of each source's n samples: draws n translations of every source from
        one encoding of it, then scores them teacher-forced from one encoding again (greedy log-probabilities: the model's
        own, not the draws' at the sampling temperature). sources: each ONE sentence, as for rerank(). Returns (responses,
        ranked): translate()'s Responses with their `samples`, and rerank()'s list over the samples' target texts."""
        responses = self.translate(model, sources, sampling=sampling, truncation=truncation, samples=n)
        ranked = self.rerank(model, sources, [[a.target.text for a in r.samples] for r in responses], mean=mean)
        return responses, ranked

    def sample_and_select(self, model: Model, sources: Sequence[str], n: int, sampling, truncation=None, max_order: int = 4,
                          beta2: int = 4, encoding: Encoding = Encoding.UTF8) -> List[Response]:
        """translate(samples=n) followed by the consensus (minimum-Bayes-risk) pick: of the n draws of every sentence, the one
        that agrees most with the others -- the mean token n-gram F (orders 1..max_order, integer beta2 = beta^2; 4 is chrF's)
        against the sentence's other draws (include/slimt_hip.h, slimt_hip_consensus_select). The pick is made on the device
        behind the fan-out call that drew the samples: no second encoding and no scorer pass (sample_and_rerank makes both).
        Returns one Response per source, built from the winners (always with scores), carrying `utility` and `sample_index`
        per sentence: sentence i's winner is sample sample_index[i] of translate(samples=n) under the same sampling. n <= 64."""
        if sampling is None or int(n) < 1:
            raise ValueError("sample_and_select: n >= 1 and sampling=(temperature, seed)")
        processed = model.processor.process_many(sources, self.wrap_length, self.workers)
        per_request = [segs for _, segs in processed]
        flat = [seg for segs in per_request for seg in segs]
        if any(len(seg) > self.ENGINE_LIMIT for seg in flat):
            raise ValueError(f"samples: a segment has more than {self.ENGINE_LIMIT} tokens")
        histories = [[None] * len(segs) for segs in per_request]
        picked = [([0.0] * len(segs), [0] * len(segs)) for segs in per_request]
        if flat:
            res, utility, index = self._engine(model, False, sampling[0], truncation).translate_consensus(
                flat, int(n), seed=int(sampling[1]), max_order=max_order, beta2=beta2)
            e = 0
            for r, segs in enumerate(per_request):
                for i in range(len(segs)):
                    histories[r][i] = (res.target(e).tolist(), res.alignment(e).copy(), res.token_scores(e).copy())
                    picked[r][0][i], picked[r][1][i] = float(utility[e]), int(index[e])
                    e += 1
            res.close()
        out = self._respond_many(model, [src for src, _ in processed], histories)
        for resp, (u, j) in zip(out, picked):
            resp.utility, resp.sample_index = u, j
            resp.to(encoding)
        return out

    def beam_search(self, model: Model, texts: Sequence[str], beam: int, mean: bool = False,
                    encoding: Encoding = Encoding.UTF8) -> List[Response]:
        """Beam search with n-best output (include/slimt_hip.h, slimt_hip_translate_beam): every sentence is decoded with
        `beam` = k slots (1..capi.MAX_BEAM) from one encoding of it and comes back as its k best hypotheses, ordered by their
        summed log-probability (mean=True: per token). Each Response carries `nbest`, its k alternatives as Responses
        (alternative j holds the rank-j hypothesis of every sentence, always with scores; a sentence with fewer
        hypotheses has an empty one there), and `hypothesis_scores`, the engine's total per sentence; the Response returned
        is rank 0. Batches follow _batches' rule with at most max_words / beam sentences per call; the calls go through one
        capi.Context per model on model.engine, under the Service's lock, with the model's lexical shortlist generated per
        batch where it has one. A segment above ENGINE_LIMIT tokens is refused."""
        k = int(beam)
        if k < 1 or k > capi.MAX_BEAM:
            raise ValueError(f"beam_search: a beam of 1..{capi.MAX_BEAM} expected, not {beam}")
        processed = model.processor.process_many(texts, self.wrap_length, self.workers)
        per_request = [segs for _, segs in processed]
        units = [_Unit(r, i, list(seg)) for r, segs in enumerate(per_request) for i, seg in enumerate(segs)]
        if any(len(u.words) > self.ENGINE_LIMIT for u in units):
            raise ValueError(f"beam_search: a segment has more than {self.ENGINE_LIMIT} tokens")
        eos = model.vocabulary.eos_id()
        ranked = [[[None] * len(segs) for segs in per_request] for _ in range(k)]
        totals_of = [[[0.0] * len(segs) for segs in per_request] for _ in range(k)]
        per_call = max(1, self.max_words // k)
        batches, cur = [], []
        for u in sorted(units, key=lambda u: (len(u.words), u.request, u.index)):  # (_batches' walk, the rows bounded too)
            if cur and ((len(cur) + 1) * len(u.words) > self.max_words or len(cur) + 1 > per_call):
                batches.append(cur)
                cur = []
            cur.append(u)
        if cur:
            batches.append(cur)
        with self._lock:
            ctx = self._beam_contexts.get(model.id)
            if ctx is None and batches:
                rows = max(self.max_words, capi.MAX_BEAM)
                ctx = capi.Context(model.engine, rows, self.ENGINE_LIMIT, max_tokens=max(self.max_words, self.ENGINE_LIMIT))
                self._beam_contexts[model.id] = ctx
            for batch in batches:
                B, S = len(batch), max(len(u.words) for u in batch)
                ids, lens = np.zeros((B, S), np.uint32), np.zeros(B, np.uint32)
                for b, u in enumerate(batch):
                    ids[b, :len(u.words)] = u.words
                    lens[b] = len(u.words)
                if model.shortlist_generator is not None:
                    out, ln, tot, sc, al = ctx.translate_beam_generated(model.shortlist_generator, ids, lens, k, self.limit_factor,
                                                                        eos, mean, want_align=True)
                else:
                    out, ln, tot, sc, al = ctx.translate_beam(ids, lens, k, None, self.limit_factor, eos, mean, want_align=True)
                for b, u in enumerate(batch):
                    for j in range(k):
                        n, L = int(ln[b, j]), int(lens[b])
                        ranked[j][u.request][u.index] = (out[b, j, :n].tolist(), al[b, j, :n, :L].copy(), sc[b, j, :n].copy())
                        totals_of[j][u.request][u.index] = float(tot[b, j])
        sources = [src for src, _ in processed]
        alts = [self._respond_many(model, sources, h) for h in ranked]
        out = alts[0]
        for j, alt in enumerate(alts):
            for r, resp in enumerate(alt):
                resp.hypothesis_scores = totals_of[j][r]
        for r, resp in enumerate(out):
            resp.nbest = [a[r] for a in alts]
            resp.to(encoding)
        return out

    def pivot(self, first: Model, second: Model, texts: Sequence[str], html: bool = False,
              scores: bool = False, sampling=None, truncation=None) -> List[Response]:
        """sampling: (temperature, seed) -- both hops sample, the first under seed and the second under seed + 1;
        truncation: (top_k, top_p) of both hops' draws.
        source -> pivot with `first`, pivot -> target with `second`, sentence for sentence;
        alignments are marginalised over the pivot tokens (Response.cc:13-195). scores: the SECOND hop's scores --
        those of the final target tokens given the pivot text (the pivot's own probability is not in them)."""
        if html:
            raise NotImplementedError("HTML markup transfer is outside the ported path (SURVEY.md §2)")
        firsts = self.translate(first, texts, encoding=Encoding.Byte, sampling=sampling, truncation=truncation)
        second_in = [second.processor.process_annotated(r.target) for r in firsts]
        histories = self._translate_segments(second, [segs for _, segs in second_in], scores,
                                             None if sampling is None else (sampling[0], int(sampling[1]) + 1), truncation)
        seconds = self._respond_many(second, [src for src, _ in second_in], histories)
        return [combine(r1, r2) for r1, r2 in zip(firsts, seconds)]

    def close(self) -> None:
        for eng in self._engines.values():
            eng.close()
        self._engines.clear()
        for ctx in self._beam_contexts.values():
            ctx.close()
        self._beam_contexts.clear()


# -------------------------------------------------------------------------------------------------
def transfer_through_characters(source_side_pivots: Sequence[Range], target_side_pivots: Sequence[Range],
                                pivot_given_targets: Alignment) -> Alignment:
    """p(q' | t) over the second model's pivot tokens q' -> p(q | t) over the first model's
    pivot tokens q: each q' spreads its probability evenly over its bytes, each q collects
    what falls into its range; a trailing zero-width q' (EOS) is shared out evenly
    (Response.cc:13-116)."""
    T, nq = len(pivot_given_targets), len(source_side_pivots)
    out = [[0.0] * nq for _ in range(T)]
    sq = qt = 0
    while sq < nq and qt < len(target_side_pivots):
        a, b = source_side_pivots[sq], target_side_pivots[qt]
        if a.begin == b.begin and a.end == b.end:
            for t in range(T):
                out[t][sq] += pivot_given_targets[t][qt]
            sq, qt = sq + 1, qt + 1
            continue
        if b.size() == 0:  # a piece without surface before the end (SentencePiece's bare "▁"): its mass
            for t in range(T):  # goes to the pivot token at its position (the reference asserts overlap
                out[t][sq] += pivot_given_targets[t][qt]  # here, Response.cc:49, and divides by 0)
            qt += 1
            continue
        if a.size() == 0:  # likewise on the first model's side: nothing to collect
            sq += 1
            continue
        left, right = max(a.begin, b.begin), min(a.end, b.end)
        if right > left:
            share = (right - left) / float(b.size())
            for t in range(T):
                out[t][sq] += share * pivot_given_targets[t][qt]
        if a.end == b.end:
            sq, qt = sq + 1, qt + 1
        elif a.end > b.end:
            qt += 1
        else:
            sq += 1
    while qt < len(target_side_pivots):  # what is left has no surface: EOS
        for t in range(T):
            gift = pivot_given_targets[t][qt] / max(1, nq)
            for s in range(nq):
                out[t][s] += gift
        qt += 1
    return out


def remap_alignments(first: Response, second: Response) -> List[Alignment]:
    """p(s | t) = sum_q p(s | q) p(q | t) per sentence (Response.cc:118-177)."""
    out = []
    for sid in range(first.source.sentence_count()):
        s_given_q, q_given_t = first.alignments[sid], second.alignments[sid]
        q1 = [first.target.word_as_range(sid, i) for i in range(first.target.word_count(sid))]
        q2 = [second.source.word_as_range(sid, i) for i in range(second.source.word_count(sid))]
        remapped = np.asarray(transfer_through_characters(q1, q2, q_given_t), np.float32).reshape(len(q_given_t), len(q1))
        sq = np.asarray(s_given_q, np.float32).reshape(len(q1), -1)
        out.append(remapped @ sq)
    return out


def combine(first: Response, second: Response) -> Response:  # Response.cc:179-191
    r = Response()
    if len(first.alignments):
        r.alignments = remap_alignments(first, second)
    r.source, r.target = first.source, second.target
    r.token_scores, r.sentence_scores = second.token_scores, second.sentence_scores
    return r
