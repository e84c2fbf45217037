"""The unit table a vocabulary gives the consensus selection over characters (text.Vocabulary.consensus_units;
include/slimt_hip.h, slimt_hip_consensus_select_units): well-formed, and the expansion of a sentence's ids is the decoded
text's characters with the whitespace removed -- what chrF counts n-grams of. No GPU."""
import io
import random

import numpy as np
import pytest

from slimt_amd import text


@pytest.fixture(scope="module")
def trained():
    """(vocabulary, sentences): a 512-piece unigram model with byte fallback, trained here on synthetic text"""
    import sentencepiece
    rnd = random.Random(7)
    words = ["".join(rnd.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 8))) for _ in range(1200)]
    words += ["über", "naïve", "日本", "語"]
    sents = []
    for _ in range(4000):
        s = " ".join(rnd.choice(words) for _ in range(rnd.randint(3, 18)))
        sents.append(s[0].upper() + s[1:] + rnd.choice(".?!"))
    out = io.BytesIO()
    sentencepiece.SentencePieceTrainer.train(sentence_iterator=iter(sents), model_writer=out, vocab_size=512,
                                             model_type="unigram", pad_id=-1, unk_id=1, bos_id=-1, eos_id=0,
                                             byte_fallback=True, minloglevel=2)
    return text.Vocabulary(out.getvalue()), sents


def test_the_table_is_well_formed(trained):
    v, _ = trained
    off, units = v.consensus_units()
    assert off.dtype == units.dtype == np.uint32 and off.shape == (v.size() + 1,) and off[0] == 0 and off[-1] == units.size
    n = np.diff(off.astype(np.int64))
    assert (n >= 0).all() and n.max() <= 255 and n.max() >= 2
    for w in range(v.size()):
        if v.sp.is_control(w) or v.sp.is_unknown(w) or v.sp.is_unused(w):
            assert n[w] == 0, w
        elif v.sp.is_byte(w):
            assert list(units[off[w]:off[w + 1]]) == [0x110000 + int(v.piece(w)[3:5], 16)], w
    assert n[v.eos_id()] == 0 and sum(v.sp.is_byte(w) for w in range(v.size())) == 256
    # a model's padding rows expand to nothing
    padded, same = v.consensus_units(v.size() + 24)
    assert np.array_equal(padded[:off.size], off) and (padded[off.size:] == off[-1]).all() and np.array_equal(same, units)


def test_a_sentence_expands_to_its_text_without_whitespace(trained):
    v, sents = trained
    off, units = v.consensus_units()
    lines = [s for s in sents if s.isascii()][:6] + ["Two  spaces and a\ttab."]  # (no character that goes through its bytes)
    for line, ids in zip(lines, v.encode_ids_batch(lines)):
        spelled = [int(u) for w in ids + [v.eos_id()] for u in units[off[w]:off[w + 1]]]
        decoded = v.decode_text_batch([ids])[0]
        assert spelled == [ord(ch) for ch in decoded if not ch.isspace()], line
        assert len(spelled) > 5
    # a character the model has never seen goes through its bytes: one unit each, above every code point
    ids = v.encode_ids_batch(["a ж"])[0]
    spelled = [int(u) for w in ids for u in units[off[w]:off[w + 1]]]
    assert spelled[-2:] == [0x110000 + b for b in "ж".encode("utf-8")]
