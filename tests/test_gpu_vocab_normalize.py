"""A normalizing vocabulary end to end (Vocab(normalizer="nfc"), Tokenizer): the ids against a plain vocabulary over
texts normalized beforehand, and against the ids recorded from the `tokenizers` library
(tests/golden/vocab/vocab_nfc.json, tools/make_vocab_nfc_golden.py)."""
import json
import os
import unicodedata

import pytest

from llmtokenizer_amd.api import BpeError
from llmtokenizer_amd.vocab import Tokenizer, Vocab

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab")


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    with open(os.path.join(GOLDEN, "vocab_nfc.json"), encoding="utf-8") as f:
        fx = json.load(f)
    with open(os.path.join(GOLDEN, fx["base"]), encoding="utf-8") as f:
        base = json.load(f)["tokenizer_json"]
    p = tmp_path_factory.mktemp("nfc") / "tokenizer.json"
    p.write_text(json.dumps(base, ensure_ascii=False), encoding="utf-8")
    plain = Vocab.from_tokenizer_json(p)
    nfc = Vocab(plain.merges, plain.byte_ids, plain.merge_ids, plain.special_ids, plain.specials, plain.rule, normalizer="nfc")
    nfc.to_tokenizer_json(p)
    return fx, plain, nfc, p


def test_file_round_trip(case):
    fx, plain, nfc, p = case
    with pytest.raises(BpeError, match="normalizer.*normalizers="):
        Vocab.from_tokenizer_json(p)
    assert Vocab.from_tokenizer_json(p, normalizers=("NFC",)) == nfc != plain
    assert "nfc" in repr(nfc) and "nfc" not in repr(plain)
    doc = json.loads(p.read_text(encoding="utf-8"))
    doc["normalizer"] = {"type": "Sequence", "normalizers": [{"type": "NFC"}]}
    p2 = p.with_name("sequence.json")
    p2.write_text(json.dumps(doc, ensure_ascii=False), encoding="utf-8")
    with pytest.raises(BpeError, match="normalizer \\('Sequence'\\)"):
        Vocab.from_tokenizer_json(p2, normalizers=("NFC", "Sequence"))


def test_ids(case):
    fx, plain, nfc, _ = case
    texts = fx["texts"]
    assert any(t != unicodedata.normalize("NFC", t) for t in texts)
    tn, tp = Tokenizer(nfc), Tokenizer(plain)
    try:
        ids, off = tn.encode_batch(texts)
        pids, poff = tp.encode_batch([unicodedata.normalize("NFC", t) for t in texts])
        assert ids.tolist() == pids.tolist() and off.tolist() == poff.tolist()
        assert [ids[a:b].tolist() for a, b in zip(off.tolist(), off.tolist()[1:])] == fx["ids"]
        assert [tn.encode(t).tolist() for t in texts[:4]] == fx["ids"][:4]
        rows = tn.encode_packed(texts, 16, 0)[0]
        assert rows.reshape(-1)[:len(ids)].tolist() == ids.tolist()
        for call in (lambda: tn.encode(texts[2], return_spans="byte"), lambda: tn.encode_batch(texts, return_spans="char")):
            with pytest.raises(BpeError, match="return_spans with a normalizing vocabulary"):
                call()
    finally:
        tn.close()
        tp.close()
